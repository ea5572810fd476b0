"""The chains the weighted Gram matrix ``NDMPS.gram(objs, weight=w)`` is tested on entry by entry, shared by
tests/test_wgram_host.py (CPU: the bar is sound and has teeth on exactly these cases) and tests/test_gpu_wgram.py (the
kernels against the dense reference on the same cases).

The reference of an entry is the fp64 sum ``sum a * w * b`` over the three dense site-order tensors
(``oracle.mps.mps_to_dense``); the bar is ``core.wgram.weighted_bound``.  It only separates a right contraction from a
wrong one when the products of magnitudes do not dwarf the value, so the cores are non-negative draws (uniform in
[0.5, 1], as tests/series_cases.py draws them), the oracle's swept cores of real volumes, or integers in {-1, 0, 1}
(where equality is the bar).  Values are exactly representable in the storage type of their object.

A case: ``dims``, ``bonds_a`` (one bond list per object), ``bonds_b`` (None: symmetric), ``bonds_w``, ``storage_a`` /
``storage_b`` (per object) / ``storage_w``, ``family`` and the ``route`` the library must take.  The ragged weight has
the bonds [1, 3, 5, 17, 5, 2, 1]: six sites need seven bonds.
"""
import zlib

import numpy as np

from oracle import chain_cases as cc
from oracle.mps import mps_to_dense
from series_cases import RAGGED

RAGGED_W = [1, 3, 5, 17, 5, 2, 1]
B64 = [1, 8, 64, 8, 1]


def _case(dims, bonds_a, storage_a, bonds_w, route, family="pos", storage_w="f32", bonds_b=None, storage_b=None):
    sa = [storage_a] * len(bonds_a) if isinstance(storage_a, str) else list(storage_a)
    sb = None
    if bonds_b is not None:
        sb = [storage_b or "f32"] * len(bonds_b) if isinstance(storage_b or "f32", str) else list(storage_b)
    return dict(dims=list(dims), bonds_a=bonds_a, bonds_b=bonds_b, bonds_w=list(bonds_w), storage_a=sa, storage_b=sb,
                storage_w=storage_w, route=route, family=family)


CASES = {
    # ---- resident (every inner bond of the objects <= 64; the weight's bonds are unrestricted)
    "uniform64": _case([8] * 4, [B64] * 3, "f32", [1, 8, 16, 8, 1], "resident"),
    "ragged_f32": _case([8] * 6, RAGGED, "f32", RAGGED_W, "resident"),
    "ragged_bf16": _case([8] * 6, RAGGED, "bf16", RAGGED_W, "resident", storage_w="bf16"),
    "ragged_f64": _case([8] * 6, RAGGED, "f64", RAGGED_W, "resident", storage_w="f64"),
    "ragged_mixed": _case([8] * 6, RAGGED, ["f32", "bf16", "f64"], RAGGED_W, "resident", storage_w="bf16"),
    "w_bond_one": _case([8] * 4, [[1, 8, 33, 8, 1], [1, 5, 17, 3, 1]], "f32", [1, 1, 1, 1, 1], "resident"),
    "all_bonds_one": _case([4, 6, 4, 6], [[1, 1, 1, 1, 1]] * 2, "f32", [1, 1, 1, 1, 1], "resident"),
    "L1": _case([37], [[1, 1]] * 3, ["f32", "bf16", "f64"], [1, 1], "resident", storage_w="f64"),
    "L2": _case([33, 65], [[1, 33, 1], [1, 7, 1]], "f32", [1, 70, 1], "resident"),  # chi_w above the resident limit
    "K1": _case([8] * 4, [B64], "f32", [1, 4, 9, 4, 1], "resident"),
    "rect_2x3": _case([8] * 6, RAGGED[:2], "f32", RAGGED_W, "resident", bonds_b=RAGGED, storage_b=["f64", "f32", "bf16"]),
    "rect_3x1": _case([8] * 6, RAGGED, "f32", RAGGED_W, "resident", storage_w="f64", bonds_b=RAGGED[1:2], storage_b="f64"),
    "disjoint": _case([8] * 4, [[1, 8, 16, 8, 1]] * 3, "f32", [1, 4, 6, 4, 1], "resident", family="disjoint"),
    "int_resident": _case([8, 16, 9, 10], [[1, 8, 16, 10, 1], [1, 3, 16, 5, 1], [1, 8, 7, 10, 1]],
                          ["f32", "bf16", "f64"], [1, 4, 7, 3, 1], "resident", family="integer"),
    "swept": _case([], [[]] * 3, "f32", [], "resident", family="swept"),
    "five": _case([8] * 4, [[1, 8, 33, 8, 1], [1, 5, 17, 3, 1], B64, [1, 2, 9, 8, 1], [1, 8, 16, 4, 1]], "f32",
                  [1, 4, 6, 4, 1], "resident"),  # five objects: the chunked workspace
    # ---- general: some inner bond of the objects above the resident limit, pair by pair
    "wide": _case([16] * 4, [[1, 16, 80, 16, 1], [1, 4, 7, 2, 1]], ["f32", "f64"], [1, 4, 8, 4, 1], "per-pair"),
    "int_wide": _case([16] * 4, [[1, 16, 80, 16, 1], [1, 4, 7, 2, 1]], ["f32", "bf16"], [1, 4, 8, 4, 1], "per-pair",
                      family="integer"),
}
# one grid of many pairs: 40 objects of tiny chains, 820 pairs
MANY = _case([2, 3, 2], [[1, 2, 2, 1]] * 40, "f32", [1, 2, 2, 1], "resident")


def _draw(name, side, idx, dims, bonds, storage, family):
    rng = np.random.default_rng(zlib.crc32(f"wgram/{name}/{side}/{idx}".encode()))
    cores = []
    for j, d in enumerate(dims):
        shape = (bonds[j], d, bonds[j + 1])
        if family == "integer":
            cores.append(rng.integers(-1, 2, size=shape).astype(np.float64))
            continue
        c = rng.uniform(0.5, 1.0, size=shape)
        if family == "disjoint" and j == 0:
            if side == "a" and idx == 0:  # object 0 lives on the first half of site 0 ...
                c[:, d // 2:, :] = 0.0
            if side == "w":               # ... and the weight on the second
                c[:, :d // 2, :] = 0.0
        cores.append(cc.to_storage(c, storage))
    return cores


_SWEPT = None


def _swept():
    """The oracle's swept cores of three synthetic_mri 32^3 volumes (max_bond 16) and of a ball indicator (max_bond 8),
    rounded to fp32.  Computed once."""
    global _SWEPT
    if _SWEPT is None:
        from oracle.metrics import synthetic_mri
        from oracle.ndmps_oracle import OracleNDMPS

        objs = []
        for seed in (11, 12, 13):
            o = OracleNDMPS.from_tensor(synthetic_mri((32, 32, 32), seed=seed), max_bond=16)
            objs.append([cc.to_storage(c, "f32") for c in o.mps._cores])
        z, y, x = np.indices((32, 32, 32))
        ball = ((z - 15.5) ** 2 + (y - 15.5) ** 2 + (x - 15.5) ** 2 <= 12.0 ** 2).astype(np.float64)
        w = [cc.to_storage(c, "f32") for c in OracleNDMPS.from_tensor(ball, max_bond=8).mps._cores]
        _SWEPT = (objs, w)
    return _SWEPT


def cores_of(name, case=None):
    """(list_a, list_b or None, w): per object the fp64 cores holding exactly the stored values."""
    case = case or CASES[name]
    if case["family"] == "swept":
        objs, w = _swept()
        return objs, None, w
    la = [_draw(name, "a", i, case["dims"], b, s, case["family"])
          for i, (b, s) in enumerate(zip(case["bonds_a"], case["storage_a"]))]
    lb = None
    if case["bonds_b"] is not None:
        lb = [_draw(name, "b", i, case["dims"], b, s, case["family"])
              for i, (b, s) in enumerate(zip(case["bonds_b"], case["storage_b"]))]
    w = _draw(name, "w", 0, case["dims"], case["bonds_w"], case["storage_w"], case["family"])
    return la, lb, w


def pairs_of(la, lb):
    """(i, k, cores_a, cores_b) of every computed entry: a <= b in the symmetric case."""
    if lb is None:
        return [(i, k, la[i], la[k]) for i in range(len(la)) for k in range(i, len(la))]
    return [(i, k, la[i], lb[k]) for i in range(len(la)) for k in range(len(lb))]


def dense_reference(la, lb, w):
    """The fp64 matrix of ``sum a * w * b`` over the dense site-order tensors (every entry, mirror included)."""
    dw = mps_to_dense(w).reshape(-1)
    da = np.stack([mps_to_dense(c).reshape(-1) for c in la])
    db = da if lb is None else np.stack([mps_to_dense(c).reshape(-1) for c in lb])
    return np.array([[float(np.sum(x * dw * y)) for y in db] for x in da])


_REFS = {}


def reference(name, case=None):
    """(la, lb, w, ref): the cores of a case and its dense reference, computed once and shared."""
    if name not in _REFS:
        la, lb, w = cores_of(name, case)
        _REFS[name] = (la, lb, w, dense_reference(la, lb, w))
    return _REFS[name]
