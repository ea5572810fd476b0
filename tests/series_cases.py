"""The chains NDMPS.gram is tested on element by element, shared by tests/test_series_host.py (CPU: the bar is sound
and has teeth on exactly these cases) and tests/test_gpu_series.py (the kernels against the oracle on the same cases).

The bar of an entry is ``max(overlap_bound(a, b), overlap_bound(b, a))`` (oracle/chain_bound.py) around
``oracle.mps.mps_overlap``: it only separates a right contraction from a wrong one when the products of magnitudes do
not dwarf the value, so the cores are non-negative draws (uniform in [0.5, 1]), the oracle's swept cores of
``synthetic_mri`` volumes, or integers (where equality is the bar).  Values are exactly representable in the storage
type of their object.  A case: ``dims``, ``bonds_a`` (one bond list per object), ``bonds_b`` (None: symmetric),
``storage_a`` / ``storage_b`` (per object: "f32", "bf16", "f64"), ``family`` and the ``route`` the library must take.
"""
import zlib

import numpy as np

from oracle import chain_cases as cc

U64 = [1, 8, 64, 64, 64, 64, 64, 8, 1]
RAGGED = [[1, 8, 33, 17, 64, 8, 1], [1, 5, 17, 64, 33, 3, 1], [1, 8, 64, 33, 17, 8, 1]]
WIDE = [1, 16, 128, 16, 1]


def _case(dims, bonds_a, storage_a, route, family="pos", bonds_b=None, storage_b=None):
    sa = [storage_a] * len(bonds_a) if isinstance(storage_a, str) else list(storage_a)
    sb = None
    if bonds_b is not None:
        sb = [storage_b or "f32"] * len(bonds_b) if isinstance(storage_b or "f32", str) else list(storage_b)
    return dict(dims=list(dims), bonds_a=bonds_a, bonds_b=bonds_b, storage_a=sa, storage_b=sb, route=route, family=family)


CASES = {
    # ---- resident (every inner bond <= 64)
    "uniform64_f32": _case([8] * 8, [U64] * 3, "f32", "resident"),
    "ragged_f32": _case([8] * 6, RAGGED, "f32", "resident"),
    "ragged_bf16": _case([8] * 6, RAGGED, "bf16", "resident"),
    "ragged_f64": _case([8] * 6, RAGGED, "f64", "resident"),
    "ragged_mixed": _case([8] * 6, RAGGED, ["f32", "bf16", "f64"], "resident"),
    "bonds_one": _case([4, 6, 4, 6], [[1, 1, 1, 1, 1]] * 2, "f32", "resident"),
    "L1": _case([37], [[1, 1]] * 3, ["f32", "bf16", "f64"], "resident"),
    "L2": _case([33, 65], [[1, 33, 1], [1, 7, 1]], "f32", "resident"),
    "K1": _case([8] * 4, [[1, 8, 64, 8, 1]], "f32", "resident"),
    "rect_2x3": _case([8] * 6, RAGGED[:2], "f32", "resident", bonds_b=RAGGED, storage_b=["f64", "f32", "bf16"]),
    "rect_1x3": _case([8] * 6, RAGGED[2:], "bf16", "resident", bonds_b=RAGGED, storage_b="f32"),
    "rect_3x1": _case([8] * 6, RAGGED, "f32", "resident", bonds_b=RAGGED[1:2], storage_b="f64"),
    "swept_mri": _case([], [[]] * 3, "f32", "resident", family="swept"),
    "disjoint": _case([8] * 4, [[1, 8, 16, 8, 1]] * 3, "f32", "resident", family="disjoint"),
    "int_resident": _case([8, 16, 9, 10], [[1, 8, 16, 10, 1], [1, 3, 16, 5, 1], [1, 8, 7, 10, 1]],
                          ["f32", "bf16", "f64"], "resident", family="integer"),
    # ---- general: equal bonds above the resident limit (batched), ragged above it (pair by pair)
    "wide_equal": _case([16] * 4, [WIDE] * 3, ["f32", "bf16", "f64"], "batched"),
    "wide_equal_rect": _case([16] * 4, [WIDE] * 2, "f32", "batched", bonds_b=[WIDE] * 3, storage_b="f32"),
    "wide_ragged": _case([16] * 4, [WIDE, [1, 16, 65, 9, 1], [1, 3, 20, 16, 1]], ["f32", "f64", "bf16"], "per-pair"),
    "int_wide": _case([16] * 4, [[1, 16, 80, 16, 1]] * 2, "f32", "batched", family="integer"),
    "int_wide_ragged": _case([16] * 4, [[1, 16, 80, 16, 1], [1, 4, 7, 2, 1]], ["f32", "f64"], "per-pair", family="integer"),
}
# the launch split: 362 objects of tiny chains, 65 703 pairs
MANY = _case([2, 3, 2], [[1, 2, 2, 1]] * 362, "f32", "resident")


def _draw(name, side, idx, dims, bonds, storage, family):
    rng = np.random.default_rng(zlib.crc32(f"{name}/{side}/{idx}".encode()))
    cores = []
    for j, d in enumerate(dims):
        shape = (bonds[j], d, bonds[j + 1])
        if family == "integer":
            cores.append(rng.integers(-1, 2, size=shape).astype(np.float64))
            continue
        c = rng.uniform(0.5, 1.0, size=shape)
        if family == "disjoint" and j == 0 and idx < 2:  # objects 0 and 1 live on different halves of site 0
            c[:, (d // 2 if idx == 0 else 0):(d if idx == 0 else d // 2), :] = 0.0
        cores.append(cc.to_storage(c, storage))
    return cores


def _swept():
    """The oracle's swept cores of three synthetic_mri 64^3 volumes (max_bond 16), rounded to fp32."""
    from oracle.metrics import synthetic_mri
    from oracle.ndmps_oracle import OracleNDMPS

    out = []
    for seed in (11, 12, 13):
        o = OracleNDMPS.from_tensor(synthetic_mri((64, 64, 64), seed=seed), max_bond=16)
        out.append([cc.to_storage(c, "f32") for c in o.mps._cores])
    return out


def cores_of(name, case=None):
    """(list_a, list_b or None): per object the fp64 cores holding exactly the stored values."""
    case = case or CASES[name]
    if case["family"] == "swept":
        return _swept(), None
    la = [_draw(name, "a", i, case["dims"], b, s, case["family"])
          for i, (b, s) in enumerate(zip(case["bonds_a"], case["storage_a"]))]
    lb = None
    if case["bonds_b"] is not None:
        lb = [_draw(name, "b", i, case["dims"], b, s, case["family"])
              for i, (b, s) in enumerate(zip(case["bonds_b"], case["storage_b"]))]
    return la, lb
