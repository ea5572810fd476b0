"""Host side of ``NDMPS.linear_combination`` / ``recompress`` (csrc/lincomb.hip): validation of the inputs and the
metadata of the result, as pure functions of the objects' metadata (no GPU, no cores read).

The device computes the TT-SVD rounding of ``sum_a w_a X^a``; see csrc/lincomb.hip for the algorithm.  Rank rule at
bond k, s the bond's singular values in descending order: keep ``s_j > max(cutoff * s_0, floor * scale)`` with
``scale = sum_a |w_a| * norm_value_a`` and the storage floor (1e-6 for fp32 work, 1e-8 for fp64), at most
``max_bond`` and ``min(prod_{j<k} d_j, d_k r_{k+1})``.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SUMMED_BOND = 4096  # the direct eigen-solver's order limit (eig_tridiag.hip kMaxN)
FLOOR_F32 = 1e-6
FLOOR_F64 = 1e-8

# storage dtype names (torch dtypes are compared by name so this module needs no torch)
_CODES = {"torch.float32": 0, "torch.bfloat16": 1, "torch.float64": 2}


def dtype_code(dtype) -> int:
    """0 fp32, 1 bf16, 2 fp64 (the kernels' storage codes)."""
    key = str(dtype)
    if key not in _CODES:
        raise ValueError(f"unsupported storage dtype {dtype}")
    return _CODES[key]


def work_is_f64(codes, dtype=None) -> bool:
    """The work type of an operation on inputs with the storage ``codes`` whose result is asked for as ``dtype`` (None or
    a torch dtype, compared by name): fp64 when fp64 is asked for, fp32 when fp32 is asked for, and otherwise (None or
    bf16, which rounds the finished cores) fp64 iff some input is fp64."""
    return str(dtype) == "torch.float64" or (str(dtype) != "torch.float32" and any(c == 2 for c in codes))


def floor_for(f64: bool) -> float:
    return FLOOR_F64 if f64 else FLOOR_F32


def check_args(n_objs: int, weights, cutoff: float, max_bond) -> list:
    """The weights as floats; ValueError for an empty list, a length mismatch, a non-finite weight, cutoff < 0 or
    max_bond < 1."""
    if n_objs < 1:
        raise ValueError("linear_combination needs at least one object")
    try:
        w = [float(v) for v in weights]
    except TypeError as exc:
        raise ValueError("weights must be a sequence of real numbers") from exc
    if len(w) != n_objs:
        raise ValueError(f"{n_objs} objects but {len(w)} weights")
    if not all(math.isfinite(v) for v in w):
        raise ValueError("every weight must be finite")
    if not (cutoff >= 0 and math.isfinite(cutoff)):
        raise ValueError("cutoff must be a finite non-negative number")
    if max_bond is not None and int(max_bond) < 1:
        raise ValueError("max_bond must be at least 1")
    return w


def check_compatible(metas) -> None:
    """metas: one dict per object with qubit_size, shape, mode, device, dims.  ValueError when they differ."""
    m0 = metas[0]
    for i, m in enumerate(metas[1:], start=1):
        for key in ("shape", "mode", "device"):
            if m[key] != m0[key]:
                raise ValueError(f"object {i} differs from object 0 in {key}: {m[key]!r} != {m0[key]!r}")
        if not np.array_equal(np.asarray(m["qubit_size"]), np.asarray(m0["qubit_size"])):
            raise ValueError(f"object {i} differs from object 0 in qubit_size")
        if list(m["dims"]) != list(m0["dims"]):
            raise ValueError(f"object {i} differs from object 0 in its site dims: {m['dims']} != {m0['dims']}")


def summed_bonds(bond_lists) -> list:
    """sum_a chi_{a,k} for every bond k (bond_lists: per object, the L + 1 bonds with the outer ones)."""
    return [int(v) for v in np.sum(np.asarray(bond_lists, dtype=np.int64), axis=0)]


def check_summed_bonds(bond_lists) -> None:
    """ValueError when some inner summed bond exceeds MAX_SUMMED_BOND."""
    sb = summed_bonds(bond_lists)
    for k in range(1, len(sb) - 1):
        if sb[k] > MAX_SUMMED_BOND:
            raise ValueError(f"bond {k}: the inputs' bonds sum to {sb[k]} > {MAX_SUMMED_BOND}, the eigen-solver's limit; "
                             f"recompress the inputs first (recompress(max_bond=...))")


def scale_of(weights, norms) -> float:
    """sum_a |w_a| * norm_value_a: the absolute scale of the storage floor."""
    return float(sum(abs(w) * float(n) for w, n in zip(weights, norms)))


def rank_cap(dims, k: int, r_next: int, max_bond) -> int:
    """The largest rank bond k can have: min(prod_{j<k} d_j, d_k r_{k+1}, max_bond)."""
    cap = min(int(np.prod(dims[:k], dtype=np.int64)), int(dims[k]) * int(r_next))
    return cap if max_bond is None else min(cap, int(max_bond))


def kept_rank(s, cutoff: float, floor: float, scale: float, cap: int) -> int:
    """Number of singular values kept at one bond (0: nothing survives -> the zero MPS)."""
    s = np.asarray(s, dtype=np.float64)
    if s.size == 0 or not s[0] > floor * scale:
        return 0
    thr = max(cutoff * s[0], floor * scale)
    return int(min(max(np.count_nonzero(s > thr), 1), cap))
