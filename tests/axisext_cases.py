"""Cases, references and bars of the extremes along axes from the cores (csrc/axisext.hip, core/axisext.py).

Nothing here touches a GPU: tests/test_axisext_host.py runs the planner and the bars on the reference and on modelled
faults, tests/test_gpu_axisext.py on what the kernels return.

Integer chains.  The chains of tests/valstat_cases.py with THREE-axis factor arrays (one row per site, the rows multiply
to the site dims), so that every single axis and every pair of axes can be reduced, and one chain of positive cores
whose padding would show: every voxel of ``int_positive`` is a sum of 64 products of five entries from {1, 2}, so it
lies in [64, 2048]; ``int_negative`` is the same chain with core 0 negated.  A padded row or column handed to the
epilogue as data is a 0, which is below every voxel of the one and above every voxel of the other.

Two bars.

* exact, on integer cores: values and indices equal NumPy's on the fp64 reference (first occurrence on ties).
* sandwich, on the real cores of ``valstat_cases.REAL_CASES`` (two-axis volumes): a computed voxel lies within
  ``bound`` of its reference, so the computed maximum of a ray lies in
  ``[max_i(ref_i - bound_i), max_i(ref_i + bound_i)]``, and the place of the computed maximum is an index i that can
  be the largest: ``ref_i + bound_i >= max_j(ref_j - bound_j)``.  Where exactly one index of a ray can be, the index
  must be NumPy's.  A ray with more than one such index is ambiguous; ``real_case`` asserts, from the reference and
  the bound alone, that at most 10 % of the rays of a case are.  The minimum mirrors this.
"""
from __future__ import annotations

import functools
import itertools
import zlib

import numpy as np

import valstat_cases as vc
from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle.mps import mps_to_dense

OPS = ("max", "min")
MAX_AMBIGUOUS = 0.10
TILE = 64  # the tile of one workgroup in the reducing product

# chain -> three-axis factor array, one row per site
FACTORS = {
    "int_8x7": [[2, 2, 2]] * 7,
    "int_wide": [[2, 2, 2], [2, 4, 2], [3, 1, 3], [5, 2, 1]],
    "int_tail_last": [[1, 6, 1], [4, 5, 5], [41, 1, 1]],
    "int_no_tail": [[3, 1, 1], [1, 2, 1], [1, 1, 2], [16, 16, 32]],
    "int_tail_all": [[5, 1, 1], [1, 7, 1], [1, 1, 3], [2, 3, 1], [1, 2, 2]],
}
POSITIVE = ([5, 7, 3, 6, 4], [1, 2, 4, 4, 2, 1])
FACTORS["int_positive"] = FACTORS["int_negative"] = FACTORS["int_tail_all"]
INT_NAMES = ("int_8x7", "int_wide", "int_tail_last", "int_no_tail", "int_tail_all", "int_positive")
SIGNED_NAMES = INT_NAMES + ("int_negative",)


def axis_sets(ndim):
    """Every single axis and every pair of axes."""
    return [(a,) for a in range(ndim)] + (list(itertools.combinations(range(ndim), 2)) if ndim > 2 else [])


def split_tables(dest, n_cols):
    """``_Plan.split_tables`` from the oracle's index map: (row_off, col_off ascending, col_perm).  ``dest`` is the
    site-order offset of every C-order voxel, so its inverse is the C-order offset of every site-order element; the
    element (r, c) of the site-order tensor seen as rows x n_cols must sit at row_off[r] + col_off[c]."""
    src = np.argsort(dest.reshape(-1), kind="stable").astype(np.int64)
    row_off, col_off = src[::n_cols].copy(), src[:n_cols].copy()
    assert np.array_equal(src.reshape(-1, n_cols), row_off[:, None] + col_off[None, :]), "the offsets are not additive"
    perm = np.argsort(col_off, kind="stable")
    return row_off, np.ascontiguousarray(col_off[perm]), perm.astype(np.int32)


class IntCase:
    """An integer chain on its three-axis volume: cores, the fp64 reference as the volume, the last product in site
    order, and the split tables."""

    def __init__(self, name, storage):
        self.name, self.storage = name, storage
        if name in ("int_positive", "int_negative"):
            self.dims, self.bonds = POSITIVE
            rng = np.random.default_rng(zlib.crc32(f"int_positive/{storage}".encode()))
            self.cores = [rng.integers(1, 3, size=(self.bonds[i], d, self.bonds[i + 1])).astype(np.float64)
                          for i, d in enumerate(self.dims)]
            if name == "int_negative":
                self.cores[0] = -self.cores[0]
        else:
            self.dims, self.bonds = vc.INT_CHAINS[name]
            self.cores = cc.draw_cores(name, self.dims, self.bonds, "integer", storage)
        cc.check_chain(self.dims, self.bonds)
        self.fa = np.array(FACTORS[name], dtype=np.int64)
        assert [int(v) for v in np.prod(self.fa, axis=1)] == list(self.dims), name
        self.shape = tuple(int(v) for v in np.prod(self.fa, axis=0))
        self.dest = cb.flat_destination_factors(self.fa)
        self.m, self.n = vc.last_product_shape(self.dims)
        self.tables = split_tables(self.dest, self.n)
        self.set_cores(self.cores)

    def set_cores(self, cores):
        with np.errstate(invalid="ignore"):
            self.site = mps_to_dense(cores).reshape(self.m, self.n)
        self.ref = cb.to_volume(self.site, self.dest.reshape(-1)).reshape(self.shape)
        self.bound = np.zeros_like(self.ref)

    def with_nan(self):
        """A copy of the case with NaN planted in one core entry (``valstat_cases.with_nan``'s place)."""
        other = IntCase.__new__(IntCase)
        other.__dict__.update(self.__dict__)
        other.cores = [x.copy() for x in self.cores]
        i = min(1, len(other.cores) - 1)
        other.cores[i][0, other.cores[i].shape[1] // 2, 0] = np.nan
        other.set_cores(other.cores)
        return other


@functools.lru_cache(maxsize=4)
def int_case(name, storage):
    return IntCase(name, storage)


class RealCase:
    """A case of ``valstat_cases`` as its two-axis volume, with the tables of its last product."""

    def __init__(self, name, family, storage):
        c = vc.case(name, family, storage)
        self.name, self.storage, self.cores, self.fa, self.shape = name, storage, c.cores, c.fa, c.shape
        self.dims, self.bonds = c.dims, c.bonds
        self.ref, self.bound = c.ref.reshape(c.shape), c.bound.reshape(c.shape)
        self.m, self.n = vc.last_product_shape(c.dims)
        self.site = c.site.reshape(self.m, self.n)
        self.dest = c.dest
        self.tables = split_tables(c.dest, self.n)


@functools.lru_cache(maxsize=2)
def real_case(name, family, storage):
    c = RealCase(name, family, storage)
    for axis in range(len(c.shape)):
        for op in OPS:
            share = ambiguous_share(c.ref, c.bound, axis, op)
            assert share <= MAX_AMBIGUOUS, f"{name}/{family}/{storage} axis {axis} {op}: {share:.3f} of the rays are ambiguous"
    return c


# ------------------------------------------------------------------------------------------------ what NumPy says
def ref_values(ref, axes, op):
    """``np.fmax.reduce`` / ``np.fmin.reduce`` over ``axes``: NaN takes no part, a ray of NaN only is NaN."""
    f = np.fmax if op == "max" else np.fmin
    out = ref
    for a in sorted(axes, reverse=True):
        out = f.reduce(out, axis=a)
    return out


def ref_index(ref, axis, op):
    """``np.argmax`` / ``np.argmin`` along ``axis`` that skips NaN; -1 for a ray of NaN only."""
    nan = np.isnan(ref)
    filled = np.where(nan, -np.inf if op == "max" else np.inf, ref)
    idx = (np.argmax if op == "max" else np.argmin)(filled, axis=axis).astype(np.int64)
    return np.where(nan.all(axis=axis), -1, idx)


def ref_flat(ref, op):
    """(flat C-order index of the first extreme that is not NaN, its value); (-1, nan) for NaN only."""
    flat = ref.reshape(-1)
    if np.isnan(flat).all():
        return -1, np.nan
    i = int((np.nanargmax if op == "max" else np.nanargmin)(flat))
    return i, float(flat[i])


def tied_share(ref, axis, op):
    """Share of the rays along ``axis`` whose extreme is attained more than once."""
    best = ref_values(ref, (axis,), op)
    return float(np.mean((ref == np.expand_dims(best, axis)).sum(axis=axis) > 1))


# ------------------------------------------------------------------------------------------------ the exact bar
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def exact_values(got, ref, axes, op):
    want = ref_values(ref, axes, op)
    assert _same(np.asarray(got, dtype=np.float64), want), (op, axes, np.argwhere(np.asarray(got) != want)[:4])


def exact_index(got, ref, axis, op):
    want = ref_index(ref, axis, op)
    got = np.asarray(got)
    assert got.dtype == np.int64 and _same(got, want), (op, axis, np.argwhere(got != want)[:4])


def exact_flat(got_index, got_value, ref, op):
    i, v = ref_flat(ref, op)
    assert got_index == i and (got_value == v or (np.isnan(v) and np.isnan(got_value))), (op, got_index, got_value, i, v)


# ------------------------------------------------------------------------------------------------ the sandwich bar
def _sign(op):
    return 1.0 if op == "max" else -1.0


def candidates(ref, bound, axis, op):
    """Boolean array: index i of its ray can hold the computed extreme, ``ref_i + bound_i >= max_j(ref_j - bound_j)``."""
    s = _sign(op)
    floor = np.max(s * ref - bound, axis=axis, keepdims=True)
    return s * ref + bound >= floor


def ambiguous_share(ref, bound, axis, op):
    return float(np.mean(candidates(ref, bound, axis, op).sum(axis=axis) > 1))


def sandwich_values(got, ref, bound, axes, op):
    s = _sign(op)
    got = s * np.asarray(got, dtype=np.float64)
    lo, hi = np.max(s * ref - bound, axis=tuple(axes)), np.max(s * ref + bound, axis=tuple(axes))
    assert got.shape == lo.shape, (got.shape, lo.shape)
    bad = ~((lo <= got) & (got <= hi))
    assert not bad.any(), (op, axes, np.argwhere(bad)[:4])


def sandwich_index(got, ref, bound, axis, op):
    """Returns the share of ambiguous rays, where the index is only required to be a candidate."""
    got = np.asarray(got)
    can = candidates(ref, bound, axis, op)
    assert got.dtype == np.int64 and got.shape == can.sum(axis=axis).shape, (got.dtype, got.shape)
    assert ((got >= 0) & (got < ref.shape[axis])).all(), "an index outside its axis"
    hit = np.take_along_axis(can, np.expand_dims(got, axis), axis=axis).squeeze(axis)
    assert hit.all(), (op, axis, np.argwhere(~hit)[:4])
    single = can.sum(axis=axis) == 1
    want = ref_index(ref, axis, op)
    assert np.array_equal(got[single], want[single]), (op, axis, np.argwhere(single & (got != want))[:4])
    return float(np.mean(~single))


# ------------------------------------------------------------------------------------------------ the kernel in NumPy
def emulate(site, tables, op, index=False, skip=None, drop_col_idx=False, unpermuted=False, last=False, nan_wins=False,
            padding=False, col_perm0=None):
    """What the epilogue computes from the last product ``site`` (m x n, site order) through the planner's ``tables``
    (core/axisext.host_tables): every element goes to cell row_out[r] + col_out[c'], c' = position in the planner's
    column order.  The keywords model faults: ``skip`` = (rows, cols) slices never reduced, or "extreme"; ``drop_col_idx``;
    ``unpermuted`` = the columns stay in ``col_perm0`` order while the tables are permuted; ``last`` occurrence on
    ties; ``nan_wins``; ``padding`` = a zero reaches every cell."""
    s = _sign(op)
    perm = np.asarray(col_perm0 if unpermuted else tables.col_perm)
    v = s * site[:, perm]
    at = tables.row_out[:, None] + tables.col_out[None, :]
    take = np.ones(v.shape, dtype=bool) if nan_wins else ~np.isnan(v)
    if isinstance(skip, str):  # "extreme": the 64 x 64 tile that holds the extreme of the whole product
        r, c = np.unravel_index(np.nanargmax(v), v.shape)
        skip = (slice(r // TILE * TILE, r // TILE * TILE + TILE), slice(c // TILE * TILE, c // TILE * TILE + TILE))
    if skip is not None:
        take[skip] = False
    best = np.full(tables.out_numel, -np.inf)
    seen = np.zeros(tables.out_numel, dtype=bool)
    with np.errstate(invalid="ignore"):
        (np.maximum if nan_wins else np.fmax).at(best, at[take], v[take])
    seen[at[take]] = True
    if padding:
        best = np.maximum(best, 0.0)
        seen[:] = True
    values = np.where(seen, s * best, np.nan).reshape(tables.out_shape)
    if not index:
        return values
    idx = tables.row_idx[:, None].astype(np.int64) + (0 if drop_col_idx else tables.col_idx[None, :].astype(np.int64))
    idx = np.broadcast_to(idx, v.shape)
    match = take & (v == best[at])
    where = np.full(tables.out_numel, -1 if last else np.iinfo(np.int64).max, dtype=np.int64)
    (np.maximum if last else np.minimum).at(where, at[match], idx[match])
    where[where == np.iinfo(np.int64).max] = -1
    return where.reshape(tables.out_shape), values


# the order-preserving key of the kernel, in Python
def key_of(v, op="max", bits=32):
    """The unsigned key of ``v`` (0 for NaN): the bits with the sign bit set for v >= 0, all bits flipped for v < 0;
    complemented for the minimum."""
    ftype, utype = (np.float32, np.uint32) if bits == 32 else (np.float64, np.uint64)
    v = ftype(v)
    if np.isnan(v):
        return 0
    b = int((v + ftype(0)).view(utype))
    full, sign = (1 << bits) - 1, 1 << (bits - 1)
    b ^= full if b & sign else sign
    return full - b if op == "min" else b


def value_of(key, op="max", bits=32):
    ftype, utype = (np.float32, np.uint32) if bits == 32 else (np.float64, np.uint64)
    if key == 0:
        return ftype(np.nan)
    full, sign = (1 << bits) - 1, 1 << (bits - 1)
    if op == "min":
        key = full - key
    key ^= sign if key & sign else full
    return utype(key).view(ftype)


def packed_key(v, idx, op="max"):
    """fp32 with indices: the value key above the complemented index, so that the integer maximum prefers the larger
    value and then the smaller index."""
    k = key_of(v, op, 32)
    return (k << 32) | (0xFFFFFFFF - idx) if k else 0
