"""Cases, references and bars of the voxels selected by value from the cores (csrc/select.hip, core/select.py).

Nothing here touches a GPU: tests/test_select_cases_host.py runs the bars on the reference and on modelled faults,
tests/test_gpu_select.py on what the kernel returns.

Integer chains.  Those of tests/axisext_cases.py on their three-axis volumes (``IntCase``, ``with_nan()``, the split
tables), and one of this file, ``int_wrap``: eleven sites of dim 4, bonds capped at 4, cores from {-1, 0, 1} (a voxel
is an integer of magnitude at most 4**10, exact in fp32).  Its last product is 1024 x 4096, which is 1024 tiles of
64 x 64: more than the 512 workgroups of the persistent grid, so a workgroup walks several tiles.

Two bars.

* exact, on integer cores: indices and values equal NumPy's on the fp64 reference, element for element.
* sandwich, on the real cores of ``valstat_cases.REAL_CASES``: a computed voxel lies within ``bound`` of its
  reference, so a voxel whose whole interval ``[ref - bound, ref + bound]`` lies inside ``[lo, hi]`` must be returned,
  one whose interval lies wholly outside must not be, and a returned value lies within ``bound`` of the reference at
  its index.  The voxels in neither set are ambiguous.  The intervals come from the reference: its 99th percentile
  upward, and the band from its 40th to its 60th percentile.  ``real_case`` asserts, from the reference and the bound
  alone, that the ambiguous voxels are at most 10 % of the certainly selected ones; ``REAL_CASES`` are the cases of
  ``valstat_cases`` that meet this in both storages, ``DROPPED`` the others.

Both bars require int64 indices that ascend strictly, which a duplicated slot and an unsorted result break.
"""
from __future__ import annotations

import functools

import numpy as np

import axisext_cases as ac
import valstat_cases as vc
from oracle import chain_bound as cb
from oracle import chain_cases as cc

MAX_AMBIGUOUS = 0.10
TILE = 64          # the tile of one workgroup in the reducing product
MAX_GROUPS = 512   # workgroups of the persistent grid

INT_NAMES = ac.SIGNED_NAMES + ("int_wrap",)
SMALL_INT_NAMES = tuple(n for n in ac.SIGNED_NAMES if n != "int_8x7")  # volumes of a few thousand voxels

WRAP_DIMS, WRAP_BONDS = [4] * 11, [1] + [4] * 10 + [1]
WRAP_FACTORS = [[2, 2, 1], [1, 2, 2], [2, 1, 2], [4, 1, 1], [1, 4, 1], [1, 1, 4], [2, 2, 1], [1, 2, 2], [2, 1, 2], [2, 2, 1],
                [1, 2, 2]]

# every case of valstat_cases meets the cap in both storages (the largest share, 0.084, is the band of the chain with
# bonds of 129 in fp32); a case that did not would be listed here and left out
DROPPED = ()
REAL_CASES = [c for c in vc.REAL_CASES if c not in DROPPED]
REAL_IDS = [f"{n}-{f}" for n, f in REAL_CASES]


class WrapCase(ac.IntCase):
    """``int_wrap`` with the fields of an ``IntCase``."""

    def __init__(self, storage):
        self.name, self.storage = "int_wrap", storage
        self.dims, self.bonds = WRAP_DIMS, WRAP_BONDS
        cc.check_chain(self.dims, self.bonds)
        self.cores = cc.draw_cores(self.name, self.dims, self.bonds, "integer", storage)
        self.fa = np.array(WRAP_FACTORS, dtype=np.int64)
        assert [int(v) for v in np.prod(self.fa, axis=1)] == list(self.dims)
        self.shape = tuple(int(v) for v in np.prod(self.fa, axis=0))
        self.dest = cb.flat_destination_factors(self.fa)
        self.m, self.n = vc.last_product_shape(self.dims)
        self.tiles = -(-self.m // TILE) * -(-self.n // TILE)
        assert self.tiles > MAX_GROUPS, (self.m, self.n, self.tiles)
        self.tables = ac.split_tables(self.dest, self.n)
        self.set_cores(self.cores)


@functools.lru_cache(maxsize=2)
def int_case(name, storage):
    return WrapCase(storage) if name == "int_wrap" else ac.int_case(name, storage)


def int_intervals(ref):
    """name -> (lo, hi, invert) for a reference of integers: ends that equal voxel values, so both ends are closed."""
    vals = np.unique(ref[~np.isnan(ref)])
    q1, q3, top = float(vals[vals.size // 4]), float(vals[(3 * vals.size) // 4]), float(vals[-1])
    return {"closed_ends": (q1, q3, False), "empty": (top + 1, top + 2, False), "everything": (None, None, False),
            "max_only": (top, top, False), "invert": (q1, q3, True), "half_line": (q3, None, False)}


class RealCase(ac.RealCase):
    """A real case with its two intervals, in the element type."""

    def __init__(self, name, family, storage):
        super().__init__(name, family, storage)
        np_type = vc.NP_TYPE[storage]
        p40, p60, p99 = (np_type(v) for v in np.percentile(self.ref, [40, 60, 99]))
        self.intervals = {"top": (p99, None), "band": (p40, p60)}


def real_case_unchecked(name, family, storage):
    return RealCase(name, family, storage)


@functools.lru_cache(maxsize=2)
def real_case(name, family, storage):
    c = RealCase(name, family, storage)
    for key, (lo, hi) in c.intervals.items():
        share = ambiguous_share(c.ref, c.bound, lo, hi)
        assert share <= MAX_AMBIGUOUS, f"{name}/{family}/{storage} {key}: {share:.3f} ambiguous per certain voxel"
    return c


# ------------------------------------------------------------------------------------------------ what NumPy says
def _ends(lo, hi):
    return (-np.inf if lo is None else float(lo)), (np.inf if hi is None else float(hi))


def _inside(flat, lo, hi):
    lo, hi = _ends(lo, hi)
    with np.errstate(invalid="ignore"):
        return (flat >= lo) & (flat <= hi)


def ref_count(ref, lo=None, hi=None, invert=False):
    flat = np.asarray(ref, dtype=np.float64).reshape(-1)
    inside = _inside(flat, lo, hi)
    return int((~inside & ~np.isnan(flat)).sum() if invert else inside.sum())


def ref_find(ref, lo=None, hi=None, invert=False):
    """(flat C-order indices ascending, fp64 values) of the non-NaN voxels inside (``invert``: outside) [lo, hi]."""
    flat = np.asarray(ref, dtype=np.float64).reshape(-1)
    inside = _inside(flat, lo, hi)
    index = np.flatnonzero(~inside & ~np.isnan(flat) if invert else inside).astype(np.int64)
    return index, flat[index]


def ref_find_nan(ref):
    return np.flatnonzero(np.isnan(np.asarray(ref).reshape(-1))).astype(np.int64)


def ref_topk(ref, k, largest=True):
    """The k largest (smallest) non-NaN voxels by value, equal values by ascending index: ``np.lexsort``."""
    flat = np.asarray(ref, dtype=np.float64).reshape(-1)
    ok = np.flatnonzero(~np.isnan(flat))
    v = flat[ok]
    order = np.lexsort((ok, -v if largest else v))[:k]
    return ok[order].astype(np.int64), v[order]


# ------------------------------------------------------------------------------------------------ the bars
def _well_formed(index, values, np_type, ascending=True):
    index, values = np.asarray(index), np.asarray(values)
    assert index.dtype == np.int64 and index.ndim == 1, (index.dtype, index.shape)
    assert values.shape == index.shape, (values.shape, index.shape)
    assert np_type is None or values.dtype == np_type, (values.dtype, np_type)
    if ascending:
        assert np.all(np.diff(index) > 0), "the indices do not ascend strictly"
    return index, values


def exact_find(index, values, ref, lo=None, hi=None, invert=False, np_type=None):
    index, values = _well_formed(index, values, np_type)
    want_index, want_values = ref_find(ref, lo, hi, invert)
    assert index.size == want_index.size, (index.size, want_index.size)
    assert np.array_equal(index, want_index), np.flatnonzero(index != want_index)[:8]
    assert np.array_equal(values.astype(np.float64), want_values), np.flatnonzero(values != want_values)[:8]


def exact_nan(index, ref):
    index = np.asarray(index)
    assert index.dtype == np.int64 and np.array_equal(index, ref_find_nan(ref)), (index[:8], ref_find_nan(ref)[:8])


def exact_topk(index, values, ref, k, largest=True, np_type=None):
    index, values = _well_formed(index, values, np_type, ascending=False)
    want_index, want_values = ref_topk(ref, k, largest)
    assert np.array_equal(index, want_index), (index[:8], want_index[:8])
    assert np.array_equal(values.astype(np.float64), want_values), (values[:8], want_values[:8])


def certain(ref, bound, lo=None, hi=None):
    """(certainly inside, certainly outside) of [lo, hi], boolean over the flat volume."""
    lo, hi = _ends(lo, hi)
    r, b = np.asarray(ref, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    return (r - b >= lo) & (r + b <= hi), (r + b < lo) | (r - b > hi)


def ambiguous_share(ref, bound, lo=None, hi=None):
    """Ambiguous voxels per certainly selected voxel."""
    must, must_not = certain(ref, bound, lo, hi)
    return float((~must & ~must_not).sum()) / max(int(must.sum()), 1)


def sandwich_find(index, values, ref, bound, lo=None, hi=None, np_type=None):
    """Returns the number of ambiguous voxels among the returned ones."""
    index, values = _well_formed(index, values, np_type)
    r, b = np.asarray(ref, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    assert index.size == 0 or (index[0] >= 0 and index[-1] < r.size), "an index outside the volume"
    must, must_not = certain(ref, bound, lo, hi)
    got = np.zeros(r.size, dtype=bool)
    got[index] = True
    assert not (must & ~got).any(), ("left out", np.flatnonzero(must & ~got)[:8])
    assert not (must_not & got).any(), ("wrongly selected", np.flatnonzero(must_not & got)[:8])
    off = np.abs(values.astype(np.float64) - r[index]) > b[index]
    assert not off.any(), ("a value beyond its bound", index[off][:8])
    return int((got & ~must).sum())


# ------------------------------------------------------------------------------------------------ the kernel in NumPy
def emulate(c, lo=None, hi=None, invert=False, nan=False, skip=None, padding=False, open_right=False, site_order=False,
            nan_by_invert=False, duplicate=False, unsorted=False):
    """What the list pass and the sort return from the last product ``c.site`` (m x n, site order) through the split
    tables of the case: (index, fp64 values).  The keywords model faults: ``skip`` = (rows, cols) slices never reduced;
    ``padding`` = the padded rows and columns of the 64 x 64 tiles are zeros taken as data (at the place of the last
    row or column); ``open_right`` = v < hi; ``site_order`` = the index is the site-order address; ``nan_by_invert`` =
    the outside predicate is the negation of the inside one; ``duplicate`` = two matches share a slot, so the second
    slot keeps what the first holds; ``unsorted`` = the first two pairs are left in the order of arrival."""
    row_off, col_off, perm = c.tables
    v = c.site[:, perm]
    at = row_off[:, None] + col_off[None, :]
    if site_order:
        at = np.arange(c.m, dtype=np.int64)[:, None] * c.n + np.asarray(perm, dtype=np.int64)[None, :]
    if padding:
        pm, pn = -(-c.m // TILE) * TILE, -(-c.n // TILE) * TILE
        rows, cols = np.minimum(np.arange(pm), c.m - 1), np.minimum(np.arange(pn), c.n - 1)
        real = (np.arange(pm) < c.m)[:, None] & (np.arange(pn) < c.n)[None, :]
        v, at = np.where(real, v[np.ix_(rows, cols)], 0.0), at[np.ix_(rows, cols)]
    a, b = _ends(lo, hi)
    with np.errstate(invalid="ignore"):
        inside = (v >= a) & ((v < b) if open_right else (v <= b))
    if nan:
        match = np.isnan(v)
    elif invert:
        match = ~inside if nan_by_invert else (~inside & ~np.isnan(v))
    else:
        match = inside
    if skip is not None:
        match = match.copy()
        match[skip] = False
    index, values = at[match].astype(np.int64), v[match]
    order = np.argsort(index, kind="stable")
    index, values = index[order], values[order]
    if duplicate and index.size > 1:
        index[1], values[1] = index[0], values[0]
    if unsorted and index.size > 1:
        index[[0, 1]], values[[0, 1]] = index[[1, 0]], values[[1, 0]]
    return index, values


# ------------------------------------------------------------------------------------------------ topk's backend in NumPy
class NumpyBackend:
    """``core.select.topk_select``'s backend on a flat array in the element type; it counts its passes and checks the
    counts ``topk_select`` hands to ``find``."""

    def __init__(self, flat, max_count):
        self.v = np.asarray(flat).reshape(-1)
        self.max_count = max_count
        self.calls = {"moments": 0, "count": 0, "bin_counts": 0, "find": 0}
        self.widest = 0

    def moments(self):
        self.calls["moments"] += 1
        ok = self.v[~np.isnan(self.v)]
        return dict(count=int(self.v.size), n_nan=int(self.v.size - ok.size), min=float(ok.min()) if ok.size else np.inf,
                    max=float(ok.max()) if ok.size else -np.inf)

    def count(self, lo, hi):
        self.calls["count"] += 1
        return ref_count(self.v, lo, hi)

    def bin_counts(self, edges):
        self.calls["bin_counts"] += 1
        assert edges.dtype == self.v.dtype and 2 <= edges.size <= 4097 and np.all(np.diff(edges) > 0)
        counts, (below, above, nan) = vc.ref_histogram(self.v.astype(np.float64), edges)
        return counts, below, above, nan

    def find(self, lo, hi, count):
        self.calls["find"] += 1
        index, _ = ref_find(self.v, lo, hi) if lo <= hi else (np.zeros(0, dtype=np.int64), None)
        assert index.size == count, ("topk_select's count is not the selection's", index.size, count)
        assert count <= self.max_count, ("a find beyond max_count", count, self.max_count)
        self.widest = max(self.widest, count)
        return index, self.v[index]

    def best(self, index, values, k, largest):
        order = np.lexsort((index, -values.astype(np.float64) if largest else values.astype(np.float64)))[:k]
        return index[order], values[order]

    def concat(self, pairs):
        return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
