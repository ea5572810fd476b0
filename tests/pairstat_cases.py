"""Cases, references and bars of the statistics of TWO chains from the cores (csrc/pairstat.hip, core/pairstat.py).

Object a of a pair is the ``valstat_cases.Case`` of its chain (one chain, of more tiles than a launch has workgroups, is
this file's own); object b has the same dims, a second bond vector that
passes ``cc.check_chain`` and cores drawn under another name.  The references are the fp64 contractions of
``oracle.mps.mps_to_dense`` as volumes, the element bounds those of ``oracle.chain_bound``.  Nothing here touches a
GPU: tests/test_pairstat_cases_host.py runs the bars on the reference and on modelled faults,
tests/test_gpu_pairstat.py on what the kernels return.

Two bars, as in tests/valstat_cases.py.

* exact, on integer cores: every field of ``pair_stats`` and the whole joint histogram with ``outside`` and ``n_nan``
  equal NumPy's on the two references (``numpy.histogram2d``, whose last bin is closed on the right on either axis), bit
  for bit.  All sums are sums of integers below 2**53, exact in any order.
* sandwich, on real cores: a computed voxel lies within its bound of its reference.  For a pair of edges the computed
  2-D cumulative count C(e_a, e_b) (the cells left of both edges; nothing from ``outside``) lies between the number
  of voxels that are surely in range and surely left of both, #{ref + bound < e} on both axes, and the number that
  are possibly in range and possibly left of both, #{ref - bound < e}; the last edge of an axis is closed (<=).
  ``outside`` lies between the voxels that cannot and those that may be in range.  A sum of N terms in fp64 in any
  order is within N 2**-53 sum|term| of the exact sum of its terms (Higham 4.2); the terms are within bound (first
  moments), 2 |x| bound + bound**2 (squares), |a| bound_b + |b| bound_a + bound_a bound_b (products) and
  2 |a - b| (bound_a + bound_b) + (bound_a + bound_b)**2 (squared differences) of the reference's.
"""
from __future__ import annotations

import functools

import numpy as np

import valstat_cases as vc
from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle.mps import mps_to_dense

STORAGES = vc.STORAGES
NP_TYPE = vc.NP_TYPE
U64 = vc.U64
TILE = vc.TILE
K_TILE = {"f32": 16, "f64": 8}  # k-tile of the reducing product per element type

# name of a's chain -> the bonds of b.  What each is for (k: the bond at the last product, a against b):
REAL_PAIRS = {
    "L1": [1, 1],                                  # L == 1
    "L2_maxbond": [1, 5, 1],                       # L == 2; k 33 > 5
    "L4_tail_last": [1, 3, 13, 40, 1],             # a last-site-only tail; k 13 < 40: straddles 16 and 8, 32 and 40
    "L5_tail_last": [1, 4, 7, 7, 16, 1],           # k 33 > 16: straddles 32 / 16 in fp32 and 32 / 16 in fp64
    "L6_tail_all": [1, 1, 1, 1, 1, 1, 1],          # bonds of 1 on one side (k 3 against 1)
    "L4_no_tail": [1, 2, 4, 12, 1],                # m = 12 < 64 with n = 8192 (dims of int_no_tail); k 7 < 12
    "L5_ragged": [1, 5, 20, 9, 4, 1],              # m = 7 and n = 1320, neither a multiple of 64; k 7 > 5
    "L4_tail_4096": [1, 9, 40, 11, 1],             # a tail of exactly 4096; k 16 > 9
    "L5_mid_tail_65": [1, 5, 40, 20, 7, 1],        # m = 90, n = 1716: several ragged tiles both ways; k 65 > 40
}
INT_PAIRS = {
    "int_tail_all": [1, 3, 2, 5, 3, 1],            # 90
    "int_tail_last": [1, 5, 2, 1],                 # 10
    "int_no_tail": [1, 3, 2, 4, 1],                # 24
    "int_wide": [1, 4, 20, 6, 1],                  # 480
    "int_8x7": [1, 4, 8, 8, 8, 8, 4, 1],           # 65536; 2**21 voxels in 512 tiles
    "int_many_tiles": [1, 2, 1],                   # 2; equal k: other cores only
}
# a chain of this file's own: m = 2 and n = 40010 make 626 tiles (the last ragged) of 80020 voxels, so that in every
# launch (512 workgroups at most) a persistent workgroup takes tile t and tile t + 512
EXTRA_CHAINS = {"int_many_tiles": ([2, 40010], [1, 2, 1])}
CHAINS = dict(vc.ALL_CHAINS, **EXTRA_CHAINS)
REAL_NAMES, INT_NAMES = sorted(REAL_PAIRS), sorted(INT_PAIRS)
RAW = ("sum_a", "sum_b", "sumsq_a", "sumsq_b", "sum_ab", "sse", "max_abs_diff", "min_a", "max_a", "min_b", "max_b")


def last_k(dims, bonds):
    """k of the chain's last product: the bond in front of the tail, or of the last site without one; 1 for L == 1."""
    if len(dims) == 1:
        return 1
    j0 = cc.tail_start(dims)
    return int(bonds[j0 if j0 < len(dims) else len(dims) - 1])


def _case(name, dims, bonds, family, storage):
    """A ``valstat_cases.Case`` of any (dims, bonds), built as its constructor builds one of its own table: object b of
    a pair (a's dims, a second bond vector, cores drawn under another name), and both objects of EXTRA_CHAINS."""
    c = vc.Case.__new__(vc.Case)
    c.name, c.family, c.storage = name, family, storage
    c.dims, c.bonds = list(dims), list(bonds)
    cc.check_chain(c.dims, c.bonds)
    c.cores = cc.draw_cores(name, c.dims, c.bonds, family, storage)
    c.fa = cc.factor_array(c.dims)
    c.shape = tuple(int(v) for v in np.prod(c.fa, axis=0))
    c.dest = cb.flat_destination_factors(c.fa).reshape(-1)
    c.site = mps_to_dense(c.cores).reshape(-1)
    c.ref = cb.to_volume(c.site, c.dest)
    if family == "integer":
        c.bound = np.zeros_like(c.ref)
    else:
        c.bound = cb.to_volume(cb.chain_bound(c.cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), c.dest)
    c.n = c.ref.size
    c.identity = bool(np.array_equal(c.dest, np.arange(c.n)))
    return c


class Pair:
    """Two chains of one shape: ``a`` and ``b`` (valstat_cases.Case each), and the k of their last products."""

    def __init__(self, name, family, storage):
        self.name, self.family, self.storage = name, family, storage
        self.a = vc.Case(name, family, storage) if name in vc.ALL_CHAINS else _case(name, *EXTRA_CHAINS[name], family, storage)
        self.b = _case(name + "/b", self.a.dims, (INT_PAIRS if family == "integer" else REAL_PAIRS)[name], family, storage)
        self.dims, self.n = self.a.dims, self.a.n
        self.k_a, self.k_b = last_k(self.dims, self.a.bonds), last_k(self.dims, self.b.bonds)
        self.m, self.cols = vc.last_product_shape(self.dims)

    def volumes(self, site_a, site_b):
        """Two site-order arrays of the last product's m x n elements as volumes."""
        return cb.to_volume(site_a, self.a.dest), cb.to_volume(site_b, self.a.dest)


@functools.lru_cache(maxsize=2)
def pair(name, family, storage):
    return Pair(name, family, storage)


# ------------------------------------------------------------------------------------------------ what NumPy says
def ref_pair_stats(ra, rb):
    with np.errstate(invalid="ignore"):
        ok = ~(np.isnan(ra) | np.isnan(rb))
        a, b = ra[ok], rb[ok]
        d = a - b
        return dict(count=int(a.size), n_nan=int(ra.size - a.size), sum_a=float(a.sum()), sum_b=float(b.sum()),
                    sumsq_a=float((a * a).sum()), sumsq_b=float((b * b).sum()), sum_ab=float((a * b).sum()),
                    sse=float((d * d).sum()), max_abs_diff=float(np.abs(d).max()), min_a=float(a.min()), max_a=float(a.max()),
                    min_b=float(b.min()), max_b=float(b.max()))


def ref_joint(ra, rb, ea, eb):
    """(counts (bins_a, bins_b), outside, n_nan): numpy.histogram2d over the voxels where neither value is NaN (it
    closes the last bin of either axis on the right and drops what lies outside)."""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    ok = ~(np.isnan(ra) | np.isnan(rb))
    a, b = ra[ok], rb[ok]
    counts = np.histogram2d(a, b, bins=(ea, eb))[0].astype(np.int64)
    inside = (a >= ea[0]) & (a <= ea[-1]) & (b >= eb[0]) & (b <= eb[-1])
    return counts, int(a.size - inside.sum()), int(ra.size - a.size)


def axis_edges(ref, np_type, placement, bins):
    """Edges in the element type for one axis of a reference of integers: the placements of
    ``valstat_cases.integer_edge_sets`` with at most ``bins`` bins."""
    ok = ref[~np.isnan(ref)]
    lo, hi = int(ok.min()), int(ok.max())
    step = -(-(hi - lo + 1) // bins)
    nb = -(-(hi - lo + 1) // step)
    q = max((hi - lo) // 4, 1)
    e = {
        "half_integers": lambda: lo - 0.5 + step * np.arange(nb + 1),
        "on_integers": lambda: lo + step * np.arange(nb + 1),             # the left-closed rule at interior edges
        "last_edge_is_max": lambda: np.unique(np.concatenate([np.arange(lo, hi, step), [hi]])),  # the closed last bin
        "one_bin": lambda: np.array([lo, hi]),
        "one_bin_inside": lambda: np.array([lo + q, max(hi - q, lo + q)]),
        "linspace": lambda: np.linspace(lo - 0.5, hi + 0.5, bins + 1),
        "range_excludes": lambda: np.linspace(lo + q, max(hi - q, lo + q + 1), bins + 1),  # voxels below and above
    }[placement]()
    return np.asarray(e, dtype=np.float64).astype(np_type)


# name -> ((placement, bins) of a, (placement, bins) of b)
INTEGER_EDGE_PAIRS = {
    "1x1": (("one_bin", 1), ("one_bin", 1)),
    "1x1024": (("one_bin_inside", 1), ("linspace", 1024)),
    "1024x16": (("linspace", 1024), ("range_excludes", 16)),
    "128x128": (("half_integers", 128), ("on_integers", 128)),
    "last_edges": (("last_edge_is_max", 64), ("last_edge_is_max", 32)),
}


def integer_edge_pairs(ra, rb, np_type):
    return {name: (axis_edges(ra, np_type, *pa), axis_edges(rb, np_type, *pb)) for name, (pa, pb) in INTEGER_EDGE_PAIRS.items()}


# ------------------------------------------------------------------------------------------------ the exact bar
def exact_pair_stats(got, ra, rb):
    want = ref_pair_stats(ra, rb)
    for key in ("count", "n_nan") + RAW:
        assert got[key] == want[key], (key, got[key], want[key])


def exact_joint(counts, outside, nan, ra, rb, ea, eb):
    want, want_outside, want_nan = ref_joint(ra, rb, ea, eb)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape == want.shape, (counts.shape, want.shape)
    assert int(counts.sum()) + outside + nan == ra.size, "cells and outliers do not sum to the voxel count"
    assert (outside, nan) == (want_outside, want_nan), ((outside, nan), (want_outside, want_nan))
    assert np.array_equal(counts, want), np.argwhere(counts != want)[:8]


# ------------------------------------------------------------------------------------------------ the sandwich bar
def sandwich_pair_stats(got, ra, ba, rb, bb):
    n = ra.size
    assert got["count"] == n and got["n_nan"] == 0, (got["count"], got["n_nan"])
    for key, ref, bound in (("a", ra, ba), ("b", rb, bb)):
        assert (ref - bound).min() <= got["min_" + key] <= (ref + bound).min(), ("min_" + key, got["min_" + key])
        assert (ref - bound).max() <= got["max_" + key] <= (ref + bound).max(), ("max_" + key, got["max_" + key])
        slack = bound.sum() + n * U64 * np.abs(ref).sum()
        assert abs(got["sum_" + key] - ref.sum()) <= slack, ("sum_" + key, got["sum_" + key], ref.sum(), slack)
        sq = ref * ref
        slack = (2 * np.abs(ref) * bound + bound * bound).sum() + (n + 2) * U64 * sq.sum()
        assert abs(got["sumsq_" + key] - sq.sum()) <= slack, ("sumsq_" + key, got["sumsq_" + key], sq.sum(), slack)
    prod = ra * rb
    slack = (np.abs(ra) * bb + np.abs(rb) * ba + ba * bb).sum() + (n + 2) * U64 * np.abs(prod).sum()
    assert abs(got["sum_ab"] - prod.sum()) <= slack, ("sum_ab", got["sum_ab"], prod.sum(), slack)
    d, bd = ra - rb, ba + bb
    sq = d * d
    # the difference and its square are formed in fp64 from the computed voxels: two roundings per term beside the sum's
    slack = (2 * np.abs(d) * bd + bd * bd).sum() + (n + 4) * U64 * (sq.sum() + (2 * np.abs(d) * bd + bd * bd).sum())
    assert abs(got["sse"] - sq.sum()) <= slack, ("sse", got["sse"], sq.sum(), slack)
    assert abs(got["max_abs_diff"] - np.abs(d).max()) <= bd.max() * (1 + 4 * U64), ("max_abs_diff", got["max_abs_diff"])


def _first_edge_above(values, edges):
    """Per value the smallest i with value < edges[i] (value <= edges[-1] for the last: the closed bin); len(edges) for
    a value above the range."""
    i = np.searchsorted(edges, values, side="right")
    i[values == edges[-1]] = edges.size - 1
    return i


def _cumulative(ia, ib, na, nb):
    """C[i, j] = #{ia <= i and ib <= j} for i < na, j < nb."""
    keep = (ia < na) & (ib < nb)
    table = np.bincount(ia[keep] * nb + ib[keep], minlength=na * nb).reshape(na, nb)
    return table.cumsum(axis=0).cumsum(axis=1)


def sandwich_joint(counts, outside, nan, ra, ba, rb, bb, ea, eb):
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    n = ra.size
    assert counts.shape == (ea.size - 1, eb.size - 1)
    assert int(counts.sum()) + outside + nan == n, "cells and outliers do not sum to the voxel count"
    assert nan == 0
    surely = (ra - ba >= ea[0]) & (ra + ba <= ea[-1]) & (rb - bb >= eb[0]) & (rb + bb <= eb[-1])
    maybe = (ra + ba >= ea[0]) & (ra - ba <= ea[-1]) & (rb + bb >= eb[0]) & (rb - bb <= eb[-1])
    assert n - int(maybe.sum()) <= outside <= n - int(surely.sum()), (outside, n - int(maybe.sum()), n - int(surely.sum()))
    got = np.zeros((ea.size, eb.size), dtype=np.int64)  # C(e_a, e_b) for every pair of edges
    got[1:, 1:] = counts.cumsum(axis=0).cumsum(axis=1)
    least = _cumulative(_first_edge_above((ra + ba)[surely], ea), _first_edge_above((rb + bb)[surely], eb), ea.size, eb.size)
    most = _cumulative(_first_edge_above(np.maximum((ra - ba)[maybe], ea[0]), ea),
                       _first_edge_above(np.maximum((rb - bb)[maybe], eb[0]), eb), ea.size, eb.size)
    bad = (got < least) | (got > most)
    assert not bad.any(), (np.argwhere(bad)[:8], got[bad][:8], least[bad][:8], most[bad][:8])


# ------------------------------------------------------------------------------------------------ modelled faults
# What a faulty kernel would see, computed from the cores: the two volumes it would reduce (or the table it would
# report).  The bars must reject each of them on at least one case.
def _matrix(p, c):
    return c.site.reshape(p.m, p.cols)


def _truncated(c, bond, k):
    """The site-order tensor of ``c`` with its bond ``bond`` cut to the first ``k`` indices."""
    cores = [x.copy() for x in c.cores]
    cores[bond - 1] = cores[bond - 1][:, :, :k]
    cores[bond] = cores[bond][:k]
    return mps_to_dense(cores).reshape(-1)


def fault_wrong_k(p):
    """The chain with the larger k at the last product contracted with the other's k (its bond cut to it): the two
    volumes, or None for equal k or a single site."""
    if p.k_a == p.k_b or len(p.dims) == 1:
        return None
    j0 = cc.tail_start(p.dims)
    bond = j0 if j0 < len(p.dims) else len(p.dims) - 1
    if p.k_a < p.k_b:
        return p.volumes(p.a.site, _truncated(p.b, bond, p.k_a))
    return p.volumes(_truncated(p.a, bond, p.k_b), p.b.site)


def fault_swapped(p):
    """The two accumulators swapped: a transposed histogram, the _a and _b fields exchanged."""
    return p.b.ref, p.a.ref


def fault_b_tile_shifted(p):
    """b's tile taken from tile t + 1 (64 x 64 tiles in the kernel's order; the last takes zeros)."""
    T = 2 * TILE
    tm, tn = -(-p.m // T), -(-p.cols // T)
    full = np.zeros((tm * T, tn * T))
    full[:p.m, :p.cols] = _matrix(p, p.b)
    tiles = full.reshape(tm, T, tn, T).transpose(0, 2, 1, 3).reshape(tm * tn, T, T)
    tiles = np.concatenate([tiles[1:], np.zeros((1, T, T))])
    moved = tiles.reshape(tm, tn, T, T).transpose(0, 2, 1, 3).reshape(tm * T, tn * T)[:p.m, :p.cols]
    return p.volumes(p.a.site, moved.reshape(-1))


def fault_padding_counted(p):
    """Both volumes with a zero for every padded element of the 32 x 32 tiles; None without padding."""
    pm, pn = -(-p.m // TILE) * TILE, -(-p.cols // TILE) * TILE
    if pm * pn == p.n:
        return None
    pad = np.zeros(pm * pn - p.n)
    return np.concatenate([p.a.ref, pad]), np.concatenate([p.b.ref, pad])


def fault_tile_left_out(p):
    """Both volumes without the first 32 x 32 tile of the last product."""
    keep = np.ones((p.m, p.cols), dtype=bool)
    keep[:TILE, :TILE] = False
    return _matrix(p, p.a)[keep], _matrix(p, p.b)[keep]


def fault_nan_of_b_ignored(ra, rb_nan, ea, eb):
    """The report of a kernel that looks for NaN in a only: the voxels where only b is NaN are not in n_nan and, in no
    bin of b, land in outside.  None without such voxels."""
    counts, outside, nan = ref_joint(ra, rb_nan, ea, eb)
    only_b = int((np.isnan(rb_nan) & ~np.isnan(ra)).sum())
    return (counts, outside + only_b, nan - only_b) if only_b else None


def fault_outside_on_a_alone(ra, rb, ea, eb):
    """The report of a kernel that decides ``outside`` on a alone: b is clamped into its first or last bin.  None where
    no voxel has a in range and b out of range."""
    eb64 = np.asarray(eb, dtype=np.float64)
    clamped = np.clip(rb, eb64[0], eb64[-1])
    if np.array_equal(clamped, rb):
        return None
    got = ref_joint(ra, clamped, ea, eb)
    return None if got[1] == ref_joint(ra, rb, ea, eb)[1] else got


def fault_last_bin_open_on_b(ra, rb, ea, eb):
    """Voxels whose b equals b's last edge (a in range) land in outside; None when there are none."""
    ea64, eb64 = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    counts, outside, nan = ref_joint(ra, rb, ea, eb)
    hit = (rb == eb64[-1]) & (ra >= ea64[0]) & (ra <= ea64[-1])
    if not hit.any():
        return None
    moved = np.histogram2d(ra[hit], rb[hit], bins=(ea64, eb64))[0].astype(np.int64)
    return counts - moved, outside + int(hit.sum()), nan
