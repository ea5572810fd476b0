"""Cases, references and bars of the value statistics from the cores (csrc/valstat.hip, core/valstat.py).

Chains and cores come from oracle/chain_cases.py, the reference is ``oracle.mps.mps_to_dense`` in fp64 mapped onto the
two-axis volume of ``cc.factor_array`` as tests/test_gpu_decode_reference.py maps it, the element bound is
``oracle.chain_bound.chain_bound`` with ``CHAIN_ROUNDOFF``.  Nothing here touches a GPU: tests/test_valstat_host.py
runs the bars on the reference and on modelled faults, tests/test_gpu_valstat.py on what the kernels return.

Two bars.

* exact, on integer cores ({-1, 0, 1}; every partial product is an integer below 2**24): what the kernels return must
  equal what NumPy computes from the fp64 reference, bit for bit.
* sandwich, on real cores: a computed voxel lies within ``bound`` of its reference, so for an edge e the computed
  cumulative count C(e) = n_below + the bins left of e obeys  #{ref + bound < e} <= C(e) <= #{ref - bound < e}.  The
  last bin is closed on the right, so C(last edge) counts v <= e and is compared with ``<=`` on both sides.
  Extremes lie between the extremes of ref -/+ bound; a sum of N terms accumulated in fp64 in any order is within
  N 2**-53 sum|term| of the exact sum of its terms (Higham 4.2), and the terms are within ``bound`` (first moments)
  or 2 |x| bound + bound**2 (squares) of the reference's.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle.mps import mps_to_dense

NP_TYPE = {"f32": np.float32, "f64": np.float64}
STORAGES = ("f32", "f64")
U64 = 2.0 ** -53

# the integer chains, and one with 2**21 voxels whose bond product 4 194 304 is still below 2**24
INT_EXTRA = {"int_8x7": ([8] * 7, [1, 8, 16, 16, 16, 16, 8, 1])}
INT_CHAINS = dict(cc.INTEGER_CHAINS, **INT_EXTRA)
REAL_CASES = [(n, "uniform") for n in cc.CHAINS if n != "L4_large"] + [(n, "graded") for n in cc.GRADED]
REAL_IDS = [f"{n}-{f}" for n, f in REAL_CASES]
ALL_CHAINS = dict(cc.CHAINS, **INT_CHAINS)

TILE = 32  # the accumulator tile of one wavefront in the reducing product


def last_product_shape(dims):
    """(rows, columns) of the chain's last product: columns are the tail's, or the last site's without a tail."""
    j0 = cc.tail_start(dims)
    n = int(np.prod(dims[j0:], dtype=np.int64)) if j0 < len(dims) else int(dims[-1])
    return int(np.prod(dims, dtype=np.int64)) // n, n


class Case:
    """One chain with its cores, its fp64 reference in site order and as the volume, and the element bound."""

    def __init__(self, name, family, storage):
        self.name, self.family, self.storage = name, family, storage
        self.dims, self.bonds = ALL_CHAINS[name]
        cc.check_chain(self.dims, self.bonds)
        self.cores = cc.draw_cores(name, self.dims, self.bonds, family, storage)
        self.fa = cc.factor_array(self.dims)
        self.shape = tuple(int(v) for v in np.prod(self.fa, axis=0))
        self.dest = cb.flat_destination_factors(self.fa).reshape(-1)
        self.site = mps_to_dense(self.cores).reshape(-1)
        self.ref = cb.to_volume(self.site, self.dest)  # flat, C order of the volume
        if family == "integer":
            self.bound = np.zeros_like(self.ref)
        else:
            self.bound = cb.to_volume(cb.chain_bound(self.cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), self.dest)
        self.n = self.ref.size
        self.identity = bool(np.array_equal(self.dest, np.arange(self.n)))

    def edges64(self):
        """Uniform bins over the reference's range, in the element type (the sandwich cases' edges): 64 of them, or, where
        more than 1 % of the voxels would lie within their bound of an edge (fp32 chains whose bound is a sizeable part
        of a bin: bonds of 129), the largest halving of 64 that meets the condition.  The smallest and the largest
        voxel sit on the outer edges; where those two alone are more than 1 % of the voxels (a chain of fewer than
        200) the range is widened by half a bin on either side.  Decided from the reference and the bound alone.  The
        chain of bond 129 is left with 4 bins in fp32 (its bound is a tenth of one of 64 bins); the same chain in fp64
        and the exact cases of 4096 bins carry the histogram there."""
        lo, hi = float(self.ref.min()), float(self.ref.max())
        bins = 64
        while True:
            pad = (hi - lo) / (2 * bins) if 2 > 0.01 * self.n else 0.0
            edges = np.linspace(lo - pad, hi + pad, bins + 1).astype(NP_TYPE[self.storage])
            if near_edge_fraction(self.ref, self.bound, edges) <= 0.01:
                return edges
            if bins == 4:
                raise AssertionError(f"{self.name}/{self.storage}: no halving of 64 bins down to 4 meets the 1 % condition")
            bins //= 2

    def original(self):
        """An original for error_to in the element type: the reference moved by 1 % of its rms, or, on integer cores,
        by planted integer offsets at a few voxels, the first and the last in C order among them."""
        if self.family == "integer":
            y = self.ref.copy()
            where = sorted({0, 1, self.n // 3, self.n // 2 + 1, self.n - 2, self.n - 1} & set(range(self.n)))
            y[where] += np.array([3, -7, 11, -2, 5, -13][:len(where)], dtype=np.float64)
            return y
        rng = np.random.default_rng(len(self.name) + self.n)
        rms = float(np.sqrt(np.mean(self.ref ** 2)))
        return cc.to_storage(self.ref + 0.01 * rms * rng.standard_normal(self.n), self.storage)


@functools.lru_cache(maxsize=2)
def case(name, family, storage):
    return Case(name, family, storage)


# ------------------------------------------------------------------------------------------------ what NumPy says
def ref_moments(ref):
    ok = ref[~np.isnan(ref)]
    return dict(count=int(ref.size), n_nan=int(ref.size - ok.size), min=float(ok.min()), max=float(ok.max()),
                sum=float(ok.sum()), sumsq=float((ok * ok).sum()))


def ref_histogram(ref, edges):
    """(counts, (n_below, n_above, n_nan)) of numpy.histogram over the finite voxels."""
    edges = np.asarray(edges, dtype=np.float64)
    ok = ref[~np.isnan(ref)]
    counts = np.histogram(ok, bins=edges)[0].astype(np.int64)
    return counts, (int((ok < edges[0]).sum()), int((ok > edges[-1]).sum()), int(ref.size - ok.size))


def ref_error(ref, y):
    d = ref - y
    return dict(sse=float((d * d).sum()), max_abs=float(np.abs(d).max()), ref_sumsq=float((y * y).sum()),
                ref_max=float(y.max()))


def integer_edge_sets(ref, np_type):
    """name -> edges in the element type, for a reference of integers: the placements of the exact bar."""
    ok = ref[~np.isnan(ref)]
    lo, hi = int(ok.min()), int(ok.max())
    step = -(-(hi - lo + 1) // 4096)
    nb = -(-(hi - lo + 1) // step)
    q = max((hi - lo) // 4, 1)
    sets = {
        "half_integers": lo - 0.5 + step * np.arange(nb + 1),
        "on_integers": lo + step * np.arange(nb + 1),            # the left-closed rule at interior edges
        "last_edge_is_max": np.unique(np.concatenate([np.arange(lo, hi, step), [hi]])),  # the closed last bin
        "one_bin": np.array([lo, hi]),
        "one_bin_inside": np.array([lo + q, max(hi - q, lo + q)]),
        "bins_4096": np.linspace(lo - 0.5, hi + 0.5, 4097),
        "range_excludes": np.linspace(lo + q, max(hi - q, lo + q + 1), 17),  # voxels below and above the range
    }
    return {k: np.asarray(v, dtype=np.float64).astype(np_type) for k, v in sets.items()}


# ------------------------------------------------------------------------------------------------ the exact bar
def exact_moments(got, ref):
    want = ref_moments(ref)
    for key in ("count", "n_nan", "min", "max", "sum", "sumsq"):
        assert got[key] == want[key], (key, got[key], want[key])


def exact_histogram(counts, outliers, ref, edges):
    want, want_out = ref_histogram(ref, edges)
    assert int(np.sum(counts)) + sum(outliers) == ref.size, "bins and outliers do not sum to the voxel count"
    assert tuple(outliers) == want_out, (tuple(outliers), want_out)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), want), np.flatnonzero(np.asarray(counts) != want)[:8]


def exact_error(got, ref, y):
    want = ref_error(ref, y)
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])


# ------------------------------------------------------------------------------------------------ the sandwich bar
def near_edge_fraction(ref, bound, edges):
    """Share of the voxels that lie within their bound of an edge."""
    edges = np.asarray(edges, dtype=np.float64)
    i = np.clip(np.searchsorted(edges, ref), 1, edges.size - 1)
    dist = np.minimum(np.abs(ref - edges[i - 1]), np.abs(ref - edges[i]))
    return float(np.mean(dist <= bound))


def sandwich_moments(got, ref, bound):
    n = ref.size
    assert got["count"] == n and got["n_nan"] == 0, (got["count"], got["n_nan"])
    assert (ref - bound).min() <= got["min"] <= (ref + bound).min(), ("min", got["min"])
    assert (ref - bound).max() <= got["max"] <= (ref + bound).max(), ("max", got["max"])
    slack = bound.sum() + n * U64 * np.abs(ref).sum()
    assert abs(got["sum"] - ref.sum()) <= slack, ("sum", got["sum"], ref.sum(), slack)
    sq = ref * ref
    slack = (2 * np.abs(ref) * bound + bound * bound).sum() + n * U64 * sq.sum()
    assert abs(got["sumsq"] - sq.sum()) <= slack, ("sumsq", got["sumsq"], sq.sum(), slack)


def sandwich_histogram(counts, outliers, ref, bound, edges):
    edges = np.asarray(edges, dtype=np.float64)
    below, above, nan = outliers
    assert int(np.sum(counts)) + below + above + nan == ref.size, "bins and outliers do not sum to the voxel count"
    assert nan == 0
    cum = below + np.concatenate([[0], np.cumsum(counts)])  # C(e) for every edge
    lo, hi = np.sort(ref + bound), np.sort(ref - bound)
    least = np.searchsorted(lo, edges, side="left")   # #{ref + bound < e}
    most = np.searchsorted(hi, edges, side="left")    # #{ref - bound < e}
    least[-1] = np.searchsorted(lo, edges[-1], side="right")  # the closed last bin: v <= e
    most[-1] = np.searchsorted(hi, edges[-1], side="right")
    bad = (cum < least) | (cum > most)
    assert not bad.any(), (np.flatnonzero(bad)[:8], cum[bad][:8], least[bad][:8], most[bad][:8])


def sandwich_error(got, ref, bound, y):
    n = ref.size
    d = ref - y
    sq = d * d
    slack = (2 * np.abs(d) * bound + bound * bound).sum() + (n + 2) * U64 * sq.sum()
    assert abs(got["sse"] - sq.sum()) <= slack, ("sse", got["sse"], sq.sum(), slack)
    assert abs(got["max_abs"] - np.abs(d).max()) <= bound.max(), ("max_abs", got["max_abs"], np.abs(d).max())
    assert abs(got["ref_sumsq"] - (y * y).sum()) <= n * U64 * (y * y).sum(), ("ref_sumsq", got["ref_sumsq"])
    assert got["ref_max"] == y.max(), ("ref_max", got["ref_max"], y.max())


# ------------------------------------------------------------------------------------------------ modelled faults
# What a faulty kernel would return, computed from the reference: the bars must reject each of them.
def _as_matrix(c):
    m, n = last_product_shape(c.dims)
    return c.site.reshape(m, n)


def fault_tile_left_out(c):
    """The voxels that remain when the first 32 x 32 tile of the last product is never reduced."""
    keep = np.ones(_as_matrix(c).shape, dtype=bool)
    keep[:TILE, :TILE] = False
    return _as_matrix(c)[keep]


def fault_padding_counted(c):
    """The voxels, and a zero for every padded row and column element of the 32 x 32 tiles; None without padding."""
    m, n = last_product_shape(c.dims)
    pm, pn = -(-m // TILE) * TILE, -(-n // TILE) * TILE
    if pm * pn == m * n:
        return None
    return np.concatenate([c.site, np.zeros(pm * pn - m * n)])


def values_histogram(values, edges):
    """The histogram call's answer for a faulty set of voxels (too few, or with padding)."""
    return ref_histogram(values, edges)


def fault_last_bin_open(ref, edges):
    """Voxels equal to the last edge land in n_above; None when there are none."""
    counts, (below, above, nan) = ref_histogram(ref, edges)
    k = int((ref == np.float64(edges[-1])).sum())
    if k == 0:
        return None
    counts = counts.copy()
    counts[-1] -= k
    return counts, (below, above + k, nan)


def fault_bins_shifted(ref, edges):
    """Every voxel one bin to the right, the last bin's into n_above."""
    counts, (below, above, nan) = ref_histogram(ref, edges)
    return np.concatenate([[0], counts[:-1]]).astype(np.int64), (below, above + int(counts[-1]), nan)


def fault_site_order_original(c, y):
    """error_to that reads y at the site-order address of a voxel instead of through the offset tables."""
    return ref_error(c.site, y)


def fault_nan_in_a_bin(ref, edges):
    """NaN voxels counted into the first bin and not in n_nan; None without NaN."""
    counts, (below, above, nan) = ref_histogram(ref, edges)
    if nan == 0:
        return None
    counts = counts.copy()
    counts[0] += nan
    return counts, (below, above, 0)


def with_nan(c):
    """The reference of the case with NaN planted in one entry of core 1 (core 0 for a single site), and the cores."""
    cores = [x.copy() for x in c.cores]
    i = min(1, len(cores) - 1)
    cores[i][0, cores[i].shape[1] // 2, 0] = np.nan
    with np.errstate(invalid="ignore"):
        ref = cb.to_volume(mps_to_dense(cores).reshape(-1), c.dest)
    return cores, ref
