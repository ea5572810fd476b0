"""Statistics of two volumes from the cores of both: pair moments, the joint histogram, mutual information.

The host side of csrc/pairstat.hip.  Two chains of one shape and one factorisation end in last products of the same
rows and columns (``chain_plan`` splits by the site dims alone), so one kernel forms both accumulator tiles of a tile
index and reduces the voxel PAIRS in registers and LDS: neither volume is written.  Every function takes two
``DeviceMPS`` of fp32 or fp64 cores with equal site dims on one device; one fp32 and one fp64 chain make the call fp64
(the fp32 cores are cast: they are small).  ``NDMPS.pair_stats`` / ``joint_histogram`` / ``mutual_information`` /
``mutual_information_many`` are thin methods over these.

A voxel with either value NaN is counted in ``n_nan`` and takes no part in anything else.  A voxel's value is computed
exactly as core/valstat.py's calls compute it, so the marginals of a joint histogram are the single histograms bit
for bit, and the same inputs give the same bits.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _lib
from . import valstat as _vs
from .mps import DeviceMPS

MAX_AXIS_BINS = 1024
MAX_CELLS = 16384


_torch = _vs._torch


def pair_chains(a, b):
    """The two chains as one call takes them: equal site dims and device (ValueError otherwise, and for bf16 cores as
    ``valstat``), both in the wider of the two element types."""
    torch = _torch()
    _vs._element(a)
    _vs._element(b)
    if list(a.dims) != list(b.dims):
        raise ValueError(f"the two objects differ in their site dims: {list(a.dims)} != {list(b.dims)} (the last products "
                         "of the two chains would differ in rows or columns, so their voxels do not correspond)")
    if a.device != b.device:
        raise ValueError(f"the two objects differ in device: {a.device} != {b.device}")
    if a.dtype != b.dtype:
        wide = lambda ch: ch if ch.dtype == torch.float64 else DeviceMPS(  # noqa: E731
            [c.to(torch.float64).contiguous() for c in ch.cores], _trusted=True)
        a, b = wide(a), wide(b)
    return a, b


def check_bins(bins_a, bins_b):
    """ValueError for an axis above MAX_AXIS_BINS bins or more than MAX_CELLS cells."""
    for which, n in (("a", bins_a), ("b", bins_b)):
        if n < 1:
            raise ValueError("bins must be at least 1")
        if n > MAX_AXIS_BINS:
            raise ValueError(f"joint_histogram takes at most {MAX_AXIS_BINS} bins per axis, got {n} for {which}")
    if bins_a * bins_b > MAX_CELLS:
        raise ValueError(f"joint_histogram takes at most {MAX_CELLS} cells, got {bins_a} x {bins_b} = {bins_a * bins_b}: "
                         "bin coarser")


def workspace_bytes(a, b, bins_a=0, bins_b=0):
    """Bytes of the one device buffer a call on the (checked) pair allocates; bins 0, 0: the moments."""
    np_type, _ = _vs._element(a)
    return int(_lib.load().ndmps_pairstat_workspace_bytes(a.L, _lib.i64_array(a.dims), _lib.i64_array(a.bonds),
                                                          _lib.i64_array(b.bonds), np.dtype(np_type).itemsize,
                                                          int(bins_a), int(bins_b)))


def _call(a, b, bins_a=0, bins_b=0):
    """``valstat._Call`` of both chains with a workspace with room for ``bins_a`` x ``bins_b`` cells."""
    ws_bytes = workspace_bytes(a, b, bins_a, bins_b)
    if ws_bytes <= 0:
        raise ValueError("the library refuses the workspace query of this pair")
    return _vs._Call(a, other=b, ws_bytes=ws_bytes)


RAW_FIELDS = ("sum_a", "sum_b", "sumsq_a", "sumsq_b", "sum_ab", "sse", "min_a", "max_a", "min_b", "max_b", "max_abs_diff")


def pair_moments(a, b):
    """The raw record of a checked pair: ``count`` (voxels where neither value is NaN), ``n_nan`` (the others) and
    RAW_FIELDS over the counted voxels."""
    call = _call(a, b)
    stats, counts = (C.c_double * 11)(), (C.c_int64 * 2)()
    with _torch().cuda.device(a.device):
        _lib.check(call.entry("pairstat_moments")(*call.head(), stats, counts, *call.tail()))
    out = dict(count=int(counts[0]), n_nan=int(counts[1]))
    out.update(zip(RAW_FIELDS, (float(v) for v in stats)))
    return out


def derive(m):
    """``mean_a, mean_b, cov, pearson, mse, rel_frob`` (``||a - b|| / ||b||``) from a raw record, in fp64 on the host;
    no counted voxel: NaN for everything but the counts."""
    out = dict(m)
    n = m["count"]
    if n == 0:
        out.update({k: math.nan for k in RAW_FIELDS + ("mean_a", "mean_b", "cov", "pearson", "mse", "rel_frob")})
        return out
    mean_a, mean_b = m["sum_a"] / n, m["sum_b"] / n
    cov = m["sum_ab"] / n - mean_a * mean_b
    var_a = max(m["sumsq_a"] / n - mean_a * mean_a, 0.0)
    var_b = max(m["sumsq_b"] / n - mean_b * mean_b, 0.0)
    denom = math.sqrt(var_a * var_b)
    out.update(mean_a=mean_a, mean_b=mean_b, cov=cov, pearson=cov / denom if denom > 0 else math.nan, mse=m["sse"] / n,
               rel_frob=math.sqrt(m["sse"] / m["sumsq_b"]) if m["sumsq_b"] > 0 else (0.0 if m["sse"] == 0 else math.inf))
    return out


def pair_stats(a, b):
    """dict of the raw record and the derived fields of two chains (checked here)."""
    a, b = pair_chains(a, b)
    return derive(pair_moments(a, b))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def split_bins(bins):
    """``bins`` of a joint histogram as one entry per axis: an int serves both, otherwise a pair, each an int or an
    explicit ascending edge array."""
    if _is_int(bins):
        return bins, bins
    try:
        if len(bins) == 2:
            return bins[0], bins[1]
    except TypeError:
        pass
    raise ValueError("bins must be an int, a pair of ints or a pair of edge arrays")


def joint_edges(a, b, bins=64, range=None):
    """The two checked edge tables of a joint histogram on a checked pair, each by ``valstat.edges_for`` on its own
    chain (an int without a range: that chain's min and max from its own moments pass)."""
    bins_a, bins_b = split_bins(bins)
    if range is None:
        range = (None, None)
    if len(range) != 2:
        raise ValueError("range must be None or ((lo_a, hi_a), (lo_b, hi_b))")
    for n in (bins_a, bins_b):
        if _is_int(n):
            check_bins(int(n), 1)
    ea = _vs.edges_for(a, bins_a, range[0] if _is_int(bins_a) else None)
    eb = _vs.edges_for(b, bins_b, range[1] if _is_int(bins_b) else None)
    check_bins(ea.size - 1, eb.size - 1)
    return ea, eb


def joint_counts(a, b, ea, eb):
    """(counts int64 (bins_a, bins_b), outside, n_nan) of a checked pair for checked edges."""
    na, nb = int(ea.size - 1), int(eb.size - 1)
    check_bins(na, nb)
    call = _call(a, b, na, nb)
    counts = np.zeros(na * nb + 2, dtype=np.int64)
    with _torch().cuda.device(a.device):
        _lib.check(call.entry("pairstat_histogram")(*call.head(), ea.ctypes.data_as(C.c_void_p), na,
                                                    eb.ctypes.data_as(C.c_void_p), nb, counts.ctypes.data_as(_lib.p_i64),
                                                    *call.tail()))
    return counts[:na * nb].reshape(na, nb).copy(), int(counts[na * nb]), int(counts[na * nb + 1])


def joint_histogram(a, b, bins=64, range=None, outliers=False):
    """``numpy.histogram2d(va.ravel(), vb.ravel(), bins, range)`` of the two volumes: (counts int64 (bins_a, bins_b),
    edges_a, edges_b in the call's element type), and with ``outliers`` also ``(outside, n_nan)``: the voxels with
    either value outside its range, and those with either value NaN (NaN wins)."""
    a, b = pair_chains(a, b)
    ea, eb = joint_edges(a, b, bins, range)
    counts, outside, nan = joint_counts(a, b, ea, eb)
    return (counts, ea, eb, (outside, nan)) if outliers else (counts, ea, eb)


def _entropy(counts, total):
    """``sum (c / total) ln(total / c)`` over the non-zero entries, fp64."""
    c = counts[counts > 0].astype(np.float64)
    return float(np.sum(c / total * np.log(total / c)))


def mutual_information_from_counts(counts, normalized=False):
    """Mutual information of a table of counts, in nats, fp64 on the host: ``sum p_ij ln(p_ij / (p_i. p_.j))`` over the
    non-empty cells with p over the binned voxels, written on the counts as ``(n_ij / N) ln(n_ij N / (r_i c_j))`` so
    that an independent table gives exactly 0.  ``normalized``: ``(H(a) + H(b)) / H(a, b)`` (Studholme), 1.0 when
    ``H(a, b) == 0``.  An empty table gives 0 (normalized: 1)."""
    counts = np.asarray(counts, dtype=np.int64)
    total = float(counts.sum())
    if total == 0:
        return 1.0 if normalized else 0.0
    rows, cols = counts.sum(axis=1), counts.sum(axis=0)
    if normalized:
        joint = _entropy(counts, total)
        return (_entropy(rows, total) + _entropy(cols, total)) / joint if joint != 0 else 1.0
    i, j = np.nonzero(counts)
    n = counts[i, j].astype(np.float64)
    return float(np.sum(n / total * np.log(n * total / (rows[i].astype(np.float64) * cols[j].astype(np.float64)))))


def mutual_information(a, b, bins=64, range=None, normalized=False):
    """Mutual information (nats) of the two volumes from their joint histogram over the binned voxels."""
    counts = joint_histogram(a, b, bins, range)[0]
    return mutual_information_from_counts(counts, normalized)


def mutual_information_many(chains, ref, bins=64, range=None, normalized=False):
    """``mutual_information(chains[t], ref, ...)`` for every t as a (T,) fp64 array.  The edges of ``ref`` are fixed once
    (one moments pass for an int without a range); entry t equals ``mutual_information(chains[t], ref, (bins_t,
    ref_edges), ...)`` bit for bit, where ``bins_t`` is the first entry of ``bins`` (with the first range).  A loop of
    single calls."""
    bins_a, bins_b = split_bins(bins)
    range_a, range_b = (None, None) if range is None else range
    out = np.zeros(len(chains), dtype=np.float64)
    ref_edges = None
    for t, chain in enumerate(chains):
        if ref_edges is None:
            _, wide_ref = pair_chains(chain, ref)
            ref_edges = _vs.edges_for(wide_ref, bins_b, range_b if _is_int(bins_b) else None).astype(np.float64)
        out[t] = mutual_information(chain, ref, (bins_a, ref_edges), (range_a, None), normalized)
    return out
