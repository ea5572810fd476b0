"""Value statistics of the volume a chain decodes to, and its error against an original, from the cores.

The host side of csrc/valstat.hip: the chain is contracted as ``to_tensor`` contracts it, but the last product -- the
only one that touches N elements -- reduces its accumulator tiles instead of storing them, so the volume is never
written.  Every function takes a ``DeviceMPS`` of fp32 or fp64 cores; the error functions also take the permutation
plan (``_Plan``) that maps the chain's site-order tensor onto the C-order volume.  ``NDMPS.value_stats`` / ``min`` /
``max`` / ``histogram`` / ``quantile`` / ``error_to`` / ``psnr_to`` are thin methods over these.

NaN voxels are counted (``n_nan``) and take no part in any statistic or bin.  The same inputs give the same bits.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _lib

MAX_BINS = 4096


def _torch():
    import torch

    return torch


def _element(chain):
    """(numpy element type, entry suffix) of a chain the kernels take; ValueError for bf16 cores."""
    torch = _torch()
    if chain.dtype == torch.float32:
        return np.float32, "f32"
    if chain.dtype == torch.float64:
        return np.float64, "f64"
    raise ValueError("value statistics run on fp32 or fp64 cores: convert bf16 cores with astype(torch.float32) first")


def workspace_bytes(chain, n_bins=0):
    """Bytes of the one device buffer a call on ``chain`` with ``n_bins`` histogram bins allocates."""
    np_type, _ = _element(chain)
    return int(_lib.load().ndmps_valstat_workspace_bytes(chain.L, _lib.i64_array(chain.dims), _lib.i64_array(chain.bonds),
                                                         np.dtype(np_type).itemsize, int(n_bins)))


class _Call:
    """The arguments every entry of the statistics family shares (core/valstat.py, axisext.py, labelstat.py,
    pairstat.py): one chain, or two of one shape (``other``: the pair entries), and the workspace -- the caller's
    (``ws``), or a new one of ``ws_bytes`` bytes, or one with room for ``n_bins`` histogram bins."""

    def __init__(self, chain, n_bins=0, other=None, ws=None, ws_bytes=None):
        torch = _torch()
        self.np_type, self.suffix = _element(chain)
        self.lib = _lib.load()
        chains = (chain,) if other is None else (chain, other)
        self._head = (chain.L, _lib.i64_array(chain.dims), *[_lib.i64_array(c.bonds) for c in chains],
                      *[c._core_ptrs() for c in chains])
        if ws is None:
            ws_bytes = workspace_bytes(chain, n_bins) if ws_bytes is None else ws_bytes
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=chain.device)
        self.ws, self.ws_bytes = ws, ws.numel()

    def entry(self, name):
        """``ndmps_<name>_f32`` or ``_f64``, by the chain's element type."""
        return getattr(self.lib, f"ndmps_{name}_{self.suffix}")

    def head(self):
        """L, dims, the bonds of each chain, the core pointers of each chain."""
        return self._head

    def tail(self):
        return self.ws.data_ptr(), self.ws_bytes, _lib.stream_ptr()


def moments(chain, clip=None):
    """``count, n_nan, taken, min, max, sum, sumsq`` of the voxels; ``clip=(lo, hi)``: the four statistics and ``taken``
    over the voxels with ``lo <= v <= hi`` only."""
    call = _Call(chain)
    lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    stats, counts = (C.c_double * 4)(), (C.c_int64 * 3)()
    with _torch().cuda.device(chain.device):
        _lib.check(call.entry("valstat_moments")(*call.head(), lo, hi, stats, counts, *call.tail()))
    return dict(count=int(counts[0]), n_nan=int(counts[1]), taken=int(counts[2]), min=float(stats[0]), max=float(stats[1]),
                sum=float(stats[2]), sumsq=float(stats[3]))


def value_stats(chain):
    """dict ``count, min, max, sum, sumsq, n_nan`` and the derived ``mean, std, norm`` (population std, Frobenius norm)
    of the non-NaN voxels; a volume of NaN only has NaN for all but the counts."""
    m = moments(chain)
    n = m["count"] - m["n_nan"]
    out = dict(count=m["count"], min=m["min"], max=m["max"], sum=m["sum"], sumsq=m["sumsq"], n_nan=m["n_nan"])
    if n == 0:
        out.update(min=math.nan, max=math.nan, sum=math.nan, sumsq=math.nan, mean=math.nan, std=math.nan, norm=math.nan)
        return out
    mean = m["sum"] / n
    out.update(mean=mean, std=math.sqrt(max(m["sumsq"] / n - mean * mean, 0.0)), norm=math.sqrt(m["sumsq"]))
    return out


def check_edges(edges, np_type):
    """An explicit edge array in the element type: one-dimensional, at least two edges, at most MAX_BINS bins, ascending,
    no NaN (ValueError otherwise)."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).astype(np_type))
    if e.ndim != 1 or e.size < 2:
        raise ValueError("bins must be an int or a one-dimensional array of at least two edges")
    if e.size - 1 > MAX_BINS:
        raise ValueError(f"histogram takes at most {MAX_BINS} bins, got {e.size - 1}: bin coarser, or narrow the range "
                         "and bin again (quantile does)")
    if np.isnan(e).any() or np.any(np.diff(e) < 0):
        raise ValueError("histogram edges must be ascending (monotonically increasing, no NaN)")
    return e


def bin_counts(chain, edges):
    """(counts int64 per bin, n_below, n_above, n_nan) for checked ``edges`` (check_edges), as numpy.histogram bins:
    ``edges[b] <= v < edges[b + 1]``, the last bin closed on the right."""
    n_bins = int(edges.size - 1)
    call = _Call(chain, n_bins)
    counts = np.zeros(n_bins + 3, dtype=np.int64)
    with _torch().cuda.device(chain.device):
        _lib.check(call.entry("valstat_histogram")(*call.head(), edges.ctypes.data_as(C.c_void_p), n_bins,
                                                   counts.ctypes.data_as(_lib.p_i64), *call.tail()))
    return counts[:n_bins].copy(), int(counts[n_bins]), int(counts[n_bins + 1]), int(counts[n_bins + 2])


def edges_for(chain, bins, range=None):
    """The checked edge table of a histogram call on ``chain``, in its element type.  ``bins``: an int (equal-width bins
    over ``range``, or over the volume's min and max, which costs a moments pass first) or an explicit ascending edge
    array.  ``histogram`` and the axes of ``pairstat.joint_histogram`` both come here: equal arguments, equal edges."""
    np_type, _ = _element(chain)
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        if bins < 1:
            raise ValueError("bins must be at least 1")
        if bins > MAX_BINS:
            raise ValueError(f"histogram takes at most {MAX_BINS} bins, got {int(bins)}: bin coarser, or narrow the range "
                             "and bin again (quantile does)")
        if range is None:
            m = moments(chain)
            lo, hi = m["min"], m["max"]
        else:
            lo, hi = float(range[0]), float(range[1])
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"histogram range [{lo}, {hi}] is not finite")
        if lo > hi:
            raise ValueError("histogram edges must be ascending: range[0] > range[1]")
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5  # numpy's rule for an empty range
        return check_edges(np.linspace(lo, hi, int(bins) + 1), np_type)
    return check_edges(bins, np_type)


def histogram(chain, bins=256, range=None, outliers=False):
    """``numpy.histogram(volume, bins, range)``: (counts int64, edges in the element type), and with ``outliers`` also
    ``(n_below, n_above, n_nan)``.  ``bins``: an int (equal-width bins over ``range``, or over the volume's min and
    max, which costs a moments pass first) or an explicit ascending edge array."""
    edges = edges_for(chain, bins, range)
    counts, below, above, nan = bin_counts(chain, edges)
    return (counts, edges, (below, above, nan)) if outliers else (counts, edges)


def quantile(chain, q, passes=2, bins=MAX_BINS):
    """The ``q``-quantile of the non-NaN voxels by repeated histograms: ``(value, (lo, hi))``.

    The wanted voxel is the one of rank ``ceil(q N)`` in ascending order (numpy's ``method="inverted_cdf"``).  A moments
    pass gives the first bracket ``[min, max]``; each of up to ``passes`` histograms of ``bins`` bins over the bracket
    narrows it to the one bin that holds the rank.  The search stops early when the bracket is a single number of the
    element type.  A last clipped moments pass looks inside the bracket: if it holds one distinct value that value is
    returned, exactly; otherwise the midpoint of the smallest and the largest voxel in it.  ``(lo, hi)`` are those
    two, so ``lo <= true quantile <= hi`` and ``hi - lo`` is the uncertainty."""
    np_type, _ = _element(chain)
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must lie in [1, {MAX_BINS}]")
    m = moments(chain)
    n = m["count"] - m["n_nan"]
    if n == 0:
        return math.nan, (math.nan, math.nan)
    rank = min(max(int(math.ceil(n * q - 1)), 0), n - 1) + 1  # 1-based, as numpy's inverted_cdf indexes
    lo, hi = np_type(m["min"]), np_type(m["max"])
    for _ in range(int(passes)):
        if lo == hi:
            break
        edges = np.linspace(float(lo), float(hi), int(bins) + 1).astype(np_type)
        edges[0], edges[-1] = lo, hi
        edges = np.unique(edges)  # strictly ascending: a narrow bracket has fewer than `bins` numbers in it
        counts, below, _, _ = bin_counts(chain, edges)
        cum = below + np.cumsum(counts)
        b = int(np.searchsorted(cum, rank, side="left"))
        b = min(b, counts.size - 1)
        last = b == counts.size - 1
        lo = edges[b]
        hi = edges[b + 1] if last else np.nextafter(edges[b + 1], np_type(-np.inf))  # the bin without its right edge
    if lo == hi:
        return float(lo), (float(lo), float(hi))
    inside = moments(chain, clip=(lo, hi))
    if inside["taken"] == 0:  # cannot happen for a bracket that holds the rank; keep the bracket
        return 0.5 * (float(lo) + float(hi)), (float(lo), float(hi))
    lo, hi = inside["min"], inside["max"]
    return (lo if lo == hi else 0.5 * (lo + hi)), (lo, hi)


def _split_columns(chain):
    """Columns of the chain's last product: the pre-contracted tail's, or the last site's for a chain without one."""
    n_tail = int(_lib.load().ndmps_chain_tail_columns(chain.L, _lib.i64_array(chain.dims)))
    return n_tail if n_tail > 0 else int(chain.dims[-1])


def error_to(chain, plan, x):
    """The error of the decoded volume against ``x`` (NumPy array or device tensor of ``plan.shape``, cast to the
    chain's element type): dict ``sse, mse, max_abs, ref_sumsq, ref_max, rel_frob`` and ``n_nan`` (voxels whose
    difference is NaN; they are left out of the rest).  ``x`` is read through the offset tables of the fused decode,
    in the order the last product produces the voxels."""
    torch = _torch()
    np_type, _ = _element(chain)
    shape = tuple(int(s) for s in plan.shape)
    if tuple(int(s) for s in x.shape) != shape:
        raise ValueError(f"the original has shape {tuple(x.shape)}, the object {shape}")
    device = chain.device
    if isinstance(x, torch.Tensor):
        ref = x.to(device=device, dtype=chain.dtype).contiguous()
    else:
        ref = torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np_type, copy=False))).to(device)
    n_cols = _split_columns(chain)
    with torch.cuda.device(device):
        row_off, col_off, col_perm = plan.split_tables(n_cols, device)
        call = _Call(chain)
        stats, counts = (C.c_double * 4)(), (C.c_int64 * 3)()
        _lib.check(call.entry("valstat_error")(*call.head(), ref.data_ptr(), row_off.data_ptr(), col_off.data_ptr(),
                                               col_perm.data_ptr(), n_cols, stats, counts, *call.tail()))
    n = int(counts[0]) - int(counts[1])
    sse, max_abs, ref_sumsq, ref_max = (float(v) for v in stats)
    return dict(sse=sse, mse=sse / n if n else math.nan, max_abs=max_abs, ref_sumsq=ref_sumsq, ref_max=ref_max,
                rel_frob=math.sqrt(sse / ref_sumsq) if ref_sumsq > 0 else (0.0 if sse == 0 else math.inf),
                n_nan=int(counts[1]))


def psnr_from(err):
    """``10 log10(max(x)^2 / mse)`` of an ``error_to`` dict, ``inf`` at mse = 0: the reference's compute_psnr (``-inf``
    like NumPy's log10 when the original's maximum is 0 and the error is not)."""
    if err["mse"] == 0:
        return math.inf
    ratio = err["ref_max"] ** 2 / err["mse"]
    return -math.inf if ratio == 0 else 10.0 * math.log10(ratio)
