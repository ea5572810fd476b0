"""Histograms, quantiles and medians per label of an atlas or segmentation, from the cores, without decoding a volume.

The host side of the label-histogram epilogue of csrc/labelhist.hip.  The chain is contracted as ``label_stats``
contracts it; its last product runs once per window of labels, each voxel's label read through the offset tables of
the fused decode (``_Plan.split_tables``) and the voxel binned against the edge row of its label by the exact search of
``histogram``.  ``label_histogram`` hands every label the same row (the edges of ``valstat.edges_for``);
``label_quantile`` hands each label a row over its own bracket and narrows it as ``valstat.quantile`` does for the whole
volume.  Only integers are added, so the same inputs give the same bits.  NaN voxels are counted per label (``n_nan``)
and take no part in any bin or rank; an infinite voxel is binned like any other.

A launch holds the counters of one window of labels in at most 64 KiB of LDS; a call that would need more than 64
launches is refused (fewer bins, or split the atlas).

``NDMPS.label_histogram`` / ``label_histogram_many`` / ``label_quantile`` / ``label_median`` and the ``mask=`` keyword
of ``histogram`` / ``quantile`` / ``median`` are thin methods over the functions below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from . import labelstat as _ls
from . import valstat as _vs

MAX_LAUNCHES = 64

_torch = _vs._torch


def plan_query(np_type, n_labels, bins, per_label):
    """dict ``window, launches, lds_bytes, table_bytes`` of a call (host arithmetic only); ValueError for label or bin
    counts outside [1, 4096] and for a call that needs more than 64 launches."""
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load().ndmps_labelhist_plan_query(np.dtype(np_type).itemsize, int(n_labels), int(bins), int(bool(per_label)), out))
    return dict(window=int(out[0]), launches=int(out[1]), lds_bytes=int(out[2]), table_bytes=int(out[3]))


def workspace_bytes(chain, n_labels, bins, per_label):
    """Bytes of the one device buffer a call on ``chain`` allocates (0 for a call that would be refused)."""
    np_type, _ = _vs._element(chain)
    return int(_lib.load().ndmps_labelhist_workspace_bytes(chain.L, _lib.i64_array(chain.dims), _lib.i64_array(chain.bonds),
                                                           np.dtype(np_type).itemsize, int(n_labels), int(bins),
                                                           int(bool(per_label))))


class _Frame:
    """One chain with the label volume, the offset tables and the workspace on the device: ``run`` is the library call."""

    def __init__(self, chain, lab, tables, n_cols, n_labels, ws):
        self.call = _vs._Call(chain, ws=ws)
        self.np_type = self.call.np_type
        self.lab, self.tables, self.n_cols, self.n_labels = lab, tables, n_cols, n_labels

    def run(self, edges):
        """``(counts (n_labels, bins + 3) int64, lo, hi, outside)`` for one shared edge row (1-D) or one row per label
        (2-D): per label the bins, then below, above and the NaN count; ``lo`` / ``hi``: the smallest and largest voxel
        of each label inside its row's range (NaN where there is none)."""
        edges = np.ascontiguousarray(edges, dtype=self.np_type)
        per_label = edges.ndim == 2
        assert not per_label or edges.shape[0] == self.n_labels
        n, bins = self.n_labels, edges.shape[-1] - 1
        counts = np.zeros((n, bins + 3), dtype=np.int64)
        minmax, info = np.zeros(2 * n, dtype=np.float64), np.zeros(2, dtype=np.int64)
        row_off, col_off, col_perm = self.tables
        call = self.call
        _lib.check(call.entry("labelhist")(*call.head(), self.lab.data_ptr(), self.lab.element_size(), row_off.data_ptr(),
                                           col_off.data_ptr(), col_perm.data_ptr(), self.n_cols, n, edges.ctypes.data, bins,
                                           int(per_label), counts.ctypes.data, minmax.ctypes.data, info.ctypes.data,
                                           *call.tail()))
        return counts, minmax[:n].copy(), minmax[n:].copy(), int(info[0])


def _check_frames(chains):
    chains = list(chains)
    if not chains:
        raise ValueError("a series needs at least one frame")
    for t, chain in enumerate(chains):
        _vs._element(chain)
        if list(chain.dims) != list(chains[0].dims) or chain.device != chains[0].device:
            raise ValueError(f"frame {t} differs from frame 0 in its site dims or its device")
    return chains


def _frames(chains, plan, labels, n_labels, configs):
    """The frames of a call: the label volume and the offset tables go to the device once, and one workspace, sized
    for the largest frame and the largest of ``configs`` (pairs ``(bins, per_label)``), serves every launch."""
    torch = _torch()
    device = chains[0].device
    n_cols = _vs._split_columns(chains[0])
    lab = _ls._on_device(labels, device)
    tables = plan.split_tables(n_cols, device)
    ws = torch.empty(max(workspace_bytes(chain, n_labels, bins, per) for chain in chains for bins, per in configs),
                     dtype=torch.uint8, device=device)
    return [_Frame(chain, lab, tables, n_cols, n_labels, ws) for chain in chains]


def _is_int(bins):
    return isinstance(bins, (int, np.integer)) and not isinstance(bins, bool)


def label_histogram_many(chains, plan, labels, n_labels=None, bins=64, range=None, outliers=False):
    """``label_histogram`` of every frame of a series against one edge table: ``(counts (T, n_labels, bins) int64,
    edges)``, and with ``outliers`` a dict of ``below``, ``above``, ``n_nan`` (each ``(T, n_labels)``) and ``outside``
    (length T).  With an int ``bins`` and ``range=None`` the range is the minimum and maximum over all frames (a
    moments pass per frame first).  Row t is ``label_histogram(chains[t], ..., bins=edges)`` bit for bit.  The label
    volume and the offset tables go to the device once and one workspace serves every frame.  Frames share their site
    dims; bonds and element types may differ (each frame bins against the edges cast to its own type; the returned
    edges are frame 0's)."""
    torch = _torch()
    chains = _check_frames(chains)
    labels, n_labels = _ls.check_labels(labels, plan.shape, n_labels)
    if _is_int(bins) and 1 <= bins <= _vs.MAX_BINS:  # the launch limit before the moments passes
        for chain in chains:
            plan_query(_vs._element(chain)[0], n_labels, bins, False)
    with torch.cuda.device(chains[0].device):
        if _is_int(bins) and range is None and 1 <= bins <= _vs.MAX_BINS:
            whole = [_vs.moments(chain) for chain in chains]
            range = (min(m["min"] for m in whole), max(m["max"] for m in whole))
        edges = _vs.edges_for(chains[0], bins, range)
        n_bins = edges.size - 1
        per_frame = [_vs.check_edges(edges, _vs._element(chain)[0]) for chain in chains]
        for chain in chains:
            plan_query(_vs._element(chain)[0], n_labels, n_bins, False)
        frames = _frames(chains, plan, labels, n_labels, [(n_bins, False)])
        got = [frame.run(e) for frame, e in zip(frames, per_frame)]
    counts = np.stack([g[0][:, :n_bins] for g in got])
    if not outliers:
        return counts, edges
    out = dict(below=np.stack([g[0][:, n_bins] for g in got]), above=np.stack([g[0][:, n_bins + 1] for g in got]),
               n_nan=np.stack([g[0][:, n_bins + 2] for g in got]), outside=np.array([g[3] for g in got], dtype=np.int64))
    return counts, edges, out


def label_histogram(chain, plan, labels, n_labels=None, bins=64, range=None, outliers=False):
    """``numpy.histogram(volume[labels == l], bins, range)`` for every label l of ``labels`` (as ``label_stats`` takes
    them): ``(counts (n_labels, bins) int64, edges)``.  The edges are ``valstat.edges_for``'s, so equal arguments give
    the edges ``histogram`` uses: with an int ``bins`` and ``range=None`` they span the whole volume's min and max.
    With ``outliers`` also a dict of ``below``, ``above``, ``n_nan`` (int64 per label) and ``outside`` (the voxels whose
    label is negative or not below ``n_labels``): every voxel is in exactly one of bins, below, above, n_nan and
    outside."""
    got = label_histogram_many([chain], plan, labels, n_labels, bins, range, outliers)
    if not outliers:
        return got[0][0], got[1]
    out = {key: (value[0] if value.ndim == 2 else int(value[0])) for key, value in got[2].items()}
    return got[0][0], got[1], out


def _bracket_rows(lo, hi, active, fill, bins, np_type):
    """``(rows (n_labels, bins + 1), k)``: for an active label ``quantile``'s edges over its bracket (linspace in the
    element type, the ends pinned, duplicates removed) padded with the last edge, and ``k`` the number of real bins;
    for the others the constant row ``fill``."""
    rows = np.repeat(fill[:, None], bins + 1, axis=1).astype(np_type)
    k = np.zeros(lo.size, dtype=np.int64)
    which = np.flatnonzero(active)
    big = float(np.finfo(np_type).max) / 2  # an infinite end: the inner edges span the finite numbers, the end stays
    a = np.where(lo[which] == -np.inf, -big, lo[which].astype(np.float64))
    b = np.where(hi[which] == np.inf, big, hi[which].astype(np.float64))
    step = (b - a) / bins
    # numpy.linspace(a, b, bins + 1) of every label at once: arange * step + start, the last entry the stop
    e = np.arange(bins + 1, dtype=np.float64)[None, :] * step[:, None] + a[:, None]
    e[:, -1] = b
    for i in np.flatnonzero(step == 0):  # a bracket of denormals: linspace takes another route there
        e[i] = np.linspace(a[i], b[i], bins + 1)
    e = e.astype(np_type)
    e[:, 0], e[:, -1] = lo[which], hi[which]
    # np.unique of an ascending row: the first of every run of equal edges, then the last edge repeated
    keep = np.concatenate([np.ones((which.size, 1), dtype=bool), e[:, 1:] != e[:, :-1]], axis=1)
    e = np.take_along_axis(e, np.argsort(~keep, axis=1, kind="stable"), axis=1)
    n_kept = keep.sum(axis=1)
    e = np.where(np.arange(bins + 1)[None, :] < n_kept[:, None], e, hi[which][:, None])
    rows[which], k[which] = e, n_kept - 1
    return rows, k


def _quantile_of(frame, q, count, lo0, hi0, passes, bins):
    """``(value, lo, hi)`` per label for one q, from the counts and extremes of the first launch."""
    np_type = frame.np_type
    filled = count > 0
    rank = np.minimum(np.maximum(np.ceil(count * q - 1).astype(np.int64), 0), count - 1) + 1  # 1-based, as quantile's
    fill = np.where(filled, lo0, 0.0).astype(np_type)  # an empty label's row must not be NaN
    lo, hi = fill.copy(), np.where(filled, hi0, 0.0).astype(np_type)
    for _ in range(int(passes)):
        active = filled & (lo < hi)
        if not active.any():
            break
        rows, k = _bracket_rows(lo, hi, active, lo, bins, np_type)
        counts = frame.run(rows)[0]
        # quantile's search per label: the first of the k real bins whose cumulative count reaches the rank, the last
        # one at the latest.  A voxel equal to the repeated last edge sits in the last padded bin, which belongs to
        # real bin k - 1, so only the cumulative counts before that bin are looked at.
        cum = counts[:, bins:bins + 1] + np.cumsum(counts[:, :bins], axis=1)
        before = (cum < rank[:, None]) & (np.arange(bins)[None, :] < (k - 1)[:, None])
        b = np.minimum(before.sum(axis=1), np.maximum(k - 1, 0))
        left = np.take_along_axis(rows, b[:, None], axis=1)[:, 0]
        right = np.take_along_axis(rows, b[:, None] + 1, axis=1)[:, 0]
        right = np.where(b == k - 1, right, np.nextafter(right, np_type(-np.inf)))  # a bin without its right edge
        lo, hi = np.where(active, left, lo), np.where(active, right, hi)
    active = filled & (lo < hi)
    vlo, vhi = lo.astype(np.float64), hi.astype(np.float64)
    if active.any():  # the smallest and the largest voxel inside each bracket
        _, inside_lo, inside_hi, _ = frame.run(np.stack([lo, np.where(active, hi, lo)], axis=1))
        got = active & ~np.isnan(inside_lo)
        vlo[got], vhi[got] = inside_lo[got], inside_hi[got]
    value = np.where(vlo == vhi, vlo, 0.5 * (vlo + vhi))
    for a in (value, vlo, vhi):
        a[~filled] = np.nan
    return value, vlo, vhi


def label_quantile(chain, plan, labels, q, n_labels=None, passes=2, bins=64):
    """The ``q``-quantile (numpy's ``method="inverted_cdf"`` on a label's non-NaN voxels) of every label, by repeated
    histograms with one edge row per label: a dict of ``value``, ``lo``, ``hi`` (float64, shape ``(n_labels,)`` for a
    scalar ``q`` and ``(n_labels, Q)`` for a sequence), ``count``, ``n_nan`` (int64 per label) and ``outside``.

    One launch over ``[-inf, +inf]`` gives count, n_nan, min and max per label; each of up to ``passes`` launches of
    ``bins`` bins narrows every label's bracket to the bin that holds its rank; a last launch finds the smallest and
    the largest voxel inside each bracket.  ``value`` is exact where the two coincide and their midpoint otherwise;
    ``lo <= true quantile <= hi``.  A label without a non-NaN voxel gives NaN.  A sequence of q runs the passes once
    per q on the first launch's counts, so it equals the scalar calls bit for bit."""
    torch = _torch()
    np_type, _ = _vs._element(chain)
    qs = np.asarray(q, dtype=np.float64)
    scalar = qs.ndim == 0
    qs = qs.reshape(-1) if scalar else qs
    if qs.ndim != 1 or qs.size == 0 or not np.all((qs >= 0.0) & (qs <= 1.0)):
        raise ValueError("q must be a number or a one-dimensional sequence of numbers in [0, 1]")
    if not 1 <= int(bins) <= _vs.MAX_BINS:
        raise ValueError(f"bins must lie in [1, {_vs.MAX_BINS}]")
    bins = int(bins)
    labels, n_labels = _ls.check_labels(labels, plan.shape, n_labels)
    configs = [(1, False), (bins, True), (1, True)]
    for n_bins, per in configs:
        plan_query(np_type, n_labels, n_bins, per)
    with torch.cuda.device(chain.device):
        frame = _frames([chain], plan, labels, n_labels, configs)[0]
        counts, lo0, hi0, outside = frame.run(np.array([-np.inf, np.inf], dtype=np_type))
        count, n_nan = counts[:, 0].copy(), counts[:, 3].copy()
        cols = [_quantile_of(frame, float(x), count, lo0, hi0, passes, bins) for x in qs]
    value, lo, hi = (cols[0][i] if scalar else np.stack([c[i] for c in cols], axis=1) for i in range(3))
    return dict(value=value, lo=lo, hi=hi, count=count, n_nan=n_nan, outside=outside)


def label_median(chain, plan, labels, n_labels=None, passes=2, bins=64):
    """``label_quantile(..., 0.5)["value"]``."""
    return label_quantile(chain, plan, labels, 0.5, n_labels, passes, bins)["value"]


# ------------------------------------------------------------------------------------------------ a mask: two labels
def mask_labels(mask):
    """A bool or integer volume as the label volume of two labels: non-zero is label 1 (inside).  TypeError for
    another element type."""
    torch = _torch()
    if not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask)
    name = _ls._type_name(mask)
    if not (name == "bool" or name.startswith("int") or name.startswith("uint")):
        raise TypeError(f"a mask must be a bool or integer volume, got {name}")
    return mask if name == "bool" else mask != 0


def masked_histogram(chain, plan, mask, bins, range, outliers):
    """``histogram`` of the voxels where ``mask`` is non-zero; with an int ``bins`` and ``range=None`` the edges span
    the whole volume's min and max, as ``histogram``'s do."""
    counts, edges, out = label_histogram(chain, plan, mask_labels(mask), 2, bins, range, True)
    if not outliers:
        return counts[1], edges
    return counts[1], edges, (int(out["below"][1]), int(out["above"][1]), int(out["n_nan"][1]))


def masked_quantile(chain, plan, mask, q, passes, bins):
    """``quantile`` of the voxels where ``mask`` is non-zero: ``(value, (lo, hi))``."""
    if np.ndim(q) != 0:
        raise ValueError("q must be a number")
    got = label_quantile(chain, plan, mask_labels(mask), float(q), 2, passes, bins)
    return float(got["value"][1]), (float(got["lo"][1]), float(got["hi"][1]))
