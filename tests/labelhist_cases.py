"""Cases, references and bars of the histograms and quantiles per label from the cores (LabelHistEpi in
csrc/labelhist.hip, core/labelhist.py).

The chains, their fp64 references and their element bounds are those of tests/valstat_cases.py (``vc.Case``), the label
volumes those of tests/labelstat_cases.py (``lc.labels``), the edge tables ``vc.integer_edge_sets`` and
``Case.edges64``; all imported and not changed.  Nothing here touches a GPU: tests/test_labelhist_host.py runs the bars
on the reference and on modelled faults, tests/test_gpu_labelhist.py on what the kernels return.

A histogram result is a dict ``counts (n_labels, bins)``, ``below``, ``above``, ``n_nan`` (int64 per label) and
``outside``; the edges are one row for every label (1-D) or one row per label (2-D; a row may repeat its last edge).

* exact, on integer cores: per label the four arrays equal ``vc.ref_histogram`` of that label's voxels, bit for bit,
  ``outside`` equals NumPy's, and bins + below + above + n_nan + outside = N.  ``label_quantile`` equals
  ``np.quantile(ref[lab == l], q, method="inverted_cdf")`` with ``lo == hi == value``, given enough passes:
  ``bins ** passes`` at least the integer range, so the last bracket is narrower than 1 (``passes_for``).
* sandwich, on real cores: ``vc.sandwich_histogram`` on each label's ``ref`` / ``bound`` sub-arrays, and per label the
  quantile bar of tests/test_gpu_valstat.py: ``lo <= value <= hi``, ``lo <= sort(ref + bound)[k]``,
  ``hi >= sort(ref - bound)[k]``.
"""
from __future__ import annotations

import numpy as np

import labelstat_cases as lc
import valstat_cases as vc

MAX_LDS = 64 * 1024
MAX_LAUNCHES = 64
QS = (0, 0.25, 0.5, 1)
KEYS = ("counts", "below", "above", "n_nan")


# ------------------------------------------------------------------------------------------------ the window rule
def window_rule(elem_bytes, n_labels, bins, per_label):
    """dict ``window, launches, lds_bytes, table_bytes`` in Python integers: a window of w labels holds its edge rows
    (one shared, or w), two keys per label in the element's width and bins + 3 32-bit counters per label in at most
    64 KiB; None for a call that needs more than 64 launches."""
    fixed = 0 if per_label else elem_bytes * (bins + 1)
    each = elem_bytes * ((bins + 1 if per_label else 0) + 2) + 4 * (bins + 3)
    window = min(n_labels, (MAX_LDS - fixed) // each)
    assert window >= 1
    launches = -(-n_labels // window)
    if launches > MAX_LAUNCHES:
        return None
    return dict(window=window, launches=launches, lds_bytes=fixed + each * window,
                table_bytes=-(-(8 * (n_labels * (bins + 5) + 1)) // 256) * 256)


# ------------------------------------------------------------------------------------------------ what NumPy says
def hist_of_by_numpy(values, vlab, n_labels, edges):
    """The result dict NumPy gives for parallel flat arrays of voxel values (fp64) and labels: ``vc.ref_histogram`` of
    each label's voxels against the shared row or the label's own row.  The definition; ``hist_of`` is the same
    numbers in one pass (tests/test_labelhist_host.py compares the two on every case)."""
    values, vlab = np.asarray(values, dtype=np.float64), np.asarray(vlab, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.shape[-1] - 1
    out = dict(counts=np.zeros((n_labels, bins), dtype=np.int64), below=np.zeros(n_labels, dtype=np.int64),
               above=np.zeros(n_labels, dtype=np.int64), n_nan=np.zeros(n_labels, dtype=np.int64),
               outside=int(((vlab < 0) | (vlab >= n_labels)).sum()))
    order, starts, filled = lc._segments(vlab, n_labels)
    ends = np.append(starts[1:], order.size)
    for l, a, b in zip(filled, starts, ends):
        row = edges[l] if edges.ndim == 2 else edges
        out["counts"][l], (out["below"][l], out["above"][l], out["n_nan"][l]) = vc.ref_histogram(values[order[a:b]], row)
    return out


def places(values, row):
    """The place of every voxel in the ascending row e[0 .. B], as numpy.histogram bins: b for e[b] <= v < e[b + 1],
    the last bin closed on the right; B: below, B + 1: above, B + 2: NaN."""
    values, row = np.asarray(values, dtype=np.float64), np.asarray(row, dtype=np.float64)
    bins = row.size - 1
    with np.errstate(invalid="ignore"):
        at = np.minimum(np.searchsorted(row, values, side="right") - 1, bins - 1)
        at = np.where(values < row[0], bins, np.where(values > row[-1], bins + 1, at))
    return np.where(np.isnan(values), bins + 2, at).astype(np.int64)


def cells_of(at, vlab, n_labels, bins):
    """The result dict from the place of every voxel (``places``) and its label."""
    inside = (vlab >= 0) & (vlab < n_labels)
    cells = np.bincount(vlab[inside] * (bins + 3) + at[inside], minlength=n_labels * (bins + 3)).astype(np.int64)
    cells = cells.reshape(n_labels, bins + 3)
    return dict(counts=cells[:, :bins].copy(), below=cells[:, bins].copy(), above=cells[:, bins + 1].copy(),
                n_nan=cells[:, bins + 2].copy(), outside=int(vlab.size - inside.sum()))


def hist_of(values, vlab, n_labels, edges):
    """``hist_of_by_numpy`` in one pass over the voxels."""
    values, vlab = np.asarray(values, dtype=np.float64), np.asarray(vlab, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.shape[-1] - 1
    if edges.ndim == 1:
        return cells_of(places(values, edges), vlab, n_labels, bins)
    at = np.zeros(values.size, dtype=np.int64)
    order, starts, filled = lc._segments(vlab, n_labels)
    ends = np.append(starts[1:], order.size)
    for l, a, b in zip(filled, starts, ends):
        at[order[a:b]] = places(values[order[a:b]], edges[l])
    return cells_of(at, vlab, n_labels, bins)


def quantile_of_by_numpy(values, vlab, n_labels, q):
    """``np.quantile(values[vlab == l], q, method="inverted_cdf")`` over the non-NaN voxels; NaN for a label without.
    The definition; ``quantiles_of`` is the same numbers from one sort."""
    out = np.full(n_labels, np.nan)
    order, starts, filled = lc._segments(vlab, n_labels)
    ends = np.append(starts[1:], order.size)
    for l, a, b in zip(filled, starts, ends):
        v = values[order[a:b]]
        v = v[~np.isnan(v)]
        if v.size:
            out[l] = np.quantile(v, q, method="inverted_cdf")
    return out


def quantiles_of(values, vlab, n_labels, qs):
    """``(n_labels, len(qs))``: per label the voxel of rank ``ceil(q n)`` among its n non-NaN voxels in ascending order
    (0-based ``min(max(ceil(n q - 1), 0), n - 1)``: numpy's ``inverted_cdf``); NaN for a label without."""
    values, vlab = np.asarray(values, dtype=np.float64), np.asarray(vlab, dtype=np.int64)
    keep = (vlab >= 0) & (vlab < n_labels) & ~np.isnan(values)
    v, l = values[keep], vlab[keep]
    if v.size and np.array_equal(v, np.rint(v)) and (v.max() - v.min() + 1) * n_labels < 2 ** 62:
        base, span = int(v.min()), int(v.max() - v.min()) + 1  # integers: one sort of label * span + value
        key = np.sort(l * span + (v.astype(np.int64) - base))
        v, l = (key % span + base).astype(np.float64), key // span
    else:
        order = np.lexsort((v, l))
        v, l = v[order], l[order]
    starts = np.searchsorted(l, np.arange(n_labels))
    n = np.bincount(l, minlength=n_labels)
    out = np.full((n_labels, len(qs)), np.nan)
    filled = n > 0
    for j, q in enumerate(qs):
        k = np.minimum(np.maximum(np.ceil(n * float(q) - 1).astype(np.int64), 0), n - 1)
        out[filled, j] = v[(starts + k)[filled]]
    return out


def quantile_of(values, vlab, n_labels, q):
    return quantiles_of(values, vlab, n_labels, [q])[:, 0]


def passes_for(ref, bins):
    """The smallest number of passes with ``bins ** passes`` at least the integer range of the reference."""
    ok = ref[~np.isnan(ref)]
    assert np.array_equal(ok, np.rint(ok)), "an integer case"
    span = int(ok.max() - ok.min()) + 1
    passes = 1
    while bins ** passes < span:
        passes += 1
    assert bins ** passes >= span
    return passes


def per_label_rows(ref, lab, n_labels, bins, np_type):
    """One edge row per label over the label's own integer range (``bins`` at least 2): from one above its minimum
    (its smallest voxels fall below) in integer steps that reach its maximum within ``bins - 1`` of them, then the
    maximum repeated up to ``bins + 1`` entries.  Every row ends in a repeated edge on which the label's largest voxel
    sits; a label without a voxel gets zeros."""
    assert bins >= 2
    lo, hi = lc.per_label(np.fmin, ref, lab, n_labels), lc.per_label(np.fmax, ref, lab, n_labels)
    rows = np.zeros((n_labels, bins + 1))
    for l in np.flatnonzero(~np.isnan(lo)):
        first = min(lo[l] + 1, hi[l])
        step = max(1, -(-int(hi[l] - first) // (bins - 1)))
        rows[l] = np.minimum(first + step * np.arange(bins + 1), hi[l])
        assert rows[l, -2] == rows[l, -1] == hi[l]
    return rows.astype(np_type)


# ------------------------------------------------------------------------------------------------ the exact bar
def exact_histogram(got, ref, lab, n_labels, edges, want=None):
    """``want``: ``hist_of(ref, lab, n_labels, edges)`` where the caller has it already."""
    want = hist_of(ref, lab, n_labels, edges) if want is None else want
    assert got["outside"] == want["outside"], ("outside", got["outside"], want["outside"])
    for key in KEYS:
        g = np.asarray(got[key])
        assert g.shape == want[key].shape and g.dtype == np.int64, (key, g.shape, g.dtype)
        bad = np.argwhere(g != want[key])
        assert bad.size == 0, (key, bad[:8].tolist())
    total = int(got["counts"].sum() + got["below"].sum() + got["above"].sum() + got["n_nan"].sum()) + got["outside"]
    assert total == ref.size, ("voxels accounted for", total, ref.size)


def exact_quantile(got, ref, lab, n_labels, q):
    """``got``: the dict of ``label_quantile`` for the scalar ``q``."""
    want = quantile_of(ref, lab, n_labels, q)
    for key in ("value", "lo", "hi"):
        g = np.asarray(got[key])
        assert g.shape == want.shape and g.dtype == np.float64, (key, g.shape, g.dtype)
        bad = np.flatnonzero(~((g == want) | (np.isnan(g) & np.isnan(want))))
        assert bad.size == 0, (key, q, bad[:8], g[bad[:8]], want[bad[:8]])
    inside = (lab >= 0) & (lab < n_labels)
    nan = np.isnan(ref)
    assert np.array_equal(got["count"], np.bincount(lab[inside & ~nan], minlength=n_labels)), "count"
    assert np.array_equal(got["n_nan"], np.bincount(lab[inside & nan], minlength=n_labels)), "n_nan"
    assert got["outside"] == int(ref.size - inside.sum()), "outside"


# ------------------------------------------------------------------------------------------------ the sandwich bar
def sandwich_histogram(got, ref, bound, lab, n_labels, edges, show=None):
    show = show or (lambda *a: None)
    inside = (lab >= 0) & (lab < n_labels)
    show("outside", got["outside"], int(ref.size - inside.sum()))
    assert got["outside"] == int(ref.size - inside.sum())
    total = int(got["counts"].sum() + got["below"].sum() + got["above"].sum() + got["n_nan"].sum()) + got["outside"]
    assert total == ref.size, ("voxels accounted for", total, ref.size)
    for l in range(n_labels):
        which = lab == l
        outliers = (int(got["below"][l]), int(got["above"][l]), int(got["n_nan"][l]))
        show("label", l, "voxels", int(which.sum()), "outliers", outliers)
        vc.sandwich_histogram(got["counts"][l], outliers, ref[which], bound[which], edges)


def sandwich_quantile(got, ref, bound, lab, n_labels, q, show=None):
    show = show or (lambda *a: None)
    for l in range(n_labels):
        which = lab == l
        n = int(which.sum())
        value, lo, hi = (float(got[key][l]) for key in ("value", "lo", "hi"))
        assert got["count"][l] == n and got["n_nan"][l] == 0
        if n == 0:
            assert np.isnan(value) and np.isnan(lo) and np.isnan(hi)
            continue
        k = min(max(int(np.ceil(n * q - 1)), 0), n - 1)
        least, most = np.sort(ref[which] - bound[which])[k], np.sort(ref[which] + bound[which])[k]
        show("label", l, "q", q, "value", value, "in", (lo, hi), "rank voxel in", (least, most))
        assert lo <= value <= hi and lo <= most and hi >= least, (l, q, value, lo, hi, least, most)


# ------------------------------------------------------------------------------------------------ modelled faults
# What a faulty kernel would return, computed from the reference.  None: the fault cannot occur on the case.
def same_result(a, b):
    return a.keys() == b.keys() and all(lc.same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _keep_all_but_first_tile(c):
    m, n = vc.last_product_shape(c.dims)
    keep = np.ones((m, n), dtype=bool)
    keep[:vc.TILE, :vc.TILE] = False
    return keep.reshape(-1)


def _padding(c):
    m, n = vc.last_product_shape(c.dims)
    return -(-m // vc.TILE) * vc.TILE * (-(-n // vc.TILE) * vc.TILE) - m * n


def _last_edge_of(vlab, n_labels, edges):
    """(the last edge, whether it repeats the one before) of every voxel's own row; voxels outside take row 0."""
    if edges.ndim == 1:
        return np.full(vlab.size, edges[-1]), np.full(vlab.size, bool(edges[-2] == edges[-1]))
    row = np.where((vlab >= 0) & (vlab < n_labels), vlab, 0)
    return edges[row, -1], edges[row, -2] == edges[row, -1]


def histogram_faults(c, ref, lab, n_labels, edges, window=None, found=None):
    """name -> faulty result dict, for every modelled fault that can occur on the case and differs from the truth.
    ``ref``: the case's reference or its NaN-planted variant (then the faults that need the site order are left out);
    ``window``: the labels of one launch (None: one launch takes all).  The place of a voxel depends on its value and
    its row alone, so with a shared row the places are found once and the faults that move labels only count again;
    ``found``: a dict that keeps those places between calls with the same ``ref`` and ``edges``."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.shape[-1] - 1
    shared = edges.ndim == 1
    found = {} if found is None else found
    if shared and "ref" not in found:
        found["ref"] = places(ref, edges)
        found["site"] = places(c.site, edges) if ref is c.ref else None
    at_ref = found["ref"] if shared else None

    def count(vlab, values=ref, at=at_ref):
        return cells_of(at, vlab, n_labels, bins) if shared else hist_of(values, vlab, n_labels, edges)

    truth = count(lab)
    outside = (lab < 0) | (lab >= n_labels)
    out = {}
    if ref is c.ref:
        at_site = found["site"] if shared else None
        out["site_order_labels"] = count(lab, c.site, at_site)  # the label read at the site-order address of a voxel
        keep = _keep_all_but_first_tile(c)  # the first 32 x 32 tile of the last product never reduced
        out["tile_left_out"] = count(lc._site_labels(c, lab)[keep], c.site[keep], at_site[keep] if shared else None)
        extra = _padding(c)
        if extra:  # every padded element of the tiles counted as a zero voxel of label 0
            zeros = np.zeros(extra)
            out["padding_counted"] = count(np.concatenate([lab, np.zeros(extra, dtype=np.int64)]), np.concatenate([ref, zeros]),
                                           np.concatenate([at_ref, places(zeros, edges)]) if shared else None)
    if window is not None and n_labels > window:  # label % window: every launch adds into the first window's cells
        out["windows_folded"] = count(np.where(outside, lab, lab % window))
    if not shared:  # row 0 for every label
        out["shared_row_used"] = hist_of(ref, lab, n_labels, edges[0])
    # what follows changes the place of some voxels
    at = at_ref if shared else np.zeros(ref.size, dtype=np.int64)
    if not shared:
        order, starts, filled = lc._segments(lab, n_labels)
        for l, a, b in zip(filled, starts, np.append(starts[1:], order.size)):
            at[order[a:b]] = places(ref[order[a:b]], edges[l])
    last, repeated = _last_edge_of(lab, n_labels, edges)
    on_last = (ref == last) & ~outside
    if on_last.any():  # the last bin open on the right: those voxels land in `above`
        out["last_bin_open"] = cells_of(np.where(on_last, bins + 1, at), lab, n_labels, bins)
    if (on_last & repeated).any():  # a search that stops at the first of the equal edges: an empty bin, the voxel lost
        gone = on_last & repeated
        out["padded_edge_lost"] = dict(cells_of(at[~gone], lab[~gone], n_labels, bins), outside=truth["outside"])
    if np.isnan(ref).any():  # NaN put into the first bin
        out["nan_in_a_bin"] = cells_of(np.where(np.isnan(ref), 0, at), lab, n_labels, bins)
    if outside.any():
        out["outside_to_first"] = count(np.where(outside, 0, lab))
        out["outside_to_last"] = count(np.where(outside, n_labels - 1, lab))
    return {k: v for k, v in out.items() if not same_result(v, truth)}


def quantile_results(values, vlab, n_labels, qs, n_total):
    """q -> the ``label_quantile`` dict a kernel exact to these voxels and labels returns."""
    table = quantiles_of(values, vlab, n_labels, qs)
    inside = (vlab >= 0) & (vlab < n_labels)
    nan = np.isnan(values)
    count = np.bincount(vlab[inside & ~nan], minlength=n_labels).astype(np.int64)
    n_nan = np.bincount(vlab[inside & nan], minlength=n_labels).astype(np.int64)
    return {q: dict(value=table[:, j].copy(), lo=table[:, j].copy(), hi=table[:, j].copy(), count=count, n_nan=n_nan,
                    outside=int(n_total - inside.sum())) for j, q in enumerate(qs)}


def quantile_truth(ref, lab, n_labels, qs):
    return quantile_results(ref, lab, n_labels, qs, ref.size)


def quantile_faults(c, lab, n_labels, qs, window=None):
    """name -> q -> the ``label_quantile`` dict of a faulty kernel (exact to its own wrong voxels), for the q where it
    differs from the truth."""
    truth = quantile_truth(c.ref, lab, n_labels, qs)
    outside = (lab < 0) | (lab >= n_labels)
    keep = _keep_all_but_first_tile(c)
    out = {
        "site_order_labels": quantile_results(c.site, lab, n_labels, qs, c.n),
        "tile_left_out": quantile_results(c.site[keep], lc._site_labels(c, lab)[keep], n_labels, qs, c.n),
    }
    if window is not None and n_labels > window:
        out["windows_folded"] = quantile_results(c.ref, np.where(outside, lab, lab % window), n_labels, qs, c.n)
    if outside.any():
        out["outside_to_first"] = quantile_results(c.ref, np.where(outside, 0, lab), n_labels, qs, c.n)
        out["outside_to_last"] = quantile_results(c.ref, np.where(outside, n_labels - 1, lab), n_labels, qs, c.n)
    out = {k: {q: r for q, r in v.items() if not same_result(r, truth[q])} for k, v in out.items()}
    return {k: v for k, v in out.items() if v}
