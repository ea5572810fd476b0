"""Cases, references and bars of the pair statistics per label from the cores (LabelPairEpi in csrc/labelpair.hip,
core/labelpair.py).

The pairs, their fp64 references and their element bounds are those of tests/pairstat_cases.py (``pc.pair``, imported
and not changed); the label volumes are those of tests/labelstat_cases.py (``lc.labels``) on chain a.  One launch takes
WINDOW = 512 labels here, so the kind ``window`` (1030 labels) spans three launches and ``max`` (4096) eight.  Nothing
here touches a GPU: tests/test_labelpair_host.py runs the bars on the reference and on modelled faults,
tests/test_gpu_labelpair.py on what the kernels return.

Two bars.

* exact, on integer cores: every field equals NumPy's on the two references, bit for bit.  A sum is ``int 2**-scale`` of
  an integer ``sum_V term 2**scale``: with all six exponents >= 0 (the host test asserts it for every integer pair) every
  term is an integer, and the integer has the 53 or fewer significant bits of ``sum_V term``.
* sandwich, on real cores.  A computed voxel lies within its bound of its reference.  Counts and ``outside`` are exact;
  an extreme lies within [ext_V(ref - bound), ext_V(ref + bound)].  For a sum over the n_V counted voxels of a label
  the terms are within the slack ``pairstat_cases.sandwich_pair_stats`` derives for the field -- bound (first moments),
  2 |x| bound + bound**2 (squares), |a| bound_b + |b| bound_a + bound_a bound_b (products),
  2 |a - b| (bound_a + bound_b) + (bound_a + bound_b)**2 (squared differences) -- of the reference's; each term is
  rounded to an integer, within 1/2 of term 2**scale; the integer sum is exact and ``ldexp`` rounds it once:
      |sum - sum_V ref term| <= sum_V slack + n_V 2**-(scale+1) + roundings,
  where the roundings are 2**-53 |sum| for a first moment (the term itself is not rounded), 2**-52 sum_V of the largest
  possible term for a square or a product (one rounding of the fp64 product, one of the result) and 5 2**-53 of that
  for a squared difference (the difference, its square and the result: (1 + u)**4 - 1 < 5 u).
"""
from __future__ import annotations

import math

import numpy as np

import labelstat_cases as lc
import pairstat_cases as pc
import valstat_cases as vc

WINDOW = 512  # labels of one launch
SCALES = ("s_a", "s2_a", "s_b", "s2_b", "s_ab", "s2_d")
COUNTS = ("count", "n_nan")
SUMS = ("sum_a", "sum_b", "sumsq_a", "sumsq_b", "sum_ab", "sse")
EXTREMES = ("min_a", "max_a", "min_b", "max_b", "max_abs_diff")
FIELDS = COUNTS + SUMS + EXTREMES
SCALE_OF = dict(sum_a="s_a", sum_b="s_b", sumsq_a="s2_a", sumsq_b="s2_b", sum_ab="s_ab", sse="s2_d")


# ------------------------------------------------------------------------------------------------ the scale rule
def scale_rule(max_a, max_b, max_d, numel):
    """The six exponents in Python integers: (s_a, s2_a) and (s_b, s2_b) by ``labelstat_cases.scale_rule``; s2_d its
    second exponent for max |a - b|; s_ab = 61 - nb - e with max_a * max_b (the fp64 product) < 2**e, e_a + e_b where
    that product is 0 or infinite, clamped to [-1000, 1000]; 0 when either maximum is 0."""
    s_a, s2_a = lc.scale_rule(max_a, numel)
    s_b, s2_b = lc.scale_rule(max_b, numel)
    s2_d = lc.scale_rule(max_d, numel)[1]
    s_ab = 0
    if max_a > 0 and max_b > 0:
        nb = (int(numel) - 1).bit_length()
        p = float(max_a) * float(max_b)
        e = lc.exponent_above(p) if 0 < p < math.inf else lc.exponent_above(max_a) + lc.exponent_above(max_b)
        s_ab = max(-1000, min(1000, 61 - nb - e))
    return dict(s_a=s_a, s2_a=s2_a, s_b=s_b, s2_b=s2_b, s_ab=s_ab, s2_d=s2_d)


def ref_scales(ra, rb):
    ok = ~(np.isnan(ra) | np.isnan(rb))
    if not ok.any():
        return scale_rule(0.0, 0.0, 0.0, ra.size)
    a, b = ra[ok], rb[ok]
    return scale_rule(float(np.abs(a).max()), float(np.abs(b).max()), float(np.abs(a - b).max()), ra.size)


# ------------------------------------------------------------------------------------------------ what NumPy says
def stats_of(va, vb, lab, n_labels):
    """The dict of label pair statistics NumPy gives for parallel flat arrays of the two values (fp64) and labels."""
    va, vb, lab = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    inside = (lab >= 0) & (lab < n_labels)
    nan = np.isnan(va) | np.isnan(vb)
    ok, bad = inside & ~nan, inside & nan
    a, b, which = va[ok], vb[ok], lab[ok]
    d = a - b
    over = lambda w: np.bincount(which, weights=w, minlength=n_labels)  # noqa: E731
    ma, mb = np.where(nan, np.nan, va), np.where(nan, np.nan, vb)  # an extreme looks at the counted voxels only
    with np.errstate(invalid="ignore"):
        diff = np.abs(ma - mb)
    ext = per_label_many(((np.fmin, ma), (np.fmax, ma), (np.fmin, mb), (np.fmax, mb), (np.fmax, diff)), lab, n_labels)
    return dict(count=np.bincount(which, minlength=n_labels).astype(np.int64),
                n_nan=np.bincount(lab[bad], minlength=n_labels).astype(np.int64),
                sum_a=over(a), sum_b=over(b), sumsq_a=over(a * a), sumsq_b=over(b * b), sum_ab=over(a * b), sse=over(d * d),
                min_a=ext[0], max_a=ext[1], min_b=ext[2], max_b=ext[3], max_abs_diff=ext[4],
                outside=int(va.size - inside.sum()))


def per_label_many(pairs, lab, n_labels):
    """``labelstat_cases.per_label`` for several (ufunc, values) over one sort of the labels."""
    order, starts, filled = lc._segments(lab, n_labels)
    out = []
    for ufunc, values in pairs:
        r = np.full(n_labels, np.nan)
        if filled.size:
            with np.errstate(invalid="ignore"):
                r[filled] = ufunc.reduceat(values[order], starts)
        out.append(r)
    return out


def ref_stats(ra, rb, lab, n_labels):
    """The references' statistics, with the scales the rule gives for them."""
    out = stats_of(ra, rb, lab, n_labels)
    out["scales"] = ref_scales(ra, rb)
    return out


# ------------------------------------------------------------------------------------------------ the bars
def same_dict(a, b):
    """Two result dicts agree bit for bit (NaN included); ``scales`` entry by entry."""
    if a.keys() != b.keys():
        return False
    for k in a:
        if isinstance(a[k], dict):
            if a[k].keys() != b[k].keys() or any(not lc.same_bits(a[k][j], b[k][j]) for j in a[k]):
                return False
        elif not lc.same_bits(a[k], b[k]):
            return False
    return True


def exact_stats(got, ra, rb, lab, n_labels, want=None):
    """The exact bar; ``want``: ``stats_of`` the same arguments, where the caller has it already."""
    want = stats_of(ra, rb, lab, n_labels) if want is None else want
    assert got["outside"] == want["outside"], ("outside", got["outside"], want["outside"])
    for key in FIELDS:
        g, w = np.asarray(got[key]), want[key]
        assert g.shape == w.shape, (key, g.shape)
        bad = np.flatnonzero(~((g == w) | (np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))))
        assert bad.size == 0, (key, bad[:8], g[bad[:8]], w[bad[:8]])
    assert int(got["count"].sum() + got["n_nan"].sum()) + got["outside"] == ra.size


def sandwich_stats(got, ra, ba, rb, bb, lab, n_labels, show=None):
    """The sandwich bar; ``show``: a function that is handed every figure before it is asserted."""
    show = show or (lambda *a: None)
    want = stats_of(ra, rb, lab, n_labels)
    scales = {k: int(v) for k, v in got["scales"].items()}
    for key in COUNTS:
        show(key, got[key], want[key])
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    show("outside", got["outside"], want["outside"])
    assert got["outside"] == want["outside"]
    n_v = want["count"].astype(np.float64)
    filled = want["count"] > 0
    nan = np.isnan(ra) | np.isnan(rb)
    hide = lambda v: np.where(nan, np.nan, v)  # noqa: E731
    for x, ref, bound in (("a", ra, ba), ("b", rb, bb)):
        for key, ufunc in (("min_" + x, np.fmin), ("max_" + x, np.fmax)):
            lo = lc.per_label(ufunc, hide(ref - bound), lab, n_labels)
            hi = lc.per_label(ufunc, hide(ref + bound), lab, n_labels)
            show(key, got[key], lo, hi)
            assert np.all(np.isnan(got[key][~filled])), (key, "an empty label has a value")
            assert np.all((lo[filled] <= got[key][filled]) & (got[key][filled] <= hi[filled])), (key, got[key], lo, hi)
    with np.errstate(invalid="ignore"):
        dref, bd = np.abs(ra - rb), ba + bb
    lo = lc.per_label(np.fmax, hide(dref - bd), lab, n_labels)
    hi = lc.per_label(np.fmax, hide(dref + bd), lab, n_labels)
    key = "max_abs_diff"
    show(key, got[key], lo, hi)
    assert np.all(np.isnan(got[key][~filled])), (key, "an empty label has a value")
    g = got[key][filled]
    # the difference of the two computed voxels is rounded once
    assert np.all((lo[filled] - 2.0 ** -52 * hi[filled] <= g) & (g <= hi[filled] * (1 + 2.0 ** -52))), (key, got[key], lo, hi)

    inside = (lab >= 0) & (lab < n_labels) & ~nan
    which = lab[inside]
    a, b, ea, eb = np.abs(ra[inside]), np.abs(rb[inside]), ba[inside], bb[inside]
    d, ed = dref[inside], bd[inside]
    over = lambda w: np.bincount(which, weights=w, minlength=n_labels)  # noqa: E731
    half = lambda key: n_v * math.ldexp(1.0, -(scales[SCALE_OF[key]] + 1))  # noqa: E731
    slacks = dict(
        sum_a=over(ea) + half("sum_a") + 2.0 ** -53 * np.abs(got["sum_a"]),
        sum_b=over(eb) + half("sum_b") + 2.0 ** -53 * np.abs(got["sum_b"]),
        sumsq_a=over(2 * a * ea + ea * ea) + half("sumsq_a") + 2.0 ** -52 * over((a + ea) ** 2),
        sumsq_b=over(2 * b * eb + eb * eb) + half("sumsq_b") + 2.0 ** -52 * over((b + eb) ** 2),
        sum_ab=over(a * eb + b * ea + ea * eb) + half("sum_ab") + 2.0 ** -52 * over((a + ea) * (b + eb)),
        sse=over(2 * d * ed + ed * ed) + half("sse") + 5 * 2.0 ** -53 * over((d + ed) ** 2),
    )
    for key in SUMS:
        show(key, got[key], want[key], slacks[key])
        assert np.all(np.abs(got[key] - want[key]) <= slacks[key]), (key, got[key], want[key], slacks[key])


# ------------------------------------------------------------------------------------------------ modelled faults
# What a faulty kernel would return, computed from the references (the scales are the references').  None: the fault
# cannot occur on the case.
def _with_scales(p, stats):
    stats["scales"] = ref_scales(p.a.ref, p.b.ref)
    return stats


def _site_labels(p, lab):
    return lc._site_labels(p.a, lab)


def fault_site_order_labels(p, lab, n_labels):
    """The label read at the site-order address of a voxel instead of through the offset tables."""
    return _with_scales(p, stats_of(p.a.site, p.b.site, lab, n_labels))


def fault_site_order_original(p, lab, n_labels):
    """The second value (an original) read at the site-order address: a and the labels are right."""
    return _with_scales(p, stats_of(p.a.ref, p.b.site, lab, n_labels))


def fault_b_tile_shifted(p, lab, n_labels):
    """b's tile taken from the neighbouring tile index (``pc.fault_b_tile_shifted``)."""
    ra, rb = pc.fault_b_tile_shifted(p)
    return _with_scales(p, stats_of(ra, rb, lab, n_labels))


def fault_swapped(p, lab, n_labels):
    """a and b swapped."""
    return _with_scales(p, stats_of(p.b.ref, p.a.ref, lab, n_labels))


def _kept(p, lab, n_labels, keep):
    keep = keep.reshape(-1)
    return _with_scales(p, stats_of(p.a.site[keep], p.b.site[keep], _site_labels(p, lab)[keep], n_labels))


def fault_tile_left_out(p, lab, n_labels):
    """The first 32 x 32 tile of the last product never reduced."""
    keep = np.ones((p.m, p.cols), dtype=bool)
    keep[:vc.TILE, :vc.TILE] = False
    return _kept(p, lab, n_labels, keep)


def fault_padding_counted(p, lab, n_labels):
    """Every padded row and column element of the 32 x 32 tiles counted as a zero pair of label 0."""
    padded = pc.fault_padding_counted(p)
    if padded is None:
        return None
    extra = padded[0].size - p.n
    return _with_scales(p, stats_of(*padded, np.concatenate([lab, np.zeros(extra, dtype=np.int64)]), n_labels))


def fault_run_not_flushed(p, lab, n_labels):
    """A held run never flushed at the end: the last row of every tile column is lost."""
    keep = np.ones((p.m, p.cols), dtype=bool)
    keep[p.m - 1, :] = False
    return _kept(p, lab, n_labels, keep)


def fault_windows_folded(p, lab, n_labels):
    """The labels of the later windows folded onto the first (label % 512)."""
    if n_labels <= WINDOW:
        return None
    folded = np.where((lab >= 0) & (lab < n_labels), lab % WINDOW, lab)
    return _with_scales(p, stats_of(p.a.ref, p.b.ref, folded, n_labels))


def fault_nan_of_b_ignored(ra, rb_nan, lab, n_labels):
    """A kernel that looks for NaN in a only: the voxels where only b is NaN are counted (and not in n_nan).  None
    without such a voxel under a label."""
    out = ref_stats(ra, rb_nan, lab, n_labels)
    only_b = np.isnan(rb_nan) & ~np.isnan(ra) & (lab >= 0) & (lab < n_labels)
    if not only_b.any():
        return None
    moved = np.bincount(lab[only_b], minlength=n_labels)
    out["count"] = out["count"] + moved
    out["n_nan"] = out["n_nan"] - moved
    return out


def fault_outside_added(p, lab, n_labels, to):
    """The voxels with a label outside [0, n_labels) added to label ``to``; None when there are none."""
    outside = (lab < 0) | (lab >= n_labels)
    if not outside.any():
        return None
    return _with_scales(p, stats_of(p.a.ref, p.b.ref, np.where(outside, to, lab), n_labels))


def fault_sum_ab_scaled_with_s2_a(p, lab, n_labels):
    """sum_ab rounded with the exponent of sumsq_a and read back with its own; None where the two are equal."""
    out = ref_stats(p.a.ref, p.b.ref, lab, n_labels)
    shift = out["scales"]["s2_a"] - out["scales"]["s_ab"]
    if shift == 0:
        return None
    out["sum_ab"] = np.ldexp(out["sum_ab"], shift)
    return out


def faults(p, lab, n_labels):
    """name -> faulty result, for every modelled fault that can occur on the case and differs from the truth."""
    truth = ref_stats(p.a.ref, p.b.ref, lab, n_labels)
    out = {
        "site_order_labels": fault_site_order_labels(p, lab, n_labels),
        "site_order_original": fault_site_order_original(p, lab, n_labels),
        "b_tile_shifted": fault_b_tile_shifted(p, lab, n_labels),
        "swapped": fault_swapped(p, lab, n_labels),
        "tile_left_out": fault_tile_left_out(p, lab, n_labels),
        "padding_counted": fault_padding_counted(p, lab, n_labels),
        "run_not_flushed": fault_run_not_flushed(p, lab, n_labels),
        "windows_folded": fault_windows_folded(p, lab, n_labels),
        "outside_to_first": fault_outside_added(p, lab, n_labels, 0),
        "outside_to_last": fault_outside_added(p, lab, n_labels, n_labels - 1),
        "sum_ab_scaled_with_s2_a": fault_sum_ab_scaled_with_s2_a(p, lab, n_labels),
    }
    return {k: v for k, v in out.items() if v is not None and not same_dict(v, truth)}
