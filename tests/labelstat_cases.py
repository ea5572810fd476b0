"""Cases, references and bars of the statistics per label from the cores (LabelEpi in csrc/labelstat.hip,
core/labelstat.py).

The chains, their fp64 references and their element bounds are those of tests/valstat_cases.py (``vc.Case``, imported
and not changed).  A label volume is built from ``c.shape`` and ``c.n`` alone, flat in C order.  Nothing here touches a
GPU: tests/test_labelstat_host.py runs the bars on the reference and on modelled faults, tests/test_gpu_labelstat.py
on what the kernels return.

Two bars, as there.

* exact, on integer cores: count, n_nan, sum, sumsq, min, max and outside equal NumPy's on the reference, bit for bit.
  The sums are ``int 2**-s`` of integers ``sum_V v 2**s``: with s >= 0 and s2 >= 0 (the host test asserts both for every
  integer case) every term is an integer, and the integer has the 53 or fewer significant bits of ``sum_V v``.
* sandwich, on real cores.  A computed voxel lies within its bound b of the reference, so with V the non-NaN voxels of
  a label and n_V their number: counts are exact; min_V(ref - b) <= min <= min_V(ref + b), and the same for max;
  a term of the sum is llrint(v 2**s), within 1/2 of v 2**s, the integer sum is exact and ``ldexp`` rounds it once:
      |sum - sum_V ref| <= sum_V b + n_V 2**-(s+1) + 2**-53 |sum|;
  a term of the squares is llrint(fl(v v) 2**s2) with fl(v v) within 2**-53 v v of v v (exact for fp32 voxels), and
  |v v - ref ref| <= 2 |ref| b + b b, v v <= (|ref| + b)**2:
      |sumsq - sum_V ref**2| <= sum_V (2 |ref| b + b**2) + n_V 2**-(s2+1) + 2**-52 sum_V (|ref| + b)**2.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import valstat_cases as vc

WINDOW = 1024  # labels of one launch
MAX_LABELS = 4096
KINDS = ("one", "blocks", "scatter", "outside", "empty", "window", "max")
REAL_KINDS = ("blocks", "scatter", "outside")
LARGE = ("int_wide", "int_8x7", "int_tail_last", "int_no_tail")  # the integer chains of at least 4096 voxels
FIELDS = ("count", "n_nan", "sum", "sumsq", "min", "max")


def kinds_for(name, n):
    """The label volumes a chain of ``n`` voxels is large enough for."""
    return [k for k in KINDS if (k != "window" or n >= 1030) and (k != "max" or name in LARGE)]


def labels(c, kind, seed=0):
    """``(flat int64 label volume in C order, n_labels)`` of a case."""
    n = c.n
    index = np.arange(n, dtype=np.int64)
    blocks = (index * 7) // n
    if kind == "one":
        return np.zeros(n, dtype=np.int64), 1
    if kind == "blocks":
        return blocks, 7
    if kind == "scatter":
        return np.random.default_rng(seed).integers(0, 7, n).astype(np.int64), 7
    if kind == "outside":
        lab = blocks.copy()
        lab[[0, n // 2]] = -1
        lab[n - 1] = 7
        return lab, 7
    if kind == "empty":
        return blocks, 9
    if kind == "window":
        return index % 1030, 1030
    if kind == "max":
        assert n >= MAX_LABELS
        return index % MAX_LABELS, MAX_LABELS
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ the scale rule
def exponent_above(x):
    """The smallest integer e with x < 2**e, for a positive float x, in exact rational arithmetic."""
    f = Fraction(x)
    e = f.numerator.bit_length() - f.denominator.bit_length()
    while f >= Fraction(2) ** e:
        e += 1
    while f < Fraction(2) ** (e - 1):
        e -= 1
    return e


def scale_rule(maxabs, numel):
    """(s, s2) in Python integers: nb = ceil(log2 numel), maxabs < 2**e, s = 61 - nb - e; e2 likewise from the fp64
    product maxabs * maxabs (2 e where that product is 0 or infinite); both clamped to [-1000, 1000]; maxabs = 0 gives
    (0, 0)."""
    if maxabs == 0:
        return 0, 0
    nb = (int(numel) - 1).bit_length()
    e = exponent_above(maxabs)
    sq = float(maxabs) * float(maxabs)
    e2 = exponent_above(sq) if 0 < sq < math.inf else 2 * e
    clamp = lambda v: max(-1000, min(1000, v))  # noqa: E731
    return clamp(61 - nb - e), clamp(61 - nb - e2)


def ref_scales(ref):
    ok = ref[~np.isnan(ref)]
    return scale_rule(float(np.abs(ok).max()) if ok.size else 0.0, ref.size)


# ------------------------------------------------------------------------------------------------ what NumPy says
def _segments(lab, n_labels):
    """(order, starts of the non-empty labels, which labels those are) of the voxels with a label in [0, n_labels)."""
    inside = np.flatnonzero((lab >= 0) & (lab < n_labels))
    order = inside[np.argsort(lab[inside], kind="stable")]
    edges = np.searchsorted(lab[order], np.arange(n_labels + 1))
    filled = np.flatnonzero(np.diff(edges) > 0)
    return order, edges[filled], filled


def per_label(ufunc, values, lab, n_labels):
    """``ufunc.reduceat`` (np.fmin / np.fmax: NaN takes no part) over the voxels of each label; NaN for an empty one."""
    order, starts, filled = _segments(lab, n_labels)
    out = np.full(n_labels, np.nan)
    if filled.size:
        with np.errstate(invalid="ignore"):
            out[filled] = ufunc.reduceat(values[order], starts)
    return out


def stats_of(values, lab, n_labels):
    """The dict of label statistics NumPy gives for parallel flat arrays of voxel values (fp64) and labels."""
    values, lab = np.asarray(values, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    inside = (lab >= 0) & (lab < n_labels)
    nan = np.isnan(values)
    ok, bad = inside & ~nan, inside & nan
    count = np.bincount(lab[ok], minlength=n_labels).astype(np.int64)
    return dict(count=count, n_nan=np.bincount(lab[bad], minlength=n_labels).astype(np.int64),
                sum=np.bincount(lab[ok], weights=values[ok], minlength=n_labels),
                sumsq=np.bincount(lab[ok], weights=values[ok] * values[ok], minlength=n_labels),
                min=per_label(np.fmin, values, lab, n_labels), max=per_label(np.fmax, values, lab, n_labels),
                outside=int(values.size - inside.sum()))


def ref_stats(ref, lab, n_labels):
    """The reference's statistics, with the scales the rule gives for it."""
    out = stats_of(ref, lab, n_labels)
    out["s"], out["s2"] = ref_scales(ref)
    return out


def fixed_point_sums(ref, lab, n_labels, s, s2):
    """(sum, sumsq) per label by the kernel's arithmetic in integers alone, for a reference of integers without NaN and
    s, s2 >= 0: v 2**s and v v 2**s2 added as int64 (nothing floating-point is summed), then ``math.ldexp``."""
    assert s >= 0 and s2 >= 0
    v = ref.astype(np.int64)
    assert np.array_equal(v, ref)
    order, starts, filled = _segments(lab, n_labels)
    q, q2 = np.zeros(n_labels, dtype=np.int64), np.zeros(n_labels, dtype=np.int64)
    if filled.size:
        q[filled] = np.add.reduceat(v[order] << s, starts)
        q2[filled] = np.add.reduceat((v[order] * v[order]) << s2, starts)
    return (np.array([math.ldexp(int(x), -s) for x in q]), np.array([math.ldexp(int(x), -s2) for x in q2]))


# ------------------------------------------------------------------------------------------------ the bars
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_dict(a, b):
    """Two result dicts agree bit for bit (NaN included)."""
    return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)


def exact_stats(got, ref, lab, n_labels):
    want = stats_of(ref, lab, n_labels)
    assert got["outside"] == want["outside"], ("outside", got["outside"], want["outside"])
    for key in FIELDS:
        g, w = np.asarray(got[key]), want[key]
        assert g.shape == w.shape, (key, g.shape)
        bad = np.flatnonzero(~((g == w) | (np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))))
        assert bad.size == 0, (key, bad[:8], g[bad[:8]], w[bad[:8]])
    assert int(got["count"].sum() + got["n_nan"].sum()) + got["outside"] == ref.size


def sandwich_stats(got, ref, bound, lab, n_labels, show=None):
    """The sandwich bar; ``show``: a function that is handed every figure before it is asserted."""
    show = show or (lambda *a: None)
    want = stats_of(ref, lab, n_labels)
    s, s2 = int(got["s"]), int(got["s2"])
    for key in ("count", "n_nan"):
        show(key, got[key], want[key])
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    show("outside", got["outside"], want["outside"])
    assert got["outside"] == want["outside"]
    n_v = want["count"].astype(np.float64)
    filled = want["count"] > 0
    for key, ufunc in (("min", np.fmin), ("max", np.fmax)):
        lo, hi = per_label(ufunc, ref - bound, lab, n_labels), per_label(ufunc, ref + bound, lab, n_labels)
        show(key, got[key], lo, hi)
        assert np.all(np.isnan(got[key][~filled])), (key, "an empty label has a value")
        assert np.all((lo[filled] <= got[key][filled]) & (got[key][filled] <= hi[filled])), (key, got[key], lo, hi)
    inside = (lab >= 0) & (lab < n_labels) & ~np.isnan(ref)
    which = lab[inside]
    r, b = ref[inside], bound[inside]
    over = lambda w: np.bincount(which, weights=w, minlength=n_labels)  # noqa: E731
    slack = over(b) + n_v * math.ldexp(1.0, -(s + 1)) + 2.0 ** -53 * np.abs(got["sum"])
    show("sum", got["sum"], want["sum"], slack)
    assert np.all(np.abs(got["sum"] - want["sum"]) <= slack), ("sum", got["sum"], want["sum"], slack)
    slack = over(2 * np.abs(r) * b + b * b) + n_v * math.ldexp(1.0, -(s2 + 1)) + 2.0 ** -52 * over((np.abs(r) + b) ** 2)
    show("sumsq", got["sumsq"], want["sumsq"], slack)
    assert np.all(np.abs(got["sumsq"] - want["sumsq"]) <= slack), ("sumsq", got["sumsq"], want["sumsq"], slack)


# ------------------------------------------------------------------------------------------------ modelled faults
# What a faulty kernel would return, computed from the reference (the scales are the reference's).  None: the fault
# cannot occur on the case.
def _site_labels(c, lab):
    """The label of every element of the site-order tensor: element i is the voxel inverse(dest)[i]."""
    inverse = np.empty(c.n, dtype=np.int64)
    inverse[c.dest] = np.arange(c.n, dtype=np.int64)
    return lab[inverse]


def _with_scales(c, stats):
    stats["s"], stats["s2"] = ref_scales(c.ref)
    return stats


def fault_site_order_labels(c, lab, n_labels):
    """The label read at the site-order address of a voxel instead of through the offset tables."""
    return _with_scales(c, stats_of(c.site, lab, n_labels))


def fault_tile_left_out(c, lab, n_labels):
    """The first 32 x 32 tile of the last product never reduced."""
    m, n = vc.last_product_shape(c.dims)
    keep = np.ones((m, n), dtype=bool)
    keep[:vc.TILE, :vc.TILE] = False
    keep = keep.reshape(-1)
    return _with_scales(c, stats_of(c.site[keep], _site_labels(c, lab)[keep], n_labels))


def fault_padding_counted(c, lab, n_labels):
    """Every padded row and column element of the 32 x 32 tiles counted as a zero voxel of label 0."""
    m, n = vc.last_product_shape(c.dims)
    extra = -(-m // vc.TILE) * vc.TILE * (-(-n // vc.TILE) * vc.TILE) - m * n
    if extra == 0:
        return None
    return _with_scales(c, stats_of(np.concatenate([c.ref, np.zeros(extra)]),
                                    np.concatenate([lab, np.zeros(extra, dtype=np.int64)]), n_labels))


def fault_run_not_flushed(c, lab, n_labels):
    """A held run never flushed at the end: the last row of every tile column is lost."""
    m, n = vc.last_product_shape(c.dims)
    keep = np.ones((m, n), dtype=bool)
    keep[m - 1, :] = False
    keep = keep.reshape(-1)
    return _with_scales(c, stats_of(c.site[keep], _site_labels(c, lab)[keep], n_labels))


def fault_windows_folded(c, lab, n_labels):
    """The labels of the later windows folded onto the first (label % 1024)."""
    if n_labels <= WINDOW:
        return None
    folded = np.where((lab >= 0) & (lab < n_labels), lab % WINDOW, lab)
    return _with_scales(c, stats_of(c.ref, folded, n_labels))


def fault_nan_counted(ref, lab, n_labels):
    """NaN voxels added into count (and not into n_nan); None without NaN under a label."""
    out = ref_stats(ref, lab, n_labels)
    if out["n_nan"].sum() == 0:
        return None
    out["count"] = out["count"] + out["n_nan"]
    out["n_nan"] = np.zeros_like(out["n_nan"])
    return out


def fault_outside_added(c, lab, n_labels, to):
    """The voxels with a label outside [0, n_labels) added to label ``to``; None when there are none."""
    outside = (lab < 0) | (lab >= n_labels)
    if not outside.any():
        return None
    return _with_scales(c, stats_of(c.ref, np.where(outside, to, lab), n_labels))


def faults(c, lab, n_labels):
    """name -> faulty result, for every modelled fault that can occur on the case and differs from the truth."""
    truth = ref_stats(c.ref, lab, n_labels)
    out = {
        "site_order_labels": fault_site_order_labels(c, lab, n_labels),
        "tile_left_out": fault_tile_left_out(c, lab, n_labels),
        "padding_counted": fault_padding_counted(c, lab, n_labels),
        "run_not_flushed": fault_run_not_flushed(c, lab, n_labels),
        "windows_folded": fault_windows_folded(c, lab, n_labels),
        "outside_to_first": fault_outside_added(c, lab, n_labels, 0),
        "outside_to_last": fault_outside_added(c, lab, n_labels, n_labels - 1),
    }
    return {k: v for k, v in out.items() if v is not None and not same_dict(v, truth)}
