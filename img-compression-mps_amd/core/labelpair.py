"""Pair statistics per label of an atlas or segmentation, from the cores: two values per voxel, under a label.

The host side of csrc/labelpair.hip.  ``label_pair_stats`` takes the voxels of two chains of one shape (correlation,
mean difference and max |a - b| per parcel of two compressed volumes); ``label_error_to`` takes the voxels of one chain
and an original read at the voxel's address (the error of an encoding per region).  Both are one computation: the
moments pass of ``pair_stats`` over the same operands fixes six power-of-two scales on the device, then the labelled
pass adds 64-bit fixed-point integers per label, ``value = int 2^-scale``.  Integer addition has no order, so the same
inputs give the same bits; and a voxel is computed as ``label_stats`` computes it, so where neither volume has a NaN
``count, sum_a, sumsq_a, min_a, max_a`` and the exponents ``s_a, s2_a`` are ``label_stats``'s ``count, sum, sumsq, min,
max, s, s2`` on a bit for bit, and likewise for b.

A voxel with either value NaN is counted in ``n_nan`` of its label and takes no part in the rest; an infinite voxel in
either volume (or in the original) is refused.

``NDMPS.label_pair_stats`` / ``label_pair_stats_many`` / ``label_error_to`` are thin methods over the functions below.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _lib
from . import labelstat as _ls
from . import pairstat as _ps
from . import valstat as _vs

SCALES = ("s_a", "s2_a", "s_b", "s2_b", "s_ab", "s2_d")
COUNTS = ("count", "n_nan")
# the raw fields in the order of the library's outputs, each with its exponent (None: an extreme)
SUMS = (("sum_a", "s_a"), ("sum_b", "s_b"), ("sum_ab", "s_ab"))
SQUARES = (("sumsq_a", "s2_a"), ("sumsq_b", "s2_b"), ("sse", "s2_d"))
EXTREMES = ("min_a", "max_a", "min_b", "max_b", "max_abs_diff")
DERIVED = ("mean_a", "mean_b", "cov", "pearson", "mse", "rel_frob")
ARRAYS = COUNTS + tuple(k for k, _ in SUMS + SQUARES) + EXTREMES + DERIVED
ERROR_ARRAYS = ("count", "n_nan", "sse", "mse", "max_abs", "ref_sumsq", "ref_max", "rel_frob", "psnr")

_torch = _vs._torch


def workspace_bytes(a, b, n_labels):
    """Bytes of the one device buffer a call allocates: on the (checked) pair ``a, b``, or with ``b=None`` on ``a`` and
    an original."""
    np_type, _ = _vs._element(a)
    return int(_lib.load().ndmps_labelpair_workspace_bytes(a.L, _lib.i64_array(a.dims), _lib.i64_array(a.bonds),
                                                           None if b is None else _lib.i64_array(b.bonds),
                                                           np.dtype(np_type).itemsize, int(n_labels)))


def scales(maxabs_a, maxabs_b, max_abs_diff, numel):
    """The six exponents ``(s_a, s2_a, s_b, s2_b, s_ab, s2_d)`` of the scale rule (host only)."""
    out = (C.c_int * 6)()
    _lib.check(_lib.load().ndmps_labelpair_scales(float(maxabs_a), float(maxabs_b), float(max_abs_diff), int(numel), out))
    return tuple(int(v) for v in out)


def _raw_call(entry, head, lab, tables, n_cols, n_labels, tail):
    """One library call: the raw result arrays."""
    row_off, col_off, col_perm = tables
    n = n_labels
    sums, sumsq = np.zeros(3 * n, dtype=np.int64), np.zeros(3 * n, dtype=np.uint64)
    counts, ext = np.zeros(2 * n, dtype=np.int64), np.zeros(5 * n, dtype=np.float64)
    info, whole = np.zeros(8, dtype=np.int64), np.zeros(5, dtype=np.float64)
    _lib.check(entry(*head, lab.data_ptr(), lab.element_size(), row_off.data_ptr(), col_off.data_ptr(), col_perm.data_ptr(),
                     n_cols, n, sums.ctypes.data, sumsq.ctypes.data, counts.ctypes.data, ext.ctypes.data, info.ctypes.data,
                     whole.ctypes.data, *tail))
    return sums, sumsq, counts, ext, info, whole


def _raw_fields(sums, sumsq, counts, ext, info, whole):
    """count, n_nan, the six sums and the five extremes per label, ``outside``, ``scales`` and the extremes of the
    whole volume (``whole``), from the raw arrays.  A sum is ``math.ldexp(int, -scale)``: the integer rounded to fp64
    once (not at all below 2**53), then an exact scaling."""
    n = counts.size // 2
    exps = dict(zip(SCALES, (int(v) for v in info[1:7])))
    out = dict(count=counts[:n].copy(), n_nan=counts[n:].copy())
    for raw, fields in ((sums, SUMS), (sumsq, SQUARES)):
        for i, (key, scale) in enumerate(fields):
            out[key] = np.ldexp(raw[i * n:(i + 1) * n].astype(np.float64), -exps[scale])
    for i, key in enumerate(EXTREMES):
        out[key] = ext[i * n:(i + 1) * n].copy()
    out.update(outside=int(info[0]), scales=exps, whole=dict(zip(EXTREMES, (float(v) for v in whole))))
    return out


def derive(m):
    """``mean_a, mean_b, cov, pearson, mse, rel_frob`` per label by the formulas of ``pairstat.derive``, vectorised in
    fp64; NaN for a label without a counted voxel."""
    n = m["count"]
    filled = n > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_a, mean_b = m["sum_a"] / n, m["sum_b"] / n
        cov = m["sum_ab"] / n - mean_a * mean_b
        var_a = np.maximum(m["sumsq_a"] / n - mean_a * mean_a, 0.0)
        var_b = np.maximum(m["sumsq_b"] / n - mean_b * mean_b, 0.0)
        denom = np.sqrt(var_a * var_b)
        pearson = np.where(denom > 0, cov / denom, np.nan)
        mse = m["sse"] / n
        rel_frob = np.where(m["sumsq_b"] > 0, np.sqrt(m["sse"] / m["sumsq_b"]), np.where(m["sse"] == 0, 0.0, np.inf))
    nan = lambda v: np.where(filled, v, np.nan)  # noqa: E731
    return dict(mean_a=nan(mean_a), mean_b=nan(mean_b), cov=nan(cov), pearson=nan(pearson), mse=nan(mse),
                rel_frob=nan(rel_frob))


def _finish(raw):
    """The result dict of ``label_pair_stats`` for one frame."""
    m = _raw_fields(*raw)
    del m["whole"]
    m.update(derive(m))
    return m


def _same_site_dims(chains):
    for t, chain in enumerate(chains):
        _vs._element(chain)
        if list(chain.dims) != list(chains[0].dims) or chain.device != chains[0].device:
            raise ValueError(f"frame {t} differs from frame 0 in its site dims or its device")


def label_pair_stats_many(chains, ref, plan, labels, n_labels=None):
    """``label_pair_stats(chains[t], ref, ...)`` for every frame: the same dict with arrays of shape ``(T, n_labels)``, a
    vector of length T for ``outside`` and, under ``scales``, a vector of length T per exponent; row t is the single
    call bit for bit.  The label volume and the offset tables go to the device once, and one workspace, sized for the
    largest frame, serves every frame.  Frames share their site dims; bonds and element types may differ (each frame
    runs in the wider of its own and the reference's).  One synchronisation per frame."""
    torch = _torch()
    chains = list(chains)
    if not chains:
        raise ValueError("a series needs at least one frame")
    _same_site_dims(chains)
    pairs = [_ps.pair_chains(chain, ref) for chain in chains]
    labels, n_labels = _ls.check_labels(labels, plan.shape, n_labels)
    device = chains[0].device
    n_cols = _vs._split_columns(chains[0])
    with torch.cuda.device(device):
        lab = _ls._on_device(labels, device)
        tables = plan.split_tables(n_cols, device)
        ws = torch.empty(max(workspace_bytes(a, b, n_labels) for a, b in pairs), dtype=torch.uint8, device=device)
        frames = []
        for a, b in pairs:
            call = _vs._Call(a, other=b, ws=ws)
            frames.append(_finish(_raw_call(call.entry("labelpair"), call.head(), lab, tables, n_cols, n_labels, call.tail())))
    out = {key: np.stack([np.asarray(f[key]) for f in frames]) for key in frames[0] if key != "scales"}
    out["scales"] = {key: np.array([f["scales"][key] for f in frames], dtype=np.int64) for key in SCALES}
    return out


def label_pair_stats(a, b, plan, labels, n_labels=None):
    """Statistics of the voxel pairs (a, b) of two chains under each label of ``labels`` (as ``label_stats`` takes
    them), over the voxels where neither value is NaN.

    A dict of NumPy arrays of length ``n_labels``: ``count`` and ``n_nan`` (int64; voxels where either value is NaN),
    ``sum_a, sum_b, sumsq_a, sumsq_b, sum_ab, sse, max_abs_diff, min_a, max_a, min_b, max_b`` and the derived ``mean_a,
    mean_b, cov, pearson, mse, rel_frob`` (float64; a label without a counted voxel has sums 0 and NaN elsewhere), the
    scalar ``outside`` and ``scales``, a dict of the six exponents."""
    many = label_pair_stats_many([a], b, plan, labels, n_labels)
    out = {key: (value[0] if value.ndim == 2 else value[0].item()) for key, value in many.items() if key != "scales"}
    out["scales"] = {key: int(value[0]) for key, value in many["scales"].items()}
    return out


def psnr_per_label(peak, mse):
    """``valstat.psnr_from`` with one peak and every label's mse; NaN where the mse is."""
    return np.array([math.nan if math.isnan(v) else _vs.psnr_from(dict(mse=float(v), ref_max=peak)) for v in mse],
                    dtype=np.float64)


def label_error_to(chain, plan, x, labels, n_labels=None):
    """The error of the decoded volume against the original ``x`` under each label: ``label_pair_stats`` with
    ``b := x`` (NumPy array or device tensor of ``plan.shape``, cast to the chain's element type as ``error_to`` casts
    it), read at the address where the label is read.

    A dict of arrays of length ``n_labels``: ``count, n_nan, sse, mse, max_abs, ref_sumsq, ref_max, rel_frob, psnr``, and
    the scalars ``outside`` and ``peak``: the maximum of ``x`` over the voxels where neither value is NaN, labelled or
    not -- ``error_to(x)["ref_max"]``, the peak of ``psnr_to`` -- so that ``psnr[l]`` (``valstat.psnr_from`` with that
    peak and the label's mse) is comparable with the global figure."""
    torch = _torch()
    np_type, _ = _vs._element(chain)
    shape = tuple(int(s) for s in plan.shape)
    if tuple(int(s) for s in x.shape) != shape:
        raise ValueError(f"the original has shape {tuple(x.shape)}, the object {shape}")
    labels, n_labels = _ls.check_labels(labels, shape, n_labels)
    device = chain.device
    if isinstance(x, torch.Tensor):
        ref = x.to(device=device, dtype=chain.dtype).contiguous()
    else:
        ref = torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np_type, copy=False))).to(device)
    n_cols = _vs._split_columns(chain)
    with torch.cuda.device(device):
        lab = _ls._on_device(labels, device)
        tables = plan.split_tables(n_cols, device)
        call = _vs._Call(chain, ws_bytes=workspace_bytes(chain, None, n_labels))
        m = _raw_fields(*_raw_call(call.entry("labelpair_original"), (*call.head(), ref.data_ptr()), lab, tables, n_cols,
                                   n_labels, call.tail()))
    d = derive(m)
    peak = m["whole"]["max_b"]
    if math.isinf(peak):  # -inf: no voxel has both values, so there is nothing to compare
        peak = math.nan
    return dict(count=m["count"], n_nan=m["n_nan"], sse=m["sse"], mse=d["mse"], max_abs=m["max_abs_diff"],
                ref_sumsq=m["sumsq_b"], ref_max=m["max_b"], rel_frob=d["rel_frob"], psnr=psnr_per_label(peak, d["mse"]),
                outside=m["outside"], peak=peak)
