"""Statistics per label of an atlas or segmentation, from the cores: count, mean, std, min and max of the voxels under
each label, and the (T, n_labels) table of a series (the parcel time courses), without decoding a volume.

The host side of the label epilogue of csrc/labelstat.hip.  The chain is contracted as ``value_stats`` contracts it; its
last product runs as the moments pass, whose extremes fix two power-of-two scales on the device, and then again over
the same operands with the label of every voxel read through the offset tables of the fused decode
(``_Plan.split_tables``), as ``error_to`` reads its original.  Sums are 64-bit fixed-point integers, ``sum = int 2^-s``
and ``sumsq = int 2^-s2``: integer addition has no order, so the same inputs give the same bits.  NaN voxels are
counted per label (``n_nan``) and take no part in the rest; an infinite voxel is refused.

``NDMPS.label_stats`` and ``NDMPS.label_stats_many`` are thin methods over the two functions below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from . import valstat as _vs

MAX_LABELS = 4096
LABEL_UPLOADS = 0  # label volumes moved or converted on the way to the kernels so far (a series counts one)

_AS_THEY_ARE = ("bool", "uint8", "int16", "int32")
_I32 = (-2 ** 31, 2 ** 31 - 1)


_torch = _vs._torch


def _type_name(labels):
    return str(labels.dtype).replace("torch.", "")


def check_labels(labels, shape, n_labels=None):
    """``(labels, n_labels)`` for a label volume of ``shape``: ``labels`` (NumPy array or tensor, left where it is) in
    uint8, int16 or int32, ``n_labels`` checked or, for None, ``max(labels) + 1`` (at least 1).  ValueError for another
    shape, labels beyond int32 or ``n_labels`` outside [1, 4096]; TypeError for labels that are not integers."""
    torch = _torch()
    is_tensor = isinstance(labels, torch.Tensor)
    if not is_tensor:
        labels = np.asarray(labels)
    shape = tuple(int(s) for s in shape)
    if tuple(int(s) for s in labels.shape) != shape:
        raise ValueError(f"the label volume has shape {tuple(labels.shape)}, the object {shape}")
    name = _type_name(labels)
    if not (name in _AS_THEY_ARE or name.startswith("int") or name.startswith("uint")):
        raise TypeError(f"labels must be integers (bool, uint8, int16, int32 or a type cast to int32), got {name}")
    empty = int(np.prod(shape, dtype=np.int64)) == 0
    top = None
    if name not in _AS_THEY_ARE:
        lo, top = (0, 0) if empty else (int(labels.min()), int(labels.max()))
        if lo < _I32[0] or top > _I32[1]:
            raise ValueError(f"labels of type {name} span [{lo}, {top}] and do not fit int32")
        labels = labels.to(torch.int32) if is_tensor else labels.astype(np.int32)
    elif name == "bool":
        labels = labels.view(torch.uint8) if is_tensor else labels.view(np.uint8)
    if n_labels is None:
        if top is None:
            top = 0 if empty else int(labels.max())
        n_labels = max(top + 1, 1)
    n_labels = int(n_labels)
    if n_labels > MAX_LABELS:
        raise ValueError(f"label statistics take at most {MAX_LABELS} labels, got {n_labels}: split the atlas")
    if n_labels < 1:
        raise ValueError(f"n_labels must be at least 1, got {n_labels}")
    return labels, n_labels


def _on_device(labels, device):
    """The checked label volume as a contiguous device tensor."""
    global LABEL_UPLOADS
    torch = _torch()
    LABEL_UPLOADS += 1
    if isinstance(labels, torch.Tensor):
        return labels.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(labels)).to(device)


def workspace_bytes(chain, n_labels):
    """Bytes of the one device buffer a call on ``chain`` with ``n_labels`` labels allocates."""
    np_type, _ = _vs._element(chain)
    return int(_lib.load().ndmps_labelstat_workspace_bytes(chain.L, _lib.i64_array(chain.dims), _lib.i64_array(chain.bonds),
                                                           np.dtype(np_type).itemsize, int(n_labels)))


def scales(maxabs, numel):
    """``(s, s2)`` of the scale rule for voxels of magnitude up to ``maxabs`` in a volume of ``numel`` (host only)."""
    s, s2 = C.c_int(), C.c_int()
    _lib.check(_lib.load().ndmps_labelstat_scales(float(maxabs), int(numel), C.byref(s), C.byref(s2)))
    return s.value, s2.value


def _one(chain, lab, tables, n_cols, n_labels, ws):
    """The library call on one chain: the raw result arrays."""
    call = _vs._Call(chain, ws=ws)
    row_off, col_off, col_perm = tables
    n = n_labels
    sums, sumsq = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint64)
    counts, minmax, info = np.zeros(2 * n, dtype=np.int64), np.zeros(2 * n, dtype=np.float64), np.zeros(4, dtype=np.int64)
    _lib.check(call.entry("labelstat")(*call.head(), lab.data_ptr(), lab.element_size(), row_off.data_ptr(),
                                       col_off.data_ptr(), col_perm.data_ptr(), n_cols, n, sums.ctypes.data, sumsq.ctypes.data,
                                       counts.ctypes.data, minmax.ctypes.data, info.ctypes.data, *call.tail()))
    return sums, sumsq, counts, minmax, info


def _finish(sums, sumsq, counts, minmax, info):
    """The result dict of one frame from the raw arrays."""
    n = sums.size
    s, s2 = int(info[1]), int(info[2])
    count, n_nan = counts[:n].copy(), counts[n:].copy()
    # math.ldexp(int, -s) per label: the integer rounded to fp64 once (not at all below 2**53), then an exact scaling
    total = np.ldexp(sums.astype(np.float64), -s)
    squares = np.ldexp(sumsq.astype(np.float64), -s2)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, total / count, np.nan)
        std = np.where(count > 0, np.sqrt(np.maximum(squares / count - mean * mean, 0.0)), np.nan)
    return dict(count=count, n_nan=n_nan, sum=total, sumsq=squares, min=minmax[:n].copy(), max=minmax[n:].copy(),
                mean=mean, std=std, outside=int(info[0]), s=s, s2=s2)


def label_stats_many(chains, plan, labels, n_labels=None):
    """``label_stats`` of every frame of a series: the same dict with arrays of shape ``(T, n_labels)`` and vectors of
    length T for ``outside``, ``s`` and ``s2``; row t is ``label_stats(chains[t], ...)`` bit for bit.  The label volume
    and the offset tables go to the device once, and one workspace, sized for the largest frame, serves every frame.
    Frames share their site dims; bonds and element types may differ (each frame runs in its own).  One
    synchronisation per frame."""
    torch = _torch()
    chains = list(chains)
    if not chains:
        raise ValueError("a series needs at least one frame")
    for t, chain in enumerate(chains):
        _vs._element(chain)
        if list(chain.dims) != list(chains[0].dims) or chain.device != chains[0].device:
            raise ValueError(f"frame {t} differs from frame 0 in its site dims or its device")
    labels, n_labels = check_labels(labels, plan.shape, n_labels)
    device = chains[0].device
    n_cols = _vs._split_columns(chains[0])
    with torch.cuda.device(device):
        lab = _on_device(labels, device)
        tables = plan.split_tables(n_cols, device)
        ws = torch.empty(max(workspace_bytes(chain, n_labels) for chain in chains), dtype=torch.uint8, device=device)
        frames = [_finish(*_one(chain, lab, tables, n_cols, n_labels, ws)) for chain in chains]
    return {key: np.stack([np.asarray(f[key]) for f in frames]) for key in frames[0]}


def label_stats(chain, plan, labels, n_labels=None):
    """Statistics of the decoded volume under each label of ``labels`` (NumPy array or device tensor of ``plan.shape``,
    C order; bool / uint8, int16 and int32 as they are, other integer types cast to int32 after a range check).

    A dict of NumPy arrays of length ``n_labels`` (None: ``max(labels) + 1``, at most 4096): ``count`` and ``n_nan``
    (int64), ``sum``, ``sumsq``, ``min``, ``max``, ``mean`` and ``std`` (float64; population std; NaN where ``count`` is
    0, with ``sum = sumsq = 0`` there), and the scalars ``outside`` (voxels whose label is negative or not below
    ``n_labels``), ``s`` and ``s2``.  The sums are ``math.ldexp`` of the exact integers: one rounding, and none while
    the integer is below 2**53."""
    many = label_stats_many([chain], plan, labels, n_labels)
    return {key: (value[0] if value.ndim == 2 else value[0].item()) for key, value in many.items()}
