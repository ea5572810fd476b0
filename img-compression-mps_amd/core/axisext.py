"""Extremes of the volume a chain decodes to along axes, and where they sit, from the cores.

The host side of the two extreme epilogues of csrc/axisext.hip (``ndmps_axisext_*``, ``ndmps_argext_*``): the chain is
contracted as ``to_tensor`` contracts it, and the last product -- the only one that touches N elements -- sends every
voxel to the cell of the projected array it belongs to instead of storing it.  ``NDMPS.amax`` / ``amin`` / ``argmax`` /
``argmin`` are thin methods over ``extreme`` and ``arg_extreme`` below.

The planner.  ``_Plan.split_tables`` gives the additive tables ``offset = row_off[r] + col_off[c]`` of the last product
in the C-order volume.  The digits of the rows and of the columns are disjoint, so the coordinates of an offset are
additive as well (no carry), and so is every linear function of them: the offset into the array that is left when some
axes are dropped, ``row_out[r] + col_out[c]``, and the coordinate along one axis, ``row_idx[r] + col_idx[c]``.
``host_tables`` builds those with NumPy and orders the columns by ``(col_out, col_idx)``, so that the columns which
share an output cell are adjacent (the kernel folds adjacent lanes before its atomic) and ascend in their coordinate.

NaN voxels take no part: values are those of ``np.fmax.reduce`` / ``np.fmin.reduce``, a ray of NaN only gives NaN and
index -1.  Ties go to the smallest index, -0.0 and +0.0 compare equal.  The same inputs give the same bits.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref

import numpy as np

from .. import _lib
from . import valstat as _vs
from .pool import normalize_axes

OPS = {"max": 0, "min": 1}

_TABLES = weakref.WeakKeyDictionary()  # plan -> {(axes, n_cols, device): Tables}
_LOCK = threading.Lock()


_torch = _vs._torch


class Tables:
    """The tables of one projection: ``row_out`` / ``col_out`` (int64), ``col_perm`` (int32, the site-order column of
    the c-th entry of the column tables), ``row_idx`` / ``col_idx`` (int32, a single reduced axis only, else None) and
    ``out_shape``, the shape without the reduced axes."""

    def __init__(self, row_out, col_out, col_perm, row_idx, col_idx, out_shape):
        self.row_out, self.col_out, self.col_perm = row_out, col_out, col_perm
        self.row_idx, self.col_idx, self.out_shape = row_idx, col_idx, tuple(int(s) for s in out_shape)
        self.out_numel = int(np.prod(self.out_shape, dtype=np.int64))


def host_tables(row_off, col_off, col_perm, shape, axes):
    """``Tables`` of NumPy arrays from the host copies of ``split_tables`` (``col_off`` in the order ``col_perm``) for
    the object's ``shape`` and the sorted reduced ``axes`` (not all of them)."""
    shape = tuple(int(s) for s in shape)
    axes = tuple(int(a) for a in axes)
    kept = [a for a in range(len(shape)) if a not in axes]
    if not kept or not axes:
        raise ValueError("a projection reduces some axes and keeps some")
    out_shape = tuple(shape[a] for a in kept)
    rows = np.unravel_index(np.asarray(row_off, dtype=np.int64), shape)
    cols = np.unravel_index(np.asarray(col_off, dtype=np.int64), shape)
    row_out = np.ravel_multi_index([rows[a] for a in kept], out_shape).astype(np.int64)
    col_out = np.ravel_multi_index([cols[a] for a in kept], out_shape).astype(np.int64)
    if len(axes) == 1:
        row_idx, col_idx = rows[axes[0]].astype(np.int32), cols[axes[0]].astype(np.int32)
        order = np.lexsort((col_idx, col_out))
        col_idx = np.ascontiguousarray(col_idx[order])
    else:
        row_idx = col_idx = None
        order = np.argsort(col_out, kind="stable")
    return Tables(np.ascontiguousarray(row_out), np.ascontiguousarray(col_out[order]),
                  np.ascontiguousarray(np.asarray(col_perm)[order].astype(np.int32)), row_idx, col_idx, out_shape)


def tables(plan, n_cols, axes, device):
    """``host_tables`` of ``plan.split_tables(n_cols, device)`` on ``device``; built once per (plan, axes, n_cols,
    device), with synchronous uploads."""
    torch = _torch()
    axes = tuple(int(a) for a in axes)
    key = (axes, int(n_cols), str(device))
    row_off, col_off, col_perm = plan.split_tables(n_cols, device)
    with _LOCK:
        per_plan = _TABLES.setdefault(plan, {})
        if key not in per_plan:
            t = host_tables(row_off.cpu().numpy(), col_off.cpu().numpy(), col_perm.cpu().numpy(), plan.shape, axes)
            up = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
            per_plan[key] = Tables(up(t.row_out), up(t.col_out), up(t.col_perm), up(t.row_idx), up(t.col_idx), t.out_shape)
            torch.cuda.synchronize(device)
        return per_plan[key]


def _ptr(t):
    return None if t is None else t.data_ptr()


def extreme(chain, plan, axes, op, index=False):
    """The extreme (``op``: "max" or "min") over the sorted ``axes`` (not all of them) of the volume ``chain`` decodes
    to: a device tensor of the kept shape in the chain's element type, and with ``index`` (one axis only) also the
    int64 tensor of the smallest coordinate along that axis at which the extreme sits."""
    torch = _torch()
    axes = tuple(int(a) for a in axes)
    if index and len(axes) != 1:
        raise TypeError("the index of an extreme is taken along one axis")
    device = chain.device
    n_cols = _vs._split_columns(chain)
    with torch.cuda.device(device):
        t = tables(plan, n_cols, axes, device)
        call = _vs._Call(chain)
        values = torch.empty(t.out_shape, dtype=chain.dtype, device=device)
        where = torch.empty(t.out_shape, dtype=torch.int64, device=device) if index else None
        _lib.check(call.entry("axisext")(*call.head(), OPS[op], t.row_out.data_ptr(), t.col_out.data_ptr(),
                                         t.col_perm.data_ptr(), n_cols, _ptr(t.row_idx) if index else None,
                                         _ptr(t.col_idx) if index else None, t.out_numel, values.data_ptr(), _ptr(where),
                                         *call.tail()))
    return values, where


def arg_extreme(chain, plan, op):
    """``(value, flat C-order index)`` of the extreme of the whole volume: a float and an int, the smallest index on
    ties; ``(nan, -1)`` for a volume of NaN only."""
    torch = _torch()
    device = chain.device
    n_cols = _vs._split_columns(chain)
    with torch.cuda.device(device):
        row_off, col_off, col_perm = plan.split_tables(n_cols, device)
        call = _vs._Call(chain)
        value, flat = C.c_double(), C.c_int64()
        _lib.check(call.entry("argext")(*call.head(), OPS[op], row_off.data_ptr(), col_off.data_ptr(), col_perm.data_ptr(),
                                        n_cols, C.byref(value), C.byref(flat), *call.tail()))
    return float(value.value), int(flat.value)


# ------------------------------------------------------------------------------------------------ NumPy's interface
def _out(t, as_torch):
    return t if as_torch else t.cpu().numpy()


def _full(value, shape, dtype, chain, as_torch):
    """A scalar result with ``keepdims``: an array of ones in every axis."""
    torch = _torch()
    if as_torch:
        return torch.full(shape, value, dtype=dtype, device=chain.device)
    return np.full(shape, value, dtype=np.int64 if dtype == torch.int64 else _vs._element(chain)[0])


def reduce_values(chain, plan, op, axis=None, keepdims=False, as_torch=False):
    """``volume.max(axis, keepdims=keepdims)`` (``op`` "max") or ``.min``: an int or a tuple of ints, negative values
    from the end.  None or every axis: the scalar of ``value_stats`` (a float).  TypeError for a non-integer axis,
    numpy's AxisError out of range, ValueError for a repeated axis."""
    shape = tuple(int(s) for s in plan.shape)
    axes = normalize_axes(axis, len(shape))
    if len(axes) == len(shape):
        value = _vs.value_stats(chain)[op]
        return _full(value, (1,) * len(shape), chain.dtype, chain, as_torch) if keepdims else value
    values, _ = extreme(chain, plan, axes, op)
    if keepdims:
        values = values.reshape([1 if a in axes else n for a, n in enumerate(shape)])
    return _out(values, as_torch)


def reduce_index(chain, plan, op, axis=None, keepdims=False, as_torch=False, return_values=False):
    """``np.argmax(volume, axis, keepdims=keepdims)`` (``op`` "max") or ``argmin``, first occurrence on ties; with
    ``return_values`` the pair ``(indices, values)`` from the same call.  ``axis=None``: the flat C-order index as an
    int (and the value as a float).  A tuple raises TypeError, as NumPy's does."""
    torch = _torch()
    shape = tuple(int(s) for s in plan.shape)
    if axis is None:
        value, flat = arg_extreme(chain, plan, op)
        if keepdims:
            ones = (1,) * len(shape)
            flat, value = _full(flat, ones, torch.int64, chain, as_torch), _full(value, ones, chain.dtype, chain, as_torch)
        return (flat, value) if return_values else flat
    if isinstance(axis, tuple):
        raise TypeError("'tuple' object cannot be interpreted as an integer")
    axes = normalize_axes(axis, len(shape))
    if len(shape) == 1:  # the one axis of a one-dimensional volume: the flat index, as a zero-dimensional result
        value, flat = arg_extreme(chain, plan, op)
        ones = (1,) if keepdims else ()
        flat, value = _full(flat, ones, torch.int64, chain, as_torch), _full(value, ones, chain.dtype, chain, as_torch)
        return (flat, value) if return_values else flat
    values, where = extreme(chain, plan, axes, op, index=True)
    if keepdims:
        kept = [1 if a in axes else n for a, n in enumerate(shape)]
        values, where = values.reshape(kept), where.reshape(kept)
    return (_out(where, as_torch), _out(values, as_torch)) if return_values else _out(where, as_torch)
