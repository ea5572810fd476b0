"""What every device layer shares, none of it aware of ``NDMPS``: the stage timer, the permutation plan of a tensor shape
and its cache, the DCT bases and theirs, the pointer table of a group-wide launch.  core/ndmps.py re-exports
``StageTimer``, ``set_stage_timer``, ``_plan_for`` and ``_dct_basis`` under these names for the benchmark and the tests."""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import numpy as np

from .. import _lib
from ..utils import core as _core
from .mps import _torch

_PLAN_CACHE = {}
_DCT_CACHE = {}


class StageTimer:
    """Optional per-stage device timing with HIP events on the stream the kernels run on
    (bench.py installs one with ``set_stage_timer``; ``None`` = no events recorded)."""

    def __init__(self):
        self.spans = []

    @contextlib.contextmanager
    def span(self, name):
        torch = _torch()
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        try:
            yield
        finally:
            stop.record()
            self.spans.append((name, start, stop))

    def totals_ms(self):
        """{stage: (total ms, count)}; synchronises the device."""
        _torch().cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            t, c = out.get(name, (0.0, 0))
            out[name] = (t + a.elapsed_time(b), c + 1)
        return out

    def reset(self):
        self.spans = []


_TIMER = None


def set_stage_timer(timer):
    global _TIMER
    _TIMER = timer


def _span(name):
    return _TIMER.span(name) if _TIMER is not None else contextlib.nullcontext()


class _Plan:
    """Permutation plan (device offset tables) for one tensor shape.  ``factor_arr`` (L, ndim): an explicit factor
    array whose columns multiply to the shape (the coarse chains of core/pool.py); ``get_factorlist(shape)`` if None."""

    def __init__(self, shape, reverse_sites=False, factor_arr=None):
        lib = _lib.load()
        self.shape = tuple(int(s) for s in shape)
        if factor_arr is None:
            self.factor_arr, _ = _core.get_factorlist(self.shape)
        else:
            self.factor_arr = np.array(factor_arr, dtype=np.int64)
        self.qubit_size = np.prod(self.factor_arr, axis=1)
        handle = C.c_void_p()
        fa = np.ascontiguousarray(self.factor_arr, dtype=np.int64)
        # reverse_sites: destination = the site-order tensor with its axes reversed (the mirrored chain a
        # left-to-right sweep is run on); qubit_size stays in the reference's order
        create = lib.ndmps_plan_create_reversed if reverse_sites else lib.ndmps_plan_create
        _lib.check(create(
            C.byref(handle), len(self.shape), _lib.i64_array(self.shape), fa.shape[0],
            fa.ctypes.data_as(_lib.p_i64)))
        self.handle = handle
        self.numel = int(np.prod(self.shape, dtype=np.int64))

        self._split = {}
        self._split_vec4 = {}
        self._sorted_rows = {}

    def split_tables(self, n_cols, device):
        """Device tables for the site-order tensor viewed as (numel / n_cols) x n_cols: element (r, c) sits at
        row_off[r] + col_off[c] of the C-order volume (offsets are additive over sites).  Returned with the
        columns in memory order: (row_off, col_off ascending, col_perm = site-order column of the c-th smallest
        offset), int64 / int64 / int32.  Built once per (n_cols, device), with synchronous uploads."""
        torch = _torch()
        key = (int(n_cols), str(device))
        with _CACHE_LOCK:
            if key not in self._split:
                rows = self.numel // int(n_cols)
                row_off = np.empty(rows, dtype=np.int64)
                col_off = np.empty(int(n_cols), dtype=np.int64)
                _lib.check(_lib.load().ndmps_plan_split_offsets(
                    self.handle, int(n_cols), row_off.ctypes.data_as(_lib.p_i64), col_off.ctypes.data_as(_lib.p_i64)))
                perm = np.argsort(col_off, kind="stable")
                col_sorted = np.ascontiguousarray(col_off[perm])
                # 16-byte gathers are possible when the sorted offsets come in aligned runs of four
                quads = col_sorted.reshape(-1, 4) if n_cols % 4 == 0 else None
                self._split_vec4[key] = bool(
                    quads is not None and np.all(quads[:, 0] % 4 == 0) and np.all(np.diff(quads, axis=1) == 1)
                    and np.all(row_off % 4 == 0))
                self._split[key] = (torch.from_numpy(row_off).to(device),
                                    torch.from_numpy(col_sorted).to(device),
                                    torch.from_numpy(perm.astype(np.int32)).to(device))
                torch.cuda.synchronize(device)
            return self._split[key]

    def sorted_rows(self, n_cols, device):
        """(split_tables' row offsets in ascending order, int64; the row each of them belongs to, int32): the order in
        which the Gram kernels and the streamed projection of the fused sweep visit the rows, so that they read the
        volume front to back.  Built once per (n_cols, device)."""
        torch = _torch()
        key = (int(n_cols), str(device))
        row_off = self.split_tables(n_cols, device)[0]
        with _CACHE_LOCK:
            if key not in self._sorted_rows:
                srt, order = torch.sort(row_off)
                self._sorted_rows[key] = (srt.contiguous(), order.to(torch.int32).contiguous())
                torch.cuda.synchronize(device)
            return self._sorted_rows[key]

    def gather_tables(self, n_cols, device):
        """split_tables when the volume can be read through them 16 bytes at a time, else None."""
        tables = self.split_tables(n_cols, device)
        return tables if self._split_vec4[(int(n_cols), str(device))] else None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().ndmps_plan_destroy(self.handle)
        except Exception:
            pass


_CACHE_LOCK = threading.Lock()  # concurrent groups (core/batch.py) reach the caches from several host threads


def _plan_for(shape, device_index, reverse_sites=False, factor_arr=None):
    key = (tuple(int(s) for s in shape), device_index) + (("reversed",) if reverse_sites else ())
    if factor_arr is not None:
        fa = np.asarray(factor_arr, dtype=np.int64)
        key = key + (("factors", fa.shape, tuple(int(v) for v in fa.ravel())),)
    with _CACHE_LOCK:
        if key not in _PLAN_CACHE:
            _PLAN_CACHE[key] = _Plan(shape, reverse_sites, factor_arr)  # plan tables are uploaded with synchronous copies
        return _PLAN_CACHE[key]


def _ptr_array(tensors):
    """Host array of the tensors' device pointers (the pointer tables of the library's group-wide launches)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _dct_basis(n, device, f64=False):
    torch = _torch()
    key = (int(n), str(device), bool(f64))
    with _CACHE_LOCK:
        if key not in _DCT_CACHE:
            basis = torch.empty((n, n), dtype=torch.float64 if f64 else torch.float32, device=device)
            fill = _lib.load().ndmps_dct_basis_f64 if f64 else _lib.load().ndmps_dct_basis_f32
            _lib.check(fill(basis.data_ptr(), n, _lib.stream_ptr()))
            # the basis is shared by every stream from now on: finish the fill before publishing it
            torch.cuda.current_stream().synchronize()
            _DCT_CACHE[key] = basis
        return _DCT_CACHE[key]


_POOL_DCT_CACHE = {}


def _pooled_dct_basis(n, block, op, device, f64=False):
    """(n / block, n) basis that turns DCT coefficient rows into block means (sums) of the voxels: y W^T."""
    torch = _torch()
    key = (int(n), int(block), op, str(device), bool(f64))
    with _CACHE_LOCK:
        if key not in _POOL_DCT_CACHE:
            basis = torch.empty((n // block, n), dtype=torch.float64 if f64 else torch.float32, device=device)
            fill = _lib.load().ndmps_pool_dct_basis_f64 if f64 else _lib.load().ndmps_pool_dct_basis_f32
            _lib.check(fill(basis.data_ptr(), n, block, 1.0 / block if op == "mean" else 1.0, _lib.stream_ptr()))
            torch.cuda.current_stream().synchronize()  # shared by every stream from now on
            _POOL_DCT_CACHE[key] = basis
        return _POOL_DCT_CACHE[key]
