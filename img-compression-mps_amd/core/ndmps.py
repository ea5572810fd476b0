"""``NDMPS``: N-dimensional tensors stored and compressed as matrix-product states, on MI355X.

Drop-in for the reference class ``imgcompressionmps.core.ndmps.NDMPS``
(src/imgcompressionmps/core/ndmps.py:11-277): same constructor, same public methods with the
same argument meaning and the same exceptions.  What differs is where the work happens:

* ``from_tensor`` (ndmps.py:36-78): norm -> last-axis DCT -> index permutation -> right-to-left
  SVD sweep all run as HIP kernels on device-resident fp32 data; the encoding map of the
  reference (8 L bytes per voxel) is never built, only small offset tables.
* ``compress`` (ndmps.py:94-108): per-bond truncated SVD of the two-site product with sqrt(s)
  absorbed on both sides (quimb's ``tensor_compress_bond`` semantics), fp64 on the small side.
* ``to_tensor`` (ndmps.py:131-153): left-to-right GEMM chain on the matrix cores, inverse
  permutation, inverse DCT.

Additions the reference lacks (BASELINE.json / SURVEY F3): ``max_bond`` (bond cap chi, applied
inside the encode sweep and in ``compress``), ``cutoff`` on ``from_tensor`` (default 1e-10 as
quimb's ``from_dense``; the fp32 path cannot resolve below 1e-6 and clamps there) and
``device``.  Arithmetic is fp32 in HBM with fp64 Gram / eigen / overlap accumulation; the
reference is fp64 end to end (ndmps.py:56).
"""
from __future__ import annotations

import ctypes as C
import gzip
import io
import math
import numbers
import os
import threading
import weakref

import numpy as np

from .. import _lib
from ..utils import core as _core
from ..utils import filetools as _ft
from . import axisop as _ax
from . import hadamard as _hd
from . import lincomb as _lc
from . import oncore as _oc
from . import pool as _pool
from . import readout as _ro
from . import region as _region
from . import series as _se
from . import sumsketch as _ss
from . import wgram as _wg
from .mps import DeviceMPS, _torch
from .plan import StageTimer, _dct_basis, _plan_for, _ptr_array, _span, set_stage_timer  # noqa: F401  (re-exported)


# ------------------------------------------------------------------------------------------------ on the cores
def _check_result_dtype(dtype):
    """The ``dtype`` argument of the operations on the cores: None or one of the three storage types."""
    torch = _torch()
    if dtype is not None and dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise ValueError("dtype must be None, torch.float32, torch.bfloat16 or torch.float64")


def _check_compatible(objs):
    """``lincomb.check_compatible`` over NDMPS objects: same qubit_size, shape, mode, device and site dims."""
    _lc.check_compatible([dict(qubit_size=o.qubit_size, shape=o._shape, mode=o.mode, device=o.mps.device,
                               dims=o.mps.dims) for o in objs])


def _checked_list(objs, phrase):
    """``objs`` as a list; TypeError ("<phrase> NDMPS objects, not ...") for an element that is no NDMPS."""
    objs = list(objs)
    for o in objs:
        if not isinstance(o, NDMPS):
            raise TypeError(f"{phrase} NDMPS objects, not {type(o).__name__}")
    return objs


def _work_is_f64(objs, dtype=None):
    """``lincomb.work_is_f64`` over NDMPS objects and the ``dtype`` argument of the call."""
    return _lc.work_is_f64([_lc.dtype_code(o.mps.dtype) for o in objs], dtype)


def _bf16_std(objs):
    """``readout.as_result``'s flag: every object has bf16 cores and the mode is Std (as_torch then gives bf16)."""
    bf16 = _torch().bfloat16
    return objs[0].mps.dtype == bf16 and objs[0].mode == "Std" and all(o.mps.dtype == bf16 for o in objs)


class _GroupState:
    """min / max of every core and the norm of every volume of a lockstep group, ISSUED with the sweep (one
    launch over the group's arena) and COLLECTED when the first object is asked for boundary_list / norm_value:
    the reference computes them inside from_tensor (ndmps.py:75-76); here nothing on the device is skipped, only
    the copy back to the host waits until somebody wants the numbers."""

    def __init__(self, objs, partial, count, n_cores, stream):
        self.refs = [weakref.ref(o) for o in objs]
        self.partial, self.count, self.n_cores, self.stream = partial, count, n_cores, stream
        self.device = partial.device
        self.done = False
        self._lock = threading.Lock()

    def resolve(self):
        # one collector at a time (the ctypes call releases the GIL): a second reader waits here and finds the values
        # stored; `done` is set only once they are, and a failing collect leaves the state unresolved for the next try
        with self._lock:
            if self.done:
                return
            self._collect()
            self.done = True

    def _collect(self):
        lib = _lib.load()
        out = (C.c_float * (2 * self.count))()
        ss = (C.c_double * self.count)()
        with _torch().cuda.device(self.device):  # the stream handle belongs to this device
            _lib.check(lib.ndmps_minmax_collect(self.count, self.partial.data_ptr(), out, ss, self.stream))
        mm = np.frombuffer(out, dtype=np.float32).astype(np.float64).reshape(-1, self.n_cores, 2)
        ssn = np.frombuffer(ss, dtype=np.float64)
        for b, ref in enumerate(self.refs):
            o = ref()
            if o is None or o.__dict__.get("_state_group") is not self:
                continue
            d = o.__dict__
            d["_state_group"] = None
            # attributes set explicitly in the meantime (update_*, compress, a caller) win
            if not d.pop("_boundary_set", False):
                d["_boundary_list"] = mm[b].copy()
            if not d.pop("_norm_set", False):
                # sites 1..L-1 are right-isometric after the sweep: mps @ mps = ||site 0||_F^2 (~1e-7 relative)
                d["_norm_value"] = np.sqrt(ssn[b * self.n_cores])
        self.partial = None


class PendingGroup:
    """A lockstep group whose sweep and decode are ENQUEUED (``NDMPS.from_tensors_begin``): ``result()`` returns what
    ``NDMPS.from_tensors`` returns.  Between the two the host thread is free -- ``core/batch.py`` enqueues the next batch
    before it asks for this one's objects, so their construction runs under the next batch's kernels instead of in
    front of them.  ``asynchronous`` is False when the group had to be encoded synchronously after all (storage types and
    shapes whose sweep decides ranks on the host): ``result()`` then only builds the objects."""

    def __init__(self, finish, asynchronous=False, redo=None, wait=None, arena=None):
        self._finish, self._redo, self._value, self._wait, self._arena = finish, redo, None, wait, arena
        self.asynchronous = bool(asynchronous)

    def arena_cores(self):
        """Before ``result()``: [volume][site] views of the group's arena in the shape the sweep wrote them -- for a sweep
        with device-side ranks the cap shape ``(cap_i, d_i, cap_{i+1})``, zeros beyond the ranks -- in the order of the
        swept chain; ``None`` once ``result()`` has been called or when the cores are compact.  For tests of the layout:
        the objects of ``result()`` hold the cores cut at their ranks."""
        return None if self._arena is None else self._arena()

    def __del__(self):
        # dropped without result(): the copies of ranks and spectra into this group's pinned buffers may still be in
        # flight -- wait for them before the buffers go back to the host allocator
        if self._value is None and self._wait is not None:
            try:
                self._wait()
            except Exception:
                pass

    def result(self):
        if self._value is None:
            try:
                value = self._finish()
            except _lib.NdmpsTeamAbort:
                # a resident tridiagonalisation gave up (the GPU is shared): the inputs are intact, the group is encoded
                # again through the synchronous call, which falls back to the per-column launches by itself
                if self._redo is None:
                    raise
                value = self._redo()
            self._value = (value,)
            self._finish = self._redo = self._wait = self._arena = None
        return self._value[0]


def _stage_inputs(tensors, device, store, norm):
    """The group's volumes on ``device`` in the storage type ``store`` (inputs are never mutated), and their shape."""
    torch = _torch()
    xs = []
    for tensor in tensors:
        if isinstance(tensor, torch.Tensor):
            if tensor.dim() == 0:
                raise ValueError("Shape cannot be empty.")
            # the volume is only written to when it is normalised in place: copy then, otherwise
            # a volume already resident on the device in the storage type is read where it lies
            if tensor.dtype == store and tensor.device == device and tensor.is_contiguous() and not tensor.requires_grad:
                x = tensor  # resident in the storage type already: read where it lies
            else:
                x = tensor.detach().to(device=device, dtype=store).contiguous()
            if norm and x.data_ptr() == tensor.data_ptr():
                x = x.clone()
        else:
            arr = np.asarray(tensor)
            if arr.ndim == 0:
                raise ValueError("Shape cannot be empty.")
            if arr.dtype.kind not in "fiub":
                raise TypeError(f"unsupported tensor dtype {arr.dtype}")
            host_type = np.float64 if store == torch.float64 else np.float32
            x = torch.from_numpy(np.ascontiguousarray(arr, dtype=host_type)).to(device).to(store)
        xs.append(x)
    shape = tuple(int(v) for v in xs[0].shape)
    if any(tuple(x.shape) != shape for x in xs):
        raise ValueError("from_tensors needs tensors of one shape; encode other shapes separately")
    return xs, shape


def _normalise_and_transform(xs, shape, norm, mode, store, device):
    """Norm (ndmps.py:60-61) and last-axis DCT (ndmps.py:62-63) of a group's staged volumes, on the current stream;
    returns them in the storage type."""
    torch = _torch()
    lib = _lib.load()
    stream = _lib.stream_ptr()
    f64 = store == torch.float64
    batch, numel = len(xs), xs[0].numel()
    if (norm or mode == "DCT") and store == torch.bfloat16:
        xs = [x.to(torch.float32) for x in xs]  # the norm / DCT kernels are fp32; rounded back to bf16 below
    if norm:
        # the norms of the whole group from ONE launch and one synchronisation (the reference divides volume by
        # volume, ndmps.py:60-61; a sum-of-squares call per volume was a host round trip per volume)
        _, sumsqs = _ft.minmax_many(xs, with_sumsq=True)
        if f64:
            for x, ss in zip(xs, sumsqs):
                _lib.check(lib.ndmps_scale_f64(x.data_ptr(), numel, 1.0 / float(np.sqrt(ss)), stream))
        else:  # one launch for the group (the reference divides volume by volume, ndmps.py:60-61)
            _lib.check(lib.ndmps_scale_many_f32(batch, _ptr_array(xs), numel,
                                                _lib.f64_array([1.0 / float(np.sqrt(ss)) for ss in sumsqs]), stream))
    if mode == "DCT":
        n = shape[-1]
        ys = list(torch.empty((batch,) + shape, dtype=xs[0].dtype, device=device).unbind(0))
        if f64:
            for x, y in zip(xs, ys):
                _lib.check(lib.ndmps_dct_last_f64(x.data_ptr(), y.data_ptr(), numel // n, n,
                                                  _dct_basis(n, device, True).data_ptr(), stream))
        else:  # one launch for the group (ndmps.py:62-63 per volume)
            _lib.check(lib.ndmps_dct_last_many_f32(batch, _ptr_array(xs), _ptr_array(ys), numel // n, n,
                                                   _dct_basis(n, device).data_ptr(), stream))
        xs = ys
    return [x.to(store) for x in xs]


class _SweptGroup:
    """One lockstep group from the reshape stage to its objects.  The stages (reshape_stage, launch_sweep,
    decode_from_arena, mark_enqueued) run on the group's device and stream and leave here, by name, everything the second
    half needs: the arena the cores lie in, the host buffers of ranks and spectra -- for a sweep with device-side ranks
    the pinned buffers they are copied into and the event behind those copies -- the layout (caps, offsets) and the
    reconstructions.  ``finish()`` is that second half: ranks and spectra to the host, objects, state launch; a
    ``PendingGroup`` (from_tensors_begin) holds this object and nothing else of the encode."""

    def __init__(self, cls, batch, shape, device, store, norm, mode, max_bond, mirrored, reconstruct):
        torch = _torch()
        lib = _lib.load()
        self.cls, self.batch, self.shape, self.device, self.store = cls, batch, shape, device, store
        self.norm, self.mode, self.mirrored, self.reconstruct = norm, mode, mirrored, reconstruct
        self.bf16, self.f64 = store == torch.bfloat16, store == torch.float64
        self.esize = 2 if self.bf16 else (8 if self.f64 else 4)
        self.ref_plan = _plan_for(shape, device.index)  # the reference's site order (qubit_size, decode)
        # mirrored (sweep_from="left"): the sweep runs on the chain read backwards -- the reshape stage writes the
        # site-order tensor with its axes reversed and `dims` below are the sites in that order
        self.plan = _plan_for(shape, device.index, reverse_sites=True) if mirrored else self.ref_plan
        self.stream = _lib.stream_ptr()
        dims = [int(q) for q in self.ref_plan.qubit_size]
        if mirrored:
            dims = dims[::-1]
        self.dims, self.L, self.cdims = dims, len(dims), _lib.i64_array(dims)
        self.mb = int(max_bond) if max_bond else 0
        # fp32, bond-capped: the reshape stage rides on the first Gram pass and the first projection of the
        # sweep (the volume is read through the permutation tables, no site-order tensor is formed)
        self.n_merge = (0 if (self.bf16 or self.f64 or os.environ.get("NDMPS_NO_FUSED_ENCODE"))
                        else int(lib.ndmps_tt_merge_columns(self.L, self.cdims, self.mb)))
        self.gather = self.plan.gather_tables(self.n_merge, device) if self.n_merge > 0 else None
        self.padded = bool(lib.ndmps_tt_sweep_pads_cores(self.L, self.cdims, self.mb))
        self.use_async = False
        self.ws = self.pin_i = self.pin_d = self.done = self.recs = None

    # ------------------------------------------------------------------ first half: enqueue
    def reshape_stage(self, xs):
        """What the sweep reads: the reshape stage of the group in one launch (ndmps.py:66-71 per volume)."""
        if self.gather is not None:
            return xs  # read in place by the fused sweep, never written
        denses = list(_torch().empty((self.batch, self.plan.numel), dtype=self.store, device=self.device).unbind(0))
        with _span("encode_permute"):
            _lib.check(_lib.load().ndmps_encode_permute_many(self.plan.handle, self.batch, _ptr_array(xs), _ptr_array(denses),
                                                             self.esize, self.stream))
        return denses

    def launch_sweep(self, denses, cutoff, defer):
        """Layout, arena, workspace and the sweep itself.  ``defer`` with a sweep that decides its ranks on the device:
        the sweep is enqueued whole (``use_async``), ranks and spectra arrive in pinned buffers."""
        torch = _torch()
        lib = _lib.load()
        batch, L, cdims, mb, device, stream = self.batch, self.L, self.cdims, self.mb, self.device, self.stream
        max_bonds = (C.c_int64 * (L + 1))()
        core_off = (C.c_int64 * (L + 1))()
        self.spec_off = spec_off = (C.c_int64 * (L + 1))()
        _lib.check(lib.ndmps_tt_layout(L, cdims, mb, max_bonds, core_off, spec_off, None))
        ws_query = lib.ndmps_tt_sweep_batched_workspace_bytes_f64 if self.f64 else lib.ndmps_tt_sweep_batched_workspace_bytes
        ws_bytes = ws_query(batch, L, cdims, mb)
        if ws_bytes < 0:
            _lib.check(_lib.EINVAL)
        # one arena for the group: volume b's cores at row b (views of it are what the objects keep)
        self.core_total = core_total = -(-int(core_off[L]) // 128) * 128  # rows stay 256-byte aligned in either storage type
        self.arena_all = torch.empty((batch, core_total), dtype=self.store, device=device)
        self.ws = ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=device)
        self.bonds = bonds = (C.c_int64 * (batch * (L + 1)))()
        spec_total = int(spec_off[L])
        self.spectra = spectra = (C.c_double * max(batch * spec_total, 1))()
        dense_ptrs = (C.c_void_p * batch)(*[d.data_ptr() for d in denses])
        self.arena_base, arena_step = self.arena_all.data_ptr(), core_total * self.esize
        arena_ptrs = (C.c_void_p * batch)(*[self.arena_base + b * arena_step for b in range(batch)])
        # everything a sweep with device-side ranks needs from the host is known now: it can be enqueued whole
        self.use_async = bool(defer and self.gather is not None and self.padded and L > 1)
        with _span("sweep"):
            if self.gather is not None:
                row_off, col_off, col_perm = self.gather
                row_sorted, row_order = self.plan.sorted_rows(self.n_merge, device)
                tables = (row_off.data_ptr(), row_sorted.data_ptr(), row_order.data_ptr(), col_off.data_ptr(),
                          col_perm.data_ptr(), self.n_merge, ws.data_ptr(), ws.numel())
                if self.use_async:
                    n_d = int(lib.ndmps_tt_sweep_async_doubles(batch, L, cdims, mb))
                    self.pin_i = torch.empty(int(lib.ndmps_tt_sweep_async_ints(batch, L)), dtype=torch.int32, pin_memory=True)
                    self.pin_d = torch.empty(max(n_d, 1), dtype=torch.float64, pin_memory=True)
                    _lib.check(lib.ndmps_tt_sweep_batched_fused_begin_f32(
                        batch, dense_ptrs, L, cdims, float(cutoff), mb, arena_ptrs, core_off, bonds, *tables,
                        self.pin_i.data_ptr(), self.pin_d.data_ptr(), stream))
                else:
                    _lib.check(lib.ndmps_tt_sweep_batched_fused_f32(
                        batch, dense_ptrs, L, cdims, float(cutoff), mb, arena_ptrs, core_off, bonds, spectra, spec_off,
                        *tables, stream))
            else:
                sweep = (lib.ndmps_tt_sweep_batched_bf16 if self.bf16 else
                         lib.ndmps_tt_sweep_batched_f64 if self.f64 else lib.ndmps_tt_sweep_batched_f32)
                _lib.check(sweep(batch, dense_ptrs, L, cdims, float(cutoff), mb, arena_ptrs, core_off, bonds,
                                 spectra, spec_off, ws.data_ptr(), ws.numel(), stream))
        # ranks decided on the device: cores sit in the arena in padded shape (cap_i, d_i, cap_{i+1}), zeros
        # beyond the actual bonds; slicing is a no-op whenever the caps bind (the usual case)
        self.bonds_np = np.frombuffer(bonds, dtype=np.int64).reshape(batch, L + 1)  # filled by the sweep / by finish
        self.spec_np = np.frombuffer(spectra, dtype=np.float64)[: batch * spec_total].reshape(batch, spec_total)
        self.caps = np.array([int(max_bonds[i]) for i in range(L + 1)], dtype=np.int64)
        self.offs = [int(core_off[i]) for i in range(L + 1)]
        self.spec_offs = [int(spec_off[i]) for i in range(L + 1)]

    def decode_from_arena(self):
        """``reconstruct=True``, where the batched fused decode serves: decode straight from the arena -- padded cores
        are valid cores of the cap bonds (zeros beyond the rank).  Otherwise ``finish()`` decodes from the objects."""
        batch, L, esize = self.batch, self.L, self.esize
        n_tail = _ro.fused_tail_columns(self.store, self.dims) if self.reconstruct and batch > 1 and not self.mirrored else 0
        if n_tail <= 0:
            return
        dec_bonds = _lib.i64_array([v for b in range(batch) for v in (self.caps if self.padded else self.bonds_np[b])])
        dec_cores = (C.c_void_p * (batch * L))(*[self.arena_base + (b * self.core_total + self.offs[i]) * esize
                                                 for b in range(batch) for i in range(L)])
        out = _ro.decode_chains_f32(batch, L, self.cdims, dec_bonds, dec_cores, n_tail, self.ref_plan, self.shape,
                                    self.device, self.mode == "DCT")
        self.recs = list(out.unbind(0))

    def mark_enqueued(self):
        """The stream ``finish()`` continues on and, behind an asynchronous sweep, the event it waits for."""
        self.tstream = _torch().cuda.current_stream(self.device)
        if self.use_async:
            self.done = _torch().cuda.Event()
            self.done.record(self.tstream)

    # ------------------------------------------------------------------ second half: objects
    def wait(self):
        """Until the copies into the pinned buffers have landed (nothing to wait for after a synchronous sweep)."""
        if self.done is not None:
            self.done.synchronize()

    def arena_cores(self):
        """[volume][site] cap-shaped views of the arena behind a sweep with device-side ranks, else None."""
        if not self.padded:
            return None
        self.wait()
        caps, offs, dims = self.caps, self.offs, self.dims
        return [[self.arena_all[b, offs[i]: offs[i] + int(caps[i]) * dims[i] * int(caps[i + 1])]
                 .view(int(caps[i]), dims[i], int(caps[i + 1])) for i in range(self.L)] for b in range(self.batch)]

    def finish(self):
        """Ranks and spectra to the host (asynchronous sweep: behind its event), objects, state launch."""
        torch = _torch()
        with torch.cuda.device(self.device), torch.cuda.stream(self.tstream):
            if self.use_async:
                self.done.synchronize()
                _lib.check(_lib.load().ndmps_tt_sweep_finish(self.batch, self.L, self.cdims, self.mb, self.pin_i.data_ptr(),
                                                             self.pin_d.data_ptr(), self.bonds, self.spectra, self.spec_off))
            per_site = self._cap_shaped_cores()
            objs = self._build_objects(per_site)
            self._launch_state(objs, per_site is not None)
            if not self.reconstruct:
                return objs
            return objs, (self.recs if self.recs is not None else self.cls.to_tensors(objs, as_torch=True))

    def _cap_shaped_cores(self):
        """[site][volume] views of the arena when every cap binds, else None."""
        if not (self.padded and bool((self.bonds_np == self.caps).all()) and not self.mirrored):
            return None
        # every cap binds: the padded cores ARE the cores; L narrow / view / unbind calls serve the whole
        # group (per-core slicing was 2 ms of host time per group of 32 with the GPU idle)
        caps, offs, dims = self.caps, self.offs, self.dims
        return [self.arena_all[:, offs[i]: offs[i] + int(caps[i]) * dims[i] * int(caps[i + 1])]
                .view(self.batch, int(caps[i]), dims[i], int(caps[i + 1])).unbind(0) for i in range(self.L)]

    def _cores_of(self, b):
        """Volume b's cores cut out of the arena at its own ranks, in the reference's site order."""
        caps, offs, dims, kb = self.caps, self.offs, self.dims, self.bonds_np[b]
        cores = []
        for i in range(self.L):
            k0, k1 = int(kb[i]), int(kb[i + 1])
            if self.padded:
                c0, c1 = int(caps[i]), int(caps[i + 1])
                full = self.arena_all[b, offs[i]: offs[i] + c0 * dims[i] * c1].view(c0, dims[i], c1)
                cores.append(full[:k0, :, :k1].contiguous())
            else:
                view = self.arena_all[b, offs[i]: offs[i] + k0 * dims[i] * k1].view(k0, dims[i], k1)
                # truncated arenas are compact, keep the views; exact sweeps own worst-case arenas
                cores.append(view if self.mb else view.clone())
        if self.mirrored:
            # back to the reference's chain: site j is mirrored site L-1-j with its bond axes swapped
            cores = [c.permute(2, 1, 0).contiguous() for c in reversed(cores)]
        return cores

    def _build_objects(self, per_site):
        L, dims, shape, spec_offs = self.L, self.dims, self.shape, self.spec_offs
        lefts = [math.prod(dims[:i]) for i in range(L)]
        objs = []
        bl0 = np.zeros((L, 2))
        for b in range(self.batch):
            kb = self.bonds_np[b]
            cores = [per_site[i][b] for i in range(L)] if per_site is not None else self._cores_of(b)
            obj = self.cls._from_mps(DeviceMPS(cores, _trusted=True), self.ref_plan.qubit_size.copy(), shape, self.norm,
                                     self.mode, len(shape), boundary_list=bl0)
            counts = [min(lefts[i], dims[i] * int(kb[i + 1])) for i in range(L)]
            row = self.spec_np[b]
            if self.mirrored:
                # the values of mirrored bond (i-1 | i) belong to bond (L-i-1 | L-i)
                obj.sweep_spectra = [None] + [row[spec_offs[L - j]: spec_offs[L - j] + counts[L - j]].copy()
                                              for j in range(1, L)]
            else:
                # singular values of the sweep, cut out of the group's buffer on first use
                obj._spectra_lazy = (row, spec_offs, counts)
            objs.append(obj)
        return objs

    def _launch_state(self, objs, cap_shaped):
        torch = _torch()
        lib = _lib.load()
        batch, L, caps, dims = self.batch, self.L, self.caps, self.dims
        with _span("state"):
            # boundary_list (ndmps.py:75) and norm_value (ndmps.py:76) of every volume from one
            # launch.  The sweep leaves sites 1..L-1 right-isometric (rows of V^T), so
            # mps @ mps = ||site 0||_F^2 up to the fp32 rounding of those rows (~1e-7 relative);
            # update_norm() evaluates the full overlap contraction like the reference.
            if cap_shaped and not self.bf16 and not self.f64 and L <= 64 and batch * L <= 65535:
                # cores = cap-shaped views of the arena: one launch now, the numbers on first access
                count = batch * L
                partial = torch.empty(int(lib.ndmps_minmax_partials_bytes(count)) // 8, dtype=torch.float64, device=self.device)
                lens = _lib.i64_array([int(caps[i]) * dims[i] * int(caps[i + 1]) for i in range(L)])
                _lib.check(lib.ndmps_minmax_arena_launch_f32(self.arena_base, self.core_total, batch, L,
                                                             _lib.i64_array(self.offs[:L]), lens, partial.data_ptr(),
                                                             self.stream))
                group = _GroupState(objs, partial, count, L, self.stream)
                for o in objs:
                    o.__dict__["_state_group"] = group
            else:
                all_cores = [c for o in objs for c in o.mps.cores]
                mm, ss = _ft.minmax_many(all_cores, with_sumsq=True)
                mm_np = np.asarray(mm, dtype=np.float64).reshape(batch, L, 2)
                for b, o in enumerate(objs):
                    o.boundary_list = mm_np[b]
                    # the site that carries the norm: 0 after a right-to-left sweep, L-1 after the mirrored one
                    o.norm_value = np.sqrt(ss[b * L + (L - 1 if self.mirrored else 0)])


class NDMPS:
    """
    Class for storing and compressing N-dimensional tensors using MPS (device resident).
    """

    def __init__(self, mps=None, qubit_size=None, encoding_map=None, boundary_list=None, norm=True,
                 norm_value=None, mode="Std", dim=None):
        self.qubit_size = qubit_size
        self._encoding_map = encoding_map
        self.mps = mps
        self.dim = dim
        self.norm = norm
        self.norm_value = norm_value
        self.mode = mode
        self.boundary_list = np.array(boundary_list)
        # tensor shape: known from the map when one is handed in (the reference's constructor allows
        # that, ndmps.py:17-35), set by from_tensors / codec.loads otherwise
        self._shape = tuple(int(v) for v in np.shape(encoding_map)[:-1]) if encoding_map is not None else None

    @classmethod
    def _from_mps(cls, mps, qubit_size, shape, norm, mode, dim, encoding_map=None, norm_value=None, boundary_list=None):
        """An object around finished cores: the fields of __init__, set without its array conversions (the encode path
        builds 32 objects per group inside the timed region), plus the tensor shape."""
        obj = cls.__new__(cls)
        obj.qubit_size = qubit_size
        obj._encoding_map = encoding_map
        obj.mps = mps
        obj.dim = dim
        obj.norm = norm
        obj.norm_value = norm_value
        obj.mode = mode
        obj.boundary_list = boundary_list
        obj._shape = shape
        return obj

    def _like(self, cores, norm=None):
        """A new object for ``cores`` (finished: contiguous, 3-D) of the tensor this one stores -- same shape, mode,
        site dimensions and encoding map; boundary_list and norm_value are left to the caller."""
        return NDMPS._from_mps(DeviceMPS(cores, _trusted=True), self.qubit_size, self._shape,
                               self.norm if norm is None else norm, self.mode, self.dim, self._encoding_map)

    # boundary_list / norm_value: plain attributes as in the reference; after from_tensors their device-side
    # reductions are in flight and the values arrive on first access (_GroupState)
    def _resolve_state(self):
        g = self.__dict__.get("_state_group")
        if g is not None:
            g.resolve()

    @property
    def boundary_list(self):
        self._resolve_state()
        return self.__dict__.get("_boundary_list")

    @boundary_list.setter
    def boundary_list(self, value):
        self.__dict__["_boundary_list"] = value
        if self.__dict__.get("_state_group") is not None:
            self.__dict__["_boundary_set"] = True

    @property
    def norm_value(self):
        self._resolve_state()
        return self.__dict__.get("_norm_value")

    @norm_value.setter
    def norm_value(self, value):
        self.__dict__["_norm_value"] = value
        if self.__dict__.get("_state_group") is not None:
            self.__dict__["_norm_set"] = True

    def __deepcopy__(self, memo):
        import copy

        self._resolve_state()
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_spectra_lazy" and v is not None:
                v = (v[0].copy(), v[1], v[2])
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    # singular values kept by the sweep, per bond (None for site 0); from_tensors stores them lazily
    @property
    def sweep_spectra(self):
        lazy = self.__dict__.get("_spectra_lazy")
        if lazy is not None:
            row, offs, counts = lazy
            self.__dict__["_sweep_spectra"] = [None] + [row[offs[i]: offs[i] + counts[i]].copy() for i in range(1, len(counts))]
            self.__dict__["_spectra_lazy"] = None
        return self.__dict__.get("_sweep_spectra")

    @sweep_spectra.setter
    def sweep_spectra(self, value):
        self.__dict__["_spectra_lazy"] = None
        self.__dict__["_sweep_spectra"] = value

    # The reference keeps the (*shape, L) int64 map; here it is built on first access only.
    @property
    def encoding_map(self):
        if self._encoding_map is None and self._shape is not None:
            _, enc = _core.gen_encoding_map(self._shape)
            self._encoding_map = np.moveaxis(enc, 0, -1)
        return self._encoding_map

    @encoding_map.setter
    def encoding_map(self, value):
        self._encoding_map = value
        if value is not None:
            self._shape = tuple(int(v) for v in np.shape(value)[:-1])

    # ---------------------------------------------------------------------- encode
    @classmethod
    def from_tensor(cls, tensor, norm: bool = False, mode: str = "Std", max_bond=None,
                    cutoff: float = 1e-10, device=None, dtype=None, sweep_from: str = "right", carry_dtype=None) -> "NDMPS":
        """
        Create an NDMPS instance from a tensor with encoding and optional normalization.

        tensor : np.ndarray or torch.Tensor (host or device); never mutated.
        norm : normalize the input tensor by its L2 norm.
        mode : "Std" for raw encoding or "DCT" for last-axis DCT preprocessing.
        max_bond : optional bond cap chi applied during the sweep (None = exact sweep).
        cutoff : relative singular-value cutoff of the sweep (quimb from_dense default).
        dtype : storage type in HBM, ``torch.float32`` (default), ``torch.bfloat16`` or ``torch.float64``
            (the reference's own element type; see from_tensors).
        sweep_from : "right" (default) or "left": which end quimb's ``from_dense`` (ndmps.py:74) starts from; see
            from_tensors.
        carry_dtype : element type of the SWEEP when it differs from the storage type ``dtype``: with
            ``dtype=torch.bfloat16, carry_dtype=torch.float32`` the volume is widened to fp32, the carried matrices of the
            sweep are fp32 (no bf16 rounding between the sites) and only the finished cores are rounded to bf16
            (``astype``); reconstruction then runs in bf16 as for any bf16 object.
        """
        if carry_dtype is not None and dtype is not None and carry_dtype != dtype:
            return cls.from_tensors([tensor], norm=norm, mode=mode, max_bond=max_bond, cutoff=cutoff, device=device,
                                    dtype=carry_dtype, sweep_from=sweep_from)[0].astype(dtype)
        return cls.from_tensors([tensor], norm=norm, mode=mode, max_bond=max_bond, cutoff=cutoff,
                                device=device, dtype=dtype, sweep_from=sweep_from)[0]

    @classmethod
    def from_tensors(cls, tensors, norm: bool = False, mode: str = "Std", max_bond=None,
                     cutoff: float = 1e-10, device=None, dtype=None, reconstruct: bool = False,
                     sweep_from: str = "right"):
        """
        Encode a list of independent tensors OF THE SAME SHAPE in one batched pass (what the
        reference does with a Python loop, evaluation/benchmark.py:73-76).  The volumes go through
        the sites in lockstep, so each site's eigenproblems are solved by one batched launch
        sequence; results equal those of ``from_tensor`` on each up to the rounding of the fp64
        eigen-solver (its summation order depends on how many matrices are in flight).

        ``dtype=torch.bfloat16`` selects bf16 STORAGE (the reference fixes float64 at ndmps.py:56;
        BASELINE config 5 asks for bf16): the volume is read as bf16 (2 bytes per voxel, no fp32 copy),
        the site-order tensor, the carried matrices of the sweep and the cores are bf16 in HBM, products
        run on the bf16 MFMA with fp32 accumulation, Gram matrices and eigen-decompositions stay fp64.
        ``to_tensor`` then contracts in bf16 as well.  Results carry bf16 rounding (2^-9 relative per
        stored value).

        ``dtype=torch.float64`` selects fp64 STORAGE, the reference's own element type (ndmps.py:56): volume,
        carried matrices and cores are fp64 in HBM, every product runs on the fp64 MFMA, norm / DCT / overlap /
        truncation / quantisation are fp64 as well, and ``to_tensor`` returns float64 -- the mode that meets the
        reference's own tolerances (round trip 1e-10, norms 1e-12).  A fidelity mode: several times slower than
        fp32 storage.  The sweep's relative cutoff is clamped below at 1e-8 (singular values come from fp64 Gram
        matrices).

        ``sweep_from`` names the convention of quimb's ``MatrixProductState.from_dense`` (ndmps.py:74), whose source is
        not available here: "right" (the default, what SURVEY states for quimb 1.9.0) sweeps site L-1 .. 1,
        keeps V^T as the site and carries U S to the left, so sites 1..L-1 are right-isometric and site 0 holds the norm;
        "left" is the other possible convention -- site 0 .. L-2, U is the site, S V^T is carried to the right, the
        norm ends up on the last site.  It is computed as the same sweep on the mirrored chain (the reshape stage writes
        the site-order tensor with its axes reversed, the cores come back transposed and in reverse order).  The two
        give the same exact MPS up to gauge, DIFFERENT truncations (each cuts the bonds in its own order), different
        ``boundary_list`` and a different starting point for ``compress``.

        ``reconstruct=True`` returns ``(objects, reconstructions)``: the chain products of the whole list are issued
        as soon as the sweep has returned, BEFORE the Python objects are built (their construction then runs
        under the decode instead of in front of it); the reconstructions (device tensors) equal
        ``NDMPS.to_tensors(objects, as_torch=True)``.
        """
        _lib.require_device()
        lib = _lib.load()
        tensors = list(tensors)
        if not tensors:
            return ([], []) if reconstruct else []
        if sweep_from not in ("right", "left"):
            raise ValueError("sweep_from must be 'right' or 'left'")
        args = (tensors, norm, mode, max_bond, cutoff, device, dtype, reconstruct, sweep_from == "left")
        try:
            return cls._encode_group(*args)
        except _lib.NdmpsTeamAbort:
            # a resident tridiagonalisation gave up waiting for its workgroups (the GPU is shared with something that
            # holds the compute units): the inputs are untouched, so the group is encoded again on the per-column
            # launches, whose only synchronisation is the kernel boundary; counted in ndmps_syevd_topk_team_fallbacks
            _lib.check(lib.ndmps_syevd_topk_note_team_fallback())
            was = lib.ndmps_syevd_topk_set_team(0)
            try:
                return cls._encode_group(*args)
            finally:
                lib.ndmps_syevd_topk_set_team(was)

    @classmethod
    def from_tensors_begin(cls, tensors, norm: bool = False, mode: str = "Std", max_bond=None, cutoff: float = 1e-10,
                           device=None, dtype=None, reconstruct: bool = False, sweep_from: str = "right"):
        """``from_tensors`` in two halves: this one enqueues the group's work on the current stream and returns a
        ``PendingGroup``; ``result()`` waits for it and returns what ``from_tensors`` returns (same kernels, same order:
        bit-identical).  For the fp32 bond-capped path nothing on the host waits in between (the sweep decides its ranks
        on the device: csrc/tt.hip SweepAsync); other paths are encoded here, synchronously, and only build their objects
        in ``result()``.  The reference has no counterpart (NumPy is synchronous, evaluation/benchmark.py:73-76)."""
        _lib.require_device()
        tensors = list(tensors)
        if not tensors:
            return PendingGroup(lambda: ([], []) if reconstruct else [])
        if sweep_from not in ("right", "left"):
            raise ValueError("sweep_from must be 'right' or 'left'")

        def redo():
            return cls.from_tensors(tensors, norm, mode, max_bond, cutoff, device, dtype, reconstruct, sweep_from)

        try:
            pend = cls._encode_group(tensors, norm, mode, max_bond, cutoff, device, dtype, reconstruct,
                                     sweep_from == "left", defer=True)
        except _lib.NdmpsTeamAbort:  # a synchronous path gave up on the resident kernels: from_tensors knows what to do
            value = redo()
            return PendingGroup(lambda: value)
        pend._redo = redo
        return pend

    @classmethod
    def _encode_group(cls, tensors, norm, mode, max_bond, cutoff, device, dtype, reconstruct, mirrored=False,
                      defer=False):
        """One lockstep group through norm / DCT / reshape stage / sweep (/ decode): the body of from_tensors.
        ``defer=True`` (from_tensors_begin) returns a ``PendingGroup``: when the sweep decides its ranks on the device
        (fp32, bond-capped) everything is only ENQUEUED -- sweep, decode, the copies of ranks and spectra into pinned host
        memory, an event -- and ``result()`` waits for the event, reads the ranks and builds the objects."""
        torch = _torch()
        first = tensors[0]
        if device is None:
            device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else "cuda"
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        store = torch.float32 if dtype is None else dtype
        if store not in (torch.float32, torch.bfloat16, torch.float64):
            raise ValueError("storage dtype must be torch.float32, torch.bfloat16 or torch.float64")
        xs, shape = _stage_inputs(tensors, device, store, norm)
        with torch.cuda.device(device):
            group = _SweptGroup(cls, len(xs), shape, device, store, norm, mode, max_bond, mirrored, reconstruct)
            xs = _normalise_and_transform(xs, shape, norm, mode, store, device)
            denses = group.reshape_stage(xs)
            del xs
            group.launch_sweep(denses, cutoff, defer)
            del denses
            group.decode_from_arena()
            # the workspace is released here, behind the decode's buffers: freed in front of them, the caching allocator cut
            # the reconstruction buffer out of its block whenever earlier reconstructions were still held by a pending batch,
            # and the next batch's workspace -- several GB -- came from a fresh hipMalloc: one second, now and then
            group.ws = None
            group.mark_enqueued()
        if defer:
            return PendingGroup(group.finish, asynchronous=group.use_async, wait=group.wait, arena=group.arena_cores)
        return group.finish()

    # ----------------------------------------------------------------- bookkeeping
    def astype(self, dtype):
        """A copy of this object with its cores stored as ``dtype`` (torch.float32, torch.bfloat16 or torch.float64): the
        cores are rounded once, ``boundary_list`` and ``norm_value`` are those of the rounded cores.  No counterpart in the
        reference (it has one element type, ndmps.py:56)."""
        torch = _torch()
        if dtype not in (torch.float32, torch.bfloat16, torch.float64):
            raise ValueError("storage dtype must be torch.float32, torch.bfloat16 or torch.float64")
        out = self._like([c.to(dtype).contiguous() for c in self.mps.cores])
        out.update_boundary_list()
        out.update_norm()
        return out

    def update_boundary_list(self):
        """Recompute min/max boundaries for each MPS tensor."""
        self.boundary_list = np.array([list(v) for v in _ft.minmax_many(self.mps.cores)])

    def update_norm(self):
        """Update stored norm of the current MPS."""
        self.norm_value = np.sqrt(self.mps @ self.mps)

    def compression_ratio(self):
        """Compute compression ratio: MPS elements / original tensor elements."""
        return self.number_elements_in_MPS() / np.prod(self.qubit_size)

    def number_elements_in_MPS(self) -> int:
        """Return the total number of elements in all MPS tensors."""
        return sum(t.size for t in self.mps)

    def bond_sizes(self):
        """Return the bond dimensions of the MPS."""
        return self.mps.bond_sizes()

    def show(self):
        """Display the MPS chain."""
        self.mps.show()

    def return_tensors_data(self):
        """Return internal MPS tensor list."""
        return [t for t in self.mps.arrays]

    def replace_tensordata(self, tensorlist):
        """Replace internal tensors in the MPS with externally provided ones."""
        arrays = self.mps.arrays
        for i in range(len(arrays)):
            assert arrays[i].shape == tuple(tensorlist[i].shape)
            arrays[i][:] = tensorlist[i]
        self.update_boundary_list()
        self.update_norm()

    # --------------------------------------------------------------------- truncate
    def compress(self, cutoff: float, max_bond=None):
        """
        Compress MPS by truncating bonds with a relative cutoff (left to right, in place).

        ``cutoff == 0`` with no ``max_bond`` leaves every bond as it is (quimb only trims when
        cutoff > 0); the product of the cores is unchanged either way.

        Each bond keeps the singular values s_j > max(cutoff, floor) * s_0 (at least one, at most
        ``max_bond``), with the storage floor 1e-6 for fp32 and bf16 cores and 1e-8 for fp64 cores.
        The floor applies with ``cutoff == 0`` too: ``compress(0, max_bond=chi)`` ("parity mode")
        keeps min(#{s_j > floor * s_0}, chi) values per bond, where the reference keeps min(n, chi),
        zeros included -- it equals the reference run at ``cutoff=floor``.
        """
        if cutoff < 0:
            raise ValueError("cutoff must be non-negative")
        if cutoff > 0 or max_bond:
            for i in range(1, len(self.mps.sites)):
                self.mps.compress_bond_(i, cutoff, max_bond)
        self.update_boundary_list()
        self.update_norm()

    # ------------------------------------------------------- linear combination / rounding (core/lincomb.py)
    @staticmethod
    def linear_combination(objs, weights, cutoff: float = 0.0, max_bond=None, dtype=None) -> "NDMPS":
        """
        The TT rounding of ``sum_a weights[a] * objs[a]`` as a new object, computed on the cores (csrc/lincomb.hip):
        its ``to_tensor()`` is ``sum_a w_a * objs[a].to_tensor()`` up to the truncation, and no volume is formed.  In DCT
        mode the combination is taken on the coefficients (the orthonormal DCT is linear).  No counterpart in the
        reference.

        Right-to-left TT-SVD of the formal sum chain, the truncation ``from_tensor`` makes: at each bond keep the
        singular values ``s_j > max(cutoff * s_0, floor * scale)``, ``scale = sum_a |w_a| * objs[a].norm_value`` and
        the storage floor 1e-6 (fp32 / bf16 work) or 1e-8 (fp64), at most ``max_bond``.  When nothing survives at
        some bond (or the scale is 0) the result is the zero MPS: every bond 1, zero cores, ``sweep_spectra`` [0.0] per
        bond.  Sites 1..L-1 of the result are
        right-isometric and site 0 carries the norm; ``norm=False``; ``sweep_spectra`` holds the kept values.

        dtype: storage of the result; None gives fp64 if any input is fp64 and fp32 otherwise (bf16 inputs are
        widened in the kernels); torch.bfloat16 rounds the finished fp32 cores once, as ``astype`` does.
        Raises ValueError for empty or mismatched inputs, a non-finite weight, ``cutoff < 0``, ``max_bond < 1``,
        objects that differ in qubit_size, shape, mode or device, or a summed bond above 4096.
        """
        objs = _checked_list(objs, "linear_combination combines")
        w = _lc.check_args(len(objs), weights, cutoff, max_bond)
        _check_result_dtype(dtype)
        _check_compatible(objs)
        _lc.check_summed_bonds([o.mps.bonds for o in objs])
        scale = _lc.scale_of(w, [o.norm_value for o in objs])
        return objs[0]._round_chains([o.mps for o in objs], w, cutoff, max_bond, dtype, scale)

    def _round_chains(self, chains, w, cutoff, max_bond, dtype, scale) -> "NDMPS":
        """``oncore.round_chains`` of DeviceMPS chains over this object's site dims (arguments already checked) as a new
        object like this one: ``norm=False``, boundary_list, norm_value and sweep_spectra set."""
        cores, _, spectra, _ = _oc.round_chains(chains, w, cutoff, max_bond, dtype, scale)
        out = self._like(cores, norm=False)
        out.update_boundary_list()
        out.update_norm()
        out.sweep_spectra = spectra
        return out

    def recompress(self, cutoff: float = 0.0, max_bond=None, dtype=None) -> "NDMPS":
        """The TT-SVD truncation of this object's own chain as a new object: ``linear_combination([self], [1.0],
        cutoff, max_bond, dtype)``.  On an exact object ``recompress(max_bond=chi)`` is the truncation
        ``from_tensor(x, max_bond=chi)`` makes.  ``compress()`` (the reference's left-to-right two-site truncation)
        is unchanged."""
        return NDMPS.linear_combination([self], [1.0], cutoff=cutoff, max_bond=max_bond, dtype=dtype)

    # ------------------------------------------------------- axis operators on the cores (core/axisop.py)
    def _axis_plan(self, axis):
        """(axis as a non-negative int, the factor array, the axis length) for an operator along ``axis``; ValueError
        without a known shape, for the last axis of a DCT-mode object, or for cores that are not over the shape's own
        factor array."""
        shape = self._require_shape()
        axis = _ax.normalize_axis(axis, len(shape))
        _ax.check_data_axis(self.mode, axis, len(shape))
        fa = _core.get_factorlist(tuple(shape))[0]
        if self.mps.dims != [int(v) for v in np.prod(fa, axis=1)]:
            raise ValueError("the cores are not over the site dims of this object's shape")
        return axis, fa, int(shape[axis])

    def _axis_rounded(self, mpo, fa, axis, cutoff, max_bond, dtype) -> "NDMPS":
        """The operator applied along ``axis`` (``fa``, ``axis``: what ``_axis_plan`` returned) and rounded like
        ``recompress``; the storage floor is relative to ``mpo.opnorm * norm_value``, a bound on the result's norm."""
        _lc.check_args(1, [1.0], cutoff, max_bond)
        _check_result_dtype(dtype)
        wide = _oc.axis_apply(self.mps, mpo, fa, axis)
        return self._round_chains([wide], [1.0], cutoff, max_bond, dtype, mpo.opnorm * float(self.norm_value))

    def roll(self, shift, axis, cutoff: float = 0.0, max_bond=None, dtype=None) -> "NDMPS":
        """
        ``np.roll(to_tensor(), shift, axis)`` as a new object, computed on the cores: the shift is digit-wise addition
        with a carry along the chain, an operator of bond 2 (core/axisop.py) that is applied to the cores in one launch
        and rounded like ``recompress`` (same ``cutoff`` / ``max_bond`` / ``dtype``); no volume is formed.  ``axis`` is
        required; tuples of shifts and axes are applied axis after axis, each with its own rounding (an int shift goes
        with every axis of a tuple).  The result's bonds are at most twice the input's before ``max_bond``.

        Raises TypeError for a non-integer shift or axis, ValueError (numpy's AxisError) for an axis out of range, for
        tuples of different lengths, for the last axis of a DCT-mode object (its digits index DCT coefficients; the
        other axes are fine) and for ``linear_combination``'s argument errors.  No counterpart in the reference.
        """
        if isinstance(axis, tuple):
            shifts = shift if isinstance(shift, tuple) else (shift,) * len(axis)
            if len(shifts) != len(axis):
                raise ValueError("shift and axis must have the same length")
            plans = [(_ax.check_shift(s), self._axis_plan(a)[0]) for s, a in zip(shifts, axis)]  # every check first
            if not plans:
                return self.recompress(cutoff, max_bond, dtype)
            out = self
            for s, a in plans:
                out = out.roll(s, a, cutoff, max_bond, dtype)
            return out
        shift = _ax.check_shift(shift)
        axis, fa, _ = self._axis_plan(axis)
        return self._axis_rounded(_ax.roll_mpo(fa[:, axis], shift), fa, axis, cutoff, max_bond, dtype)

    def shift(self, shift, axis, cutoff: float = 0.0, max_bond=None, dtype=None) -> "NDMPS":
        """The volume moved by ``shift`` voxels along ``axis`` with zeros shifted in (``out[i] = x[i - shift]`` inside
        the volume); ``abs(shift) >= n`` gives the zero MPS, as ``linear_combination`` returns it.  Otherwise as
        ``roll`` with a single axis."""
        shift = _ax.check_shift(shift)
        axis, fa, n = self._axis_plan(axis)
        if abs(shift) >= n:
            return NDMPS.linear_combination([self], [0.0], cutoff=cutoff, max_bond=max_bond, dtype=dtype)
        return self._axis_rounded(_ax.shift_mpo(fa[:, axis], shift), fa, axis, cutoff, max_bond, dtype)

    def correlate1d(self, weights, axis=-1, mode: str = "constant", origin: int = 0, cutoff: float = 0.0,
                    max_bond=None, dtype=None) -> "NDMPS":
        """
        ``scipy.ndimage.correlate1d(to_tensor(), weights, axis, mode=mode, cval=0, origin=origin)`` on the cores:
        ``out[i] = sum_j weights[j] * x[i + j - len(weights) // 2 - origin]`` with ``x`` zero outside the volume
        (``mode="constant"``) or periodic (``"wrap"``).  The stencil is an operator of bond 3 (wider only at the finest
        bond when the radius exceeds the finest digit), rounded like ``recompress`` with the storage floor relative to
        ``sum |weights| * norm_value``.  Raises ValueError for weights that are not a non-empty 1-D array of finite
        numbers, another ``mode``, an origin scipy refuses or a radius ``>= n``; axis errors as ``roll``.
        """
        _ax.check_taps(weights)
        _ax.check_mode(mode)
        axis, fa, n = self._axis_plan(axis)
        taps = _ax.correlate_taps(weights, origin, n)
        return self._axis_rounded(_ax.offsets_mpo(fa[:, axis], taps, mode), fa, axis, cutoff, max_bond, dtype)

    def cumsum(self, axis, cutoff: float = 0.0, max_bond=None, dtype=None) -> "NDMPS":
        """``np.cumsum(to_tensor(), axis)`` on the cores: an operator of bond 2, rounded like ``recompress``.  The
        operator's norm is bounded by n, so the absolute storage floor is ``1e-6 * n * norm_value`` (1e-8 for fp64
        work): directions of the result below that are dropped.  Axis errors as ``roll``."""
        axis, fa, _ = self._axis_plan(axis)
        return self._axis_rounded(_ax.cumsum_mpo(fa[:, axis]), fa, axis, cutoff, max_bond, dtype)

    def flip(self, axis) -> "NDMPS":
        """``np.flip(to_tensor(), axis)``: every digit of the axis reversed, a site-local permutation.  The cores are
        permuted copies in the same storage type; bonds, gauge, ``norm``, ``norm_value``, ``boundary_list`` and
        ``sweep_spectra`` are those of this object and nothing is rounded.  Axis errors as ``roll``."""
        axis, fa, _ = self._axis_plan(axis)
        cores = [c.view(c.shape[0], pre, f, post, c.shape[2]).flip(2).reshape(c.shape).contiguous()
                 for c, (pre, f, post) in zip(self.mps.cores, _ax.site_split(fa, axis))]
        out = self._like(cores)
        out.boundary_list = None if self.boundary_list is None else np.array(self.boundary_list, copy=True)
        out.norm_value = self.norm_value
        spec = self.sweep_spectra
        out.sweep_spectra = None if spec is None else [None if s is None else np.array(s, copy=True) for s in spec]
        return out

    # ------------------------------------------------------- elementwise product on the cores (core/hadamard.py)
    def multiply(self, other, max_bond=None, cutoff: float = 0.0, oversample=None, seed: int = 0, dtype=None) -> "NDMPS":
        """
        The elementwise (Hadamard) product ``to_tensor() * other.to_tensor()`` as a new object, computed on the cores
        (csrc/hadamard.hip, core/hadamard.py): mask x volume, squares, windows.  No volume is formed, and neither is the
        product chain of bond ``chi_a chi_b``: a random chain of bond ``max_bond + oversample`` sketches it down
        ("randomise then orthogonalise" TT rounding), and the sketched chain is rounded like ``recompress`` (same
        ``cutoff`` / ``max_bond`` / ``dtype``, gauge and ``sweep_spectra``; the storage floor is relative to the norm of
        the sketched product).  ``oversample=None`` is ``max(8, max_bond)``; the random cores are drawn on the host
        from ``numpy.random.default_rng(seed)``, so the same seed gives the same bits.  ``max_bond=None`` takes the
        sketch bonds ``chi_a chi_b``: the exact product, nothing random.  A zero product is the zero MPS, as
        ``linear_combination`` returns it.  ``a * b`` with two objects still raises TypeError (``*`` is scaling by a
        number): the product needs ``max_bond`` for anything but small bonds, so it is a method.  No counterpart in the
        reference.

        Raises TypeError for a non-NDMPS operand; ValueError for objects that differ in qubit_size, shape, mode,
        device or site dims, for DCT mode (a product of coefficient volumes is not the product of the volumes), for a
        sketch bond above 512 (``max_bond + oversample`` must be <= 512; without ``max_bond``: pass ``max_bond``), for a
        workspace above 2 GiB (recompress the inputs first), for ``oversample < 0``, a non-integer seed and the
        ``dtype`` / ``cutoff`` / ``max_bond`` errors of ``linear_combination``.
        """
        torch = _torch()
        if not isinstance(other, NDMPS):
            raise TypeError(f"multiply takes an NDMPS, not {type(other).__name__}")
        max_bond, oversample, seed = _hd.check_args(max_bond, cutoff, oversample, seed)
        _check_result_dtype(dtype)
        _check_compatible((self, other))
        if self.mode == "DCT":
            raise ValueError("DCT mode stores DCT coefficients: their product is not the product of the volumes")
        dims = self.mps.dims
        ell = _hd.sketch_bonds(dims, self.mps.bonds, other.mps.bonds, max_bond, oversample)
        sketched = _oc.hadamard_sketch(self.mps, other.mps, ell, _hd.sketch_cores(dims, ell, seed))
        scale = float(torch.linalg.vector_norm(sketched.cores[-1]))
        if dtype is None:
            dtype = torch.float64 if _work_is_f64((self, other)) else torch.float32
        return self._round_chains([sketched], [1.0], cutoff, max_bond, dtype, scale)

    def square(self, max_bond=None, cutoff: float = 0.0, oversample=None, seed: int = 0, dtype=None) -> "NDMPS":
        """``multiply(self, ...)``: the voxelwise square."""
        return self.multiply(self, max_bond=max_bond, cutoff=cutoff, oversample=oversample, seed=seed, dtype=dtype)

    # ------------------------------------------------------- sums of many objects by a sketch (core/sumsketch.py)
    @staticmethod
    def linear_combinations(objs, weights, max_bond=None, cutoff: float = 0.0, oversample=None, seed: int = 0,
                            dtype=None) -> list:
        """
        The TT roundings of ``sum_a weights[j, a] * objs[a]`` for every row j of ``weights`` (``(K, T)``; a 1-D array
        of length T is one row) as a list of K new objects, computed on the cores by a randomised sketch
        (csrc/sumsketch.hip, core/sumsketch.py).  Unlike ``linear_combination`` there is no limit on the summed bond
        ``sum_a chi_a``: a random chain of bond ``max_bond + oversample`` sketches the formal sum chain down frame by
        frame ("randomise then orthogonalise" TT rounding), the cost is linear in T, no eigenproblem exceeds
        ``max_bond + oversample``, and the right environments are shared by all K rows.  The sketched chains are
        rounded like ``multiply``'s (same ``cutoff`` / ``max_bond`` / ``dtype``, gauge, ``norm=False``,
        ``boundary_list``, ``norm_value`` and ``sweep_spectra``; the storage floor is relative to the norm of the
        sketched sum).  ``oversample=None`` is ``max(8, max_bond)``; the random cores are drawn on the host from
        ``numpy.random.default_rng(seed)`` and every sum over frames runs in ascending order without atomics, so the
        same arguments give the same bits.  ``max_bond=None`` takes the sketch bonds equal to the summed bonds: the
        exact sum, allowed while they are <= 512.  In DCT mode the combination is taken on the coefficients.  A frame
        whose weights are zero in every row is never read, and a zero entry is skipped in that row; a row of zeros,
        or a sum that vanishes, gives the zero MPS of ``linear_combination``.  ``dtype=None`` is fp64 if any input is
        fp64 and fp32 otherwise.  No counterpart in the reference.

        Raises TypeError for a non-NDMPS; ValueError for an empty list, weights whose last dimension is not T or with
        more than two dimensions, a non-finite weight, ``cutoff < 0``, ``max_bond < 1``, ``oversample < 0``, a bad
        seed, objects that differ in qubit_size, shape, mode, device or site dims, a sketch bond above 512 or a
        workspace above 2 GiB (recompress the inputs first).  Objects whose bonds are all <= 64 run in the resident
        kernels; an object with a larger bond takes a general route through fp64 dense products.
        """
        torch = _torch()
        objs = _checked_list(objs, "linear_combinations combines")
        w = _ss.check_weights(len(objs), weights)
        max_bond, oversample, seed = _hd.check_args(max_bond, cutoff, oversample, seed)
        _check_result_dtype(dtype)
        _check_compatible(objs)
        first = objs[0]
        dims = first.mps.dims
        if dtype is None:
            dtype = torch.float64 if _work_is_f64(objs) else torch.float32
        used = _ss.used_frames(w)
        if used:
            frames = [objs[a].mps for a in used]
            ell = _ss.sketch_bonds(dims, [m.bonds for m in frames], max_bond, oversample)
            chains = _oc.sum_sketch(frames, w[:, used], ell, _hd.sketch_cores(dims, ell, seed))
        else:
            chains = [_oc.zero_chain(dims, first.mps.device) for _ in range(w.shape[0])]
        out = []
        for sketched in chains:
            scale = float(torch.linalg.vector_norm(sketched.cores[-1]))
            out.append(first._round_chains([sketched], [1.0], cutoff, max_bond, dtype, scale))
        return out

    @staticmethod
    def pca_sketched(objs, n_components=None, max_bond=None, center: bool = True, cutoff: float = 0.0, oversample=None,
                     seed: int = 0, dtype=None):
        """
        ``pca`` with its last step replaced: ``G = gram(objs)``, the weights (``core.series.pca_weights``), the kept
        set, the signs and ``explained_variance`` are those of ``pca``; the components and, when ``center``, the mean
        come from ONE ``linear_combinations`` call with the weight matrix ``[W[:, 0], ..., W[:, r-1], (1/T, ..., 1/T)]``,
        so a series of any length is accepted and all outputs share the right environments.  ``max_bond``, ``cutoff``,
        ``oversample``, ``seed`` and ``dtype`` as in ``linear_combinations``.  Returns a ``SeriesPCA``.
        """
        objs = list(objs)
        _se.check_components(n_components)
        _hd.check_args(max_bond, cutoff, oversample, seed)
        _check_result_dtype(dtype)
        G = NDMPS.gram(objs)
        T = len(objs)
        sigma, U, W = _se.pca_weights(G, n_components, center, _lc.floor_for(_work_is_f64(objs, dtype)))
        rows = [W[:, k] for k in range(len(sigma))] + ([np.full(T, 1.0 / T)] if center else [])
        outs = NDMPS.linear_combinations(objs, np.stack(rows), max_bond=max_bond, cutoff=cutoff, oversample=oversample,
                                         seed=seed, dtype=dtype) if rows else []
        components, mean = (outs[:-1], outs[-1]) if center else (outs, None)
        return _se.SeriesPCA(sigma, _se.explained_variance(sigma, T, center), U * sigma[None, :], W, components, mean)

    # ------------------------------------------------------- Gram matrix and PCA of a series (core/series.py)
    @staticmethod
    def _gram_chains(objs, others, weight):
        """The checked arguments of ``gram`` / ``gram_route`` as chains: (rows, columns or None, weight chain or None)."""
        objs = list(objs)
        rows = _checked_list(objs if others is None else objs + list(others), "gram takes")
        _se.check_lists(len(objs), None if others is None else len(rows) - len(objs))
        _check_compatible(rows)
        if weight is not None:
            _wg.check_weight_type(weight, NDMPS)
            _check_compatible(rows + [weight])
            _wg.check_mode(weight.mode)
        return ([o.mps for o in objs], None if others is None else [o.mps for o in rows[len(objs):]],
                None if weight is None else weight.mps)

    @staticmethod
    def gram_route(objs, others=None, *, weight=None) -> str:
        """Which path ``gram`` takes for these lists: "resident" (every inner bond <= 64: one launch, one workgroup
        per pair), "batched" (larger bonds, equal in all objects) or "per-pair" (larger ragged bonds).  With a
        ``weight`` (csrc/wgram.hip): "resident" (every inner bond of the objects <= 64, whatever the weight's bonds)
        or "per-pair"."""
        return _oc.gram_route(*NDMPS._gram_chains(objs, others, weight))

    @staticmethod
    def gram(objs, others=None, as_torch: bool = False, *, weight=None):
        """
        The fp64 Gram matrix ``G[a, b] = objs[a].mps @ others[b].mps`` of a series, computed on the cores in one call
        (csrc/series.hip); ``others=None`` gives the symmetric K x K matrix, where only a <= b is computed and
        ``G[b, a]`` is a copy.  In Std and DCT mode ``G[a, b]`` is the voxel inner product of the two ``to_tensor()``
        results (the DCT is orthonormal).  Covariance, correlation, squared distances and the temporal PCA of a
        series (``pca``) are functions of G.  Storage types may mix; the same inputs give the same bits.  NumPy
        array by default, device tensor with ``as_torch=True``.  No counterpart in the reference.

        ``weight`` (an NDMPS of the same shape, site dims and mode: a mask, an ROI indicator, a window) gives the
        second moments under it, ``G_w[a, b] = sum_x w(x) X^a(x) X^b(x)``, by the exact three-chain contraction on
        the cores (csrc/wgram.hip): nothing is decoded, rounded or sketched, the weight's bonds are unrestricted, and
        the same inputs give the same bits.  ``norm`` / ``norm_value`` play no part, as without a weight.  The pairs
        are processed in chunks that keep the workspace within ``wgram.WS_LIMIT_BYTES``.

        Raises TypeError for a non-NDMPS (``weight`` included), ValueError for an empty list or objects that differ in
        qubit_size, shape, mode, device or site dims (as ``linear_combination``; the weight counts as one of them), for
        a weight in DCT mode (a product of coefficient volumes is not the product of the volumes) and when a single
        pair does not fit the workspace limit.
        """
        return _oc.gram(*NDMPS._gram_chains(objs, others, weight), as_torch=as_torch)

    def inner(self, other, *, weight=None) -> float:
        """``<self, other>``: the entry of ``NDMPS.gram([self], [other])``; with ``weight`` the entry of
        ``NDMPS.gram([self], [other], weight=weight)``, ``sum_x w(x) self(x) other(x)``."""
        return float(NDMPS.gram([self], [other], weight=weight)[0, 0])

    @staticmethod
    def pca(objs, n_components=None, center: bool = True, cutoff: float = 0.0, max_bond=None, dtype=None, *, weight=None):
        """
        Temporal PCA of a series without a decoded volume (core/series.py): from ``G = gram(objs)`` the centred Gram
        matrix ``H G H = U diag(lam) U^T`` (host, fp64), ``sigma_k = sqrt(lam_k)``; component k is the unit volume
        ``sum_a c_{a,k} objs[a]``, ``c_k = H u_k / sigma_k``, built by one ``linear_combination(objs, c_k, cutoff,
        max_bond, dtype)`` on the original objects.  Kept: ``sigma_k`` above the storage floor (1e-6 for fp32 / bf16
        work, 1e-8 for fp64) times ``max(sigma_0, largest frame norm)``, at most ``n_components``.  The entry of
        ``u_k`` with the largest magnitude is positive.  Returns a ``SeriesPCA``: singular_values, explained_variance
        (``lam / (K - 1)``, or ``lam / K`` uncentred), scores (K x r), weights (K x r), components (NDMPS) and mean
        (``linear_combination(objs, [1/K] * K, cutoff, max_bond, dtype)`` when ``center``, else None).  Errors as
        ``gram`` and ``linear_combination`` (the summed bonds of the series must not exceed 4096).

        ``weight`` (see ``gram``) makes this the PCA under the weighted inner product ``<x, y>_w = sum_x w x y``:
        ``G_w = gram(objs, weight=weight)`` takes the place of G, the components are still linear combinations of the
        unmasked objects, and each is unit-norm in the weighted norm, ``inner(c_k, c_l, weight=weight) = delta_kl``.
        The weight should be non-negative: a weight with negative values can make ``G_w`` indefinite, and its negative
        eigenvalues are clipped to zero like rounding noise.
        """
        objs = list(objs)
        _se.check_components(n_components)
        _lc.check_args(max(len(objs), 1), [0.0] * max(len(objs), 1), cutoff, max_bond)
        G = NDMPS.gram(objs, weight=weight)
        K = len(objs)
        sigma, U, W = _se.pca_weights(G, n_components, center, _lc.floor_for(_work_is_f64(objs, dtype)))
        components = [NDMPS.linear_combination(objs, W[:, k], cutoff=cutoff, max_bond=max_bond, dtype=dtype)
                      for k in range(len(sigma))]
        mean = NDMPS.linear_combination(objs, [1.0 / K] * K, cutoff=cutoff, max_bond=max_bond, dtype=dtype) if center else None
        return _se.SeriesPCA(sigma, _se.explained_variance(sigma, K, center), U * sigma[None, :], W, components, mean)

    def _scaled(self, c: float) -> "NDMPS":
        """A copy with site 0 multiplied by ``c`` (no rounding; bonds unchanged)."""
        cores = [t.clone() for t in self.mps.cores]
        cores[0].mul_(c)
        out = self._like(cores)
        out.update_boundary_list()
        out.norm_value = abs(c) * float(self.norm_value)
        spec = self.sweep_spectra
        if spec is not None:
            out.sweep_spectra = [None if s is None else abs(c) * np.asarray(s) for s in spec]
        return out

    @staticmethod
    def _real_scalar(c):
        return isinstance(c, numbers.Real) and not isinstance(c, bool) and math.isfinite(float(c))

    def __add__(self, other):
        if not isinstance(other, NDMPS):
            return NotImplemented
        return NDMPS.linear_combination([self, other], [1.0, 1.0])

    def __sub__(self, other):
        if not isinstance(other, NDMPS):
            return NotImplemented
        return NDMPS.linear_combination([self, other], [1.0, -1.0])

    def __neg__(self):
        return self._scaled(-1.0)

    def __mul__(self, c):
        if not self._real_scalar(c):
            return NotImplemented
        return self._scaled(float(c))

    __rmul__ = __mul__

    def __truediv__(self, c):
        if not self._real_scalar(c):
            return NotImplemented
        return self._scaled(1.0 / float(c))

    def continuous_compress(self, cutoff: float, print_ratio: bool = True):
        """Apply compression across a range of 20 cutoff values up to ``cutoff``."""
        for c in np.linspace(0, 1, 20) * cutoff:
            self.compress(c)
            if print_ratio:
                print(f"Compression ratio at {c}: {self.compression_ratio()}")

    # ------------------------------------------------------------------ reconstruct
    def _require_shape(self):
        if self._shape is None:
            raise ValueError("this NDMPS was not created by from_tensor; the tensor shape is unknown")
        return self._shape

    def to_tensor(self, as_torch: bool = False, dtype=None):
        """
        Convert MPS back to tensor format (with optional inverse DCT).

        Returns a NumPy array like the reference; ``as_torch=True`` keeps the result in HBM and
        ``dtype`` (e.g. ``torch.bfloat16``) selects its storage type (arithmetic stays fp32).  fp64 cores
        (``from_tensor(dtype=torch.float64)``) are contracted on the fp64 MFMA and give a float64 result.
        """
        shape = self._require_shape()
        device = self.mps.device
        with _torch().cuda.device(device):
            out = _ro.decode(self.mps, _plan_for(shape, device.index or 0), shape, self.mode == "DCT")
        if self.mode not in ("Std", "DCT"):
            return None  # ndmps.py:150-153: unknown modes fall through
        return _ro.as_result(out, as_torch, dtype, _bf16_std([self]))

    @staticmethod
    def to_tensors(objs, as_torch: bool = False):
        """
        Reconstruct a list of NDMPS (what the reference does with a Python loop, evaluation/benchmark.py:80-100).
        fp32 objects of one shape on one device are contracted by ONE library call that issues the launches of
        every volume (the per-volume Python between them left the GPU idle); anything else falls back to
        ``to_tensor`` per object.  Results equal ``[o.to_tensor() for o in objs]`` bit for bit.
        """
        torch = _torch()
        objs = list(objs)
        if not objs:
            return []
        first = objs[0]
        group = (len(objs) > 1 and first._shape is not None and first.mode in ("Std", "DCT")
                 and all(o._shape == first._shape and o.mode == first.mode and o.mps.dtype == first.mps.dtype
                         and o.mps.device == first.mps.device and o.mps.dims == first.mps.dims for o in objs))
        if not group:
            return [o.to_tensor(as_torch=as_torch) for o in objs]
        device, shape = first.mps.device, tuple(first._shape)
        with torch.cuda.device(device):
            out = _ro.decode_many([o.mps for o in objs], _plan_for(shape, device.index or 0), shape, first.mode == "DCT")
        return [_ro.as_result(r, as_torch, None, _bf16_std([o])) for o, r in zip(objs, out.unbind(0))]

    # ---------------------------------------------------------------- region decode
    def decode_region(self, key, as_torch: bool = False, dtype=None):
        """
        ``to_tensor(as_torch, dtype)[key]`` without decoding the whole volume.

        ``key`` is a NumPy OUTER index, one entry per axis: an int (negative allowed; drops its axis), a slice (any
        start / stop / step) or a 1-D integer array or list (unsorted, repeats allowed); one ``Ellipsis`` and missing
        trailing entries are full slices.  The result, its shape and its dtype are those of ``to_tensor`` indexed with
        ``np.ix_`` of the per-axis indices.  Only the prefixes of the chain that the region reaches are contracted
        (core/region.py), so time and memory follow the region, not the volume.

        Raises IndexError (index out of range, too many entries), TypeError (non-integer entries) or ValueError (no
        known shape) before anything runs on the device; returns None for modes other than Std / DCT, like to_tensor.

        DCT mode stores the last axis in the DCT domain: the last axis is decoded in full for every selected row,
        transformed back, then indexed.  A region restricted only on the last axis costs a full decode there.
        """
        shape = tuple(self._require_shape())
        return NDMPS._region(_ro.region_outer, [self], (), shape, _region.normalize_key(key, shape), as_torch, dtype)

    def values_at(self, coords, as_torch: bool = False, dtype=None):
        """
        ``to_tensor()[tuple(coords.T)]`` for an (N, ndim) integer array of points (negative indices allowed), without
        decoding the whole volume: an (N,) result of to_tensor's dtype.  Errors as ``decode_region``; in DCT mode every
        distinct row of the last axis that the points touch is decoded in full.
        """
        shape = tuple(self._require_shape())
        pts = _region.normalize_points(coords, shape)
        return NDMPS._region(_ro.region_points, [self], (), shape, (pts,), as_torch, dtype)

    # ------------------------------------------------- region decode of a series (one plan, one upload)
    @staticmethod
    def _region_series_objs(objs):
        """The checked list of a series call: TypeError for a non-NDMPS, ValueError for an empty list, objects that
        differ (``lincomb.check_compatible``) or an unknown shape."""
        objs = _checked_list(objs, "a series takes")
        if not objs:
            raise ValueError("a series needs at least one object")
        _check_compatible(objs)
        objs[0]._require_shape()
        return objs

    @staticmethod
    def _region(skeleton, objs, lead, shape, selection, as_torch, dtype):
        """``skeleton`` (``readout.region_outer`` / ``region_points``) of the normalised ``selection``, converted for the
        caller: over the chain of one object through the single entry (``lead = ()``), or over a series' chains
        (``lead = (T,)``).  None for modes other than Std / DCT, before anything runs on the device."""
        if objs[0].mode not in ("Std", "DCT"):
            return None
        first, chains = objs[0].mps, [o.mps for o in objs]
        contract = ((lambda rplan: _ro.region_series_values(chains, rplan)) if lead else
                    (lambda rplan: _ro.region_values(first, rplan)))
        with _torch().cuda.device(first.device):
            res = skeleton(contract, lead, shape, *selection, objs[0].mode == "DCT", _ro.series_work_dtype(chains),
                           first.device)
        return _ro.as_result(res, as_torch, dtype, _bf16_std(objs))

    @staticmethod
    def decode_regions(objs, key, as_torch: bool = False, dtype=None):
        """
        ``decode_region(key)`` of every frame of a series in one call: a result of shape ``(T,) + shape of
        objs[0].decode_region(key)`` whose entry ``[t]`` is ``objs[t].decode_region(key, as_torch, dtype)`` -- a voxel
        or ROI time course, a slice through time, the principal volumes of ``pca`` at a region.  The plan is built
        and uploaded once and every launch covers all frames (csrc/region.hip); a frame's values are
        those of its own ``decode_region``, bit for bit.

        ``key`` means what it means for one object, with the same IndexError / TypeError / ValueError; the list
        checks are those of ``gram`` (TypeError for a non-NDMPS, ValueError for an empty list or objects that differ
        in qubit_size, shape, mode, device or site dims).  All are raised before anything runs on the device.  Bonds
        may differ between frames.  Storage types may mix: with an fp64 frame the call contracts in fp64 (the other
        frames' cores are widened exactly) and returns float64, otherwise it contracts in fp32 and returns float32;
        ``as_torch=True`` gives bf16 only when every frame is bf16 in Std mode.  An empty region gives an empty result
        without a launch; modes other than Std / DCT return None.  No counterpart in the reference.
        """
        objs = NDMPS._region_series_objs(objs)
        shape = tuple(objs[0]._shape)
        selection = _region.normalize_key(key, shape)
        return NDMPS._region(_ro.region_outer, objs, (len(objs),), shape, selection, as_torch, dtype)

    @staticmethod
    def values_at_many(objs, coords, as_torch: bool = False, dtype=None):
        """
        ``values_at(coords)`` of every frame of a series in one call: a (T, N) result whose row ``t`` is
        ``objs[t].values_at(coords, as_torch, dtype)``, bit for bit.  Arguments, errors, mixed storage and result types
        as ``decode_regions``; ``N == 0`` gives a (T, 0) result without a launch.
        """
        objs = NDMPS._region_series_objs(objs)
        shape = tuple(objs[0]._shape)
        pts = _region.normalize_points(coords, shape)
        return NDMPS._region(_ro.region_points, objs, (len(objs),), shape, (pts,), as_torch, dtype)

    # ------------------------------------------------------------ block-averaged decode
    def _pool_levels(self, levels):
        """(factor_arr, normalised levels) for this object's shape; ValueError without one."""
        shape = self._require_shape()
        fa = _core.get_factorlist(tuple(shape))[0]
        return fa, _pool.normalize_levels(levels, len(shape), fa.shape[0])

    def block_shape(self, levels):
        """Block size ``B_a = prod(factor_arr[L - levels[a]:, a])`` per axis: the voxels that ``downsample(levels)``
        averages into one value.  ``levels`` is an int in ``[0, L]`` (L = number of sites) or one int per axis.
        Host only."""
        fa, lev = self._pool_levels(levels)
        return _pool.block_shape(fa, lev)

    def downsample(self, levels=1, op: str = "mean", as_torch: bool = False, dtype=None):
        """
        The volume averaged (``op="mean"``) or summed (``op="sum"``) over blocks of ``block_shape(levels)`` voxels:
        ``to_tensor()`` reshaped to ``(n0 / B0, B0, n1 / B1, B1, ...)`` and reduced over the odd axes, without
        decoding the whole volume.  ``levels`` is an int in ``[0, L]`` or one per axis; axis ``a`` is reduced over
        the digits of its last ``levels[a]`` sites.  ``levels = 0`` equals ``to_tensor()``; ``levels = L`` gives a
        ``(1, ..., 1)`` array.

        The last sites of the chain carry the finest digits, so the reduction is a site-local sum over the cores
        (core/pool.py, csrc/pool.hip); only the coarse volume is contracted.  In DCT mode a full reduction of the
        last axis picks its DC coefficient on the sites; a partial one decodes the coefficient rows of the coarse
        volume and pools them with one GEMM.

        Result types as ``decode_region``.  Raises TypeError (non-integer levels) or ValueError (levels outside
        [0, L], wrong count, unknown ``op``, no known shape) before anything runs on the device; returns None for
        modes other than Std / DCT, like to_tensor.
        """
        if op not in ("mean", "sum"):
            raise ValueError(f"op must be 'mean' or 'sum', got {op!r}")
        fa, lev = self._pool_levels(levels)
        if self.mode not in ("Std", "DCT"):
            return None
        with _torch().cuda.device(self.mps.device):
            res = _ro.pooled(self.mps, self._shape, fa, lev, op, self.mode == "DCT")
        return _ro.as_result(res, as_torch, dtype, _bf16_std([self]))

    def _axis_reduce(self, axis, keepdims, op, as_torch, dtype):
        shape = self._require_shape()
        ndim = len(shape)
        axes = _pool.normalize_axes(axis, ndim)
        fa = _core.get_factorlist(tuple(shape))[0]
        lev = np.array([fa.shape[0] if a in axes else 0 for a in range(ndim)], dtype=np.int64)
        if self.mode not in ("Std", "DCT"):
            return None
        with _torch().cuda.device(self.mps.device):
            res = _ro.pooled(self.mps, self._shape, fa, lev, op, self.mode == "DCT")
            if not keepdims:
                res = res.reshape([n for a, n in enumerate(res.shape) if a not in axes])
        return _ro.as_result(res, as_torch, dtype, _bf16_std([self]))

    def sum(self, axis=None, keepdims: bool = False, as_torch: bool = False, dtype=None):
        """``to_tensor().sum(axis=axis, keepdims=keepdims)`` without decoding the whole volume (``downsample`` with
        every level on the reduced axes).  ``axis``: None, an int or a tuple (negative allowed).  ``axis=None``
        without keepdims gives a NumPy scalar.  TypeError for non-integer axes, numpy's AxisError out of range,
        ValueError for a repeated axis or no known shape; None for modes other than Std / DCT."""
        return self._axis_reduce(axis, keepdims, "sum", as_torch, dtype)

    def mean(self, axis=None, keepdims: bool = False, as_torch: bool = False, dtype=None):
        """``to_tensor().mean(axis=axis, keepdims=keepdims)`` without decoding the whole volume; as ``sum``."""
        return self._axis_reduce(axis, keepdims, "mean", as_torch, dtype)

    # ---------------------------------------------------- value statistics on the cores (core/valstat.py)
    def _valstat_chain(self, what, with_plan=False):
        """The chain of a statistics call (``with_plan``: and the permutation plan of its shape, for the calls that read
        an original), or the ValueError that refuses it."""
        if self.mode == "DCT":
            raise ValueError(f"DCT mode stores DCT coefficients: {what} of the chain is not {what} of the volume")
        if self.mode != "Std":
            raise ValueError(f"{what} needs a Std mode object, this one has mode {self.mode!r}")
        if self.mps.dtype == _torch().bfloat16:
            raise ValueError(f"{what} runs on fp32 or fp64 cores: convert bf16 cores with astype(torch.float32) first")
        shape = self._require_shape()
        return (self.mps, _plan_for(shape, self.mps.device.index or 0)) if with_plan else self.mps

    def value_stats(self) -> dict:
        """``count, min, max, sum, sumsq, n_nan`` of ``to_tensor()`` and the derived ``mean``, ``std`` (population) and
        ``norm`` (Frobenius), without decoding the volume: the chain's last product reduces its tiles instead of storing
        them (csrc/valstat.hip, csrc/valstat_device.h), so only the small left and tail buffers of the decode are written.  Sums are fp64; NaN
        voxels are counted in ``n_nan`` and left out of everything else; the same object gives the same bits.  The
        voxel values are those of ``to_tensor()`` within the forward error bound of the chain, not bit for bit.

        Raises ValueError for DCT mode (the chain holds coefficients), bf16 cores (``astype(torch.float32)`` first) and
        an unknown shape.  Std mode, fp32 and fp64 cores.  No counterpart in the reference."""
        from . import valstat as _vs

        chain = self._valstat_chain("value_stats")
        return _vs.value_stats(chain)

    def min(self, axis=None):
        """``to_tensor().min()`` from the cores (``value_stats``); an ``axis`` raises NotImplementedError: ``amin`` takes one."""
        if axis is not None:
            raise NotImplementedError("min over an axis is not implemented: only the whole volume (axis=None)")
        return self.value_stats()["min"]

    def max(self, axis=None):
        """``to_tensor().max()`` from the cores (``value_stats``); an ``axis`` raises NotImplementedError: ``amax`` takes one."""
        if axis is not None:
            raise NotImplementedError("max over an axis is not implemented: only the whole volume (axis=None)")
        return self.value_stats()["max"]

    def amax(self, axis=None, keepdims: bool = False, as_torch: bool = False):
        """``to_tensor().max(axis, keepdims=keepdims)`` from the cores, in the cores' element type: a maximum-intensity
        projection without the volume (core/axisext.py).  ``axis``: an int or a tuple of ints, negative values from the
        end; None or every axis gives the scalar of ``value_stats``.  A NumPy array, or a device tensor with
        ``as_torch``.  NaN voxels take no part (``np.fmax.reduce``); a ray of NaN only gives NaN.  numpy's AxisError for
        an axis out of range, ValueError for a repeated axis and what ``value_stats`` refuses."""
        from . import axisext as _ax

        chain, plan = self._valstat_chain("amax", with_plan=True)
        return _ax.reduce_values(chain, plan, "max", axis, keepdims, as_torch)

    def amin(self, axis=None, keepdims: bool = False, as_torch: bool = False):
        """``to_tensor().min(axis, keepdims=keepdims)`` from the cores; as ``amax``."""
        from . import axisext as _ax

        chain, plan = self._valstat_chain("amin", with_plan=True)
        return _ax.reduce_values(chain, plan, "min", axis, keepdims, as_torch)

    def argmax(self, axis=None, keepdims: bool = False, as_torch: bool = False, return_values: bool = False):
        """``np.argmax(to_tensor(), axis, keepdims=keepdims)`` from the cores: an int64 array of the first occurrence
        along an int ``axis``, or with ``axis=None`` the flat C-order index as an int.  ``return_values=True`` returns
        ``(indices, values)`` from the same call.  NaN voxels take no part; a ray (or a volume) of NaN only has index
        -1.  TypeError for a tuple ``axis``, as NumPy's; otherwise the refusals of ``amax``."""
        from . import axisext as _ax

        chain, plan = self._valstat_chain("argmax", with_plan=True)
        return _ax.reduce_index(chain, plan, "max", axis, keepdims, as_torch, return_values)

    def argmin(self, axis=None, keepdims: bool = False, as_torch: bool = False, return_values: bool = False):
        """``np.argmin(to_tensor(), axis, keepdims=keepdims)`` from the cores; as ``argmax``."""
        from . import axisext as _ax

        chain, plan = self._valstat_chain("argmin", with_plan=True)
        return _ax.reduce_index(chain, plan, "min", axis, keepdims, as_torch, return_values)

    def count_between(self, lo=None, hi=None, invert: bool = False) -> int:
        """The number of non-NaN voxels of ``to_tensor()`` with ``lo <= v <= hi`` (None: unbounded; ``invert``: the
        non-NaN voxels outside the interval), from the cores: the clipped moments pass of ``value_stats``.  The bounds
        are cast to the cores' element type and compared with the computed voxel in that type, so the count equals
        ``len(find(lo, hi)[0])`` and the one bin of ``histogram(bins=[lo, hi])``.  ValueError for a NaN bound,
        ``lo > hi`` and what ``value_stats`` refuses."""
        from . import select as _sel

        chain = self._valstat_chain("count_between")
        return _sel.count_between(chain, lo, hi, invert)

    def find(self, lo=None, hi=None, *, invert: bool = False, max_count: int = 1 << 20, coords: bool = False,
             as_torch: bool = False):
        """``(index, values)`` of the voxels of ``to_tensor()`` with ``lo <= v <= hi``, without the volume
        (core/select.py, csrc/select.hip): ``index`` is ``np.flatnonzero((v >= lo) & (v <= hi))``, int64 flat C-order
        indices ascending, or with ``coords`` their ``np.unravel_index`` as a (K, ndim) int64 array, and ``values`` the
        voxels there in the cores' element type.  ``invert`` selects the non-NaN voxels outside the interval; NaN voxels
        are never selected (``find_nan`` lists them).  The call counts first and allocates exactly the K slots; more
        than ``max_count`` matches raise ValueError naming the count, nothing is truncated.  NumPy arrays, or device
        tensors with ``as_torch``; the same object gives the same bytes.  ValueError for a NaN bound, ``lo > hi``, a
        negative ``max_count`` and what ``value_stats`` refuses."""
        from . import select as _sel

        _sel.check_find(self._valstat_chain("find"), lo, hi, max_count)  # the refusals that need no device, first
        chain, plan = self._valstat_chain("find", with_plan=True)
        return _sel.find(chain, plan, lo, hi, invert, max_count, coords, as_torch)

    def find_nan(self, max_count: int = 1 << 20, coords: bool = False):
        """The flat C-order indices (``coords``: the (K, ndim) coordinates) of the NaN voxels of ``to_tensor()``,
        ascending, from the cores; as ``find``."""
        from . import select as _sel

        _sel.check_find(self._valstat_chain("find_nan"), None, None, max_count)
        chain, plan = self._valstat_chain("find_nan", with_plan=True)
        return _sel.find_nan(chain, plan, max_count, coords)

    def topk(self, k, largest: bool = True, *, max_count: int = 1 << 20, coords: bool = False, as_torch: bool = False):
        """``(index, values)`` of the ``k`` largest (``largest=False``: smallest) non-NaN voxels of ``to_tensor()``, from
        the cores: ordered by value and among equal values by ascending flat index, ``np.lexsort((flat_index, -v))[:k]``;
        all of them where fewer than ``k`` are not NaN.  Histogram passes bracket the k-th value as ``quantile``'s do,
        until one ``find`` of at most ``max_count`` voxels holds the answer; where more than that tie at the k-th value
        ``t`` the strictly better voxels come first and the first ties in C order fill up.  ValueError for ``k < 1``, for
        ``k`` or the ties at ``t`` beyond ``max_count``, and what ``find`` refuses."""
        from . import select as _sel

        _sel.check_topk(self._valstat_chain("topk"), k, max_count)
        chain, plan = self._valstat_chain("topk", with_plan=True)
        return _sel.topk(chain, plan, k, largest, max_count, coords, as_torch)

    def histogram(self, bins=256, range=None, outliers: bool = False, mask=None):
        """``numpy.histogram(to_tensor(), bins, range)`` from the cores: ``(counts int64, edges)``.  ``bins`` is an int
        or an explicit ascending edge array (at most 4096 bins; the edges are cast to the cores' element type and
        returned as used); bin b holds ``edges[b] <= v < edges[b + 1]`` and the last bin its right edge too, exactly,
        for the voxel values the chain computes.  ``range=None`` with an int runs the moments pass first for min and
        max.  ``outliers=True`` adds ``(n_below, n_above, n_nan)``; bins and outliers always sum to the voxel count.

        ``mask`` (a bool or integer volume of the object's shape, non-zero meaning inside) bins only the voxels inside
        it, through ``label_histogram`` with two labels; the edges are the same (an int ``bins`` with ``range=None``
        spans the whole volume's min and max) and bins and outliers sum to the voxels inside the mask.

        Raises ValueError for more than 4096 bins, edges that are not ascending, a range that is not finite, and what
        ``value_stats`` refuses; with a mask TypeError for one that is not bool or integer and ValueError for another
        shape."""
        from . import valstat as _vs

        if mask is not None:
            from . import labelhist as _lh

            chain, plan = self._valstat_chain("histogram", with_plan=True)
            return _lh.masked_histogram(chain, plan, mask, bins, range, outliers)
        chain = self._valstat_chain("histogram")
        return _vs.histogram(chain, bins, range, outliers)

    def quantile(self, q, passes: int = 2, bins: int = 4096, mask=None):
        """The ``q``-quantile of the voxels (rank ``ceil(q N)``, numpy's ``method="inverted_cdf"``) by repeated
        histograms from the cores: ``(value, (lo, hi))``.  After each of up to ``passes`` histograms the bracket is the
        one bin that holds the rank, and the next pass bins inside it; the search stops early once the bracket is one
        number.  A last pass looks inside the bracket: one distinct value there is returned exactly, otherwise
        ``value`` is the midpoint of the bracket ``(lo, hi)``, its smallest and largest voxel.  ``mask`` (as
        ``histogram`` takes it) gives the quantile of the voxels inside it, through ``label_quantile`` with two labels.
        ValueError for ``q`` outside [0, 1], ``bins`` outside [1, 4096] and what ``value_stats`` refuses."""
        from . import valstat as _vs

        if mask is not None:
            from . import labelhist as _lh

            chain, plan = self._valstat_chain("quantile", with_plan=True)
            return _lh.masked_quantile(chain, plan, mask, q, passes, bins)
        chain = self._valstat_chain("quantile")
        return _vs.quantile(chain, q, passes, bins)

    def median(self, mask=None) -> float:
        """The median of the voxels (``quantile(0.5, mask=mask)[0]``: numpy's ``method="inverted_cdf"``), of the whole
        volume or of the voxels inside ``mask``; NaN where there is no non-NaN voxel."""
        return self.quantile(0.5, mask=mask)[0]

    def error_to(self, x) -> dict:
        """The error of ``to_tensor()`` against ``x`` (NumPy array or device tensor of the object's shape, cast to the
        cores' element type) without decoding: ``sse, mse, max_abs, ref_sumsq, ref_max, rel_frob`` (and ``n_nan``, the
        voxels whose difference is NaN).  ``x`` is read once, through the offset tables of the fused decode.
        ValueError for another shape and what ``value_stats`` refuses."""
        from . import valstat as _vs

        chain, plan = self._valstat_chain("error_to", with_plan=True)
        return _vs.error_to(chain, plan, x)

    def psnr_to(self, x) -> float:
        """``compute_psnr(x, to_tensor())`` from the cores: ``10 log10(max(x)^2 / mse)``, ``inf`` at mse = 0."""
        from . import valstat as _vs

        chain, plan = self._valstat_chain("psnr_to", with_plan=True)
        return _vs.psnr_from(_vs.error_to(chain, plan, x))

    def label_stats(self, labels, n_labels=None) -> dict:
        """Statistics of ``to_tensor()`` under each label of an atlas or segmentation, without decoding: ``labels`` is an
        integer NumPy array or device tensor of the object's shape, and the result a dict of arrays of length
        ``n_labels`` (None: ``max(labels) + 1``; at most 4096): ``count``, ``n_nan``, ``sum``, ``sumsq``, ``min``,
        ``max``, ``mean``, ``std`` (population; NaN for a label without a voxel), and the scalars ``outside`` (voxels
        whose label is negative or not below ``n_labels``), ``s`` and ``s2`` (core/labelstat.py).  The sums are 64-bit
        fixed-point integers scaled by ``2**-s`` and ``2**-s2``, added in integer arithmetic: the same inputs give
        the same bits.  NaN voxels are counted per label and left out of the rest.

        Raises TypeError for labels that are not integers, ValueError for another shape, labels beyond int32, more
        than 4096 labels, an infinite voxel, and what ``value_stats`` refuses."""
        from . import labelstat as _ls

        chain, plan = self._valstat_chain("label_stats", with_plan=True)
        return _ls.label_stats(chain, plan, labels, n_labels)

    @staticmethod
    def label_stats_many(objs, labels, n_labels=None) -> dict:
        """``label_stats`` of every frame of a series against one atlas: the same dict with arrays of shape
        ``(T, n_labels)``, so ``["mean"]`` holds the parcel time courses; ``outside``, ``s`` and ``s2`` have length T.
        The atlas and the offset tables go to the device once and one workspace serves every frame; row t equals
        ``objs[t].label_stats(labels, n_labels)`` bit for bit.  Bonds and storage types (fp32, fp64) may differ between
        frames.  The list checks are those of ``decode_regions``; otherwise the refusals of ``label_stats``."""
        from . import labelstat as _ls

        objs = NDMPS._region_series_objs(objs)
        pairs = [o._valstat_chain("label_stats_many", with_plan=True) for o in objs]
        return _ls.label_stats_many([chain for chain, _ in pairs], pairs[0][1], labels, n_labels)

    def label_histogram(self, labels, n_labels=None, bins=64, range=None, outliers: bool = False):
        """``numpy.histogram(to_tensor()[labels == l], bins, range)`` for every label l of an atlas, without decoding:
        ``(counts (n_labels, bins) int64, edges)`` (core/labelhist.py, csrc/labelhist.hip).  ``labels`` and ``n_labels``
        are ``label_stats``'s; ``bins`` and ``range`` are ``histogram``'s and give the edges it uses (an int ``bins``
        with ``range=None`` spans the whole volume's min and max).  ``outliers=True`` adds a dict of ``below``,
        ``above``, ``n_nan`` (int64 per label) and ``outside``: every voxel is in exactly one of the five.  Only
        integers are added: the same inputs give the same bits.

        Raises what ``label_stats`` and ``histogram`` raise, except that an infinite voxel is binned and not refused, and
        ValueError for a call whose labels and bins need more than 64 launches (fewer bins, or split the atlas)."""
        from . import labelhist as _lh

        chain, plan = self._valstat_chain("label_histogram", with_plan=True)
        return _lh.label_histogram(chain, plan, labels, n_labels, bins, range, outliers)

    @staticmethod
    def label_histogram_many(objs, labels, n_labels=None, bins=64, range=None, outliers: bool = False):
        """``label_histogram`` of every frame of a series against one atlas and one edge table: counts of shape
        ``(T, n_labels, bins)``.  With an int ``bins`` and ``range=None`` the range is the minimum and maximum over all
        frames.  The atlas and the offset tables go to the device once and one workspace serves every frame; row t
        equals ``objs[t].label_histogram(labels, n_labels, edges)`` bit for bit.  The list checks are those of
        ``label_stats_many``."""
        from . import labelhist as _lh

        objs = NDMPS._region_series_objs(objs)
        pairs = [o._valstat_chain("label_histogram_many", with_plan=True) for o in objs]
        return _lh.label_histogram_many([chain for chain, _ in pairs], pairs[0][1], labels, n_labels, bins, range, outliers)

    def label_quantile(self, labels, q, n_labels=None, passes: int = 2, bins: int = 64) -> dict:
        """The ``q``-quantile (numpy's ``method="inverted_cdf"``; ``q`` a number or a 1-D sequence) of the voxels under
        each label, without decoding: a dict of ``value``, ``lo``, ``hi`` (float64, ``(n_labels,)`` or ``(n_labels, Q)``),
        ``count``, ``n_nan`` and ``outside``.  Histograms with one edge row per label narrow every label's bracket
        ``passes`` times by ``bins``; a last launch finds the smallest and largest voxel inside each bracket, so
        ``value`` is exact where they coincide and their midpoint otherwise, and ``lo <= true quantile <= hi``.  NaN for
        a label without a non-NaN voxel.  The refusals of ``label_histogram``."""
        from . import labelhist as _lh

        chain, plan = self._valstat_chain("label_quantile", with_plan=True)
        return _lh.label_quantile(chain, plan, labels, q, n_labels, passes, bins)

    def label_median(self, labels, n_labels=None, passes: int = 2, bins: int = 64):
        """``label_quantile(labels, 0.5, ...)["value"]``: the median of the voxels under each label."""
        from . import labelhist as _lh

        chain, plan = self._valstat_chain("label_median", with_plan=True)
        return _lh.label_median(chain, plan, labels, n_labels, passes, bins)

    # ---------------------------------------------------- statistics of two objects on the cores (core/pairstat.py)
    def _pairstat_chains(self, other, what):
        """The two chains of a pair call, or the error that refuses it: TypeError for a non-NDMPS, ValueError naming what
        differs (shape, mode, qubit_size -- the factor array --, device, site dims) and what ``value_stats`` refuses."""
        if not isinstance(other, NDMPS):
            raise TypeError(f"{what} takes NDMPS objects, not {type(other).__name__}")
        chains = self._valstat_chain(what), other._valstat_chain(what)
        _check_compatible([self, other])
        return chains

    def pair_stats(self, other) -> dict:
        """Moments of this volume (a) and ``other`` (b) over the voxels where neither is NaN, from the cores of both,
        with neither volume decoded (csrc/pairstat.hip): ``count`` (those voxels), ``n_nan`` (the others), ``sum_a,
        sum_b, sumsq_a, sumsq_b, sum_ab, sse`` (``sum (a - b)^2``), ``max_abs_diff, min_a, max_a, min_b, max_b``, and
        derived on the host in fp64 ``mean_a, mean_b, cov, pearson, mse, rel_frob`` (``||a - b|| / ||b||``).  Sums are
        fp64; the same objects give the same bits.  One fp32 and one fp64 object make the call fp64.

        Raises TypeError for a non-NDMPS, ValueError for objects that differ in shape, mode, qubit_size, device or site
        dims, and what ``value_stats`` refuses of either (DCT mode, bf16 cores, an unknown shape)."""
        from . import pairstat as _ps

        return _ps.pair_stats(*self._pairstat_chains(other, "pair_stats"))

    def joint_histogram(self, other, bins=64, range=None, outliers: bool = False):
        """``numpy.histogram2d(self.to_tensor().ravel(), other.to_tensor().ravel(), bins, range)`` from the cores of
        both: ``(counts int64 (bins_a, bins_b), edges_a, edges_b)``.  ``bins`` is an int, a pair of ints or a pair of
        explicit ascending edge arrays (at most 1024 bins per axis and 16384 cells); ``range`` is None or
        ``((lo_a, hi_a), (lo_b, hi_b))``, and with None an int takes that object's own min and max from a moments
        pass.  The edges of an axis are those ``histogram`` builds from the same arguments, and the row and column sums
        are the single histograms bit for bit.  ``outliers=True`` adds ``(outside, n_nan)``: the voxels with either
        value out of range, and those with either value NaN; cells and outliers always sum to the voxel count.
        Errors as ``pair_stats`` and ``histogram``."""
        from . import pairstat as _ps

        return _ps.joint_histogram(*self._pairstat_chains(other, "joint_histogram"), bins, range, outliers)

    def mutual_information(self, other, bins=64, range=None, normalized: bool = False) -> float:
        """Mutual information of the two volumes in nats, from ``joint_histogram(other, bins, range)`` on the host in
        fp64: ``sum p_ij ln(p_ij / (p_i. p_.j))`` over the non-empty cells, p over the binned voxels -- the similarity
        measure of multi-modal registration, where the cross-correlation of ``inner`` fails.  ``normalized=True``
        returns ``(H(a) + H(b)) / H(a, b)`` (Studholme), 1.0 when ``H(a, b) == 0``."""
        from . import pairstat as _ps

        return _ps.mutual_information(*self._pairstat_chains(other, "mutual_information"), bins, range, normalized)

    @staticmethod
    def mutual_information_many(objs, ref, bins=64, range=None, normalized: bool = False):
        """``objs[t].mutual_information(ref, ...)`` for every frame as a ``(T,)`` fp64 array.  The edges of ``ref`` are
        fixed once; entry t equals the single call with those edges bit for bit.  A loop of single calls."""
        from . import pairstat as _ps

        objs = _checked_list(objs, "mutual_information_many takes")
        pairs = [o._pairstat_chains(ref, "mutual_information_many") for o in objs]
        return _ps.mutual_information_many([a for a, _ in pairs], pairs[0][1] if pairs else None, bins, range, normalized)

    # ---------------------------------------------------- two values per voxel under an atlas (core/labelpair.py)
    def label_pair_stats(self, other, labels, n_labels=None) -> dict:
        """``pair_stats`` of this volume (a) and ``other`` (b) under each label of an atlas, from the cores of both with
        neither decoded (csrc/labelpair.hip).  ``labels`` and ``n_labels`` are ``label_stats``'s.  A dict of arrays of
        length ``n_labels`` over the voxels of each label where neither value is NaN: ``count``, ``n_nan`` (voxels
        where either is), ``sum_a, sum_b, sumsq_a, sumsq_b, sum_ab, sse, max_abs_diff, min_a, max_a, min_b, max_b``, the
        derived ``mean_a, mean_b, cov, pearson, mse, rel_frob`` (NaN for a label without a counted voxel, whose sums
        are 0), the scalar ``outside`` and ``scales``, a dict of the six exponents of the 64-bit fixed-point sums.
        Only integers are added: the same inputs give the same bits, and where neither volume has a NaN the fields of
        a and of b are those of ``label_stats`` bit for bit.  One fp32 and one fp64 object make the call fp64.

        Raises what ``pair_stats`` and ``label_stats`` raise, an infinite voxel in either volume included."""
        from . import labelpair as _lp

        a, b = self._pairstat_chains(other, "label_pair_stats")
        _, plan = self._valstat_chain("label_pair_stats", with_plan=True)
        return _lp.label_pair_stats(a, b, plan, labels, n_labels)

    @staticmethod
    def label_pair_stats_many(objs, ref, labels, n_labels=None) -> dict:
        """``objs[t].label_pair_stats(ref, labels, n_labels)`` for every frame of a series against one reference
        object: the same dict with arrays of shape ``(T, n_labels)``; ``outside`` and each entry of ``scales`` have
        length T.  The atlas and the offset tables go to the device once and one workspace serves every frame; row t
        equals the single call bit for bit.  The list checks are those of ``label_stats_many``."""
        from . import labelpair as _lp

        objs = NDMPS._region_series_objs(objs)
        pairs = [o._pairstat_chains(ref, "label_pair_stats_many") for o in objs]
        _, plan = objs[0]._valstat_chain("label_pair_stats_many", with_plan=True)
        return _lp.label_pair_stats_many([a for a, _ in pairs], pairs[0][1], plan, labels, n_labels)

    def label_error_to(self, x, labels, n_labels=None) -> dict:
        """``error_to(x)`` under each label of an atlas, without decoding: the error of the encoding in the lesion, the
        hippocampus or the cortex ribbon and not in the air around the head.  ``x`` is the original (cast to the
        cores' element type), read at the address where the label is read.  A dict of arrays of length ``n_labels``:
        ``count, n_nan, sse, mse, max_abs, ref_sumsq, ref_max, rel_frob, psnr``, and the scalars ``outside`` and
        ``peak``, the maximum of ``x`` that ``psnr_to`` uses (``error_to(x)["ref_max"]``); ``psnr[l]`` is
        ``10 log10(peak^2 / mse[l])``, comparable with ``psnr_to(x)``.  The same computation as ``label_pair_stats``
        with ``b := x``.  Raises what ``error_to`` and ``label_stats`` raise, and ValueError for an infinite element
        of ``x``."""
        from . import labelpair as _lp

        chain, plan = self._valstat_chain("label_error_to", with_plan=True)
        return _lp.label_error_to(chain, plan, x, labels, n_labels)

    # ---------------------------------------------------- quantise / on-disk size
    def compress_to_dtype(self, dtype=np.uint16, replace: bool = False):
        """Integer-truncate each MPS tensor to the given unsigned dtype (ndmps.py:182-207)."""
        arrays = self.mps.arrays
        q_dev = [_ft.scale_to_dtype(a.tensor, dtype) for a in arrays]
        if replace:
            back = [_ft.scale_back(q, b[0], b[1], dtype, out_dtype=a.tensor.dtype)
                    for q, b, a in zip(q_dev, self.boundary_list, arrays)]
            self.replace_tensordata(back)
        return [_ft.to_numpy_uint(q, dtype) for q in q_dev]

    def get_bytesize_on_disk(self, dtype=np.uint16, replace: bool = False) -> int:
        """Estimate gzipped bytesize of MPS after dtype compression (gzip runs on the host)."""
        total_bytes = 0
        for arr in self.compress_to_dtype(dtype, replace):
            buf = io.BytesIO()
            with gzip.GzipFile(fileobj=buf, mode="wb") as gz:
                gz.write(arr.tobytes())
            total_bytes += len(buf.getvalue())
        return total_bytes

    def compression_ratio_on_disk(self, dtype=np.uint16, replace: bool = False) -> float:
        """Compressed size (gzipped) / uncompressed original size in the target dtype."""
        original_size = np.prod(self.qubit_size) * _ft.get_num_bits(dtype) / 8.0
        return self.get_bytesize_on_disk(dtype, replace) / original_size

    def get_storage_space(self, dtype=np.uint16, verbose: bool = False) -> float:
        """Estimate uncompressed storage in bytes using the given dtype."""
        size_bytes = self.number_elements_in_MPS() * _ft.get_num_bits(dtype) / 8
        if verbose:
            print(f"The storage space is approximately: {size_bytes / 1024:.2f} KB")
        return size_bytes
