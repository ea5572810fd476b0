"""The device layer of the decoders: everything that turns cores back into voxels.  Every ctypes call of
``ndmps_chain_contract_scatter_batched_f32``, ``ndmps_chain_batched_workspace_bytes``, ``ndmps_decode_permute`` /
``_many``, ``ndmps_idct_last_*``, ``ndmps_region_*`` and ``ndmps_pool_*``, the dense products of the pooled decode and
the read-out use of ``ndmps_chain_tail_columns``.

The convention of core/valstat.py and core/oncore.py: functions take ``DeviceMPS`` chains, a permutation plan
(core/plan.py) and plain metadata, and return device tensors.  Nothing here knows ``NDMPS``: its methods check keys,
modes and lists, call in here, and convert with ``as_result``.  The four region decoders are two skeletons,
``region_outer`` and ``region_points``, whose leading axes ``lead`` are ``()`` for one object and ``(T,)`` for a series.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _lib
from . import pool as _pool
from . import region as _region
from .mps import DeviceMPS, _torch
from .plan import _dct_basis, _plan_for, _pooled_dct_basis, _ptr_array, _span


def as_result(res, as_torch, dtype, bf16_std):
    """A decoded device tensor as what the caller asked for -- to_tensor's result types: float64 if the call contracted
    in fp64, float32 otherwise; as_torch with ``bf16_std`` (every frame has bf16 cores and the mode is Std) gives bf16
    like to_tensor's bf16 chain (the NumPy result keeps the fp32 contraction unrounded)."""
    torch = _torch()
    if as_torch:
        if dtype is None and bf16_std:
            dtype = torch.bfloat16
        return res if dtype is None else res.to(dtype)
    arr = (res if res.dtype == torch.float64 else res.to(torch.float32)).cpu().numpy()
    return arr[()] if arr.ndim == 0 else arr  # all-int keys give a NumPy scalar, as to_tensor()[i, j, k]


# ------------------------------------------------------------------------------------------------ full decode
def fused_tail_columns(dtype, dims):
    """Columns of the chain's last product that scatter straight into the C-order volume (the fused decode of fp32
    cores); 0: contract the chain in site order and permute afterwards."""
    if dtype != _torch().float32 or os.environ.get("NDMPS_NO_FUSED_DECODE"):  # the switch: A/B timing
        return 0
    return int(_lib.load().ndmps_chain_tail_columns(len(dims), _lib.i64_array(dims)))


def decode_chain(chain, plan, shape):
    """One chain (a DeviceMPS whose site-order tensor ``plan`` maps onto ``shape``) as a C-order device tensor in the
    chain's own type.  Runs on the chain's device, which the caller has made current."""
    torch = _torch()
    device = chain.device
    n_tail = fused_tail_columns(chain.dtype, chain.dims)
    if n_tail > 0:
        # fp32: the inverse permutation rides on the last product of the chain; no site-order tensor
        out = torch.empty(shape, dtype=torch.float32, device=device)
        with _span("chain"):
            chain.to_volume(out, n_tail, plan.split_tables(n_tail, device))
    else:
        with _span("chain"):
            dense = chain.to_dense()
        out = torch.empty(shape, dtype=dense.dtype, device=device)
        with _span("decode_permute"):
            _lib.check(_lib.load().ndmps_decode_permute(plan.handle, dense.data_ptr(), out.data_ptr(),
                                                        dense.element_size(), _lib.stream_ptr()))
    return out


def decode_chains_f32(batch, L, cdims, bonds, cores, n_tail, plan, shape, device, dct):
    """``batch`` fp32 chains of one shape -- ``cores``: batch x L device pointers, ``bonds``: batch x (L + 1) -- as one
    (batch,) + shape tensor, inverse DCT included (``dct``): ONE library call issues the launches of every volume.
    Buffers are taken in the order reconstruction, chain workspace, IDCT output, and the workspace is held until the
    IDCT is enqueued (the encode path depends on that order: the allocator note in NDMPS._encode_group)."""
    torch = _torch()
    lib = _lib.load()
    row_off, col_off, col_perm = plan.split_tables(n_tail, device)
    out = torch.empty((batch,) + tuple(shape), dtype=torch.float32, device=device)
    ws_bytes = int(lib.ndmps_chain_batched_workspace_bytes(batch, L, cdims, bonds))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    base, step = out.data_ptr(), plan.numel * 4
    outs = (C.c_void_p * batch)(*[base + b * step for b in range(batch)])
    with _span("chain"):
        _lib.check(lib.ndmps_chain_contract_scatter_batched_f32(
            batch, L, cdims, bonds, cores, outs, row_off.data_ptr(), col_off.data_ptr(), col_perm.data_ptr(),
            n_tail, ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
    # the volumes sit back to back in `out`: their rows are the rows of one tall matrix, one launch
    return idct_last(out, shape[-1]) if dct else out


def idct_last(x, n):
    """Inverse DCT along rows of length ``n`` that lie contiguous in ``x`` (a volume's last axis, the volumes of a
    group back to back, the rows of a region), as a new tensor of x's shape: float64 for float64, float32 otherwise."""
    torch = _torch()
    lib = _lib.load()
    f64 = x.dtype == torch.float64
    if not f64:
        x = x.to(torch.float32)  # the IDCT kernel is fp32 (bf16 storage: upcast copy)
    rec = torch.empty_like(x)
    idct = lib.ndmps_idct_last_f64 if f64 else lib.ndmps_idct_last_f32
    _lib.check(idct(x.data_ptr(), rec.data_ptr(), x.numel() // n, n, _dct_basis(n, x.device, f64).data_ptr(),
                    _lib.stream_ptr()))
    return rec


def decode(chain, plan, shape, dct):
    """``to_tensor``: the chain as a C-order volume, inverse DCT of the last axis included (``dct``)."""
    out = decode_chain(chain, plan, shape)
    return idct_last(out, shape[-1]) if dct else out


def decode_many(chains, plan, shape, dct):
    """``to_tensors`` of a group (chains of one type, device and site dims over one shape) as one (batch,) + shape tensor.
    fp32 cores: the fused decode of the group in one library call; otherwise a chain per volume, then the inverse
    permutation and the IDCT of the whole group in one launch each (to_tensor's steps, ndmps.py:140-153)."""
    torch = _torch()
    first, batch = chains[0], len(chains)
    device, dims = first.device, first.dims
    n_tail = fused_tail_columns(first.dtype, dims)
    if n_tail > 0:
        bonds = _lib.i64_array([k for m in chains for k in m.bonds])
        cores = _ptr_array([c for m in chains for c in m.cores])
        return decode_chains_f32(batch, len(dims), _lib.i64_array(dims), bonds, cores, n_tail, plan, shape, device, dct)
    with _span("chain"):
        denses = [m.to_dense() for m in chains]
    out = torch.empty((batch,) + tuple(shape), dtype=denses[0].dtype, device=device)
    with _span("decode_permute"):
        _lib.check(_lib.load().ndmps_decode_permute_many(plan.handle, batch, _ptr_array(denses),
                                                         _ptr_array(list(out.unbind(0))), denses[0].element_size(),
                                                         _lib.stream_ptr()))
    del denses
    return idct_last(out, shape[-1]) if dct else out


# ------------------------------------------------------------------------------------------------ region decode
def _region_tables(dims, rplan, device):
    """What both region entries take of a plan (core/region.py): (site dims, nodes, tiles, device tables), every table
    in one upload."""
    return (_lib.i64_array(dims), _lib.i64_array(rplan.nodes), _lib.i64_array(rplan.n_tiles),
            _torch().from_numpy(rplan.tables()).to(device))


def region_values(chain, rplan):
    """The plan's output elements contracted from the cores (ndmps_region_contract_*): a flat device tensor, fp64 for
    fp64 cores, fp32 otherwise (bf16 cores are upcast as for the overlap)."""
    torch = _torch()
    lib = _lib.load()
    f64 = chain.dtype == torch.float64
    work = torch.float64 if f64 else torch.float32
    keep, ptrs = chain._ptrs_as(work)
    L, device, bonds = chain.L, chain.device, _lib.i64_array(chain.bonds)
    dims, nodes, tiles, tables = _region_tables(chain.dims, rplan, device)
    ws_bytes = int(lib.ndmps_region_workspace_bytes(L, bonds, nodes, 8 if f64 else 4))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    out = torch.empty(rplan.n_out, dtype=work, device=device)
    fn = lib.ndmps_region_contract_f64 if f64 else lib.ndmps_region_contract_f32
    with _span("region"):
        _lib.check(fn(L, dims, bonds, ptrs, nodes, tiles, tables.data_ptr(), tables.numel(), rplan.n_out,
                      out.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
    del keep
    return out


def series_work_dtype(chains):
    """The type a series call contracts in and returns: fp64 if any frame has fp64 cores, fp32 otherwise."""
    torch = _torch()
    return torch.float64 if any(m.dtype == torch.float64 for m in chains) else torch.float32


def region_series_values(chains, rplan):
    """``rplan``'s output elements of every frame (ndmps_region_series_contract_*): a (T, n_out) device tensor, fp64
    if any frame has fp64 cores (the others are widened exactly), fp32 otherwise (bf16 cores upcast as in
    ``region_values``).  The tables are uploaded once; each chunk of frames (``region.plan_series``) uploads its
    records -- core pointers, then bonds -- in one copy and issues L launches."""
    torch = _torch()
    lib = _lib.load()
    work = series_work_dtype(chains)
    f64 = work == torch.float64
    first = chains[0]
    T, L, device = len(chains), first.L, first.device
    keep = [[c if c.dtype == work else c.to(work) for c in m.cores] for m in chains]
    ptrs = np.array([[c.data_ptr() for c in frame] for frame in keep], dtype=np.int64).reshape(T, L)
    bonds = np.array([[1] + [c.shape[2] for c in frame] for frame in keep], dtype=np.int64).reshape(T, L + 1)
    layout = _region.plan_series(bonds, rplan, 8 if f64 else 4)
    dims, nodes, tiles, tables = _region_tables(first.dims, rplan, device)  # once for the series
    ws = torch.empty(max(layout.ws_bytes, 1), dtype=torch.uint8, device=device)
    out = torch.empty((T, rplan.n_out), dtype=work, device=device)
    fn = lib.ndmps_region_series_contract_f64 if f64 else lib.ndmps_region_series_contract_f32
    with _span("region_series"):
        for a, b in layout.chunks:
            records = torch.from_numpy(np.concatenate([ptrs[a:b].ravel(), bonds[a:b].ravel()])).to(device)
            h_bonds = np.ascontiguousarray(bonds[a:b])
            _lib.check(fn(b - a, L, dims, h_bonds.ctypes.data_as(_lib.p_i64), nodes, tiles, tables.data_ptr(),
                          tables.numel(), records.data_ptr(), rplan.n_out, out[a].data_ptr(), ws.data_ptr(),
                          layout.ws_bytes, _lib.stream_ptr()))
    del keep
    return out


def region_outer(contract, lead, shape, idx, keep, dct, work, device):
    """``volume[np.ix_(*idx)]`` without the int axes (``keep`` False), behind the leading axes ``lead``: ``()`` for one
    object, ``(T,)`` for a series.  ``contract(rplan)`` is ``region_values`` or ``region_series_values`` bound to its
    chain(s) and returns ``work``.  An empty selection launches nothing.  ``dct``: the last axis is decoded in full for
    every selected row (the rows of all frames lie back to back: one launch), transformed back, then indexed."""
    torch = _torch()
    out_shape = list(lead) + [i.size for i, k in zip(idx, keep) if k]
    if any(i.size == 0 for i in idx):
        return torch.empty(out_shape, dtype=work, device=device)
    if not dct:
        return contract(_region.plan_outer(shape, idx)).view(out_shape)
    n = shape[-1]
    rows = contract(_region.plan_outer(shape, idx[:-1] + [np.arange(n, dtype=np.int64)]))
    rec = idct_last(rows, n).view(*lead, -1, n)
    return rec.index_select(len(lead) + 1, torch.from_numpy(idx[-1]).to(device)).reshape(out_shape)


def region_points(contract, lead, shape, pts, dct, work, device):
    """``volume[tuple(pts)]`` for the (ndim, N) points ``pts`` behind the leading axes ``lead``; arguments as
    ``region_outer``.  In DCT mode every distinct row of the last axis that the points touch is decoded in full."""
    torch = _torch()
    if pts.shape[1] == 0:
        return torch.empty(tuple(lead) + (0,), dtype=work, device=device)
    if not dct:
        return contract(_region.plan_points(shape, pts))
    full, sel = _region.full_rows_of_points(shape, pts)
    rec = idct_last(contract(_region.plan_points(shape, full)), shape[-1]).view(*lead, -1)
    return rec.index_select(len(lead), torch.from_numpy(sel).to(device))


# ------------------------------------------------------------------------------------------------ pooled decode
def rank_safe(cores):
    """The chain with every bond at most the product of the site dims on either side of it (what ndmps_chain_*
    require; a reduced chain can have wider bonds): the two sites around a wider bond are contracted into one.
    The site-order tensor is unchanged."""
    torch = _torch()
    lib = _lib.load()
    dims = [int(c.shape[1]) for c in cores]
    numel = int(np.prod(dims, dtype=np.int64))
    out, left = [cores[0]], dims[0]
    for c in cores[1:]:
        chi = int(c.shape[0])
        if chi > left or chi > numel // left:
            prev = out.pop()
            m, n = int(prev.shape[0]) * int(prev.shape[1]), int(c.shape[1]) * int(c.shape[2])
            merged = torch.empty((int(prev.shape[0]), int(prev.shape[1]) * int(c.shape[1]), int(c.shape[2])),
                                 dtype=c.dtype, device=c.device)
            gemm = lib.ndmps_dgemm if c.dtype == torch.float64 else lib.ndmps_sgemm
            _lib.check(gemm(0, 0, m, n, chi, prev.data_ptr(), chi, c.data_ptr(), n, merged.data_ptr(), n,
                            _lib.stream_ptr()))
            out.append(merged)
        else:
            out.append(c)
        left *= int(c.shape[1])
    return out


def pooled(chain, shape, fa, lev, op, dct):
    """The volume of ``shape`` (factor array ``fa``) reduced over the blocks of ``lev`` (core/pool.py) as a device
    tensor of the plan's out_shape, fp64 for fp64 cores, fp32 otherwise (bf16 cores are reduced and contracted in
    fp32)."""
    torch = _torch()
    lib = _lib.load()
    plan = _pool.PoolPlan(fa, lev, op, dct=dct)
    device = chain.device
    f64 = chain.dtype == torch.float64
    work = torch.float64 if f64 else torch.float32
    code = 2 if f64 else 1 if chain.dtype == torch.bfloat16 else 0
    L, Lk = plan.L, plan.L_keep
    bonds = chain.bonds
    outs = []
    for l in range(max(Lk, 1)):
        if Lk == 0:
            outs.append(torch.empty((1, 1, 1), dtype=work, device=device))
        elif l == Lk - 1 and Lk < L:
            outs.append(torch.empty((bonds[l], int(plan.dprime[l]), 1), dtype=work, device=device))
        elif plan.passthrough[l] and chain.cores[l].dtype == work:
            outs.append(None)  # nothing reduced: the core itself
        else:
            outs.append(torch.empty((bonds[l], int(plan.dprime[l]), bonds[l + 1]), dtype=work, device=device))
    ptrs = chain._core_ptrs()
    with torch.cuda.device(device):
        stream = _lib.stream_ptr()
        offs = torch.from_numpy(plan.offsets).to(device)  # every site's offsets in one upload
        ws_bytes = int(lib.ndmps_pool_workspace_bytes(L, _lib.i64_array(bonds))) if Lk < L else 0
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
        out_ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() if o is not None else None for o in outs])
        with _span("pool"):
            _lib.check(lib.ndmps_pool_cores(code, L, _lib.i64_array(chain.dims), _lib.i64_array(bonds), ptrs, Lk,
                                            _lib.i64_array(plan.sites.ravel()), _lib.f64_array(plan.weight),
                                            offs.data_ptr(), offs.numel(), out_ptrs, ws.data_ptr(), ws_bytes,
                                            stream))
        if Lk == 0:
            res = outs[0].view(plan.coarse_shape)
        else:
            cores = rank_safe([o if o is not None else chain.cores[l] for l, o in enumerate(outs)])
            cplan = _plan_for(plan.coarse_shape, device.index or 0, factor_arr=plan.out_factor)
            res = decode_chain(DeviceMPS(cores, _trusted=True), cplan, plan.coarse_shape)
        if dct and lev[-1] < L:
            n = int(shape[-1])
            rows = res.numel() // n
            if plan.dct_pool > 1:
                # coefficient rows times the pooled basis (n / B, n): about 1 / prod_{a < last} B_a of the
                # full decode's transform
                nb = n // plan.dct_pool
                basis = _pooled_dct_basis(n, plan.dct_pool, op, device, f64)
                rec = torch.empty(rows * nb, dtype=work, device=device)
                gemm = lib.ndmps_dgemm if f64 else lib.ndmps_sgemm
                _lib.check(gemm(0, 1, rows, nb, n, res.data_ptr(), n, basis.data_ptr(), n, rec.data_ptr(), nb,
                                stream))
                res = rec
            else:
                res = idct_last(res, n)
    return res.view(plan.out_shape)
