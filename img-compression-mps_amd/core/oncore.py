"""The device layer of the operators on the cores: every ctypes call of ``ndmps_lincomb_*``, ``ndmps_axisop_*``,
``ndmps_hadamard_layout`` / ``_sketch``, ``ndmps_sumsketch_layout`` / ``_sketch`` and ``ndmps_series_*``.

The convention of core/valstat.py: functions take ``DeviceMPS`` chains and plain metadata (checked by the NumPy-only
modules lincomb, axisop, hadamard, sumsketch, series and wgram) and return ``DeviceMPS`` chains, device tensors or host
values.  Nothing here knows ``NDMPS``: its methods check types, modes and compatibility and build the result objects.
Every operator with an output arena runs the one launch sequence ``_launch``.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import axisop as _ax
from . import hadamard as _hd
from . import lincomb as _lc
from . import series as _se
from . import wgram as _wg
from .mps import DeviceMPS, _torch
from .plan import _span


def chain_list_args(chains):
    """The C arguments of a list of chains: (bonds, storage codes, core pointers), chain by chain."""
    return (_lib.i64_array([b for m in chains for b in m.bonds]),
            (C.c_int * len(chains))(*[_lc.dtype_code(m.dtype) for m in chains]),
            (C.c_void_p * (len(chains) * chains[0].L))(*[c.data_ptr() for m in chains for c in m.cores]))


def sketch_table(R):
    """The random cores of a sketch as one flat fp64 table, site by site."""
    return np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.float64).ravel() for r in R]))


def zero_chain(dims, device):
    """The zero MPS: bond-1 zero cores in fp64."""
    return DeviceMPS([_torch().zeros((1, d, 1), dtype=_torch().float64, device=device) for d in dims], _trusted=True)


def carve_cores(arena, out_off, bonds, dims):
    """The cores ``(bonds[k], dims[k], bonds[k + 1])`` of an output arena as views: core k starts at ``out_off[k]``."""
    return [arena[out_off[k]: out_off[k] + bonds[k] * d * bonds[k + 1]].view(bonds[k], d, bonds[k + 1])
            for k, d in enumerate(dims)]


def _layout(entry, L, *args, tail=()):
    """A layout entry's answer ``(total elements, out_off, workspace bytes)``; ``tail``: further out-parameters."""
    out_off = (C.c_int64 * (L + 1))()
    ws_bytes = C.c_int64(0)
    total = _lib.check(entry(*args, out_off, C.byref(ws_bytes), *tail))
    return int(total), out_off, int(ws_bytes.value)


def _launch(total, ws_bytes, dtype, device, span, launch):
    """The launch sequence: the arena (``total`` elements of ``dtype``) is allocated first, the workspace second,
    ``launch(arena, ws)`` runs under the stage span, and the workspace is released before anything else is allocated
    (what is carved out of the arena keeps it alive).  Returns (arena, the launch's return code)."""
    torch = _torch()
    with torch.cuda.device(device):
        arena = torch.empty(max(total, 1), dtype=dtype, device=device)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
        with _span(span):
            rc = _lib.check(launch(arena, ws))
        del ws
    return arena, rc


def round_chains(chains, w, cutoff, max_bond, dtype, scale):
    """The TT-SVD rounding of ``sum_a w[a] * chains[a]`` (chains over the same site dims, arguments already checked)
    through ndmps_lincomb_round: ``(cores, bonds, spectra per bond, is_zero)``.  The cores are of the work type
    (``lincomb.work_is_f64``), rounded once to bf16 when ``dtype`` asks for it; ``spectra``: None for site 0, then the kept
    singular values per bond, ``[0.0]`` for the zero MPS.  ``scale`` is the absolute scale of the storage floor."""
    torch = _torch()
    lib = _lib.load()
    c_bonds, codes, ptrs = chain_list_args(chains)
    f64 = _lc.work_is_f64(codes, dtype)
    first = chains[0]
    K, L, dims = len(chains), first.L, first.dims
    mb = int(max_bond) if max_bond is not None else 0
    c_dims = _lib.i64_array(dims)
    stride = C.c_int64(0)
    total, out_off, ws_bytes = _layout(lib.ndmps_lincomb_layout, L, K, L, c_dims, c_bonds, mb, tail=(C.byref(stride),))
    st = int(stride.value)
    out_bonds = (C.c_int64 * (L + 1))()
    spectra = np.zeros(L * max(st, 1), dtype=np.float64)
    arena, rc = _launch(total, ws_bytes, torch.float64 if f64 else torch.float32, first.device, "lincomb",
                        lambda arena, ws: lib.ndmps_lincomb_round(
                            K, L, c_dims, c_bonds, codes, ptrs, _lib.f64_array(w), float(cutoff), mb, 2 if f64 else 0, scale,
                            arena.data_ptr(), arena.numel(), out_bonds, spectra.ctypes.data_as(_lib.p_f64), st,
                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    r = [int(v) for v in out_bonds]
    cores = carve_cores(arena, out_off, r, dims)
    if dtype == torch.bfloat16:
        cores = [c.to(torch.bfloat16) for c in cores]
    if rc > 0:  # the zero MPS: every bond 1 with the singular value 0
        return cores, r, [None] + [np.zeros(1) for _ in range(1, L)], True
    return cores, r, [None] + [spectra[k * st: k * st + r[k]].copy() for k in range(1, L)], False


def axis_apply(chain, mpo, fa, axis) -> DeviceMPS:
    """The unrounded wide chain of the operator ``mpo`` (core/axisop.py AxisMPO) applied to ``chain`` along ``axis`` of the
    factor array ``fa``: bonds ``D_k chi_k``, fp64 cores for fp64 storage and fp32 otherwise, one launch (csrc/axisop.hip)."""
    torch = _torch()
    lib = _lib.load()
    _ax.check_plan(mpo, fa, axis, chain.dims)
    _ax.check_wide_bonds(mpo.bonds, chain.bonds)
    code = _lc.dtype_code(chain.dtype)
    L, dims = chain.L, chain.dims
    c_dims, c_bonds = _lib.i64_array(dims), _lib.i64_array(chain.bonds)
    c_f = _lib.i64_array(mpo.factors)
    c_post = _lib.i64_array([post for _, _, post in _ax.site_split(fa, axis)])
    c_D = _lib.i64_array(mpo.bonds)
    table = np.concatenate([m.ravel() for m in mpo.cores])
    total, out_off, ws_bytes = _layout(lib.ndmps_axisop_layout, L, L, c_dims, c_bonds, c_f, c_D)
    arena, _ = _launch(total, ws_bytes, torch.float64 if code == 2 else torch.float32, chain.device, "axisop",
                       lambda arena, ws: lib.ndmps_axisop_apply(
                           L, c_dims, c_bonds, code, chain._core_ptrs(), c_f, c_post, c_D, table.ctypes.data_as(_lib.p_f64),
                           table.size, arena.data_ptr(), arena.numel(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    wide = [d * b for d, b in zip(mpo.bonds, chain.bonds)]
    return DeviceMPS(carve_cores(arena, out_off, wide, dims), _trusted=True)


def hadamard_sketch(a, b, ell, R) -> DeviceMPS:
    """The unrounded sketched chain of the elementwise product of the chains ``a`` and ``b`` (csrc/hadamard.hip): fp64,
    left-orthonormal up to its last site, bonds ``r_k <= ell[k]``; ``ell`` the sketch bonds, ``R`` the random cores of
    core/hadamard.py (host fp64).  A zero product: bond-1 zero cores.  ValueError above ``hadamard.WS_LIMIT_BYTES``."""
    lib = _lib.load()
    L, dims, device = a.L, a.dims, a.device
    c_dims, c_ba, c_bb = _lib.i64_array(dims), _lib.i64_array(a.bonds), _lib.i64_array(b.bonds)
    c_ell = _lib.i64_array(ell)
    total, out_off, ws_bytes = _layout(lib.ndmps_hadamard_layout, L, L, c_dims, c_ba, c_bb, c_ell)
    _hd.check_workspace(ws_bytes)
    table = sketch_table(R)
    ranks = (C.c_int64 * (L + 1))()
    arena, rc = _launch(total, ws_bytes, _torch().float64, device, "hadamard",
                        lambda arena, ws: lib.ndmps_hadamard_sketch(
                            L, c_dims, c_ba, _lc.dtype_code(a.dtype), a._core_ptrs(), c_bb, _lc.dtype_code(b.dtype),
                            b._core_ptrs(), c_ell, table.ctypes.data_as(_lib.p_f64), table.size, arena.data_ptr(),
                            arena.numel(), ranks, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    if rc > 0:  # the zero product
        return zero_chain(dims, device)
    return DeviceMPS(carve_cores(arena, out_off, [int(v) for v in ranks], dims), _trusted=True)


def sum_sketch(chains, w, ell, R) -> list:
    """The unrounded sketched chains of ``sum_a w[j, a] * chains[a]`` for every row j (csrc/sumsketch.hip): fp64,
    left-orthonormal up to their last sites, bonds ``r_k <= ell[k]``.  ``chains``: the frames some row uses; a zero
    output comes back as bond-1 zero cores.  ValueError when the workspace would exceed ``hadamard.WS_LIMIT_BYTES``."""
    lib = _lib.load()
    first = chains[0]
    T, K, L, dims, device = len(chains), int(w.shape[0]), first.L, first.dims, first.device
    c_dims = _lib.i64_array(dims)
    c_bonds, codes, ptrs = chain_list_args(chains)
    c_ell = _lib.i64_array(ell)
    total, out_off, ws_bytes = _layout(lib.ndmps_sumsketch_layout, L, T, K, L, c_dims, c_bonds, c_ell)
    _hd.check_workspace(ws_bytes)
    table = sketch_table(R)
    weights = np.ascontiguousarray(w, dtype=np.float64)
    ranks = (C.c_int64 * (K * (L + 1)))()
    zero = (C.c_int * K)()
    arena, _ = _launch(total, ws_bytes, _torch().float64, device, "sumsketch",
                       lambda arena, ws: lib.ndmps_sumsketch_sketch(
                           T, K, L, c_dims, c_bonds, codes, ptrs, weights.ctypes.data_as(_lib.p_f64), c_ell,
                           table.ctypes.data_as(_lib.p_f64), table.size, arena.data_ptr(), arena.numel(), ranks, zero,
                           ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    chain = int(out_off[L])
    out = []
    for j in range(K):
        if zero[j]:
            out.append(zero_chain(dims, device))
            continue
        r = [int(v) for v in ranks[j * (L + 1):(j + 1) * (L + 1)]]
        out.append(DeviceMPS(carve_cores(arena[j * chain:(j + 1) * chain], out_off, r, dims), _trusted=True))
    return out


def _gram_call(chains_a, chains_b, weight):
    """The arguments of the ndmps_series_* calls for the rows ``chains_a``, the columns ``chains_b`` (None: the symmetric
    matrix of the rows) and an optional weight chain: ``(Ka, Kb, sym, L, dims)``, the bond arrays, the full lists and
    ``(span, entry, route entry)``.  The plain and the weighted entry points are told apart here only."""
    lib = _lib.load()
    first = chains_a[0]
    sa = chain_list_args(chains_a)
    sb = sa if chains_b is None else chain_list_args(chains_b)
    head = (len(chains_a), len(chains_a if chains_b is None else chains_b), 1 if chains_b is None else 0, first.L,
            _lib.i64_array(first.dims))
    if weight is None:
        return head, (sa[0], sb[0]), sa + sb, ("gram", lib.ndmps_series_gram, lib.ndmps_series_gram_route)
    sw = (_lib.i64_array(weight.bonds), _lc.dtype_code(weight.dtype), weight._core_ptrs())
    return head, (sa[0], sb[0], sw[0]), sa + sb + sw, ("wgram", lib.ndmps_series_wgram, lib.ndmps_series_wgram_route)


def gram_route(chains_a, chains_b=None, weight=None) -> str:
    """The route of ``gram`` for these chains: "resident", "batched" or "per-pair" (core/series.py ROUTES)."""
    (Ka, Kb, _, L, dims), bonds, _, (_, _, route_entry) = _gram_call(chains_a, chains_b, weight)
    return _se.ROUTES[_lib.check(route_entry(Ka, Kb, L, dims, *bonds))]


def gram(chains_a, chains_b=None, weight=None, as_torch: bool = False):
    """The fp64 Gram matrix ``G[a, b] = <chains_a[a], chains_b[b]>`` (csrc/series.hip; ``chains_b=None``: the symmetric
    matrix of ``chains_a``), under the weight chain when one is given (csrc/wgram.hip; its workspace stays under
    ``wgram.WS_LIMIT_BYTES``, ValueError when not one pair fits).  NumPy array, or the device tensor with ``as_torch``."""
    lib = _lib.load()
    (Ka, Kb, sym, L, dims), bonds, lists, (span, entry, _) = _gram_call(chains_a, chains_b, weight)
    if weight is None:
        nbytes = int(_lib.check(lib.ndmps_series_gram_workspace_bytes(Ka, Kb, L, dims, *bonds)))
    else:
        nbytes = lib.ndmps_series_wgram_workspace_bytes(Ka, Kb, sym, L, dims, *bonds, _wg.WS_LIMIT_BYTES)
        if nbytes != _lib.EWORKSPACE:
            _lib.check(nbytes)
        nbytes = _wg.check_workspace(nbytes)
    G, _ = _launch(Ka * Kb, nbytes, _torch().float64, chains_a[0].device, span,
                   lambda G, ws: entry(Ka, Kb, sym, L, dims, *lists, G.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr()))
    G = G.view(Ka, Kb)
    return G if as_torch else G.cpu().numpy()
