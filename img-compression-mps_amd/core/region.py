"""Host planner of the region decode (``NDMPS.decode_region`` / ``NDMPS.values_at``): integer NumPy only.

Site ``s`` of the chain carries digit ``s`` of every axis (``get_factorlist`` / ``hierarchical_block_indexing``):
the physical index there is ``ravel_multi_index(digits[s], factor_arr[s])`` over the axes in C order, and the
digits of axis ``a`` at sites ``0 .. s`` are ``index // prod[s + 1, a]`` (its "prefix").  A left-to-right contraction
restricted to a set of voxels therefore only needs, after each site, the rows of the distinct prefixes that set
reaches ("live prefixes", the nodes of level ``s``).  Node ``k`` of level ``s`` has a parent node of level ``s - 1``
(the root for ``s = 0``) and a physical index ``phys[k]`` at site ``s``:

    E_s[k, :] = E_{s-1}[parent[k], :] . A_s[:, phys[k], :]

Level ``s`` has at most ``min(#voxels, d_0 ... d_s)`` nodes, so work and workspace scale with the region.  The last
site is not a level: every output element is the dot product of its level ``L - 2`` row with a column of the last
core, written to its place in the C-order result (repeats of an index are separate output elements).

``RegionPlan.tables`` is what ``ndmps_region_contract_*`` (csrc/region.hip) reads: per level ``parent`` (nodes sorted
by ``phys``) and tiles ``(phys, row0, count <= TILE_ROWS)`` of rows that share ``phys``; then ``leaf_parent`` and
``leaf_phys``.  Everything is range-checked here before it is uploaded.

A series (``NDMPS.decode_regions`` / ``values_at_many``) uses one plan for all its frames; ``plan_series`` lays the
frames' slabs out in the workspace of ``ndmps_region_series_contract_*`` and cuts the series into chunks.
"""
from __future__ import annotations

import numbers
import operator

import numpy as np

from ..utils import core as _core

TILE_ROWS = 32  # rows of one gathered product tile (csrc/region.hip kTileRows)
MAX_SERIES_FRAMES = 65535  # frames of one ndmps_region_series_contract_* call (a grid dimension)
# Largest workspace one chunk of a series may take (``plan_series``).  A memory policy, not a measurement: 1 GiB is
# well under a percent of the card's HBM and holds both buffers of 64 frames of a 256 x 256 slice at chi = 64 (2 MiB
# a frame) five hundred times over, so real series run in one chunk, while a huge ROI on thousands of frames cannot
# take the memory the cores and the result need.  A single frame that needs more than this is a chunk of its own.
SERIES_WS_BYTES = 1 << 30
_I32_MAX = np.iinfo(np.int32).max


# ------------------------------------------------------------------------------------------------- keys
def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def _axis_indices(entry, n, axis):
    """One key entry -> (int64 indices in [0, n), keeps_axis)."""
    if _is_int(entry):
        i = operator.index(entry)
        if not -n <= i < n:
            raise IndexError(f"index {i} is out of bounds for axis {axis} with size {n}")
        return np.array([i % n], dtype=np.int64), False
    if isinstance(entry, slice):
        for v in (entry.start, entry.stop, entry.step):
            if v is not None and not _is_int(v):
                raise TypeError(f"slice indices must be integers or None, got {type(v).__name__}")
        return np.arange(*entry.indices(n), dtype=np.int64), True
    if entry is None or isinstance(entry, (bool, np.bool_, float, str, bytes)):
        raise TypeError(f"unsupported index {entry!r} for axis {axis}: int, slice or 1-D integer array expected")
    if hasattr(entry, "detach") and hasattr(entry, "cpu"):  # torch tensor
        entry = entry.detach().cpu().numpy()
    arr = np.asarray(entry)
    if arr.size == 0 and arr.dtype.kind not in "b":
        arr = arr.astype(np.int64)
    if arr.dtype.kind not in "iu":
        raise TypeError(f"index arrays must be integer, got dtype {arr.dtype} for axis {axis}")
    if arr.ndim != 1:
        raise TypeError(f"index arrays must be 1-D (outer indexing), got {arr.ndim}-D for axis {axis}")
    arr = arr.astype(np.int64)
    if arr.size and (arr.min() < -n or arr.max() >= n):
        bad = int(arr[(arr < -n) | (arr >= n)][0])
        raise IndexError(f"index {bad} is out of bounds for axis {axis} with size {n}")
    return arr % n, True


def normalize_key(key, shape):
    """NumPy outer-indexing key -> (list of per-axis int64 index arrays, list of the axes kept in the result).

    One entry per axis: an int (negative allowed; drops its axis), a slice, or a 1-D integer array / list (unsorted,
    repeats allowed).  One ``Ellipsis`` and missing trailing entries mean full slices.  Out-of-range indices and too
    many entries raise IndexError, non-integer entries TypeError."""
    shape = tuple(int(s) for s in shape)
    if not isinstance(key, tuple):
        key = (key,)
    n_ell = sum(1 for k in key if k is Ellipsis)
    if n_ell > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if len(key) - n_ell > len(shape):
        raise IndexError(f"too many indices: the volume is {len(shape)}-dimensional, {len(key) - n_ell} were indexed")
    if n_ell:
        i = next(j for j, k in enumerate(key) if k is Ellipsis)
        key = key[:i] + (slice(None),) * (len(shape) - len(key) + 1) + key[i + 1:]
    key = key + (slice(None),) * (len(shape) - len(key))
    idx, keep = [], []
    for a, (entry, n) in enumerate(zip(key, shape)):
        arr, k = _axis_indices(entry, n, a)
        idx.append(arr)
        keep.append(k)
    return idx, keep


def normalize_points(coords, shape):
    """(N, ndim) integer points (negative allowed) -> (ndim, N) int64 in range."""
    shape = tuple(int(s) for s in shape)
    if hasattr(coords, "detach") and hasattr(coords, "cpu"):
        coords = coords.detach().cpu().numpy()
    arr = np.asarray(coords)
    if arr.size == 0 and arr.dtype.kind != "b":
        arr = arr.astype(np.int64).reshape(0, len(shape))
    if arr.dtype.kind not in "iu":
        raise TypeError(f"coordinates must be integer, got dtype {arr.dtype}")
    if arr.ndim != 2 or arr.shape[1] != len(shape):
        raise IndexError(f"coordinates must have shape (N, {len(shape)}), got {arr.shape}")
    arr = arr.astype(np.int64).T
    n = np.asarray(shape, dtype=np.int64)[:, None]
    bad = (arr < -n) | (arr >= n)
    if bad.any():
        a, j = np.argwhere(bad)[0]
        raise IndexError(f"index {int(arr[a, j])} is out of bounds for axis {int(a)} with size {int(n[a, 0])}")
    return np.ascontiguousarray(arr % n)


def full_rows_of_points(shape, pts):
    """DCT mode decodes the last axis in full: the points (ndim, U * n) of every distinct last-axis row that ``pts``
    (``normalize_points``) touches, row after row, and for each point of ``pts`` its position among them."""
    n, N = shape[-1], pts.shape[1]
    if len(shape) > 1:
        row_key = np.ravel_multi_index(tuple(pts[:-1]), shape[:-1])
        uniq, inv = np.unique(row_key, return_inverse=True)
        lead = np.stack(np.unravel_index(uniq, shape[:-1])).astype(np.int64)
    else:
        uniq, inv, lead = np.zeros(1, np.int64), np.zeros(N, np.int64), np.zeros((0, 1), np.int64)
    full = np.concatenate([np.repeat(lead, n, axis=1), np.tile(np.arange(n, dtype=np.int64), uniq.size)[None]])
    return full, inv.ravel() * n + pts[-1]


# ------------------------------------------------------------------------------------------------- plan
class RegionPlan:
    """Level tables of one region.  ``levels[s] = (parent, phys)`` for ``s < L - 1`` (nodes sorted by phys);
    ``leaf_parent`` / ``leaf_phys`` per output element; ``tiles[s]`` = (T, 3) int32 (phys, row0, count)."""

    def __init__(self, site_dims, levels, leaf_parent, leaf_phys):
        self.site_dims = [int(d) for d in site_dims]
        L = len(self.site_dims)
        self.levels, self.tiles = [], []
        rank_prev = None
        for s, (parent, phys) in enumerate(levels):
            if rank_prev is not None:
                parent = rank_prev[parent]
            order = np.argsort(phys, kind="stable")
            parent, phys = parent[order], phys[order]
            rank_prev = np.empty_like(order)
            rank_prev[order] = np.arange(order.size, dtype=order.dtype)
            self.levels.append((parent.astype(np.int64), phys.astype(np.int64)))
            self.tiles.append(_tiles(phys))
        if rank_prev is not None:
            leaf_parent = rank_prev[leaf_parent]
        self.leaf_parent = np.asarray(leaf_parent, dtype=np.int64).ravel()
        self.leaf_phys = np.asarray(leaf_phys, dtype=np.int64).ravel()
        assert len(self.levels) == L - 1
        self.n_out = int(self.leaf_parent.size)
        self._check()

    @property
    def nodes(self):
        return [int(p.size) for p, _ in self.levels]

    @property
    def n_tiles(self):
        return [int(t.shape[0]) for t in self.tiles]

    def _check(self):
        """Every index in range (the kernels also guard, but a bad plan is a bug to report, not to mask)."""
        n_prev = 1
        for s, ((parent, phys), tiles) in enumerate(zip(self.levels, self.tiles)):
            n = parent.size
            if n == 0 or n >= _I32_MAX:
                raise ValueError(f"region level {s}: {n} nodes")
            if parent.min() < 0 or parent.max() >= n_prev or phys.min() < 0 or phys.max() >= self.site_dims[s]:
                raise ValueError(f"region level {s}: table index out of range")
            if (tiles[:, 2] < 1).any() or (tiles[:, 2] > TILE_ROWS).any() or tiles[:, 1].min() < 0 \
                    or (tiles[:, 1] + tiles[:, 2]).max() > n or int(tiles[:, 2].sum()) != n:
                raise ValueError(f"region level {s}: bad tiles")
            n_prev = n
        if self.n_out == 0 or self.n_out >= _I32_MAX:
            raise ValueError(f"region of {self.n_out} elements")
        if self.leaf_parent.min() < 0 or self.leaf_parent.max() >= n_prev or self.leaf_phys.min() < 0 \
                or self.leaf_phys.max() >= self.site_dims[-1]:
            raise ValueError("region leaves: table index out of range")

    def tables(self):
        """The int32 buffer of ndmps_region_contract_* (one upload)."""
        parts = []
        for (parent, _), tiles in zip(self.levels, self.tiles):
            parts += [parent, tiles.ravel()]
        parts += [self.leaf_parent, self.leaf_phys]
        return np.concatenate(parts).astype(np.int32)


class SeriesLayout:
    """Workspace layout of one region on T frames (``plan_series``): ``caps[s] = max_t bonds[t][s]``, the slab of a
    frame ``frame_stride`` in elements, ``chunks`` = [(start, stop), ...] frame ranges contracted in turn, and
    ``ws_bytes``, the workspace of the largest chunk (what ``ndmps_region_series_workspace_bytes`` returns for as many
    frames of these caps)."""

    def __init__(self, caps, frame_stride, ws_bytes, chunks):
        self.caps, self.frame_stride, self.ws_bytes, self.chunks = caps, frame_stride, ws_bytes, chunks


def plan_series(bonds, plan, elem_bytes, ws_limit=None):
    """Layout of ``plan`` on a series whose frames have the bond lists ``bonds`` (T, L + 1), elements of
    ``elem_bytes`` bytes.  Frame t of a chunk owns a slab of ``frame_stride = max_s nodes_s * cap_{s+1}`` elements in
    each of the two ping-pong buffers, whatever its own bonds; a chunk holds at most MAX_SERIES_FRAMES frames and as
    many as keep ``2 * round_up(frames * frame_stride * elem_bytes, 256)`` within ``ws_limit`` (SERIES_WS_BYTES), but
    at least one."""
    b = np.asarray(bonds, dtype=np.int64)
    L = len(plan.site_dims)
    if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] != L + 1:
        raise ValueError(f"bond lists of shape {b.shape}, expected (T >= 1, {L + 1})")
    if (b < 1).any() or (b[:, 0] != 1).any() or (b[:, L] != 1).any():
        raise ValueError("open chains with bonds >= 1 expected")
    T = b.shape[0]
    limit = SERIES_WS_BYTES if ws_limit is None else int(ws_limit)
    caps = [int(v) for v in b.max(axis=0)]
    stride = max([1] + [n * caps[s + 1] for s, n in enumerate(plan.nodes)])
    per = min(T, MAX_SERIES_FRAMES)
    if L > 1:
        per = max(1, min(per, (limit // 2) // 256 * 256 // (stride * elem_bytes)))
    ws = 0 if L == 1 else 2 * (-(-per * stride * elem_bytes // 256) * 256)
    return SeriesLayout(caps, stride, ws, [(a, min(a + per, T)) for a in range(0, T, per)])


def _tiles(phys):
    """Tiles of up to TILE_ROWS consecutive rows that share phys (phys sorted)."""
    n = phys.size
    starts = np.flatnonzero(np.r_[True, phys[1:] != phys[:-1]])
    lens = np.diff(np.r_[starts, n])
    per = (lens + TILE_ROWS - 1) // TILE_ROWS
    g = np.repeat(np.arange(starts.size), per)
    j = np.arange(g.size) - np.repeat(np.cumsum(per) - per, per)
    row0 = starts[g] + j * TILE_ROWS
    cnt = np.minimum(TILE_ROWS, lens[g] - j * TILE_ROWS)
    return np.stack([phys[row0], row0, cnt], axis=1).astype(np.int32)


def _site_strides(factor_arr):
    """C-order strides of the axes in the physical index of every site, (L, ndim)."""
    f = np.asarray(factor_arr, dtype=np.int64)
    st = np.ones_like(f)
    for a in range(f.shape[1] - 2, -1, -1):
        st[:, a] = st[:, a + 1] * f[:, a + 1]
    return st


def _grid_sum(parts):
    """sum_a parts[a] broadcast along axis a, flattened C order (outer sum)."""
    D = len(parts)
    out = np.zeros((1,) * D, dtype=np.int64)
    for a, p in enumerate(parts):
        out = out + p.reshape((1,) * a + (-1,) + (1,) * (D - a - 1))
    return out.ravel()


def plan_outer(shape, idx):
    """Plan of the outer product of per-axis index arrays (``normalize_key``, none of them empty), output in
    C order."""
    shape = tuple(int(s) for s in shape)
    factor_arr, prod = _core.get_factorlist(shape)
    L, D = factor_arr.shape
    strides = _site_strides(factor_arr)
    uniq = [np.unique(i) for i in idx]
    levels = []
    vals_prev = [np.zeros(1, dtype=np.int64)] * D  # prefixes before site 0: the root
    for s in range(L - 1):
        vals = [np.unique(u // prod[s + 1, a]) for a, u in enumerate(uniq)]
        sizes_prev = [v.size for v in vals_prev]
        pstride = np.cumprod([1] + sizes_prev[::-1])[:-1][::-1]
        par = _grid_sum([np.searchsorted(vals_prev[a], v // factor_arr[s, a]) * pstride[a] for a, v in enumerate(vals)])
        phys = _grid_sum([(v % factor_arr[s, a]) * strides[s, a] for a, v in enumerate(vals)])
        levels.append((par, phys))
        vals_prev = vals
    sizes_prev = [v.size for v in vals_prev]
    pstride = np.cumprod([1] + sizes_prev[::-1])[:-1][::-1]
    # prod[0] is the int64 maximum: with L == 1 every index's prefix is the root's 0
    leaf_par = _grid_sum([np.searchsorted(vals_prev[a], i // prod[L - 1, a]) * pstride[a] for a, i in enumerate(idx)])
    leaf_phys = _grid_sum([(i % factor_arr[L - 1, a]) * strides[L - 1, a] for a, i in enumerate(idx)])
    return RegionPlan(np.prod(factor_arr, axis=1), levels, leaf_par, leaf_phys)


def plan_points(shape, pts):
    """Plan of a list of N >= 1 points, (ndim, N) int64 in range (``normalize_points``); output in point order."""
    shape = tuple(int(s) for s in shape)
    factor_arr, prod = _core.get_factorlist(shape)
    L, D = factor_arr.shape
    strides = _site_strides(factor_arr)
    N = pts.shape[1]
    levels = []
    node_prev = np.zeros(N, dtype=np.int64)  # node of every point at the previous level (the root)
    for s in range(L - 1):
        pre = [pts[a] // prod[s + 1, a] for a in range(D)]
        key = np.ravel_multi_index(tuple(pre), tuple(int(shape[a] // prod[s + 1, a]) for a in range(D)))
        _, first, node = np.unique(key, return_index=True, return_inverse=True)
        phys = sum((pre[a][first] % factor_arr[s, a]) * strides[s, a] for a in range(D))
        levels.append((node_prev[first], np.asarray(phys, dtype=np.int64)))
        node_prev = node.ravel().astype(np.int64)
    leaf_phys = sum((pts[a] % factor_arr[L - 1, a]) * strides[L - 1, a] for a in range(D))
    return RegionPlan(np.prod(factor_arr, axis=1), levels, node_prev, np.asarray(leaf_phys, dtype=np.int64))
