"""Host planner of the block-averaged decode (``NDMPS.downsample`` / ``NDMPS.sum`` / ``NDMPS.mean``): integer NumPy.

Site ``l`` of the chain carries digit ``l`` of every axis, coarsest first (``get_factorlist``,
``hierarchical_block_indexing``), and its physical index ravels those digits in C order over the axes with the
factors ``factor_arr[l]``.  The digits of axis ``a`` at its last ``k`` sites therefore enumerate the offsets inside
the blocks ``i_a // B_a`` with ``B_a = prod(factor_arr[L - k:, a])``: summing the cores over those digits sums the
volume over the blocks.  That is a site-local linear map on the cores:

    out_l[x, q, y] = w_l * sum_r A_l[x, qoff_l[q] + roff_l[r], y]

``qoff_l`` ravels the digits of the axes kept at site ``l``, ``roff_l`` those of the reduced axes (C order over the
axes, as the physical index does), ``w_l`` is ``1 / prod(reduced factors)`` for a mean and 1 for a sum.  Sites where
every axis is reduced (the suffix ``l >= L - min(levels)``; balanced factor lists have no factor 1 unless L == 1) get
``d'_l = 1`` and collapse to matrices, applied right to left to a vector that the last kept site absorbs.  The kept
sites form an MPS of the coarse volume over the factor array ``factor_arr[:L']`` with 1 in each reduced entry.

DCT mode stores the last axis as orthonormal DCT-II coefficients ``y`` (``x = y B^T``, ``sum_j B[j][k] = sqrt(n)
delta_k0``).  A full reduction of the last axis is then a selection of its digit 0 at every site ("pick"), weighted
``sqrt(f)`` per site for a sum and ``1 / sqrt(f)`` for a mean (``sqrt(n)`` / ``1 / sqrt(n)`` over the chain).  A
partial reduction of the last axis keeps its digits on the sites (``chain_levels`` 0 there); the caller pools the
decoded coefficient rows with one GEMM against the block-summed basis (``ndmps_pool_dct_basis_*``).
"""
from __future__ import annotations

import numbers
import operator

import numpy as np

KEEP, SUM, PICK = 0, 1, 2  # what happens to an axis at a site
_I32_MAX = np.iinfo(np.int32).max


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def normalize_levels(levels, ndim, L):
    """``levels`` (an int in [0, L] or one int per axis) -> int64 array of ndim entries.  TypeError for a non-integer
    (bools included), ValueError for a value outside [0, L] or a sequence of the wrong length."""
    if _is_int(levels):
        lv = [operator.index(levels)] * ndim
    else:
        if isinstance(levels, (str, bytes)) or not hasattr(levels, "__len__"):
            raise TypeError(f"levels must be an int or a sequence of ints, got {type(levels).__name__}")
        lv = list(levels)
        for v in lv:
            if not _is_int(v):
                raise TypeError(f"levels must be integers, got {type(v).__name__}")
        if len(lv) != ndim:
            raise ValueError(f"levels has {len(lv)} entries, the tensor has {ndim} axes")
        lv = [operator.index(v) for v in lv]
    for v in lv:
        if not 0 <= v <= L:
            raise ValueError(f"level {v} outside [0, {L}] (the chain has {L} sites)")
    return np.asarray(lv, dtype=np.int64)


def normalize_axes(axis, ndim):
    """NumPy's ``axis`` argument -> sorted tuple of axes (None: all).  TypeError for non-integers, numpy's AxisError
    out of range, ValueError for a repeated axis."""
    if axis is None:
        return tuple(range(ndim))
    items = axis if isinstance(axis, tuple) else (axis,)
    out = []
    for a in items:
        if not _is_int(a):
            raise TypeError(f"axis must be an integer or a tuple of integers, got {type(a).__name__}")
        a = operator.index(a)
        if not -ndim <= a < ndim:
            raise np.exceptions.AxisError(a, ndim)
        out.append(a % ndim)
    if len(set(out)) != len(out):
        raise ValueError("duplicate value in 'axis'")
    return tuple(sorted(out))


def block_shape(factor_arr, levels):
    """B_a = prod(factor_arr[L - levels[a]:, a]) for every axis."""
    fa = np.asarray(factor_arr, dtype=np.int64)
    L = fa.shape[0]
    return tuple(int(np.prod(fa[L - int(k):, a], dtype=np.int64)) for a, k in enumerate(levels))


def _ravel_offsets(factors, strides):
    """Offsets sum_a digit_a * stride_a over every digit combination, C order over the given axes."""
    off = np.zeros(1, dtype=np.int64)
    for f, s in zip(factors, strides):
        off = (off[:, None] + np.arange(f, dtype=np.int64)[None, :] * s).ravel()
    return off


class PoolPlan:
    """What the device needs to reduce every site (see the module docstring).

    ``modes`` (L, ndim): KEEP / SUM / PICK per site and axis.  ``L_keep``: number of kept sites (the chain of the
    coarse volume); sites from there on collapse.  ``out_factor`` (L_keep, ndim): factor array of the coarse chain.
    ``coarse_shape``: shape the coarse chain decodes to.  Per site: ``dprime`` (kept physical dimension), ``n_red``
    (reduced combinations), ``weight`` and ``passthrough`` (nothing reduced, weight 1).  ``offsets``: int32 table of
    every site's qoff then roff; ``sites`` (L, 4) int64: d', n_red, qoff start, roff start."""

    def __init__(self, factor_arr, levels, op="mean", dct=False):
        fa = np.asarray(factor_arr, dtype=np.int64)
        L, nd = fa.shape
        lev = np.broadcast_to(np.asarray(levels, dtype=np.int64), (nd,)).copy()
        if op not in ("mean", "sum"):
            raise ValueError(f"op must be 'mean' or 'sum', got {op!r}")
        self.factor_arr, self.levels, self.op, self.dct = fa, lev, op, bool(dct)
        self.L, self.ndim = L, nd
        chain_lev = lev.copy()
        # DCT: the last axis is reduced on the sites only in full (digit 0 picked); a partial block stays on them
        self.dct_pool = 1  # block of the last axis that the caller pools after the decode (1: none)
        if self.dct and 0 < lev[-1] < L:
            chain_lev[-1] = 0
            self.dct_pool = int(np.prod(fa[L - lev[-1]:, -1], dtype=np.int64))
        self.chain_levels = chain_lev
        modes = np.zeros((L, nd), dtype=np.int64)
        for a in range(nd):
            modes[L - chain_lev[a]:, a] = SUM
        if self.dct and lev[-1] == L:
            modes[:, -1] = PICK
        self.modes = modes
        self.L_keep = int(L - chain_lev.min())
        mean = op == "mean"
        dprime, n_red, weight, qoffs, roffs = [], [], [], [], []
        for l in range(L):
            f = fa[l]
            strides = np.ones(nd, dtype=np.int64)
            for a in range(nd - 2, -1, -1):
                strides[a] = strides[a + 1] * f[a + 1]
            keep = [a for a in range(nd) if modes[l, a] == KEEP]
            red = [a for a in range(nd) if modes[l, a] == SUM]
            qoffs.append(_ravel_offsets(f[keep], strides[keep]))
            roffs.append(_ravel_offsets(f[red], strides[red]))
            dprime.append(qoffs[-1].size)
            n_red.append(roffs[-1].size)
            w = 1.0
            for a in range(nd):
                if modes[l, a] == SUM and mean:
                    w /= float(f[a])
                elif modes[l, a] == PICK:
                    w *= (1.0 / np.sqrt(float(f[a]))) if mean else np.sqrt(float(f[a]))
            weight.append(w)
        self.dprime = np.asarray(dprime, dtype=np.int64)
        self.n_red = np.asarray(n_red, dtype=np.int64)
        self.weight = np.asarray(weight, dtype=np.float64)
        self.passthrough = (self.n_red == 1) & (self.dprime == np.prod(fa, axis=1)) & (self.weight == 1.0)
        if np.any(self.dprime[self.L_keep:] != 1):
            raise AssertionError("internal: a collapsed site keeps an axis")
        out_factor = np.where(modes[: self.L_keep] == KEEP, fa[: self.L_keep], 1)
        self.out_factor = np.ascontiguousarray(out_factor, dtype=np.int64)
        self.coarse_shape = tuple(int(v) for v in np.prod(self.out_factor, axis=0)) if self.L_keep else (1,) * nd
        table = np.concatenate([np.concatenate([q, r]) for q, r in zip(qoffs, roffs)])
        if table.size and (table.min() < 0 or table.max() > _I32_MAX):
            raise ValueError("pool: offset table out of the int32 range")
        starts = np.cumsum([0] + [q.size + r.size for q, r in zip(qoffs, roffs)])
        self.sites = np.stack([self.dprime, self.n_red, starts[:-1], starts[:-1] + self.dprime], axis=1).astype(np.int64)
        self.offsets = table.astype(np.int32)
        self._qoffs, self._roffs = qoffs, roffs

    @property
    def out_shape(self):
        """Shape of the result: ``n_a // B_a`` per axis (DCT: the last axis is pooled after the decode)."""
        shape = list(self.coarse_shape)
        if self.dct_pool > 1:
            shape[-1] //= self.dct_pool
        return tuple(shape)

    def reduce_core(self, core, l):
        """NumPy emulation of the device's site reduction: (chi_l, d'_l, chi_r) from a (chi_l, d_l, chi_r) core."""
        q, r = self._qoffs[l], self._roffs[l]
        return self.weight[l] * core[:, q[:, None] + r[None, :], :].sum(axis=2)


def emulate(cores, plan):
    """fp64 NumPy emulation of the device path: the reduced kept cores, the suffix collapsed right to left into a
    vector and absorbed by the last kept site.  Returns the kept cores (the last one with right bond 1), or
    ``[scalar]`` as a (1, 1, 1) core when every site collapses."""
    L, Lk = plan.L, plan.L_keep
    red = [plan.reduce_core(np.asarray(c, dtype=np.float64), l) for l, c in enumerate(cores)]
    if Lk == L:
        return red
    vec = np.ones(1)
    for l in range(L - 1, Lk - 1, -1):
        vec = red[l][:, 0, :] @ vec
    if Lk == 0:
        return [vec.reshape(1, 1, 1)]
    last = red[Lk - 1] @ vec  # the absorbing site is reduced like any kept site, then contracted with the vector
    return red[: Lk - 1] + [last[:, :, None]]


def site_order_positions(shape, factor_arr):
    """For every voxel of ``shape`` in C order, its position in the site-order tensor of the chain over the explicit
    ``factor_arr`` (gen_encoding_map's digits, raveled over the sites).  Host reference for the coarse plans."""
    fa = np.asarray(factor_arr, dtype=np.int64)
    L = fa.shape[0]
    idx = np.indices(tuple(shape)).reshape(len(shape), -1)
    below = np.ones((L + 1, fa.shape[1]), dtype=np.int64)
    for l in range(L - 1, -1, -1):
        below[l] = below[l + 1] * fa[l]
    pos = np.zeros(idx.shape[1], dtype=np.int64)
    for l in range(L):
        digits = (idx // below[l + 1][:, None]) % fa[l][:, None]
        phys = np.ravel_multi_index(tuple(digits), tuple(int(v) for v in fa[l]))
        pos = pos * int(np.prod(fa[l])) + phys
    return pos
