"""Cases, fp64 reference and error bars of the DCT-mode decoders (NumPy / SciPy only).

Used by tests/test_dct_decode_cases_host.py (CPU: the bars are sound and have teeth) and tests/test_gpu_dct_decode.py
(the device against the same reference and bars).  Nothing here is measured from, or tuned to, a kernel.

Cases.  ``SHAPES`` puts the last axis ``n`` on every route of the inverse transform (``TABLE``): the basis product
(n = 20, 32 below the FFT range, 680 long, 2048 above the range) and the in-LDS FFT (n = 64 and 1024, its two ends;
fp32 only -- fp64 always takes the basis product).  Cores are drawn by ``oracle.chain_cases.draw_cores`` over the site
dims of the shape and bonds capped at 12, in two families: "uniform" (dense, non-smooth: every DCT coefficient
carries the same weight) and "integer" ({-1, 0, 1}, exact in every storage type).

Reference.  ``y`` is the fp64 contraction of the cores carried to volume order (the coefficient tensor), ``x`` its
orthonormal inverse DCT along the last axis by ``scipy.fft.idct`` in float64, ``M = |A_0| ... |A_{L-1}|`` in volume
order.  With ``C = idct(eye(n))`` the transform is ``x = y @ C``, ``C[k, m] = s_k cos(pi (2 m + 1) k / (2 n))``,
``s_0 = sqrt(1 / n)``, ``s_k = sqrt(2 / n)``.

Bar of a decoded element: two terms.

* propagation: the chain's forward bound ``b_y = chain_factor(u_acc, u_store) * M`` (oracle/chain_bound.py) carried
  through the exact transform, ``b_y @ |C|``.  Roundoffs as in tests/test_gpu_decode_reference.py: ``to_tensor``
  contracts in the storage type (bf16: 2**-24 / 2**-8), region and pool calls widen bf16 cores to fp32 (2**-24 /
  2**-24).  An integer chain whose partial products cannot leave the exactly representable integers (product of the
  bonds below 2**24, 2**53, or at most 256 for a bf16 chain) has no error in this stage: the term is 0.
* transform, basis product: ``1.01 (n + 2) u (|y| @ |C|)``: Higham's gamma_n |y| |C| for an inner product of length
  n in any order (``chain_bound.gemm_bound``, the bar ndmps_sgemm / ndmps_dgemm are held to) plus one ``u`` for the
  rounding of each basis entry and one for the rounding of the result.
* transform, FFT: ``8 (log2(n) / 2 + 3) 2**-24 ||y row||_2`` for every entry of the row: ``stream_cases.idct_bar(n)``
  (the bar ndmps_idct_last_f32 is held to on rows of entry magnitude <= 1) applied to the row norm; an FFT's error is
  normwise, relative to ``||y||_2``, not entry by entry.

Bar of a pooled element (``downsample`` / ``sum`` / ``mean``).  Reductions over the other axes are site-local sums on
the cores, so ``y`` and ``M`` are reduced the same way (``y_r``, ``M_r``) and the factor of the chain stays.

* last axis kept (level 0): the decoded-element bar on ``y_r``, ``M_r``.
* last axis reduced in part by blocks of ``Bk``: the device multiplies the coefficient rows by
  ``W[j, k] = w sum_{m in block j} C[k, m]`` (``w = 1 / Bk`` for a mean).  With
  ``Wabs[j, k] = w sum_{m in block j} |C[k, m]|`` -- not ``|W|``: the block sum cancels and the device forms it term
  by term -- propagation is ``(factor M_r) @ Wabs^T`` and the transform term ``1.01 (n + Bk + 2) u (|y_r| @ Wabs^T)``.
* last axis reduced in full ("pick"): no transform; ``sum_m x_m = sqrt(n) y_0``.  Reference: the reduction of ``x``
  (for integer cores the same number formed from the coefficients, the fp64 reduction of ``y[..., 0]`` times the
  weight, so that an exact zero is a zero); bar: the chain factor times the reduced ``M[..., 0]`` times ``sqrt(n)``
  (sum) or ``1 / sqrt(n)`` (mean).
* integer cores: a sum that stays on integers below 2**24 / 2**53 (product of the bonds times the voxels summed
  per block on the cores) has propagation 0.  A mean weights the cores by ``1 / f`` and a pick by ``sqrt(f)`` or
  ``1 / sqrt(f)`` per site; those are rounded where ``f`` is no power of two (resp. of four), so the weighted cores
  are no integers and the general factor stands.  When every site collapses (all levels L) the device carries an
  fp64 vector from site to site and rounds once into the result: the bar is then ``u_result |ref|`` plus the fp64
  chain factor (with 3 roundings per site for the weights) times the reduced ``M``.

Bar of ``ndmps_pool_dct_basis_*`` against ``W`` (``pooled_basis``, formed in extended precision and rounded once).
The first count, ``4 (Bk + 1) 2**-53 w sqrt(2 / n)`` per entry, did not leave the factor of 4: the kernel's formula
evaluated in float64 on the CPU reached 0.26 of it at (n, Bk) = (20, 5).  It allowed 4 units of ``u = 2**-53`` per
term for the cosine alone and forgot the rounding of its argument.  Derived again, the kernel computes
``W = fl(w s_k acc)``, ``acc = sum_{i < Bk} cospi(fl(num_i / 2n))`` added term by term:

* argument: ``x = num / 2n < 2`` is rounded with relative error ``u``, so the angle ``pi x`` moves by at most
  ``2 pi u`` and the cosine (slope at most 1) by at most ``2 pi u``;
* cospi itself: at most 4 ulp (the OpenCL full-profile bound for double, the weakest documented one), and an ulp of a
  value below 1 is at most ``u``: ``4 u``;
* the Bk - 1 additions: ``u |s_i|`` each, ``s_i`` the partial sums, which are known exactly from the reference;
* the scaling: ``sqrt``, two products and the rounding of ``w``: ``3 u |W|`` (times 1.01 for higher orders).

Per entry: ``u w sqrt(2 / n) ((2 pi + 4) Bk + sum_i |s_i|) + 1.01 * 3 u |W|``, plus ``2**-24 |W|`` for the fp32
kernel's one rounding.  test_dct_decode_cases_host.py evaluates the kernel's formula in float64 on the CPU and holds it
to a quarter of this bar; a block that starts one row late misses it by ten orders of magnitude.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.fft import idct

import stream_cases as sc
from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle import index_map as im
from oracle.mps import mps_to_dense

MAX_BOND = 12
# shape -> (sites L, factors of the last axis coarsest first, n, transform at fp32)
TABLE = {
    (30, 45, 20): (3, (2, 2, 5), 20, "gemm"),
    (16, 16, 8, 32): (3, (4, 4, 2), 32, "gemm"),
    (64, 64, 64): (6, (2,) * 6, 64, "fft"),
    (512, 680): (5, (17, 5, 2, 2, 2), 680, "gemm"),
    (8, 1024): (3, (16, 16, 4), 1024, "fft"),
    (16, 2048): (4, (16, 8, 4, 4), 2048, "gemm"),
}
SHAPES = list(TABLE)
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
FAMILIES = ("uniform", "integer")
STORAGES = cc.STORAGES
U = {"f32": cb.U_F32, "f64": cb.U_F64, "bf16": cb.U_BF16}
EXACT_LIMIT = {"f32": 2 ** 24, "f64": 2 ** 53, "bf16": 256}
BASIS_TERM_UNITS = 2 * np.pi + 4  # units of 2**-53 per cosine term of the pooled basis (module docstring)
BASIS_CASES = [(20, 5), (20, 20), (32, 2), (64, 2), (64, 64), (680, 8), (680, 40), (1024, 4), (2048, 16)]


# ------------------------------------------------------------------------------------------------ the chains
def factor_array(shape):
    return im.get_factorlist(tuple(int(v) for v in shape))[0]


def site_dims(shape):
    return [int(v) for v in np.prod(factor_array(shape), axis=1)]


def capped_bonds(shape, cap=MAX_BOND):
    """min(cap, left, right) at every inner bond: what a sweep capped at ``cap`` leaves on a volume of full rank."""
    dims = site_dims(shape)
    numel = int(np.prod(dims, dtype=np.int64))
    bonds, left = [1], 1
    for d in dims[:-1]:
        left *= d
        bonds.append(int(min(cap, left, numel // left)))
    return bonds + [1]


def work_of(storage):
    """Type the region and pool calls contract in, and every call transforms in."""
    return "f64" if storage == "f64" else "f32"


def fft_route(n, work):
    """Whether the inverse transform of rows of length ``n`` takes the FFT (csrc/reduce.hip: dct_fft_ok)."""
    return work == "f32" and 64 <= n <= 1024 and n & (n - 1) == 0


def roundoff(storage, call):
    """(u_acc, u_store) of the chain: ``call`` is "to_tensor" (the storage type's chain) or "wide"."""
    return cb.CHAIN_ROUNDOFF[storage if call == "to_tensor" else work_of(storage)]


@functools.lru_cache(maxsize=None)
def basis(n):
    """``C`` (n, n) float64 with ``x = y @ C``: row k is the inverse transform of the k-th unit coefficient."""
    c = idct(np.eye(n), type=2, norm="ortho", axis=-1)
    c.setflags(write=False)
    return c


class Case:
    """One chain: ``cores`` (fp64, exact in ``storage``), ``y`` / ``x`` / ``M`` in volume order (read-only)."""

    def __init__(self, shape, family, storage, bonds, salt):
        self.shape, self.family, self.storage, self.salt = tuple(shape), family, storage, salt
        self.dims, self.bonds = site_dims(shape), list(bonds)
        cc.check_chain(self.dims, self.bonds)
        self.n = int(shape[-1])
        self.cores = cc.draw_cores(f"dct/{self.shape}", self.dims, self.bonds, family, storage, salt=salt)
        dest = im.flat_destination(self.shape).reshape(-1)
        self.y = cb.to_volume(mps_to_dense(self.cores), dest).reshape(self.shape)
        self.x = idct(self.y, type=2, norm="ortho", axis=-1)
        self.M = cb.to_volume(cb.abs_dense(self.cores), dest).reshape(self.shape)
        for a in (self.y, self.x, self.M, *self.cores):
            a.setflags(write=False)
        self._bars = {}

    @property
    def label(self):
        return f"{'x'.join(map(str, self.shape))}/{self.family}/{self.storage}"

    def chain_exact(self, chain_type, summed=1):
        """An integer chain contracted in ``chain_type`` (after ``summed`` voxels were added per block on the cores)
        whose every partial product is an exactly representable integer, in any association."""
        if self.family != "integer":
            return False
        prod = int(np.prod(self.bonds, dtype=object)) * int(summed)
        return prod <= 256 if chain_type == "bf16" else prod < EXACT_LIMIT[chain_type]

    def factor(self, call, summed=1):
        """The scalar in front of ``M`` in the propagation term."""
        chain_type = self.storage if call == "to_tensor" else work_of(self.storage)
        if self.chain_exact(chain_type, summed):
            return 0.0
        return cb.chain_factor(self.cores, *roundoff(self.storage, call))

    def decode_bar(self, call):
        """Bar of every element of the decoded volume, shape ``shape`` (cached).  ``call``: "to_tensor", "wide", or
        "f64" for a frame of a series that an fp64 frame makes the call contract and transform in fp64."""
        if call not in self._bars:
            if call == "f64":
                factor = 0.0 if self.chain_exact("f64") else cb.chain_factor(self.cores, *cb.CHAIN_ROUNDOFF["f64"])
                bar = element_bar(self.y, self.M, factor, "f64")
            else:
                bar = element_bar(self.y, self.M, self.factor(call), work_of(self.storage))
            bar.setflags(write=False)
            self._bars[call] = bar
        return self._bars[call]


@functools.lru_cache(maxsize=None)
def case(shape, family, storage, bonds=None, salt=0):
    return Case(shape, family, storage, capped_bonds(shape) if bonds is None else bonds, salt)


# ------------------------------------------------------------------------------------------------ bars
def transform_term(y, work):
    """The transform's own error on coefficient rows ``y`` (..., n) in ``work`` arithmetic, per output entry."""
    n = y.shape[-1]
    if fft_route(n, work):
        return np.broadcast_to(sc.idct_bar(n) * np.linalg.norm(y, axis=-1, keepdims=True), y.shape).copy()
    return cb.HIGHER_ORDER * (n + 2) * U[work] * (np.abs(y) @ np.abs(basis(n)))


def element_bar(y, M, factor, work):
    """Propagation of the chain bound ``factor * M`` through the exact transform, plus the transform term."""
    n = y.shape[-1]
    prop = factor * (M @ np.abs(basis(n))) if factor else 0.0
    return prop + transform_term(y, work)


def block_shape(shape, levels):
    fa = factor_array(shape)
    L = fa.shape[0]
    return tuple(int(np.prod(fa[L - int(k):, a], dtype=np.int64)) for a, k in enumerate(levels))


def block_reduce(vol, blocks, op):
    inter = [v for n, b in zip(vol.shape, blocks) for v in (n // b, b)]
    r = np.asarray(vol, dtype=np.float64).reshape(inter)
    odd = tuple(range(1, 2 * vol.ndim, 2))
    return r.mean(axis=odd) if op == "mean" else r.sum(axis=odd)


def normalize_levels(shape, levels):
    nd = len(shape)
    return [int(levels)] * nd if np.isscalar(levels) else [int(v) for v in levels]


def level_list(shape):
    """The level arguments every pooled test runs (DCT and Std mode)."""
    L, nd = factor_array(shape).shape
    return [0, 1, L, [1] * (nd - 1) + [0], [0] * (nd - 1) + [1], [0] * (nd - 1) + [L], [1] * (nd - 1) + [L - 1],
            [L] + [0] * (nd - 2) + [1]]


def axis_list(shape):
    nd = len(shape)
    return [None, 0, -1, (0, nd - 1), tuple(range(1, nd))]


def axis_levels(shape, axis):
    L, nd = factor_array(shape).shape
    axes = range(nd) if axis is None else [a % nd for a in (axis if isinstance(axis, tuple) else (axis,))]
    return [L if a in axes else 0 for a in range(nd)]


def pooled_weights(n, Bk, w):
    """(Wt, Wabs_t), both (n, n / Bk): ``x_pooled = y @ Wt``; Wabs_t sums the magnitudes of the same terms."""
    c = basis(n)
    return w * c.reshape(n, n // Bk, Bk).sum(axis=-1), w * np.abs(c).reshape(n, n // Bk, Bk).sum(axis=-1)


def pooled(cs, levels, op):
    """(kind, reference, bar) of ``downsample(levels, op)`` on a DCT-mode object holding ``cs``'s cores; kind is
    "pooled" (last axis kept or reduced in part) or "pick" (reduced in full).  Both arrays have the result's shape."""
    shape, n = cs.shape, cs.n
    L = factor_array(shape).shape[0]
    lev = normalize_levels(shape, levels)
    blocks = block_shape(shape, lev)
    others = blocks[:-1] + (1,)
    summed = int(np.prod(others, dtype=np.int64))
    work = work_of(cs.storage)
    ref = block_reduce(cs.x, blocks, op)
    y_r, M_r = block_reduce(cs.y, others, op), block_reduce(cs.M, others, op)
    mean_rounds = op == "mean" and any(b & (b - 1) for b in others)  # 1 / f is rounded
    if lev[-1] == L:
        w = 1.0 / np.sqrt(n) if op == "mean" else np.sqrt(float(n))
        M0 = w * M_r[..., :1]
        if cs.family == "integer":
            # the fp64 reduction of the integer coefficient tensor times the weight: exact zeros stay zeros, which
            # the reduction of the transformed ``x`` only reproduces to a few 2**-53 of the row
            assert np.allclose(ref, w * y_r[..., :1], rtol=0, atol=1e-13 * np.abs(cs.x).sum() / ref.size)
            ref = w * y_r[..., :1]
        if cs.family == "integer" and all(v == L for v in lev):
            chi = sum(cs.bonds[1:-1])
            bar = U[work] * np.abs(ref) + cb.HIGHER_ORDER * (chi + 3 * L) * cb.U_F64 * M0
        else:
            bar = _general_factor(cs) * M0
        return "pick", ref, bar
    factor = _general_factor(cs) if mean_rounds else cs.factor("wide", summed=summed)
    if lev[-1] == 0:
        return "pooled", ref, element_bar(y_r, M_r, factor, work)
    Bk = blocks[-1]
    _, wabs_t = pooled_weights(n, Bk, 1.0 / Bk if op == "mean" else 1.0)
    bar = factor * (M_r @ wabs_t) + cb.HIGHER_ORDER * (n + Bk + 2) * U[work] * (np.abs(y_r) @ wabs_t)
    return "pooled", ref, bar


def _general_factor(cs):
    """The chain factor of the region / pool calls regardless of the family (weighted cores are no integers)."""
    return cb.chain_factor(cs.cores, *roundoff(cs.storage, "wide"))


# ------------------------------------------------------------------------------------------------ pooled basis
_PI = np.longdouble("3.14159265358979323846264338327950288")


def _cos_terms(n, dtype):
    """cos(pi num / (2 n)) for num = 0 .. 4 n - 1 in ``dtype``, the argument reduced on the integers to [0, pi / 4]."""
    num = np.arange(4 * n, dtype=np.int64)
    num = np.where(num > 2 * n, 4 * n - num, num)
    sign = np.where(num > n, -1.0, 1.0)
    num = np.where(num > n, 2 * n - num, num)
    pi = _PI if dtype is np.longdouble else dtype(np.pi)
    small = 2 * num <= n
    val = np.where(small, np.cos(pi * num.astype(dtype) / dtype(2 * n)),
                   np.sin(pi * (n - num).astype(dtype) / dtype(2 * n)))
    return (sign.astype(dtype) * val).astype(dtype)


@functools.lru_cache(maxsize=None)
def pooled_basis(n, Bk, w):
    """``W`` (n / Bk, n) = ``w sum_{m in block j} C[k, m]``, summed in extended precision and rounded once to float64
    (where long double is no wider than double the terms are still reduced exactly and summed by math.fsum)."""
    m = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(n, dtype=np.int64)[None, :]
    idx = ((2 * m + 1) * k) % (4 * n)
    if np.finfo(np.longdouble).nmant >= 63:
        terms = _cos_terms(n, np.longdouble)[idx]                                  # (m, k)
        acc = terms.reshape(n // Bk, Bk, n).sum(axis=1)
        sk = np.sqrt(np.where(k == 0, np.longdouble(1), np.longdouble(2)) / np.longdouble(n))
        out = (np.longdouble(w) * sk * acc).astype(np.float64)
    else:
        import math

        terms = _cos_terms(n, np.float64)[idx].reshape(n // Bk, Bk, n)
        acc = np.array([[math.fsum(terms[j, :, kk]) for kk in range(n)] for j in range(n // Bk)])
        out = w * np.sqrt(np.where(k == 0, 1.0, 2.0) / n) * acc
    out.setflags(write=False)
    return out


def basis_bar(n, Bk, w, f32):
    """Per-entry bar of ndmps_pool_dct_basis_f64 (``f32``: of _f32) against ``pooled_basis(n, Bk, w)``."""
    m = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(n, dtype=np.int64)[None, :]
    terms = _cos_terms(n, np.float64)[((2 * m + 1) * k) % (4 * n)].reshape(n // Bk, Bk, n)
    partial = np.abs(np.cumsum(terms, axis=1))[:, 1:, :].sum(axis=1)           # sum_i |s_i| over the Bk - 1 additions
    W = np.abs(pooled_basis(n, Bk, w))
    bar = cb.U_F64 * abs(w) * np.sqrt(2.0 / n) * (BASIS_TERM_UNITS * Bk + partial) + cb.HIGHER_ORDER * 3 * cb.U_F64 * W
    return bar + cb.U_F32 * W if f32 else bar


def _cospi64(x):
    """cospi of float64 ``x`` in [0, 2): exact reflections to [0, 1 / 4], then cos or sin of the rounded angle."""
    x = np.where(x > 1.0, 2.0 - x, x)
    sign = np.where(x > 0.5, -1.0, 1.0)
    x = np.where(x > 0.5, 1.0 - x, x)
    return sign * np.where(x <= 0.25, np.cos(np.pi * x), np.sin(np.pi * (0.5 - x)))


def kernel_model_basis(n, Bk, w, f32, first=0):
    """The kernel's formula (csrc/pool.hip: pool_dct_basis_kernel) evaluated in float64 on the CPU, term by term in
    its order.  ``first``: a fault, the block of row j starts at ``j Bk + first``."""
    k = np.arange(n, dtype=np.int64)[None, :]
    sk = np.where(k == 0, np.sqrt(1.0 / n), np.sqrt(2.0 / n))
    acc = np.zeros((n // Bk, n))
    j = np.arange(n // Bk, dtype=np.int64)[:, None]
    for i in range(Bk):
        m = j * Bk + i + first
        acc = acc + _cospi64((((2 * m + 1) * k) % (4 * n)).astype(np.float64) / float(2 * n))
    out = w * sk * acc
    return out.astype(np.float32).astype(np.float64) if f32 else out


# ------------------------------------------------------------------------------------------------ regions, points
def extra_region_keys(shape):
    """Keys that restrict, reverse, gather or fix the last axis only (the transformed one)."""
    n = shape[-1]
    rng = np.random.default_rng(n)
    picks = [int(v) for v in rng.integers(-n, n, 9)] + [0, 0, -1, n - 1, n - 1]
    return [(Ellipsis, slice(3, 9)), (Ellipsis, slice(None, None, -2)), (Ellipsis, np.array(picks)), (Ellipsis, n - 2)]


def ix(a, key, shape):
    """a[np.ix_(per-axis indices)] with int axes dropped: the outer-indexing meaning of ``key``."""
    key = key if isinstance(key, tuple) else (key,)
    if any(k is Ellipsis for k in key):
        i = next(j for j, k in enumerate(key) if k is Ellipsis)
        key = key[:i] + (slice(None),) * (len(shape) - len(key) + 1) + key[i + 1:]
    key = key + (slice(None),) * (len(shape) - len(key))
    idx, out_shape = [], []
    for k, n in zip(key, shape):
        if isinstance(k, (int, np.integer)):
            idx.append(np.array([k % n]))
        elif isinstance(k, slice):
            idx.append(np.arange(*k.indices(n)))
            out_shape.append(idx[-1].size)
        else:
            idx.append(np.asarray(k) % n)
            out_shape.append(idx[-1].size)
    return a[np.ix_(*idx)].reshape(out_shape)


def points(shape):
    """(500, ndim) points with negative indices: points 0 and 1 are equal, points 2 .. 59 lie in one last-axis row."""
    rng = np.random.default_rng(len(shape) * 1000 + shape[-1])
    pts = np.stack([rng.integers(-n, n, 500) for n in shape], axis=1)
    pts[1] = pts[0]
    pts[2:60, :-1] = pts[2, :-1]
    return pts


def points_one_row(shape):
    """(40, ndim) points that touch exactly one last-axis row (its lead given with mixed signs), with repeats."""
    rng = np.random.default_rng(7 + shape[-1])
    pts = np.empty((40, len(shape)), dtype=np.int64)
    lead = [n - 1 for n in shape[:-1]]
    pts[:, :-1] = lead
    pts[::2, :-1] = [-1] * (len(shape) - 1)   # the same row, written with negative indices
    pts[:, -1] = rng.integers(-shape[-1], shape[-1], 40)
    return pts
