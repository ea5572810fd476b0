"""Oracle (test infrastructure): element-wise forward error bounds for the decoders, NumPy fp64.

A product of L matrices ``A_0 A_1 ... A_{L-1}`` with inner extents ``chi_1 .. chi_{L-1}``, evaluated in floating
point in ANY association and ANY order of summation, with accumulator unit roundoff ``u_acc`` and every
intermediate (the result included) rounded once to a type of unit roundoff ``u_store``, differs from the exact
product by at most, element-wise and to first order,

    (u_acc * sum_i chi_i  +  u_store * (L - 1)) * M,        M = |A_0| |A_1| ... |A_{L-1}|

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.5 for one product -- gamma_k |A||B| --
and section 3.7 for products of several matrices).  The factor 1.01 below pays for the higher-order terms, which
are of relative size ``sum(chi) * u`` (< 1e-2 for every chain this project can hold).  Nothing here is measured
from, or tuned to, a kernel.

Unit roundoffs: fp32 2**-24, fp64 2**-53, bf16 2**-8 (8 significant bits).  The chain kernels accumulate bf16
products in fp32 (``u_acc = 2**-24``) and store every intermediate as bf16 (``u_store = 2**-8``).
"""
from __future__ import annotations

import numpy as np

from .mps import mps_overlap, mps_to_dense

U_F32 = 2.0 ** -24
U_F64 = 2.0 ** -53
U_BF16 = 2.0 ** -8
HIGHER_ORDER = 1.01

# (u_acc, u_store) of the chain contraction per storage type of the cores
CHAIN_ROUNDOFF = {"f32": (U_F32, U_F32), "f64": (U_F64, U_F64), "bf16": (U_F32, U_BF16)}


def _abs64(cores):
    return [np.abs(np.asarray(c, dtype=np.float64)) for c in cores]


def abs_dense(cores):
    """``M = |A_0| |A_1| ... |A_{L-1}|`` in site order, shape ``(d_0, ..., d_{L-1})``."""
    return mps_to_dense(_abs64(cores))


def abs_overlap(a_cores, b_cores):
    """``mps_overlap`` of the element-wise absolute values of both chains."""
    return mps_overlap(_abs64(a_cores), _abs64(b_cores))


def chain_factor(cores, u_acc, u_store):
    """The scalar in front of ``M``: ``1.01 * (u_acc * sum_{i=1..L-1} chi_i + u_store * (L - 1))``; 0 for L == 1."""
    L = len(cores)
    chi = sum(int(c.shape[0]) for c in cores[1:])
    return HIGHER_ORDER * (u_acc * chi + u_store * (L - 1))


def chain_bound(cores, u_acc, u_store):
    """Element-wise bound on ``|computed - mps_to_dense(cores)|``, shape ``(d_0, ..., d_{L-1})``.  Where it is 0
    (an element all of whose terms vanish, or L == 1) the computed value must equal the reference exactly."""
    return chain_factor(cores, u_acc, u_store) * abs_dense(cores)


def overlap_bound(a_cores, b_cores, u_acc=U_F64, u_store=U_F64):
    """Bound on ``|computed - mps_overlap(a, b)|`` for the transfer-matrix contraction: per site two products,
    ``E^T A`` of inner extent ``chi_a`` and ``X^T B`` of inner extent ``chi_b * d`` (oracle.mps.mps_overlap)."""
    inner = 0
    for a, b in zip(a_cores, b_cores):
        inner += int(a.shape[0]) + int(b.shape[0]) * int(a.shape[1])
    return HIGHER_ORDER * (u_acc * inner + u_store * 2 * len(a_cores)) * abs_overlap(a_cores, b_cores)


def gemm_bound(a, b, u):
    """Element-wise bound ``1.01 * u * k * |A| |B|`` on one product with inner extent ``k``."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    b = np.abs(np.asarray(b, dtype=np.float64))
    return HIGHER_ORDER * u * a.shape[1] * (a @ b)


# ------------------------------------------------------------------------------------------------ index map
def flat_destination_factors(factor_arr):
    """``oracle.index_map.flat_destination`` for an explicit factor array ``(L, ndim)`` whose columns multiply to the
    shape: the offset in the site-order tensor (site dims = row products) of every voxel of the C-order volume.
    Site 0 holds the coarsest digit of every axis, the digits of one site are ravelled row-major
    (utils/core.py:6-35 of the reference, restated as oracle.index_map.dest_tables for get_factorlist(shape))."""
    fa = np.asarray(factor_arr, dtype=np.int64)
    L, nd = fa.shape
    shape = tuple(int(v) for v in np.prod(fa, axis=0))
    site_dim = np.prod(fa, axis=1)
    site_stride = np.ones(L, dtype=np.int64)
    for lvl in range(L - 2, -1, -1):
        site_stride[lvl] = site_stride[lvl + 1] * site_dim[lvl + 1]
    dest = np.zeros(shape, dtype=np.int64)
    for j in range(nd):
        x = np.arange(shape[j], dtype=np.int64)
        t = np.zeros(shape[j], dtype=np.int64)
        w = 1
        for lvl in range(L - 1, -1, -1):
            f = int(fa[lvl, j])
            inner = int(np.prod(fa[lvl, j + 1:]))
            t += ((x // w) % f) * inner * int(site_stride[lvl])
            w *= f
        dest += t.reshape((1,) * j + (-1,) + (1,) * (nd - 1 - j))
    return dest


def to_volume(site_order, dest):
    """The C-order volume of a site-order tensor (or of its bound): ``volume[x] = site_order.flat[dest[x]]``."""
    return np.asarray(site_order).reshape(-1)[dest]
