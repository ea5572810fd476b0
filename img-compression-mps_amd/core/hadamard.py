"""Host side of ``NDMPS.multiply`` / ``square`` (csrc/hadamard.hip): the elementwise product of two objects by a
randomised sketch on the cores.  NumPy only: the argument checks, the sketch bonds, the random cores and an fp64
emulation of the device's whole sketch.

The product chain ``Z_k[(a,a'), i, (b,b')] = A_k[a,i,b] B_k[a',i,b']`` decodes to the product of the two volumes (both
objects share one encoding map) and has the bonds ``m_k = chi_a chi_b``.  It is never formed.  Following
"randomise then orthogonalise" (Al Daas, Ballard, Cazeaux et al., *Randomized algorithms for rounding in the
tensor-train format*, SISC 2023) it is multiplied from the right by a random chain ``R`` of bonds ``l_k``:

1. right environments, k = L-1 .. 1, ``W_L = [1]``:
   ``W_k[a,a',lam] = sum_{i,b,b',mu} A_k[a,i,b] B_k[a',i,b'] W_{k+1}[b,b',mu] R_k[lam,i,mu]``
   (a bond with ``l_k = m_k`` needs none: the sketch is the identity there);
2. forward, k = 0 .. L-2, carrying ``X_k`` (``(r_k d_k) x m_{k+1}``), ``X_0 = A_0 (x) B_0``:
   ``S = X_k W_{k+1}``, orthonormalised twice through its Gram matrix (``G = S^T S = V diag(s^2) V^T``, keep
   ``s_j > SKETCH_FLOOR s_0``, ``S <- S V_r diag(1/s)``), site k = the result ``Q``, ``M = Q^T X_k``,
   ``X_{k+1}[rho,i] = A_{k+1}[:,i,:]^T M_rho B_{k+1}[:,i,:]``; the last site is ``X_{L-1}``.

The sketched chain is left-orthonormal with bonds ``r_k <= l_k``; ``ndmps_lincomb_round`` rounds it like every other
operator's result.  The condition number of ``S`` after the floor is at most 1e7, so ``eps cond^2 ~ 1e-2 < 1`` and the
second pass restores orthonormality to rounding.
"""
from __future__ import annotations

import math
import numbers
import operator

import numpy as np

MAX_SKETCH_BOND = 512  # largest order handed to the eigen-solver
SKETCH_FLOOR = 1e-7    # singular values of a sketched bond below this fraction of the largest are dropped
WS_LIMIT_BYTES = 2 << 30


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def check_args(max_bond, cutoff, oversample, seed):
    """(max_bond or None, oversample, seed) as ints.  ValueError for cutoff < 0, max_bond < 1, oversample < 0 or a
    non-integer seed.  ``oversample=None`` is ``max(8, max_bond)``."""
    if not (isinstance(cutoff, numbers.Real) and cutoff >= 0 and math.isfinite(cutoff)):
        raise ValueError("cutoff must be a finite non-negative number")
    if max_bond is not None:
        if not _is_int(max_bond) or int(max_bond) < 1:
            raise ValueError("max_bond must be an integer of at least 1")
        max_bond = operator.index(max_bond)
    if oversample is None:
        oversample = max(8, max_bond or 0)
    elif not _is_int(oversample) or int(oversample) < 0:
        raise ValueError("oversample must be a non-negative integer")
    if not _is_int(seed) or int(seed) < 0:
        raise ValueError("seed must be a non-negative integer")
    return max_bond, operator.index(oversample), operator.index(seed)


def product_bonds(bonds_a, bonds_b) -> list:
    return [int(a) * int(b) for a, b in zip(bonds_a, bonds_b)]


def sketch_bonds(dims, bonds_a, bonds_b, max_bond, oversample) -> list:
    """``l_k = min(max_bond + oversample, m_k, prod_{j<k} d_j, prod_{j>=k} d_j)`` with ``l_0 = l_L = 1``;
    ``max_bond=None``: ``l_k = m_k`` (the exact product, nothing random).  ValueError when some ``l_k`` exceeds
    MAX_SKETCH_BOND."""
    if len(bonds_a) != len(dims) + 1 or len(bonds_b) != len(dims) + 1:
        raise ValueError("bonds must have one entry more than dims")
    return sketch_bonds_of(dims, product_bonds(bonds_a, bonds_b), max_bond, oversample, "product")


def sketch_bonds_of(dims, m, max_bond, oversample, what) -> list:
    """The sketch bonds over the bonds ``m`` (L + 1 entries) of the chain that is sketched, the ``what`` ("product",
    "sum") of the message: the rule of ``sketch_bonds``, shared with core/sumsketch.py."""
    dims = [int(d) for d in dims]
    L = len(dims)
    if max_bond is None:
        ell = list(m)
    else:
        if oversample < 0:
            raise ValueError("oversample must be a non-negative integer")
        cap = int(max_bond) + int(oversample)
        ell = [min(cap, m[k], math.prod(dims[:k]), math.prod(dims[k:])) for k in range(L + 1)]
    ell[0] = ell[L] = 1
    for k in range(1, L):
        if ell[k] > MAX_SKETCH_BOND:
            if max_bond is None:
                raise ValueError(f"bond {k}: the exact {what} has bond {ell[k]} > {MAX_SKETCH_BOND}; pass max_bond")
            raise ValueError(f"bond {k}: max_bond + oversample must be <= {MAX_SKETCH_BOND}, got {cap}")
    return ell


def sketch_cores(dims, ell, seed) -> list:
    """The random cores ``R_k`` (``l_k, d_k, l_{k+1}``, fp64): ``numpy.random.default_rng(seed).standard_normal``, site 0
    first, each scaled by ``1 / sqrt(d_k l_{k+1})``."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((int(ell[k]), int(d), int(ell[k + 1]))) / math.sqrt(int(d) * int(ell[k + 1]))
            for k, d in enumerate(dims)]


def check_workspace(ws_bytes) -> None:
    if int(ws_bytes) > WS_LIMIT_BYTES:
        raise ValueError(f"the sketch needs a workspace of {int(ws_bytes)} bytes > {WS_LIMIT_BYTES}; recompress the inputs "
                         f"first (recompress(max_bond=...))")


def _gram_pass(S):
    """One Gram orthonormalisation of S (rows x l): (Q, r), r = 0 when S is zero."""
    w, V = np.linalg.eigh(S.T @ S)
    w, V = w[::-1], V[:, ::-1]
    if not w[0] > 0.0:
        return None, 0
    s0 = math.sqrt(w[0])
    r = 0
    while r < w.size and w[r] > 0.0 and math.sqrt(w[r]) > SKETCH_FLOOR * s0:
        r += 1
    r = min(r, S.shape[0])
    return (S @ V[:, :r]) / np.sqrt(w[:r])[None, :], r


def emulate(cores_a, cores_b, dims, ell, R):
    """The device's whole sketch (steps 1-2 of the module docstring) in NumPy fp64 on ``(chi, d, chi')`` cores:
    ``(sketched cores, ranks)``; ``(None, [1] * (L + 1))`` for the zero product."""
    A = [np.asarray(c, dtype=np.float64) for c in cores_a]
    B = [np.asarray(c, dtype=np.float64) for c in cores_b]
    L = len(dims)
    m = product_bonds([1] + [c.shape[2] for c in A], [1] + [c.shape[2] for c in B])
    W = [None] * (L + 1)  # W[k]: (l_k, chi_a, chi_b), None where the sketch is the identity
    for k in range(L - 1, 0, -1):
        if ell[k] == m[k]:
            continue
        ca2, cb2 = A[k].shape[2], B[k].shape[2]
        if W[k + 1] is None:
            Y = np.asarray(R[k], dtype=np.float64).reshape(ell[k], dims[k], ca2, cb2)
        else:
            Y = np.einsum("lim,mbc->libc", R[k], W[k + 1], optimize=True)
        W[k] = np.einsum("aib,libc,eic->lae", A[k], Y, B[k], optimize=True)
    ranks = [1] * (L + 1)
    out = []
    M = np.ones((1, 1, 1))
    for k in range(L):
        X = np.einsum("aib,rac,cid->ribd", A[k], M, B[k], optimize=True)
        r, d, ca2, cb2 = X.shape
        X = X.reshape(r * d, ca2 * cb2)
        if k == L - 1:
            out.append(X.reshape(r, d, 1))
            break
        S = X if W[k + 1] is None else X @ W[k + 1].reshape(ell[k + 1], -1).T
        Q, r1 = _gram_pass(S)
        if r1:
            Q, r1 = _gram_pass(Q)
        if not r1:
            return None, [1] * (L + 1)
        ranks[k + 1] = r1
        out.append(Q.reshape(r, d, r1))
        M = (Q.T @ X).reshape(r1, ca2, cb2)
    return out, ranks
