"""Host side of ``NDMPS.linear_combinations`` / ``pca_sketched`` (csrc/sumsketch.hip): K weighted sums of T objects,
rounded by a randomised sketch on the cores.  NumPy only: the argument checks, the sketch bonds and an fp64 emulation of
the device's whole sketch.

The formal sum chain of the frames ``A_a`` is block-diagonal with the bonds ``m_k = sum_a chi_{a,k}``; the exact
Gram-SVD sweep of ``linear_combination`` has eigenproblems of that order.  Following "randomise then orthogonalise"
(Al Daas, Ballard, Cazeaux et al., *Randomized algorithms for rounding in the tensor-train format*, SISC 2023, sum of
TT tensors) the sum chain is never formed: it is multiplied from the right by a random chain ``R`` of bonds ``l_k``
(``core.hadamard.sketch_cores``), frame by frame:

1. right environments, once per call (they do not depend on the weights), k = L-1 .. 1, ``W_{a,L} = [1]``:
   ``W_{a,k}[al,lam] = sum_{i,be,mu} A_{a,k}[al,i,be] W_{a,k+1}[be,mu] R_k[lam,i,mu]``;
2. forward, per output row j, k = 0 .. L-2, ``M_{a,0} = [w_{j,a}]``:
   ``X_a = M_{a,k} A_{a,k}`` (``(r_k d_k) x chi_{a,k+1}``), ``S = sum_a X_a W_{a,k+1}`` (a ascending), orthonormalised
   twice through its Gram matrix exactly as ``multiply`` does (``core.hadamard._gram_pass``, ``SKETCH_FLOOR``), site k =
   the result ``Q``, ``M_{a,k+1} = Q^T X_a``; the last site is ``sum_a X_{a,L-1}``.

A frame whose weights are zero in every row is read in neither pass, and a zero entry is skipped in that row's forward
pass.  The cost is linear in T and no eigenproblem exceeds ``max_bond + oversample``.
"""
from __future__ import annotations

import numpy as np

from . import hadamard as _hd


def check_weights(n_objs, weights) -> np.ndarray:
    """``weights`` as a ``(K, T)`` fp64 array (a 1-D array of length T is one row).  ValueError for an empty list of
    objects, more than two dimensions, a last dimension that is not T, no row, or a non-finite entry."""
    if n_objs < 1:
        raise ValueError("linear_combinations needs at least one object")
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"weights must be a real array: {e}") from None
    if w.ndim == 1:
        w = w[None, :]
    if w.ndim != 2:
        raise ValueError(f"weights must have one or two dimensions, got {w.ndim}")
    if w.shape[1] != n_objs:
        raise ValueError(f"weights has {w.shape[1]} columns for {n_objs} objects")
    if w.shape[0] < 1:
        raise ValueError("weights has no row")
    if not np.all(np.isfinite(w)):
        raise ValueError("weights must be finite")
    return np.ascontiguousarray(w)


def used_frames(w) -> list:
    """The frames some row gives a non-zero weight, ascending."""
    return [a for a in range(w.shape[1]) if np.any(w[:, a] != 0.0)]


def summed_bonds(bond_lists, frames=None) -> list:
    """``m_k = sum_a chi_{a,k}`` over ``frames`` (all by default)."""
    frames = range(len(bond_lists)) if frames is None else frames
    L1 = len(bond_lists[0])
    return [sum(int(bond_lists[a][k]) for a in frames) for k in range(L1)]


def sketch_bonds(dims, bond_lists, max_bond, oversample, frames=None) -> list:
    """``l_k = min(max_bond + oversample, m_k, prod_{j<k} d_j, prod_{j>=k} d_j)`` with ``l_0 = l_L = 1`` and ``m_k``
    over ``frames``; ``max_bond=None``: ``l_k = m_k`` (the exact sum, nothing truncated by the sketch).  ValueError when
    some ``l_k`` exceeds ``hadamard.MAX_SKETCH_BOND``."""
    if any(len(bl) != len(dims) + 1 for bl in bond_lists):
        raise ValueError("bonds must have one entry more than dims")
    # a bond no frame reaches (m_k = 0, no frames) is sketched as bond 1
    return _hd.sketch_bonds_of(dims, [max(1, v) for v in summed_bonds(bond_lists, frames)], max_bond, oversample, "sum")


def emulate(cores_per_frame, weights, dims, ell, R):
    """The device's whole sketch (steps 1-2 of the module docstring) in NumPy fp64.  ``cores_per_frame[a][k]`` is
    ``(chi, d, chi')``; ``weights`` is ``(K, T)``.  A list of K ``(sketched cores, ranks)``; ``(None, [1] * (L + 1))``
    for a zero output."""
    w = check_weights(len(cores_per_frame), weights)
    K, T = w.shape
    L = len(dims)
    used = used_frames(w)
    A = {a: [np.asarray(c, dtype=np.float64) for c in cores_per_frame[a]] for a in used}
    R = [np.asarray(r, dtype=np.float64) for r in R]
    W = {}
    for a in used:
        Wa = [None] * (L + 1)
        Wa[L] = np.ones((1, 1))
        for k in range(L - 1, 0, -1):
            Wa[k] = np.einsum("aib,bm,lim->al", A[a][k], Wa[k + 1], R[k], optimize=True)
        W[a] = Wa
    results = []
    for j in range(K):
        frames = [a for a in used if w[j, a] != 0.0]
        ranks = [1] * (L + 1)
        if not frames:
            results.append((None, ranks))
            continue
        M = {a: np.full((1, 1), w[j, a]) for a in frames}
        out, r = [], 1
        for k in range(L):
            d = int(dims[k])
            X = {a: np.einsum("ra,aib->rib", M[a], A[a][k]).reshape(r * d, -1) for a in frames}
            if k == L - 1:
                S = np.zeros((r * d, 1))
                for a in frames:
                    S = S + X[a]
                out.append(S.reshape(r, d, 1))
                break
            S = np.zeros((r * d, int(ell[k + 1])))
            for a in frames:
                S = S + X[a] @ W[a][k + 1]
            Q, r1 = _hd._gram_pass(S)
            if r1:
                Q, r1 = _hd._gram_pass(Q)
            if not r1:
                out = None
                break
            ranks[k + 1] = r1
            out.append(Q.reshape(r, d, r1))
            M = {a: Q.T @ X[a] for a in frames}
            r = r1
        results.append((out, ranks) if out is not None else (None, [1] * (L + 1)))
    return results
