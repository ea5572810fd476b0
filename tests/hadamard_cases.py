"""Inputs shared by tests/test_hadamard_host.py and tests/test_gpu_hadamard.py (NumPy only)."""
import math

import numpy as np

from oracle.mps import mps_from_dense, mps_to_dense

PLANTED_DIMS = [8] * 5
PLANTED_RANKS = [1, 8, 12, 12, 8, 1]  # min(3 * 4, prod d on either side)


def gaussian_cores(dims, bonds, rng):
    return [rng.standard_normal((bonds[k], dims[k], bonds[k + 1])) for k in range(len(dims))]


def embed(cores, chi, rng):
    """The same chain in bond ``chi``: every core zero-padded, then ``G_k^{-1} . G_{k+1}`` with random invertible
    gauges on the inner bonds."""
    L = len(cores)
    G = [np.eye(1)] + [rng.standard_normal((chi, chi)) + 3.0 * np.eye(chi) for _ in range(L - 1)] + [np.eye(1)]
    out = []
    for k, c in enumerate(cores):
        left, right = (1 if k == 0 else chi), (1 if k == L - 1 else chi)
        p = np.zeros((left, c.shape[1], right))
        p[: c.shape[0], :, : c.shape[2]] = c
        out.append(np.einsum("ab,bic,cd->aid", np.linalg.inv(G[k]), p, G[k + 1]))
    return out


def planted(seed=0, chi=10, dims=PLANTED_DIMS):
    """a of true bond 3 and b of true bond 4, each embedded in bond ``chi``."""
    rng = np.random.default_rng(1000 + seed)
    L = len(dims)
    a = gaussian_cores(dims, [1] + [3] * (L - 1) + [1], rng)
    b = gaussian_cores(dims, [1] + [4] * (L - 1) + [1], rng)
    return embed(a, chi, rng), embed(b, chi, rng)


def bonds_of(cores):
    return [1] + [int(c.shape[2]) for c in cores]


def dense_product(cores_a, cores_b):
    """The product of the two chains' site-order tensors."""
    return mps_to_dense(cores_a) * mps_to_dense(cores_b)


def rel_err(cores, want):
    return float(np.linalg.norm(mps_to_dense(cores) - want) / np.linalg.norm(want))


def truncation_error(dense, dims, max_bond):
    """Frobenius error of the exact TT-SVD of ``dense`` at ``max_bond``."""
    cores, _ = mps_from_dense(dense, dims, cutoff=0.0, max_bond=max_bond)
    return float(np.linalg.norm(mps_to_dense(cores) - dense))


def hmt_bar(L, max_bond, p, best, norm):
    """Halko-Martinsson-Tropp's expectation bound summed over the L - 1 bonds, plus the sketch floor."""
    return math.sqrt(L - 1) * math.sqrt(1.0 + max_bond / (p - 1)) * best + 1e-7 * norm
