"""Host side of ``NDMPS.gram`` / ``inner`` / ``pca`` (csrc/series.hip): the argument checks and the K x K linear
algebra of the temporal PCA, as pure NumPy functions (no GPU, no cores read; importable without torch).

The device computes the Gram matrix ``G[a, b] = <X^a, X^b>`` of a series on its cores.  Everything a PCA of the
series needs is a function of G: with ``H = I - 11^T / K`` the centred Gram matrix is ``Gc = H G H = U diag(lam) U^T``,
the singular values of the centred series are ``sigma_k = sqrt(lam_k)``, the scores (coordinates of every frame) are
``U diag(sigma)``, and the unit component k is ``V_k = sum_a c_{a,k} X^a`` with ``c_k = H u_k / sigma_k`` -- weights on
the ORIGINAL frames, so the mean is never formed.  Kept: ``sigma_k > floor * max(sigma_0, s)``, s the largest frame
norm (the project's storage floor, core/lincomb.floor_for: eigenvalues of a Gram matrix resolve singular values to
about sqrt(eps) times the scale of the data), at most ``n_components``.  Sign: the entry of ``u_k`` with the largest
magnitude is positive.
"""
from __future__ import annotations

import numpy as np

ROUTES = {0: "resident", 1: "batched", 2: "per-pair"}


def check_lists(n_objs: int, n_others=None) -> None:
    """ValueError for an empty list."""
    if n_objs < 1:
        raise ValueError("gram needs at least one object")
    if n_others is not None and n_others < 1:
        raise ValueError("gram needs at least one object in `others`")


def check_components(n_components) -> None:
    if n_components is not None and int(n_components) < 1:
        raise ValueError("n_components must be at least 1")


def centre(G) -> np.ndarray:
    """``H G H`` with ``H = I - 11^T / K``, symmetrised (fp64)."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be a square matrix")
    Gc = G - G.mean(axis=0, keepdims=True)
    Gc = Gc - Gc.mean(axis=1, keepdims=True)
    return 0.5 * (Gc + Gc.T)


def pca_weights(G, n_components=None, center: bool = True, floor: float = 1e-6):
    """(sigma (r), U (K x r), weights (K x r)) of the series whose Gram matrix is G; see the module docstring.
    r may be 0 (a constant series, centred)."""
    check_components(n_components)
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be a square matrix")
    K = G.shape[0]
    Gc = centre(G) if center else 0.5 * (G + G.T)
    lam, U = np.linalg.eigh(Gc)
    lam, U = lam[::-1], U[:, ::-1]
    sigma = np.sqrt(np.clip(lam, 0.0, None))
    # sigma_k > floor * sigma_0, and above the absolute floor of the data (the largest frame norm), as the rank rule of
    # linear_combination has it: the centred Gram matrix of a constant series is rounding noise of that size
    scale = np.sqrt(max(float(np.max(np.diag(G))), 0.0))
    r = int(np.count_nonzero(sigma > floor * max(float(sigma[0]), scale)))
    if n_components is not None:
        r = min(r, int(n_components))
    sigma, U = sigma[:r], U[:, :r].copy()
    for k in range(r):
        if U[np.argmax(np.abs(U[:, k])), k] < 0:
            U[:, k] = -U[:, k]
    C = U - U.mean(axis=0, keepdims=True) if center else U.copy()
    C = C / sigma[None, :] if r else C
    return sigma, U, C.reshape(K, r)


def explained_variance(sigma, K: int, center: bool) -> np.ndarray:
    """``sigma^2 / (K - 1)`` (centred; K = 1 gives zeros) or ``sigma^2 / K``."""
    sigma = np.asarray(sigma, dtype=np.float64)
    den = (K - 1) if center else K
    return sigma ** 2 / den if den > 0 else np.zeros_like(sigma)


class SeriesPCA:
    """Result of ``NDMPS.pca``: ``singular_values`` (r), ``explained_variance`` (r), ``scores`` (K x r, the
    coordinates of every frame: ``U diag(sigma)``), ``weights`` (K x r: component k is ``sum_a weights[a, k] X^a``),
    ``components`` (r unit-norm NDMPS) and ``mean`` (NDMPS, or None when uncentred)."""

    def __init__(self, singular_values, explained_variance, scores, weights, components, mean):
        self.singular_values = singular_values
        self.explained_variance = explained_variance
        self.scores = scores
        self.weights = weights
        self.components = components
        self.mean = mean

    def __repr__(self):
        return f"SeriesPCA(n_components={len(self.components)}, frames={self.scores.shape[0]})"
