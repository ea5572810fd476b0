"""Host side of the masked / weighted Gram matrix ``NDMPS.gram(objs, weight=w)`` (csrc/wgram.hip): the argument
checks, the workspace limit, an fp64 restatement of the contraction and its error bar, as pure NumPy functions (no GPU;
importable without torch).

The device computes ``G_w[a, b] = sum_x w(x) X^a(x) X^b(x)`` on the cores of three chains.  For one pair the transfer
object is a stack of matrices ``E_j[w]`` (``w < chi_{w,j}``, each ``chi_{a,j} x chi_{b,j}``, ``E_0 = [[1]]``)::

    P_j[w, i]   = A_j[:, i, :]^T ( E_j[w] B_j[:, i, :] )
    E_{j+1}[w'] = sum_{(w,i)} W_j[w, i, w'] P_j[w, i]
    G_w[a, b]   = E_L[0][0, 0]

Three nested products per site, with inner extents ``chi_b``, ``chi_a`` and ``chi_w d``.  Their forward error bound is
the bar ``weighted_bound``: ``1.01 * 2**-53 * N * S`` with ``N = sum_j (chi_{a,j} + chi_{b,j} + chi_{w,j} d_j + 4)`` and
``S`` the same triple sum over the absolute values of all cores (so ``S = 0`` demands an exact 0).
"""
from __future__ import annotations

import numpy as np

WS_LIMIT_BYTES = 1 << 30  # cap of one call's workspace; more pairs than fit are processed in chunks
U64 = 2.0 ** -53


def check_weight_type(weight, cls) -> None:
    """TypeError unless ``weight`` is an instance of ``cls`` (NDMPS)."""
    if not isinstance(weight, cls):
        raise TypeError(f"weight must be an NDMPS object, not {type(weight).__name__}")


def check_mode(mode) -> None:
    """ValueError in DCT mode, for the reason ``multiply`` gives."""
    if mode == "DCT":
        raise ValueError("DCT mode stores DCT coefficients: their product is not the product of the volumes")


def check_workspace(ws_bytes, limit=None) -> int:
    """The answer of ``ndmps_series_wgram_workspace_bytes`` under the cap ``limit``: ValueError when not even one pair
    fits (the library answers with a negative code), else the bytes."""
    limit = WS_LIMIT_BYTES if limit is None else int(limit)
    if int(ws_bytes) < 0:
        raise ValueError(f"one pair of the weighted Gram matrix needs a workspace above {limit} bytes; recompress the "
                         f"inputs or the weight first (recompress(max_bond=...))")
    return int(ws_bytes)


def _as_cores(cores):
    out = [np.asarray(c, dtype=np.float64) for c in cores]
    for c in out:
        if c.ndim != 3:
            raise ValueError("cores must be (chi_left, d, chi_right)")
    return out


def _check_chains(a, w, b) -> None:
    if not (len(a) == len(w) == len(b)) or len(a) < 1:
        raise ValueError("the three chains need the same number of sites (at least one)")
    for j, (A, W, B) in enumerate(zip(a, w, b)):
        if not (A.shape[1] == W.shape[1] == B.shape[1]):
            raise ValueError(f"site {j}: physical dims differ: {A.shape[1]}, {W.shape[1]}, {B.shape[1]}")
    for c in (a, w, b):
        if c[0].shape[0] != 1 or c[-1].shape[2] != 1:
            raise ValueError("the outer bonds must be 1")


def emulate(cores_a, cores_w, cores_b) -> float:
    """``sum_x a(x) w(x) b(x)`` in fp64 in the shipped association order (module docstring)."""
    a, w, b = _as_cores(cores_a), _as_cores(cores_w), _as_cores(cores_b)
    _check_chains(a, w, b)
    E = np.ones((1, 1, 1))  # [w][chi_a][chi_b]
    for A, W, B in zip(a, w, b):
        cw, d, cw2 = W.shape
        P = np.empty((cw, d, A.shape[2], B.shape[2]))
        for v in range(cw):
            for i in range(d):
                P[v, i] = A[:, i, :].T @ (E[v] @ B[:, i, :])
        E = (W.reshape(cw * d, cw2).T @ P.reshape(cw * d, -1)).reshape(cw2, A.shape[2], B.shape[2])
    return float(E[0, 0, 0])


def steps(cores_a, cores_w, cores_b) -> int:
    """``N = sum_j (chi_{a,j} + chi_{b,j} + chi_{w,j} d_j + 4)``: the summed inner extents of the three products."""
    return int(sum(A.shape[0] + B.shape[0] + W.shape[0] * W.shape[1] + 4 for A, W, B in zip(cores_a, cores_w, cores_b)))


def weighted_bound(cores_a, cores_w, cores_b) -> float:
    """The bar of one entry: ``1.01 * 2**-53 * N * S`` (module docstring)."""
    a, w, b = _as_cores(cores_a), _as_cores(cores_w), _as_cores(cores_b)
    S = emulate([np.abs(c) for c in a], [np.abs(c) for c in w], [np.abs(c) for c in b])
    return 1.01 * U64 * steps(a, w, b) * S
