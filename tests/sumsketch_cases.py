"""Inputs shared by tests/test_sumsketch_host.py and tests/test_gpu_sumsketch.py (NumPy only)."""
import math

import numpy as np

from oracle.metrics import synthetic_mri
from oracle.mps import mps_to_dense

import hadamard_cases as hc

PLANTED_DIMS = [8] * 5
PLANTED_T = 12
PLANTED_RANKS = [1, 6, 6, 6, 6, 1]  # three bond-2 chains span every frame: min(3 * 2, prod d on either side)

# Sketch seeds for which ``emulate`` alone stays inside ``hadamard_cases.hmt_bar`` in every case of
# test_sumsketch_host.py::test_quality_on_image_like_frames (the bar bounds an expectation, so the seeds are fixed);
# the GPU tests use exactly these.
SEEDS = (0, 1)


def direct_sum(chains, coef):
    """The chain of ``sum_c coef[c] * chains[c]``: block-diagonal cores, the coefficients in the first."""
    L = len(chains[0])
    if L == 1:
        return [sum(c * ch[0] for c, ch in zip(coef, chains))]
    out = [np.concatenate([c * ch[0] for c, ch in zip(coef, chains)], axis=2)]
    for k in range(1, L - 1):
        d = chains[0][k].shape[1]
        rows, cols = [ch[k].shape[0] for ch in chains], [ch[k].shape[2] for ch in chains]
        core = np.zeros((sum(rows), d, sum(cols)))
        r = c = 0
        for ch in chains:
            core[r: r + ch[k].shape[0], :, c: c + ch[k].shape[2]] = ch[k]
            r, c = r + ch[k].shape[0], c + ch[k].shape[2]
        out.append(core)
    out.append(np.concatenate([ch[L - 1] for ch in chains], axis=0))
    return out


def planted(seed=0, chi=10, dims=PLANTED_DIMS, T=PLANTED_T):
    """T frames, each a random combination of three fixed bond-2 chains, embedded in bond ``chi`` with random gauges,
    and a (2, T) Gaussian weight matrix."""
    rng = np.random.default_rng(2000 + seed)
    L = len(dims)
    base = [hc.gaussian_cores(dims, [1] + [2] * (L - 1) + [1], rng) for _ in range(3)]
    frames = [hc.embed(direct_sum(base, rng.standard_normal(3)), chi, rng) for _ in range(T)]
    return frames, rng.standard_normal((2, T))


def ragged(seed=0):
    """dims [8] * 4, T = 3 frames of ragged bonds, K = 2 rows."""
    rng = np.random.default_rng(3000 + seed)
    dims = [8] * 4
    bonds = [[1, 3, 5, 2, 1], [1, 8, 7, 8, 1], [1, 2, 9, 4, 1]]
    return dims, [hc.gaussian_cores(dims, b, rng) for b in bonds], rng.standard_normal((2, 3))


def dense_sum(frames, w_row):
    """``sum_a w_row[a] * frames[a]`` as the site-order tensor."""
    return sum(float(w) * mps_to_dense(f) for w, f in zip(w_row, frames) if w != 0.0)


def series_weights(T):
    """Three rows over T frames: the mean, the difference of the halves, a cosine."""
    half = np.where(np.arange(T) < T // 2, 1.0, -1.0) / T
    return np.stack([np.full(T, 1.0 / T), half, np.cos(2 * math.pi * np.arange(T) / T) / T])


def series_volumes(shape, T, seed=0, noise=1e-3):
    """T fp32 volumes: random combinations of three base volumes plus small noise, so that sums truncate meaningfully."""
    rng = np.random.default_rng(4000 + seed)
    base = np.stack([synthetic_mri(shape, seed=s).astype(np.float64) for s in (2025, 7, 11)])
    coef = rng.standard_normal((T, 3)) + np.array([2.0, 0.0, 0.0])
    scale = float(np.sqrt(np.mean(base ** 2)))
    vols = np.tensordot(coef, base, axes=1) + noise * scale * rng.standard_normal((T,) + tuple(shape))
    return vols.astype(np.float32)
