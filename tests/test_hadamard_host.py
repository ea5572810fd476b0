"""Host side of NDMPS.multiply (core/hadamard.py): sketch bonds, argument checks and the fp64 emulation of the
randomised sketch, against dense products.  No GPU.

Bars: the emulation at full bonds and on planted ranks is exact up to fp64 rounding (1e-12 and 1e-10 of the product's
norm: products of up to five Gaussian cores and gauges of condition ~10).  On image-like cores the error after an
exact TT-SVD to ``max_bond`` is held against the Halko-Martinsson-Tropp expectation bound summed over the bonds,
``sqrt(L - 1) sqrt(1 + max_bond / (p - 1)) best + 1e-7 |product|``; the seeds are fixed.
"""
import os
import re

import numpy as np
import pytest

from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import hadamard as hd
from imgcompressionmps_amd.utils import core as _core
from oracle.metrics import synthetic_mri
from oracle.mps import mps_from_dense, mps_to_dense
from oracle.ndmps_oracle import OracleNDMPS

import hadamard_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sketch_bonds_follow_the_rule():
    dims = [8] * 5
    bonds = [1, 8, 10, 10, 8, 1]
    assert hd.sketch_bonds(dims, bonds, bonds, 12, 8) == [1, 8, 20, 20, 8, 1]
    assert hd.sketch_bonds(dims, [1, 10, 10, 10, 10, 1], [1, 10, 10, 10, 10, 1], 12, 8) == [1, 8, 20, 20, 8, 1]
    assert hd.sketch_bonds(dims, bonds, bonds, 12, 4) == [1, 8, 16, 16, 8, 1]
    # m_k caps: bonds 2 x 3
    assert hd.sketch_bonds(dims, [1, 2, 2, 2, 2, 1], [1, 3, 3, 3, 3, 1], 12, 8) == [1, 6, 6, 6, 6, 1]
    # no max_bond: the product bonds themselves, prod d caps not applied
    assert hd.sketch_bonds(dims, bonds, [1, 3, 3, 3, 3, 1], None, 0) == [1, 24, 30, 30, 24, 1]
    # uneven dims: prod_{j<k} d_j on the left, prod_{j>=k} d_j on the right
    assert hd.sketch_bonds([2, 3, 50, 2], [1, 9, 9, 9, 1], [1, 9, 9, 9, 1], 40, 8) == [1, 2, 6, 2, 1]
    assert hd.sketch_bonds([4], [1, 1], [1, 1], 3, 2) == [1, 1]


def test_rejected_arguments():
    dims = [8] * 4
    big = [1, 64, 64, 64, 1]
    with pytest.raises(ValueError, match=r"max_bond \+ oversample must be <= 512"):
        hd.sketch_bonds([64] * 4, big, big, 300, 300)
    with pytest.raises(ValueError, match="pass max_bond"):
        hd.sketch_bonds(dims, big, big, None, 0)
    with pytest.raises(ValueError):
        hd.sketch_bonds(dims, big[:-1], big, 4, 4)
    assert hd.check_args(None, 0.0, None, 0) == (None, 8, 0)
    assert hd.check_args(16, 0.0, None, 3) == (16, 16, 3)
    assert hd.check_args(4, 1e-3, None, 3) == (4, 8, 3)
    assert hd.check_args(4, 0.0, 0, np.int64(5)) == (4, 0, 5)
    for bad in [dict(oversample=-1), dict(oversample=1.5), dict(seed=1.0), dict(seed="0"), dict(seed=None), dict(seed=True),
                dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(max_bond=0), dict(max_bond=2.5)]:
        kw = dict(max_bond=4, cutoff=0.0, oversample=None, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            hd.check_args(**kw)
    hd.check_workspace(hd.WS_LIMIT_BYTES)
    with pytest.raises(ValueError, match="recompress the inputs first"):
        hd.check_workspace(hd.WS_LIMIT_BYTES + 1)
    assert (hd.MAX_SKETCH_BOND, hd.SKETCH_FLOOR, hd.WS_LIMIT_BYTES) == (512, 1e-7, 2 << 30)


def test_sketch_cores_are_reproducible_and_scaled():
    dims, ell = [8, 4, 8], [1, 8, 6, 1]
    R = hd.sketch_cores(dims, ell, 7)
    assert [r.shape for r in R] == [(1, 8, 8), (8, 4, 6), (6, 8, 1)] and all(r.dtype == np.float64 for r in R)
    rng = np.random.default_rng(7)
    for k, r in enumerate(R):  # site 0 first, one draw per core
        assert np.array_equal(r, rng.standard_normal(r.shape) / np.sqrt(dims[k] * ell[k + 1]))
    assert all(np.array_equal(x, y) for x, y in zip(R, hd.sketch_cores(dims, ell, 7)))


@pytest.mark.parametrize("seed", range(12))
def test_emulate_at_full_bonds_is_the_dense_product(seed):
    dims = [8, 8, 8, 8]
    rng = np.random.default_rng(seed)
    bonds = [1, 8, 8, 8, 1]
    a, b = hc.gaussian_cores(dims, bonds, rng), hc.gaussian_cores(dims, bonds, rng)
    ell = hd.sketch_bonds(dims, bonds, bonds, None, 0)
    assert ell == [1, 64, 64, 64, 1]
    cores, ranks = hd.emulate(a, b, dims, ell, hd.sketch_cores(dims, ell, seed))
    assert ranks == [1, 8, 64, 64, 1]  # the left interfaces' ranks: nothing is sketched from the right
    assert hc.rel_err(cores, hc.dense_product(a, b)) <= 1e-12


@pytest.mark.parametrize("oversample", [4, 8])
@pytest.mark.parametrize("seed", range(6))
def test_planted_rank_is_revealed(seed, oversample):
    dims = hc.PLANTED_DIMS
    a, b = hc.planted(seed)
    assert hc.bonds_of(a) == [1, 10, 10, 10, 10, 1]
    ell = hd.sketch_bonds(dims, hc.bonds_of(a), hc.bonds_of(b), 12, oversample)
    cores, ranks = hd.emulate(a, b, dims, ell, hd.sketch_cores(dims, ell, seed))
    assert ranks == hc.PLANTED_RANKS
    assert [c.shape for c in cores] == [(ranks[k], 8, ranks[k + 1]) for k in range(5)]
    err = hc.rel_err(cores, hc.dense_product(a, b))
    print(f"planted seed {seed} p {oversample}: rel err {err:.2e}")
    assert err <= 1e-10
    for c in cores[:-1]:  # left-orthonormal
        q = c.reshape(-1, c.shape[2])
        assert np.max(np.abs(q.T @ q - np.eye(q.shape[1]))) <= 1e-12


def test_zero_product_is_reported():
    dims = [4, 4, 4]
    rng = np.random.default_rng(3)
    a = hc.gaussian_cores(dims, [1, 2, 2, 1], rng)
    b = hc.gaussian_cores(dims, [1, 2, 2, 1], rng)
    a[1][:, 2:, :] = 0.0  # a lives on digits 0, 1 of site 1 and b on digits 2, 3
    b[1][:, :2, :] = 0.0
    ell = hd.sketch_bonds(dims, [1, 2, 2, 1], [1, 2, 2, 1], 3, 2)
    cores, ranks = hd.emulate(a, b, dims, ell, hd.sketch_cores(dims, ell, 0))
    assert cores is None and ranks == [1, 1, 1, 1]


@pytest.fixture(scope="module")
def image_cores():
    """Oracle cores of two synthetic volumes per (shape, input bond), with the dense product and its norm."""
    out = {}
    for shape in [(32, 32, 32), (16, 24, 20)]:
        dims = [int(d) for d in _core.site_dims(shape)]
        for chi in (8, 12):
            a = OracleNDMPS.from_tensor(synthetic_mri(shape, seed=2025), max_bond=chi).mps.cores
            b = OracleNDMPS.from_tensor(synthetic_mri(shape, seed=7), max_bond=chi).mps.cores
            want = hc.dense_product(a, b)
            out[shape, chi] = (dims, a, b, want, hc.truncation_error(want, dims, 2 * chi))
    return out


@pytest.mark.parametrize("p", [None, 8, 4], ids=["p=max_bond", "p=8", "p=4"])
@pytest.mark.parametrize("chi", [8, 12])
@pytest.mark.parametrize("shape", [(32, 32, 32), (16, 24, 20)], ids=["32c", "16x24x20"])
def test_quality_on_image_like_cores(image_cores, shape, chi, p):
    dims, a, b, want, best = image_cores[shape, chi]
    max_bond = 2 * chi
    _, oversample, seed = hd.check_args(max_bond, 0.0, p, 0)
    ell = hd.sketch_bonds(dims, hc.bonds_of(a), hc.bonds_of(b), max_bond, oversample)
    cores, _ = hd.emulate(a, b, dims, ell, hd.sketch_cores(dims, ell, seed))
    rounded, _ = mps_from_dense(mps_to_dense(cores), dims, cutoff=0.0, max_bond=max_bond)  # the exact TT-SVD of the sketch
    total = float(np.linalg.norm(mps_to_dense(rounded) - want))
    bar = hc.hmt_bar(len(dims), max_bond, oversample, best, float(np.linalg.norm(want)))
    print(f"{shape} chi {chi} p {oversample}: error {total:.4e} best {best:.4e} ratio {total / best:.3f} bar ratio {bar / best:.3f}")
    assert total <= bar


def test_signatures_match_the_header():
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    for name in ("ndmps_hadamard_layout", "ndmps_hadamard_sketch", "ndmps_hadamard_sandwich"):
        decl = re.search(name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(","))
