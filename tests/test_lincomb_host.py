"""Host checks of NDMPS.linear_combination / recompress (core/lincomb.py, csrc/lincomb.hip), no GPU.

* The validation helpers raise on the cases the public methods reject before anything runs on the device.
* An fp64 NumPy emulation of exactly the device algorithm -- weighted pair environments for the left Gram
  matrices, the Gram-metric bond step (GL = W D W^T, H = D^1/2 W^T G2 W D^1/2), the right-isometric sites
  diag(1/s) V^T D^1/2 W^T A and the ragged block projection X^a x_3 P_a, summed with the weights at site 0 -- is
  compared with the right-to-left TT-SVD of the dense sum (oracle.mps.mps_from_dense): the same bonds and a
  reconstruction within 1e-10 relative.  The Gram route squares the condition number: on random chains the smallest
  kept singular value is about 1e-2 of the largest, so the reconstruction error is about 1e-16 * 1e4, far inside.
"""
import numpy as np
import pytest

from imgcompressionmps_amd.core import lincomb as lc
from oracle.mps import mps_from_dense, mps_to_dense

DOUBT = 1e-13  # eigenvalues of GL at or below DOUBT * max are zeros (tt.hip kDirectDoubt)


def _chain(rng, dims, bonds):
    return [rng.standard_normal((bonds[i], dims[i], bonds[i + 1])) for i in range(len(dims))]


def _bonds_for(rng, dims, chi):
    L = len(dims)
    b = [1]
    left = 1
    for k in range(1, L):
        left *= dims[k - 1]
        right = int(np.prod(dims[k:]))
        b.append(int(min(left, right, chi + rng.integers(0, 3))))
    return b + [1]


def emulate(chains, w, cutoff=0.0, max_bond=None, floor=lc.FLOOR_F64):
    """fp64 emulation of csrc/lincomb.hip.  Returns (cores, spectra) with spectra[k] the kept values at bond k."""
    K, L = len(chains), len(chains[0])
    dims = [int(c.shape[1]) for c in chains[0]]
    chi = [[int(c.shape[0]) for c in ch] + [1] for ch in chains]
    S = [sum(chi[a][j] for a in range(K)) for j in range(L + 1)]
    S[0] = K
    off = [[int(sum(chi[b][j] for b in range(a))) if j > 0 else a for j in range(L + 1)] for a in range(K)]
    scale = lc.scale_of(w, [np.linalg.norm(mps_to_dense(ch)) for ch in chains])
    GL = [np.outer(w, w)]
    for j in range(L - 1):
        G = np.zeros((S[j + 1], S[j + 1]))
        for a in range(K):
            for b in range(a, K):
                E = GL[j][off[a][j]: off[a][j] + chi[a][j], off[b][j]: off[b][j] + chi[b][j]]
                Z = E @ chains[b][j].reshape(chi[b][j], -1)
                blk = chains[a][j].reshape(-1, chi[a][j + 1]).T @ Z.reshape(-1, chi[b][j + 1])
                G[off[a][j + 1]: off[a][j + 1] + chi[a][j + 1], off[b][j + 1]: off[b][j + 1] + chi[b][j + 1]] = blk
                G[off[b][j + 1]: off[b][j + 1] + chi[b][j + 1], off[a][j + 1]: off[a][j + 1] + chi[a][j + 1]] = blk.T
        GL.append(G)
    C = np.vstack([chains[a][L - 1].reshape(chi[a][L - 1], -1) for a in range(K)])
    cores, spectra = [None] * L, [None] * L
    r_next = 1
    for k in range(L - 1, 0, -1):
        A = C.reshape(S[k], -1)
        G2 = A @ A.T
        dw, W = np.linalg.eigh(GL[k])
        dw = np.where(dw > DOUBT * max(dw.max(), 0.0), dw, 0.0)
        Lt = W * np.sqrt(dw)
        h, V = np.linalg.eigh(Lt.T @ G2 @ Lt)
        h, V = h[::-1], V[:, ::-1]
        s = np.sqrt(np.clip(h, 0.0, None))
        r = lc.kept_rank(s, cutoff, floor, scale, lc.rank_cap(dims, k, r_next, max_bond))
        if r == 0:
            return [np.zeros((1, d, 1)) for d in dims], [None] + [np.zeros(1)] * (L - 1)
        Vr, sr = V[:, :r], s[:r]
        cores[k] = (((Lt @ Vr).T @ A) / sr[:, None]).reshape(r, dims[k], r_next)
        spectra[k] = sr
        P = (G2 @ Lt @ Vr) / sr
        blocks = [chains[a][k - 1].reshape(-1, chi[a][k]) @ P[off[a][k]: off[a][k] + chi[a][k]] for a in range(K)]
        if k == 1:
            C = sum(w[a] * blocks[a] for a in range(K))
        else:
            C = np.vstack(blocks).reshape(S[k - 1], -1)
        r_next = r
    cores[0] = C.reshape(1, dims[0], r_next)
    return cores, spectra


CASES = [([8, 8, 8], 1), ([8, 8, 8], 2), ([8, 8, 8], 4), ([2] * 12, 1), ([2] * 12, 3), ([4, 8, 2, 16], 4)]


@pytest.mark.parametrize("dims,K", CASES, ids=[f"{'x'.join(map(str, d))}-K{k}" for d, k in CASES])
def test_emulation_matches_tt_svd_of_dense_sum(dims, K):
    rng = np.random.default_rng(len(dims) * 10 + K)
    chains = [_chain(rng, dims, _bonds_for(rng, dims, 3 + a)) for a in range(K)]
    w = list(rng.uniform(-2.0, 2.0, K))
    dense = sum(wa * mps_to_dense(ch) for wa, ch in zip(w, chains))
    cores, spectra = emulate(chains, w)
    ref, ref_spec = mps_from_dense(dense, dims, cutoff=1e-10)
    assert [c.shape[2] for c in cores[:-1]] == [c.shape[2] for c in ref[:-1]]
    got = mps_to_dense(cores)
    assert np.linalg.norm(got - dense) <= 1e-10 * np.linalg.norm(dense)
    for k in range(1, len(dims)):  # sites 1.. are right-isometric
        m = cores[k].reshape(cores[k].shape[0], -1)
        assert np.abs(m @ m.T - np.eye(m.shape[0])).max() < 1e-9  # eps (s_0 / s_r)^2 of the Gram route
        np.testing.assert_allclose(spectra[k], ref_spec[k][: len(spectra[k])], rtol=0, atol=1e-10 * ref_spec[k][0])


@pytest.mark.parametrize("kw", [dict(cutoff=1e-2), dict(cutoff=1e-1), dict(max_bond=4), dict(max_bond=2)],
                         ids=["c1e-2", "c1e-1", "b4", "b2"])
def test_truncated_emulation_is_tt_svd(kw):
    rng = np.random.default_rng(7)
    dims = [8, 8, 8]
    chains = [_chain(rng, dims, _bonds_for(rng, dims, 5 + a)) for a in range(3)]
    w = [1.0, -0.5, 0.25]
    dense = sum(wa * mps_to_dense(ch) for wa, ch in zip(w, chains))
    cores, _ = emulate(chains, w, **kw)
    ref, _ = mps_from_dense(dense, dims, cutoff=kw.get("cutoff", 1e-10), max_bond=kw.get("max_bond"))
    assert [c.shape[2] for c in cores[:-1]] == [c.shape[2] for c in ref[:-1]]
    err = np.linalg.norm(mps_to_dense(cores) - dense)
    ref_err = np.linalg.norm(mps_to_dense(ref) - dense)
    assert err <= (1 + 1e-9) * ref_err + 1e-10 * np.linalg.norm(dense)


def test_cancellation_and_duplication():
    rng = np.random.default_rng(3)
    dims = [8, 8, 8]
    a = _chain(rng, dims, [1, 6, 5, 1])
    zero, spec = emulate([a, a], [1.0, -1.0])
    assert [c.shape for c in zero] == [(1, 8, 1)] * 3 and all(not c.any() for c in zero)
    assert all(s.tolist() == [0.0] for s in spec[1:])
    two, _ = emulate([a, a], [1.0, 1.0])
    assert [c.shape[2] for c in two[:-1]] == [6, 5]
    dense = mps_to_dense(a)
    assert np.linalg.norm(mps_to_dense(two) - 2 * dense) <= 1e-10 * np.linalg.norm(dense)


def test_zero_scale_is_the_zero_mps():
    """Zero weights (or zero inputs) make scale = 0: nothing survives, never a division by s_0 = 0."""
    rng = np.random.default_rng(4)
    dims = [8, 8, 8]
    a, b = _chain(rng, dims, [1, 6, 5, 1]), _chain(rng, dims, [1, 4, 7, 1])
    for chains, w in [([a, b], [0.0, 0.0]), ([[0 * c for c in a]], [1.0])]:
        cores, spec = emulate(chains, w)
        assert [c.shape for c in cores] == [(1, 8, 1)] * 3
        assert all(np.isfinite(c).all() and not c.any() for c in cores)
        assert all(s.tolist() == [0.0] for s in spec[1:])
    assert lc.kept_rank(np.zeros(4), 0.0, 1e-8, 0.0, 4) == 0


def test_validation_helpers():
    with pytest.raises(ValueError):
        lc.check_args(0, [], 0.0, None)
    with pytest.raises(ValueError):
        lc.check_args(2, [1.0], 0.0, None)
    with pytest.raises(ValueError):
        lc.check_args(1, [float("nan")], 0.0, None)
    with pytest.raises(ValueError):
        lc.check_args(1, [float("inf")], 0.0, None)
    with pytest.raises(ValueError):
        lc.check_args(1, [1.0], -1e-3, None)
    with pytest.raises(ValueError):
        lc.check_args(1, [1.0], 0.0, 0)
    assert lc.check_args(2, (1, -2), 0.0, 3) == [1.0, -2.0]
    m = dict(qubit_size=np.array([8, 8, 8]), shape=(8, 8, 8), mode="Std", device="cuda:0", dims=[8, 8, 8])
    lc.check_compatible([m, dict(m)])
    for key, val in [("shape", (8, 8, 9)), ("mode", "DCT"), ("device", "cuda:1"), ("qubit_size", np.array([8, 8, 4]))]:
        with pytest.raises(ValueError, match=key):
            lc.check_compatible([m, dict(m, **{key: val})])
    lc.check_summed_bonds([[1, 2048, 2048, 1], [1, 2048, 2048, 1]])
    with pytest.raises(ValueError, match="bond 2"):
        lc.check_summed_bonds([[1, 2048, 2049, 1], [1, 2048, 2048, 1]])


def test_rank_rule():
    s = np.array([10.0, 1.0, 1e-3, 1e-7])
    assert lc.kept_rank(s, 0.0, 1e-6, 10.0, 99) == 3       # 1e-7 <= 1e-6 * 10
    assert lc.kept_rank(s, 1e-2, 1e-6, 10.0, 99) == 2      # 1e-3 <= 1e-2 * 10
    assert lc.kept_rank(s, 0.0, 1e-6, 10.0, 2) == 2
    assert lc.kept_rank(s, 0.0, 1e-6, 1e7, 99) == 0        # s_0 below the absolute floor: zero MPS
    assert lc.rank_cap([8, 8, 8], 1, 8, None) == 8
    assert lc.rank_cap([8, 8, 8], 2, 1, None) == 8
    assert lc.rank_cap([2, 2, 2, 2], 2, 2, 3) == 3
    assert lc.floor_for(True) == 1e-8 and lc.floor_for(False) == 1e-6
    assert lc.dtype_code("torch.bfloat16") == 1
    assert lc.work_is_f64([0, 1, 2]) and not lc.work_is_f64([0, 1])


@pytest.mark.parametrize("dtype,with_f64,without_f64", [
    (None, True, False),               # the inputs decide
    ("torch.float32", False, False),   # fp32 asked for: fp32 work whatever the inputs
    ("torch.bfloat16", True, False),   # bf16 only rounds the finished cores: the inputs decide
    ("torch.float64", True, True),     # fp64 asked for
])
def test_work_type_truth_table(dtype, with_f64, without_f64):
    """``work_is_f64(codes, dtype)`` on all eight rows: dtype in {None, fp32, bf16, fp64} x {some fp64 input, none}."""
    assert lc.work_is_f64([0, 2, 1], dtype) is with_f64
    assert lc.work_is_f64([0, 1, 1], dtype) is without_f64


def test_work_type_takes_torch_dtypes():
    torch = pytest.importorskip("torch")
    for dtype in (None, torch.float32, torch.bfloat16, torch.float64):
        for codes in ([0, 2], [1, 0]):
            assert lc.work_is_f64(codes, dtype) == lc.work_is_f64(codes, None if dtype is None else str(dtype))
    assert lc.work_is_f64([0], torch.float64) and not lc.work_is_f64([2], torch.float32)


@pytest.mark.parametrize("K", [361, 362, 400, 4096])
def test_many_inputs_pass_validation(K):
    """K (K + 1) / 2 pair tasks exceed one launch's 65535 from K = 362 on; the host accepts such K whenever the summed
    bond stays within MAX_SUMMED_BOND (csrc/lincomb.hip issues the pair tasks in launches of at most 65535)."""
    assert K * (K + 1) // 2 > 65535 or K == 361
    w = lc.check_args(K, [1.0 / K] * K, 0.0, None)
    assert len(w) == K
    bonds = [[1] + [1 + a % 2 if K <= 2048 else 1] * 4 + [1] for a in range(K)]
    lc.check_summed_bonds(bonds)
    assert max(lc.summed_bonds(bonds)) <= lc.MAX_SUMMED_BOND
