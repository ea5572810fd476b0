"""NDMPS.linear_combinations / pca_sketched on the MI355X (csrc/sumsketch.hip, core/sumsketch.py).

Bars, and where they come from:

* Kernel family (``ndmps_sumsketch_step``, three forms): every input is a small integer (|v| <= 4), exact in fp32, bf16
  and fp64, and every partial sum stays below 2**53 (at most 8 * 64 * 130 terms of at most 64), so the fp64 results
  equal NumPy's exactly whatever the order of summation; the output buffer is pre-filled with a sentinel and
  everything past the results keeps it.
* Sketch (``oncore.sum_sketch``) against ``core.sumsketch.emulate`` with the same random cores: identical ranks, and the
  decoded chains agree within ``1e-9 |sum|`` (the bar tests/test_gpu_hadamard.py uses for the same comparison).
* End to end on planted ranks: ``|out.to_tensor() - dense sum| <= tol |sum|`` (Frobenius), tol 1e-5 for fp32 / bf16 work
  and 1e-7 for fp64 (tests/test_gpu_hadamard.py, tests/test_gpu_lincomb.py).
* Truncation: ``hadamard_cases.hmt_bar`` with ``best`` the error of the oracle's exact TT-SVD of the dense sum at
  ``max_bond``, the sketch seeds those vetted in tests/test_sumsketch_host.py (``sumsketch_cases.SEEDS``).
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import hadamard as hd  # noqa: E402
from imgcompressionmps_amd.core import oncore  # noqa: E402
from imgcompressionmps_amd.core import sumsketch as ss  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.utils import core as _core  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402
from oracle.ndmps_oracle import OracleNDMPS  # noqa: E402

import hadamard_cases as hc  # noqa: E402  (tests/ is on the path: rootdir conftest)
import sumsketch_cases as sc  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CODE = {F32: 0, BF16: 1, F64: 2}
STORAGES = [F32, BF16, F64]
SENTINEL = -12345.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _tol(*storages):
    return 1e-7 if any(s == F64 for s in storages) else 1e-5


def _bonds(dims, chi):
    return [1] + [int(min(chi, np.prod(dims[:i]), np.prod(dims[i:]))) for i in range(1, len(dims))] + [1]


def _object(cores, shape, storage, mode="Std"):
    """An NDMPS around host cores (nothing encoded), with its boundary_list and norm_value."""
    dev = [torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(storage).contiguous() for c in cores]
    dims = _core.site_dims(shape)
    obj = NDMPS._from_mps(DeviceMPS(dev), dims, tuple(shape), False, mode, len(shape))
    obj.update_boundary_list()
    obj.update_norm()
    return obj


def _dense(obj):
    """fp64 to_tensor (bf16 cores widened exactly first)."""
    o = obj.astype(F32) if obj.mps.dtype == BF16 else obj
    return np.asarray(o.to_tensor(), dtype=np.float64)


def _host(mps):
    return [c.to(F64).cpu().numpy() for c in mps.cores]


def _same_bits(x, y):
    return all(torch.equal(a, b) for a, b in zip(x.mps.cores, y.mps.cores))


# ------------------------------------------------------------------------------------------------ the kernel family
# (d, frame bonds chi, chi', l0, l1): bonds 10, 17 and 64 mixed in one batch; l = 24, 72, 130 (one, two and three chunks
# of 64, ragged last chunk); T = 1, 3, 5, and T = 9 where the sketch form splits the frames into two shares
STEP_CASES = {
    "T1-d8-l24x24": (8, [10], [17], 24, 24),
    "T3-d6-l72x130": (6, [10, 17, 64], [64, 10, 17], 72, 130),
    "T5-d8-l130x72": (8, [64, 10, 17, 64, 10], [17, 64, 10, 64, 17], 130, 72),
    "T9-d6-l24x24": (6, [10, 17, 64] * 3, [17, 64, 10] * 3, 24, 24),
    "T3-d8-l72x24-80": (8, [10, 80, 64], [80, 17, 64], 72, 24),  # a frame bond of 80: those two frames on the general route
}


def _ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _step_case(name):
    d, chi, chi2, l0, l1 = STEP_CASES[name]
    rng = np.random.default_rng(len(name) + d + l0 + l1)
    T = len(chi)
    A = [_ints(rng, (chi[a], d, chi2[a])) for a in range(T)]
    Wn = [_ints(rng, (chi2[a], l1)) for a in range(T)]
    M = [_ints(rng, (l0, chi[a])) for a in range(T)]
    R, Q = _ints(rng, (l0, d, l1)), _ints(rng, (l0, d, l1))
    env = [np.einsum("aib,bm,lim->al", A[a], Wn[a], R, optimize=True) for a in range(T)]
    sketch = sum(np.einsum("ra,aib,bl->ril", M[a], A[a], Wn[a], optimize=True) for a in range(T))
    project = [np.einsum("rip,ra,aib->pb", Q, M[a], A[a], optimize=True) for a in range(T)]
    return A, Wn, M, R, Q, env, sketch, project


def _cat(mats):
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(m).ravel() for m in mats])).to(DEV)


@pytest.mark.parametrize("form", [0, 1, 2], ids=["env", "sketch", "project"])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_equals_numpy_exactly(name, form):
    lib = _lib.load()
    d, chi, chi2, l0, l1 = STEP_CASES[name]
    A, Wn, M, R, Q, env, sketch, project = _step_case(name)
    T = len(chi)
    storages = [STORAGES[a % 3] for a in range(T)]  # mixed across the frames
    cores = [torch.from_numpy(A[a]).to(DEV).to(storages[a]).contiguous() for a in range(T)]
    want = [np.concatenate([w.ravel() for w in env]), sketch.ravel(), np.concatenate([w.ravel() for w in project])][form]
    d_in = _cat(Wn) if form == 0 else _cat(M)
    d_in2 = _cat(Wn)
    d_mat = torch.from_numpy([R, R, Q][form]).to(DEV).contiguous()
    out = torch.full((want.size + 64,), SENTINEL, dtype=F64, device=DEV)
    wide = [a for a in range(T) if max(chi[a], chi2[a]) > 64]
    ws = torch.empty(68 * T + 8 * 16 * l0 * d * l1 + 1024 + sum(8 * chi[a] * d * chi2[a] + 256 for a in wide)
                     + 8 * l0 * d * max(chi2) + 8 * l0 * d * l1 + 512, dtype=torch.uint8, device=DEV)
    rc = lib.ndmps_sumsketch_step(form, T, d, _lib.i64_array(chi), _lib.i64_array(chi2), (C.c_int * T)(*[CODE[s] for s in storages]),
                                  (C.c_void_p * T)(*[c.data_ptr() for c in cores]), l0, l1, d_in.data_ptr(), d_in2.data_ptr(),
                                  d_mat.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    assert rc == _lib.OK, lib.ndmps_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[want.size:] == SENTINEL), (name, form)
    assert np.array_equal(got[: want.size], want), (name, form, float(np.max(np.abs(got[: want.size] - want))))


# ------------------------------------------------------------------------------------------------ sketch against emulate
def _graded_cores(shape, chi, seed):
    """Gaussian cores whose right bond index b carries the weight 2**-b: the spectrum of a compressed image."""
    dims = [int(d) for d in _core.site_dims(shape)]
    bonds = _bonds(dims, chi)
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((bonds[k], dims[k], bonds[k + 1])) * 2.0 ** -np.arange(bonds[k + 1])[None, None, :]
            for k in range(len(dims))]


def _sketch_and_emulate(frames, w, shape, storage, max_bond, oversample, seed):
    objs = [_object(f, shape, storage) for f in frames]
    held = [_host(o.mps) for o in objs]  # what the storage type holds
    dims = objs[0].mps.dims
    ell = ss.sketch_bonds(dims, [o.mps.bonds for o in objs], max_bond, oversample)
    R = hd.sketch_cores(dims, ell, seed)
    got = oncore.sum_sketch([o.mps for o in objs], np.asarray(w, dtype=np.float64), ell, R)
    return got, ss.emulate(held, w, dims, ell, R), [sc.dense_sum(held, row) for row in w]


@pytest.mark.parametrize("oversample", [4, 8])
def test_sketch_of_planted_ranks_matches_emulate(oversample):
    frames, w = sc.planted(0)
    got, want, sums = _sketch_and_emulate(frames, w, (32, 32, 32), F64, 6, oversample, sc.SEEDS[0])
    for g, (cores, ranks), total in zip(got, want, sums):
        assert g.bonds == ranks == sc.PLANTED_RANKS
        assert all(c.dtype == F64 for c in g.cores)
        dist = np.linalg.norm(mps_to_dense(_host(g)) - mps_to_dense(cores)) / np.linalg.norm(total)
        print(f"planted p {oversample}: sketch vs emulate {dist:.2e}")
        assert dist <= 1e-9
        assert hc.rel_err(_host(g), total) <= 1e-10
        for c in _host(g)[:-1]:
            q = c.reshape(-1, c.shape[2])
            assert np.max(np.abs(q.T @ q - np.eye(q.shape[1]))) <= 1e-12


@pytest.mark.parametrize("storage,wide", [(F32, False), (F64, False), (F32, True)], ids=["f32", "f64", "f32-one-frame-at-80"])
def test_sketch_at_bond_64_matches_emulate(storage, wide):
    shape, T = (64, 64, 64), 6
    frames = [_graded_cores(shape, 80 if wide and a == 2 else 64, 10 + a) for a in range(T)]  # 80: the general route
    w = sc.series_weights(T)[:2]
    got, want, sums = _sketch_and_emulate(frames, w, shape, storage, 16, 16, sc.SEEDS[1])
    for g, (cores, ranks), total in zip(got, want, sums):
        assert g.bonds == ranks
        dist = np.linalg.norm(mps_to_dense(_host(g)) - mps_to_dense(cores)) / np.linalg.norm(total)
        print(f"chi 64 {storage}: ranks {ranks} sketch vs emulate {dist:.2e}")
        assert dist <= 1e-9


# ------------------------------------------------------------------------------------------------ end to end, planted
def _eighths(rng, shape):
    return rng.integers(-64, 65, size=shape).astype(np.float64) / 8


def _planted_exact(seed, T=12):
    """T frames in the span of three bond-2 chains, bonds [1, 8, 10, 10, 8, 1], exact in every storage type: cores in
    multiples of 1/8, combined with power-of-two coefficients, zero-padded and gauged by signed permutations with
    power-of-two scales."""
    rng = np.random.default_rng(seed)
    dims = sc.PLANTED_DIMS
    L = len(dims)
    chi = _bonds(dims, 10)
    base = [[_eighths(rng, ((1 if k == 0 else 2), dims[k], (1 if k == L - 1 else 2))) for k in range(L)] for _ in range(3)]
    frames = []
    for _ in range(T):
        cores = sc.direct_sum(base, 2.0 ** rng.integers(-1, 2, size=3) * rng.choice([-1.0, 1.0], size=3))
        perm = [None] + [rng.permutation(chi[k]) for k in range(1, L)] + [None]
        scale = [None] + [2.0 ** rng.integers(-1, 2, size=chi[k]) * rng.choice([-1.0, 1.0], size=chi[k])
                          for k in range(1, L)] + [None]
        emb = []
        for k, c in enumerate(cores):
            p = np.zeros((chi[k], dims[k], chi[k + 1]))
            p[: c.shape[0], :, : c.shape[2]] = c
            if k > 0:
                p = (p / scale[k][:, None, None])[np.argsort(perm[k])]
            if k < L - 1:
                p = (p * scale[k + 1][None, None, :])[:, :, np.argsort(perm[k + 1])]
            emb.append(p)
        frames.append(emb)
    return frames


def _check_gauge_and_spectra(obj, bonds):
    assert obj.mps.bonds == bonds
    for c in _host(obj.mps)[1:]:
        q = c.reshape(c.shape[0], -1)
        assert np.max(np.abs(q @ q.T - np.eye(q.shape[0]))) <= (1e-10 if obj.mps.dtype == F64 else 1e-4)
    spec = obj.sweep_spectra
    assert spec[0] is None and [len(s) for s in spec[1:]] == bonds[1:-1]
    assert obj.norm is False


@pytest.mark.parametrize("kw", [dict(), dict(max_bond=8, oversample=4)], ids=["exact", "sketched"])
@pytest.mark.parametrize("storages", [(F32,), (BF16, F32), (F64,), (F32, F64)], ids=["f32", "bf16+f32", "f64", "f32+f64"])
def test_linear_combinations_reveal_planted_ranks(storages, kw):
    shape = (32, 32, 32)
    frames = _planted_exact(5)
    objs = [_object(f, shape, storages[a % len(storages)]) for a, f in enumerate(frames)]
    dense = [_dense(o) for o in objs]
    w = np.random.default_rng(1).standard_normal((2, len(objs)))
    outs = NDMPS.linear_combinations(objs, w, **kw)
    assert len(outs) == 2
    for row, out in zip(w, outs):
        want = sum(c * v for c, v in zip(row, dense))
        assert out.mps.dtype == (F64 if F64 in storages else F32)
        err = np.linalg.norm(_dense(out) - want) / np.linalg.norm(want)
        print(f"planted {storages} {kw}: rel err {err:.2e} bonds {out.mps.bonds}")
        assert err <= _tol(*storages)
        _check_gauge_and_spectra(out, sc.PLANTED_RANKS)


# ------------------------------------------------------------------------------------------------ past the wall
@functools.lru_cache(maxsize=None)
def _series(shape, T, max_bond, seed=0):
    """T objects from ``from_tensors(max_bond)`` of ``sumsketch_cases.series_volumes``, and their fp64 decodes."""
    objs = NDMPS.from_tensors(list(sc.series_volumes(shape, T, seed=seed)), max_bond=max_bond, device=DEV)
    dense = np.stack([np.asarray(v, dtype=np.float64) for v in NDMPS.to_tensors(objs)])
    return objs, dense


def _oracle_best(want, max_bond):
    return float(np.linalg.norm(OracleNDMPS.from_tensor(want, max_bond=max_bond).to_tensor() - want))


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_65_frames_of_bond_64_past_the_wall(seed):
    objs, dense = _series((64, 64, 64), 65, 64)
    assert sum(max(o.mps.bonds) for o in objs) == 4160
    W = sc.series_weights(65)
    with pytest.raises(ValueError, match="recompress"):
        NDMPS.linear_combination(objs, W[0], max_bond=32)
    outs = NDMPS.linear_combinations(objs, W, max_bond=32, seed=seed)
    assert len(outs) == 3
    for j, out in enumerate(outs):
        want = np.tensordot(W[j], dense, axes=1)
        best, norm = _oracle_best(want, 32), float(np.linalg.norm(want))
        err = float(np.linalg.norm(_dense(out) - want))
        bar = hc.hmt_bar(out.mps.L, 32, 32, best, norm)
        print(f"65 x 64^3 row {j} seed {seed}: error {err:.4e} best {best:.4e} ratio {err / best:.3f} bar {bar:.4e} "
              f"bonds {out.mps.bonds}")
        assert max(out.mps.bonds) <= 32
        assert err <= bar


def test_65_frames_of_32_cubed_at_full_bonds_are_exact():
    objs, dense = _series((32, 32, 32), 65, 64)
    W = sc.series_weights(65)
    dims = objs[0].mps.dims
    assert ss.sketch_bonds(dims, [o.mps.bonds for o in objs], 64, 64) == _bonds(dims, 64)  # every sketch bond is full
    for j, out in enumerate(NDMPS.linear_combinations(objs, W, max_bond=64, seed=sc.SEEDS[0])):
        want = np.tensordot(W[j], dense, axes=1)
        err = float(np.linalg.norm(_dense(out) - want) / np.linalg.norm(want))
        print(f"65 x 32^3 row {j}: rel err {err:.2e} bonds {out.mps.bonds}")
        assert err <= _tol(F32)


def test_agrees_with_linear_combination_where_it_is_allowed():
    objs, dense = _series((64, 64, 64), 8, 64)
    w = sc.series_weights(8)[2]
    want = np.tensordot(w, dense, axes=1)
    exact = NDMPS.linear_combination(objs, w, max_bond=16)
    sketched = NDMPS.linear_combinations(objs, w, max_bond=16, seed=sc.SEEDS[0])[0]
    e_exact, e_sketch = (float(np.linalg.norm(_dense(o) - want)) for o in (exact, sketched))
    best = _oracle_best(want, 16)
    bar = hc.hmt_bar(exact.mps.L, 16, 16, best, float(np.linalg.norm(want)))
    print(f"T 8: exact {e_exact:.4e} sketched {e_sketch:.4e} best {best:.4e} bar {bar:.4e}")
    assert sketched.mps.bonds == exact.mps.bonds
    assert e_sketch <= bar


# ------------------------------------------------------------------------------------------------ PCA
def test_pca_sketched_against_pca():
    objs, dense = _series((32, 32, 32), 12, 12)
    T = len(objs)
    ref = NDMPS.pca(objs, n_components=3, max_bond=12)
    got = NDMPS.pca_sketched(objs, n_components=3, max_bond=12, seed=sc.SEEDS[0])
    for name in ("singular_values", "scores", "weights", "explained_variance"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert len(got.components) == len(ref.components) == 3
    rows = [got.weights[:, k] for k in range(3)] + [np.full(T, 1.0 / T)]
    for row, out in zip(rows, list(got.components) + [got.mean]):
        want = np.tensordot(row, dense, axes=1)
        best, norm = _oracle_best(want, 12), float(np.linalg.norm(want))
        err = float(np.linalg.norm(_dense(out) - want))
        print(f"pca: error {err:.4e} best {best:.4e} bar {hc.hmt_bar(out.mps.L, 12, 12, best, norm):.4e}")
        assert err <= hc.hmt_bar(out.mps.L, 12, 12, best, norm)
    assert NDMPS.pca_sketched(objs, n_components=2, max_bond=12, center=False).mean is None


def test_pca_sketched_past_the_wall():
    objs, _ = _series((64, 64, 64), 65, 64)
    with pytest.raises(ValueError, match="recompress"):
        NDMPS.pca(objs, n_components=2, max_bond=16)
    got = NDMPS.pca_sketched(objs, n_components=2, max_bond=16, seed=sc.SEEDS[0])
    assert len(got.components) == 2 and got.mean is not None
    assert all(max(c.mps.bonds) <= 16 for c in list(got.components) + [got.mean])


# ------------------------------------------------------------------------------------------------ behaviour
def test_determinism_and_skipping():
    objs, dense = _series((32, 32, 32), 12, 12)
    objs = list(objs)
    W = sc.series_weights(12)
    W[:, 5] = 0.0   # a frame no row uses
    W[1, 2] = 0.0   # a zero entry
    W = np.vstack([W, np.zeros(12)])  # and a row of zeros
    a = NDMPS.linear_combinations(objs, W, max_bond=8, seed=3)
    b = NDMPS.linear_combinations(objs, W, max_bond=8, seed=3)
    c = NDMPS.linear_combinations(objs, W, max_bond=8, seed=4)
    assert all(_same_bits(x, y) for x, y in zip(a, b))
    assert not all(_same_bits(x, y) for x, y in zip(a[:3], c[:3]))
    poisoned = list(objs)
    poisoned[5] = _object([np.full(tuple(t.shape), np.nan) for t in objs[5].mps.cores], (32, 32, 32), F32)
    p = NDMPS.linear_combinations(poisoned, W, max_bond=8, seed=3)
    assert all(_same_bits(x, y) for x, y in zip(a, p))
    zero = a[3]
    assert zero.mps.bonds == [1] * (zero.mps.L + 1)
    assert all(float(t.abs().max()) == 0.0 for t in zero.mps.cores)
    assert all(np.array_equal(s, [0.0]) for s in zero.sweep_spectra[1:])
    assert float(zero.norm_value) == 0.0
    gone = NDMPS.linear_combinations([objs[0], objs[0]], [1.0, -1.0], max_bond=8)[0]  # a sum that vanishes
    assert np.linalg.norm(_dense(gone)) <= 1e-5 * np.linalg.norm(dense[0])
    one_d = NDMPS.linear_combinations(objs, W[0], max_bond=8, seed=3)
    two_d = NDMPS.linear_combinations(objs, W[:1], max_bond=8, seed=3)
    assert len(one_d) == 1 and _same_bits(one_d[0], two_d[0])


def test_dct_mode_and_mixed_storage():
    vols = list(sc.series_volumes((32, 32, 32), 4, seed=1))
    dct = [NDMPS.from_tensor(v, max_bond=12, mode="DCT", device=DEV) for v in vols]
    w = np.array([0.5, -1.0, 2.0, 0.25])
    out = NDMPS.linear_combinations(dct, w)[0]  # summed bonds <= 48: the exact sum
    want = sum(c * _dense(o) for c, o in zip(w, dct))
    assert out.mode == "DCT"
    assert np.linalg.norm(_dense(out) - want) <= _tol(F32) * np.linalg.norm(want)
    std = [NDMPS.from_tensor(v, max_bond=12, device=DEV) for v in vols]
    assert NDMPS.linear_combinations(std, w, max_bond=8)[0].mps.dtype == F32
    assert NDMPS.linear_combinations([std[0].astype(BF16)] + std[1:], w, max_bond=8)[0].mps.dtype == F32
    assert NDMPS.linear_combinations([std[0].astype(F64)] + std[1:], w, max_bond=8)[0].mps.dtype == F64
    assert NDMPS.linear_combinations(std, w, max_bond=8, dtype=BF16)[0].mps.dtype == BF16
    assert NDMPS.linear_combinations(std, w, max_bond=8, dtype=F64)[0].mps.dtype == F64
    with pytest.raises(ValueError, match="mode"):
        NDMPS.linear_combinations([std[0], dct[1]], [1.0, 1.0], max_bond=8)


def test_rejected_arguments():
    objs, _ = _series((32, 32, 32), 12, 12)
    a = objs[0]
    with pytest.raises(TypeError):
        NDMPS.linear_combinations([a, 2.0], [1.0, 1.0])
    for lst, w in [([], []), ([a, a], [1.0]), ([a, a], np.ones((2, 3))), ([a, a], np.ones((1, 1, 2))), ([a], [float("nan")]),
                   ([a], [float("inf")])]:
        with pytest.raises(ValueError):
            NDMPS.linear_combinations(lst, w, max_bond=8)
    for kw in (dict(cutoff=-1.0), dict(max_bond=0), dict(oversample=-1), dict(seed=0.5), dict(seed=-1), dict(dtype=torch.float16)):
        with pytest.raises(ValueError):
            NDMPS.linear_combinations([a, a], [1.0, 1.0], **{**dict(max_bond=8), **kw})
    with pytest.raises(ValueError, match="shape"):
        NDMPS.linear_combinations([a, NDMPS.from_tensor(sc.series_volumes((16, 32, 32), 1)[0], max_bond=8, device=DEV)], [1.0, 1.0])
    big, _ = _series((64, 64, 64), 65, 64)
    with pytest.raises(ValueError, match="pass max_bond"):
        NDMPS.linear_combinations(big, np.ones(65))
    huge = _object(_graded_cores((256, 256, 256), 64, 0), (256, 256, 256), F32)  # prod d reaches 4096
    with pytest.raises(ValueError, match=r"must be <= 512"):
        NDMPS.linear_combinations([huge] * 10, np.ones(10), max_bond=300, oversample=300)
    # the neighbours keep their refusals
    with pytest.raises(TypeError):
        a * a
    with pytest.raises(ValueError, match="recompress"):
        NDMPS.linear_combination(list(big[:9]) * 8, [1.0] * 72)
