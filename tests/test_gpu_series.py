"""NDMPS.gram / inner / pca on the MI355X (csrc/series.hip, core/series.py).

Bars, and where they come from:

* Element bar of G on arbitrary cores: ``|G[a, b] - mps_overlap(a, b)| <= max(overlap_bound(a, b), overlap_bound(b, a))``
  (oracle/chain_bound.py, u = 2**-53: the inputs are widened exactly and every product accumulates in fp64), on the
  cores as stored, for all three routes.  Where the bound is 0 the entry is exactly 0; the integer cases come out bit
  for bit.  tests/test_series_host.py proves on the CPU that this bar holds for a NumPy restatement of the kernels'
  association and rejects a dropped physical index / a transposed core on every case used here
  (tests/series_cases.py).
* Objects from ``from_tensor``: ``|G[a, b] - <to_tensor(a), to_tensor(b)>| <= tol * |a| |b|`` with the tolerance of
  an exact combination in tests/test_gpu_lincomb.py (1e-5 fp32 / bf16, 1e-7 fp64) and its reasoning: the comparison
  includes the decoder's own rounding in the storage type (about 1e-7 relative per core at fp32).
* PCA: singular values and scores against NumPy's SVD of the decoded, centred series within ``tol * sigma_0``;
  components orthonormal within ``e_k + e_l + e_k e_l``, ``e_k = tol * sum_a |c_{a,k}| norm_value_a`` (the guarantee
  of an exact ``linear_combination``), for the components with ``sigma_k >= 1e-3 sigma_0`` only: beyond that
  ``1 / sigma_k`` amplifies the storage noise of the frames, which is the method, not a defect.
* Memory: the Gram matrix of 8 objects of 256^3 at chi = 64 raises the allocator peak by less than one decoded volume.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import series_cases as sc  # noqa: E402
from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_overlap  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"f32": F32, "bf16": BF16, "f64": F64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _objects(cores_list, storages):
    """NDMPS objects around the given fp64 cores, stored as ``storages`` (the values are representable: exact)."""
    out = []
    for cores, st in zip(cores_list, storages):
        dev = [torch.from_numpy(np.ascontiguousarray(c)).to(device=DEV, dtype=DT[st]) for c in cores]
        dims = np.array([c.shape[1] for c in cores])
        out.append(NDMPS(DeviceMPS(dev), dims, None, None, False, None, "Std", 3))
    return out


def _stored(obj):
    return [c.to(F64).cpu().numpy() for c in obj.mps.cores]


def _check_entries(G, objs, others, integer=False):
    sa = [_stored(o) for o in objs]
    sb = sa if others is None else [_stored(o) for o in others]
    worst = 0.0
    for i, a in enumerate(sa):
        for k, b in enumerate(sb):
            if others is None and k < i:
                continue
            ref = mps_overlap(a, b)
            tol = max(cb.overlap_bound(a, b), cb.overlap_bound(b, a))
            if integer:
                assert G[i, k] == ref, (i, k, G[i, k], ref)
            if tol == 0.0:
                assert G[i, k] == 0.0, (i, k, G[i, k])
                continue
            worst = max(worst, abs(G[i, k] - ref) / tol)
            assert abs(G[i, k] - ref) <= tol, (i, k, G[i, k], ref, tol)
    print(f"worst |G - ref| / bar = {worst:.3g}")


@pytest.mark.parametrize("name", list(sc.CASES))
def test_gram_entries_against_the_oracle(name):
    case = sc.CASES[name]
    la, lb = sc.cores_of(name)
    objs = _objects(la, case["storage_a"])
    others = None if lb is None else _objects(lb, case["storage_b"])
    assert NDMPS.gram_route(objs, others) == case["route"]
    G = NDMPS.gram(objs, others)
    assert G.dtype == np.float64 and G.shape == (len(objs), len(objs if others is None else others))
    _check_entries(G, objs, others, integer=case["family"] == "integer")
    G2 = NDMPS.gram(objs, others)
    assert np.array_equal(G, G2), "two calls must give identical bits"
    if others is None:
        assert np.array_equal(G, G.T), "G[b, a] is a copy of G[a, b]"
        # the rectangular call on the same list computes [b, a] itself (other order of summation): same bar
        _check_entries(NDMPS.gram(objs, list(objs)), objs, list(objs), integer=case["family"] == "integer")
        for i, o in enumerate(objs):  # the diagonal against the pair contraction of the parent commit
            a = _stored(o)
            assert abs(G[i, i] - (o.mps @ o.mps)) <= 2 * cb.overlap_bound(a, a)
        assert objs[0].inner(objs[-1]) == G[0, -1]
    else:
        assert objs[0].inner(others[-1]) == G[0, -1]
        _check_entries(NDMPS.gram(others, objs), others, objs, integer=case["family"] == "integer")
    t = NDMPS.gram(objs, others, as_torch=True)
    assert t.dtype == F64 and t.is_cuda and np.array_equal(t.cpu().numpy(), G)


def test_gram_of_362_tiny_chains_entry_by_entry():
    la, _ = sc.cores_of("many", sc.MANY)
    objs = _objects(la, sc.MANY["storage_a"])
    assert NDMPS.gram_route(objs) == "resident" and len(objs) * (len(objs) + 1) // 2 == 65703
    G = NDMPS.gram(objs)
    assert np.array_equal(G, G.T)
    _check_entries(G, objs, None)


def _make(shape, variant, storage=F32, mode="Std", seed=17):
    """The variants of tests/test_gpu_lincomb.py::_make."""
    x = synthetic_mri(shape, seed=seed)
    dt = F64 if storage == F64 else None
    if variant == "exact":
        obj = NDMPS.from_tensor(x, mode=mode, device=DEV, dtype=dt)
    elif variant == "max_bond":
        obj = NDMPS.from_tensor(x, mode=mode, max_bond=12, device=DEV, dtype=dt)
    elif variant == "compress":
        obj = NDMPS.from_tensor(x, mode=mode, device=DEV, dtype=dt)
        obj.compress(0.01)
    elif variant == "left":
        obj = NDMPS.from_tensor(x, mode=mode, max_bond=12, device=DEV, dtype=dt, sweep_from="left")
    elif variant == "replaced":
        obj = NDMPS.from_tensor(x, mode=mode, max_bond=8, device=DEV, dtype=dt)
        rng = np.random.default_rng(seed)
        obj.replace_tensordata([rng.standard_normal(t.shape).astype(np.float64 if dt else np.float32) * 0.1
                                for t in obj.return_tensors_data()])
    else:
        raise AssertionError(variant)
    return obj.astype(BF16) if storage == BF16 else obj


def _dense(obj):
    o = obj.astype(F32) if obj.mps.dtype == BF16 else obj
    return np.asarray(o.to_tensor(), dtype=np.float64)


def _tol(storage):
    return 1e-7 if storage == F64 else 1e-5


VARIANTS = ("exact", "max_bond", "compress", "left", "replaced")


@pytest.mark.parametrize("mode", ["Std", "DCT"])
@pytest.mark.parametrize("storage", [F32, BF16, F64], ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("shape", [(64, 64, 64), (30, 45, 20)], ids=["64c", "30x45x20"])
def test_gram_of_encoded_objects_against_decoded_volumes(shape, storage, mode):
    objs = [_make(shape, v, storage, mode, seed=s) for s, v in enumerate(VARIANTS, start=1)]
    route = NDMPS.gram_route(objs)
    # 64^3 exact: bonds 8, 64, 512, 64, 8 beside capped ones -> the per-pair general route
    assert route == "per-pair" if shape == (64, 64, 64) else route in ("resident", "per-pair"), route
    G = NDMPS.gram(objs)
    X = np.stack([_dense(o).reshape(-1) for o in objs])
    want = X @ X.T
    nrm = np.sqrt(np.diag(want))
    assert np.all(np.abs(G - want) <= _tol(storage) * np.outer(nrm, nrm)), np.max(np.abs(G - want) / np.outer(nrm, nrm))
    others = objs[1:3]
    Gr = NDMPS.gram(objs, others)
    assert np.all(np.abs(Gr - want[:, 1:3]) <= _tol(storage) * np.outer(nrm, nrm[1:3]))


def test_gram_errors_are_those_of_linear_combination():
    a = _make((16, 16, 16), "max_bond")
    with pytest.raises(ValueError):
        NDMPS.gram([])
    with pytest.raises(ValueError):
        NDMPS.gram([a], [])
    with pytest.raises(TypeError):
        NDMPS.gram([a, 3.0])
    with pytest.raises(TypeError):
        NDMPS.gram([a], [a, "x"])
    for bad in (_make((16, 16, 32), "max_bond"), _make((16, 16, 16), "max_bond", mode="DCT")):
        with pytest.raises(ValueError) as e1:
            NDMPS.gram([a, bad])
        with pytest.raises(ValueError) as e2:
            NDMPS.linear_combination([a, bad], [1.0, 1.0])
        assert str(e1.value) == str(e2.value)
        with pytest.raises(ValueError):
            NDMPS.gram([a], [bad])
    if torch.cuda.device_count() > 1:
        other = NDMPS.from_tensor(synthetic_mri((16, 16, 16), seed=3), max_bond=12, device="cuda:1")
        with pytest.raises(ValueError):
            NDMPS.gram([a, other])
    with pytest.raises(ValueError):
        NDMPS.pca([a, a], n_components=0)
    with pytest.raises(ValueError):
        NDMPS.pca([])


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.load()
    a = _make((16, 16, 16), "max_bond")
    L = a.mps.L
    dims, bonds = _lib.i64_array(a.mps.dims), _lib.i64_array(a.mps.bonds)
    ptrs = (C.c_void_p * L)(*[c.data_ptr() for c in a.mps.cores])
    G = torch.full((1, 1), 7.0, dtype=F64, device=DEV)
    ws = torch.empty(lib.ndmps_series_gram_workspace_bytes(1, 1, L, dims, bonds, bonds), dtype=torch.uint8, device=DEV)
    call = lambda codes, nbytes: lib.ndmps_series_gram(1, 1, 1, L, dims, bonds, (C.c_int * 1)(codes), ptrs, bonds,  # noqa: E731
                                                       (C.c_int * 1)(codes), ptrs, G.data_ptr(), ws.data_ptr(), nbytes,
                                                       _lib.stream_ptr())
    assert call(3, ws.numel()) == _lib.EINVAL and b"dtype code" in lib.ndmps_last_error()
    assert call(0, 8) == _lib.EWORKSPACE
    torch.cuda.synchronize()
    assert float(G[0, 0]) == 7.0
    assert call(0, ws.numel()) == _lib.OK
    torch.cuda.synchronize()
    assert float(G[0, 0]) == NDMPS.gram([a])[0, 0]


def test_gram_memory_stays_below_one_volume():
    rng = np.random.default_rng(0)
    objs = []
    for s in range(8):
        cores = [torch.from_numpy(rng.uniform(0.5, 1.0, size=(sc.U64[j], 8, sc.U64[j + 1])).astype(np.float32)).to(DEV)
                 for j in range(8)]
        objs.append(NDMPS(DeviceMPS(cores), np.array([8] * 8), None, None, False, None, "Std", 3))
    assert NDMPS.gram_route(objs) == "resident"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    G = NDMPS.gram(objs, as_torch=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 256 ** 3 * 4, peak
    assert bool(torch.isfinite(G).all()) and bool((G > 0).all())


# ------------------------------------------------------------------------------------------------------- PCA
def _series():
    """K = 12 volumes of 64^3: three fixed synthetic_mri volumes mixed by a known 12 x 3 matrix, plus small noise."""
    rng = np.random.default_rng(42)
    base = np.stack([synthetic_mri((64, 64, 64), seed=s) for s in (1, 2, 3)]).astype(np.float64)
    mix = rng.uniform(-1.0, 1.0, size=(12, 3)) + np.array([2.0, 0.0, 0.0])
    frames = np.tensordot(mix, base, axes=1) + 1e-4 * rng.standard_normal((12, 64, 64, 64))
    return [NDMPS.from_tensor(f.astype(np.float32), max_bond=16, device=DEV) for f in frames]


def test_pca_of_a_mixed_series():
    objs = _series()
    K, tol = len(objs), _tol(F32)
    res = NDMPS.pca(objs)
    X = np.stack([_dense(o).reshape(-1) for o in objs])
    Xc = X - X.mean(axis=0, keepdims=True)
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    r = len(res.singular_values)
    assert 3 <= r <= K - 1 and len(res.components) == r and res.scores.shape == (K, r) and res.weights.shape == (K, r)
    np.testing.assert_allclose(res.singular_values, s[:r], rtol=0, atol=tol * s[0])
    np.testing.assert_allclose(res.explained_variance, s[:r] ** 2 / (K - 1), rtol=0, atol=2 * tol * s[0] ** 2 / (K - 1))
    strong = [k for k in range(r) if s[k] >= 1e-3 * s[0]]  # beyond that 1 / sigma_k amplifies storage noise
    assert len(strong) >= 3
    for k in strong:
        sign = np.sign(U[np.argmax(np.abs(U[:, k])), k])
        np.testing.assert_allclose(res.scores[:, k], sign * U[:, k] * s[k], rtol=0, atol=tol * s[0])
    comps = [res.components[k] for k in strong]
    Gc = NDMPS.gram(comps)
    norms = np.array([float(o.norm_value) for o in objs])
    e = np.array([tol * float(np.abs(res.weights[:, k]) @ norms) for k in strong])
    for i in range(len(strong)):
        for j in range(len(strong)):
            assert abs(Gc[i, j] - (i == j)) <= e[i] + e[j] + e[i] * e[j], (i, j, Gc[i, j], e[i], e[j])
    mean = np.asarray(res.mean.to_tensor(), dtype=np.float64).reshape(-1)
    assert np.linalg.norm(mean - X.mean(axis=0)) <= tol * float(np.mean(norms))


def test_pca_options():
    objs = _series()
    capped = NDMPS.pca(objs, n_components=2, max_bond=8)
    assert len(capped.components) == 2 and capped.scores.shape == (12, 2)
    assert all(max(c.bond_sizes()) <= 8 for c in capped.components) and max(capped.mean.bond_sizes()) <= 8
    raw = NDMPS.pca(objs, n_components=1, center=False)
    assert raw.mean is None and len(raw.components) == 1
    X = np.stack([_dense(o).reshape(-1) for o in objs])
    s = np.linalg.svd(X, compute_uv=False)
    np.testing.assert_allclose(raw.singular_values, s[:1], rtol=0, atol=_tol(F32) * s[0])
    np.testing.assert_allclose(raw.explained_variance, s[:1] ** 2 / 12, rtol=0, atol=2 * _tol(F32) * s[0] ** 2 / 12)
