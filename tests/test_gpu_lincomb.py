"""NDMPS.linear_combination / recompress and the NDMPS operators on the MI355X (csrc/lincomb.hip, core/lincomb.py).

Bars, and where they come from:

* Exact combination: ``|got - want| <= tol * scale`` (Frobenius), ``scale = sum_a |w_a| norm_value_a``, against
  ``sum_a w_a to_tensor(a)`` in fp64 (bf16 inputs: ``to_tensor(a.astype(F32))``, since the kernels widen bf16 cores
  exactly).  tol 1e-5 for fp32 / bf16 work and 1e-7 for fp64.  The rounding drops directions below the storage floor
  (1e-6 * scale, 1e-8 * scale); each dropped one costs at most the floor, and the fp32 result cores add their own
  rounding (about 1e-7 relative per core).  1e-5 leaves room for about 100 dropped directions at fp32, 1e-7 for 10 at
  fp64 (the synthetic volumes of an exact combination drop only noise).
* TT-SVD parity: the same truncation as ``oracle.mps.mps_from_dense`` on the fp64 site-order sum: equal bonds, except
  that the rule may drop oracle values at or below its own threshold ``max(cutoff s_0, floor scale)`` (the oracle has
  no absolute floor) and may differ by near-ties within 1e-3 of the cutoff; under ``max_bond`` alone a bond can only be
  smaller by values below the floor.  ``|R - S| <= (1 + 1e-3) |T - S| + tol scale``
  and the kept spectra within 1e-5 s_0 (the fp64 Gram route resolves singular values to about 1e-8 s_0).
* Gauge: sites 1..L-1 right-isometric to 1e-5 (fp32 cores: rounding of the stored cores) and 2e-9 for fp64.  A row
  of a site is diag(1/s) of a Gram-route projection, so its error grows like eps s_0 / s_j, and an exact
  combination keeps values down to the 1e-8 floor: 1e-10 cannot be met.  Measured 4.4e-10 on the 30x45x20
  combination below (deterministic inputs); 2e-9 leaves a factor of 4.5.
* Memory: the combination of four 256^3 objects raises the allocator peak by less than one decoded volume.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import codec  # noqa: E402
from imgcompressionmps_amd.utils.metrics import compute_overlap  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_from_dense, mps_to_dense  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SHAPES = [(64, 64, 64), (30, 45, 20), (512, 680), (16, 16, 8, 32)]
SHAPE_IDS = ["64c", "30x45x20", "512x680", "16x16x8x32"]
STORAGES = [F32, BF16, F64]
ST_IDS = ["f32", "bf16", "f64"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _make(shape, variant, storage=F32, mode="Std", seed=17):
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
    """fp64 to_tensor (bf16 cores widened exactly first)."""
    o = obj.astype(F32) if obj.mps.dtype == BF16 else obj
    return np.asarray(o.to_tensor(), dtype=np.float64)


def _site_dense(obj):
    return mps_to_dense([c.to(F64).cpu().numpy() for c in obj.mps.cores])


def _scale(objs, w):
    return sum(abs(a) * float(o.norm_value) for a, o in zip(w, objs))


def _tol(storage):
    return 1e-7 if storage == F64 else 1e-5


@pytest.mark.parametrize("mode", ["Std", "DCT"])
@pytest.mark.parametrize("storage", STORAGES, ids=ST_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_exact_combination(shape, storage, mode):
    objs = [_make(shape, v, storage, mode, seed=s)
            for s, v in zip((1, 2, 3, 4, 5), ("max_bond", "compress", "left", "replaced", "max_bond"))]
    w = [1.0, -0.75, 0.5, 2.0, -1.25]
    r = NDMPS.linear_combination(objs, w)
    want = sum(a * _dense(o) for a, o in zip(w, objs))
    got = np.asarray(r.to_tensor(), dtype=np.float64)
    assert r.mps.dtype == (F64 if storage == F64 else F32)
    assert np.linalg.norm(got - want) <= _tol(storage) * _scale(objs, w)
    assert r.norm is False and r.mode == mode and r._shape == objs[0]._shape
    assert r.sweep_spectra[0] is None and [len(s) for s in r.sweep_spectra[1:]] == r.bond_sizes()


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_weighted_mean_of_eight(storage):
    objs = [_make((64, 64, 64), "max_bond", storage, seed=100 + s) for s in range(8)]
    w = [1.0 / 8] * 8
    r = NDMPS.linear_combination(objs, w)
    want = sum(a * _dense(o) for a, o in zip(w, objs))
    assert np.linalg.norm(np.asarray(r.to_tensor(), np.float64) - want) <= _tol(storage) * _scale(objs, w)


def _check_tt_svd(r, objs, w, cutoff, max_bond, storage):
    dims = r.mps.dims
    S = sum(a * _site_dense(o) for a, o in zip(w, objs))
    ref, spec = mps_from_dense(S, dims, cutoff=cutoff if cutoff else 1e-10, max_bond=max_bond)
    got_b, ref_b = r.bond_sizes(), [c.shape[2] for c in ref[:-1]]
    floor_abs = (1e-8 if storage == F64 else 1e-6) * _scale(objs, w)
    for k, (g, e) in enumerate(zip(got_b, ref_b), start=1):
        s = spec[k]
        # the rule's own threshold; the oracle has cutoff * s_0 (or 1e-10 s_0) and no absolute floor
        thr = max(cutoff * s[0], floor_abs)
        if g < e:  # values the oracle keeps and the rule drops: at or below its threshold, up to a near-tie
            assert np.all(s[g:e] <= (1 + 1e-3) * thr), (k, g, e, s[g:e], thr)
        elif g > e:  # values kept above the oracle's cutoff: only a near-tie at that cutoff (never under max_bond alone)
            assert cutoff > 0 and np.all(np.abs(s[e:g] - cutoff * s[0]) <= 1e-3 * cutoff * s[0]), (k, g, e)
        m = min(g, e)
        np.testing.assert_allclose(r.sweep_spectra[k][:m], spec[k][:m], rtol=0, atol=1e-5 * spec[k][0])
    err = np.linalg.norm(_site_dense(r) - S)
    ref_err = np.linalg.norm(mps_to_dense(ref) - S)
    assert err <= (1 + 1e-3) * ref_err + _tol(storage) * _scale(objs, w)
    # what was measured, for callers that add bars of their own (tests/test_gpu_lincomb_scale.py)
    return dict(S=S, spec=spec, ref_bonds=ref_b, err=err, ref_err=ref_err, slack=_tol(storage) * _scale(objs, w))


@pytest.mark.parametrize("kw", [dict(cutoff=1e-3), dict(cutoff=1e-2), dict(max_bond=4), dict(max_bond=12)],
                         ids=["c1e-3", "c1e-2", "b4", "b12"])
@pytest.mark.parametrize("storage", STORAGES, ids=ST_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tt_svd_parity(shape, storage, kw):
    objs = [_make(shape, v, storage, seed=s) for s, v in zip((7, 8, 9), ("max_bond", "compress", "left"))]
    w = [0.5, 1.5, -1.0]
    r = NDMPS.linear_combination(objs, w, **kw)
    _check_tt_svd(r, objs, w, kw.get("cutoff", 0.0), kw.get("max_bond"), storage)


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_recompress_is_from_tensor_truncation(shape, storage):
    x = synthetic_mri(shape, seed=5).astype(np.float64)
    dt = F64 if storage == F64 else None
    exact = NDMPS.from_tensor(x, device=DEV, dtype=dt)
    for chi in (4, 12):
        r = exact.recompress(max_bond=chi)
        ft = NDMPS.from_tensor(x, max_bond=chi, device=DEV, dtype=dt)
        assert r.bond_sizes() == ft.bond_sizes()
        e_r = np.linalg.norm(np.asarray(r.to_tensor(), np.float64) - x)
        e_f = np.linalg.norm(np.asarray(ft.to_tensor(), np.float64) - x)
        assert e_r <= (1 + 1e-3) * e_f + _tol(storage) * np.linalg.norm(x)
        again = r.recompress()
        assert again.bond_sizes() == r.bond_sizes()
        d = np.linalg.norm(np.asarray(again.to_tensor(), np.float64) - np.asarray(r.to_tensor(), np.float64))
        assert d <= 1e-5 * np.linalg.norm(x)


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_gauge(storage):
    objs = [_make((30, 45, 20), v, storage, seed=s) for s, v in zip((1, 2), ("max_bond", "compress"))]
    r = NDMPS.linear_combination(objs, [1.0, -0.5])
    tol = 2e-9 if storage == F64 else 1e-5
    for c in r.mps.cores[1:]:
        m = c.to(F64).reshape(c.shape[0], -1)
        assert (m @ m.T - torch.eye(m.shape[0], dtype=F64, device=m.device)).abs().max().item() <= tol
    site0 = torch.linalg.norm(r.mps.cores[0].to(F64)).item()
    assert abs(float(r.norm_value) - site0) <= 1e-5 * site0


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_cancellation_and_duplication(storage):
    a = _make((64, 64, 64), "compress", storage, seed=3)
    z = a - a
    scale = 2 * float(a.norm_value)
    if storage == F32:
        assert z.bond_sizes() == [1] * len(a.bond_sizes())
        assert not np.asarray(z.to_tensor()).any()
    else:
        assert float(z.norm_value) <= 10 * 1e-8 * scale
    two = a + a
    assert two.bond_sizes() == a.bond_sizes()
    assert np.linalg.norm(np.asarray(two.to_tensor(), np.float64) - 2 * _dense(a)) <= _tol(storage) * scale


def _assert_zero_mps(z, L):
    assert z.bond_sizes() == [1] * (L - 1)
    assert all(torch.isfinite(c).all().item() and not c.any().item() for c in z.mps.cores)
    assert float(z.norm_value) == 0.0
    assert [s.tolist() for s in z.sweep_spectra[1:]] == [[0.0]] * (L - 1)
    assert not np.asarray(z.to_tensor()).any()


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_zero_scale_gives_the_zero_mps(storage):
    """scale = sum |w_a| norm_value_a = 0 (zero weights, or zero inputs): the zero MPS, finite, every bond 1."""
    a = _make((30, 45, 20), "max_bond", storage, seed=1)
    b = _make((30, 45, 20), "compress", storage, seed=2)
    L = a.mps.L
    _assert_zero_mps(NDMPS.linear_combination([a, b], [0.0, 0.0]), L)
    _assert_zero_mps(0 * a + 0.0 * b, L)
    z = a - a if storage == F32 else NDMPS.linear_combination([a, b], [0.0, 0.0])
    _assert_zero_mps(z.recompress(), L)
    _assert_zero_mps(z + z, L)
    r = NDMPS.linear_combination([a, z], [1.0, 3.0])  # a zero input next to a live one
    assert r.bond_sizes() == a.bond_sizes()
    assert np.linalg.norm(np.asarray(r.to_tensor(), np.float64) - _dense(a)) <= _tol(storage) * float(a.norm_value)


def test_storage_types():
    a32 = _make((30, 45, 20), "max_bond", F32, seed=1)
    b16 = _make((30, 45, 20), "max_bond", BF16, seed=2)
    c64 = _make((30, 45, 20), "max_bond", F64, seed=3)
    assert NDMPS.linear_combination([a32, b16], [1.0, 1.0]).mps.dtype == F32
    assert NDMPS.linear_combination([a32, c64], [1.0, 1.0]).mps.dtype == F64
    assert NDMPS.linear_combination([b16, c64], [1.0, 1.0]).mps.dtype == F64
    r = NDMPS.linear_combination([a32, b16], [1.0, 1.0], dtype=BF16)
    assert all(c.dtype == BF16 for c in r.mps.cores)


@pytest.mark.parametrize("mode", ["Std", "DCT"])
def test_downstream_paths(mode):
    objs = [_make((64, 64, 64), v, F32, mode, seed=s) for s, v in zip((1, 2), ("max_bond", "compress"))]
    r = NDMPS.linear_combination(objs, [1.0, 0.5])
    full = np.asarray(r.to_tensor(), np.float64)
    key = (slice(8, 40), slice(0, 64, 3), 17)
    region = np.asarray(r.decode_region(key), np.float64)
    np.testing.assert_allclose(region, full[8:40, 0:64:3, 17], rtol=0, atol=1e-5 * np.abs(full).max())
    coarse = np.asarray(r.downsample(1), np.float64)
    bs = r.block_shape(1)
    want = full.reshape(full.shape[0] // bs[0], bs[0], full.shape[1] // bs[1], bs[1],
                        full.shape[2] // bs[2], bs[2]).mean(axis=(1, 3, 5))
    np.testing.assert_allclose(coarse, want, rtol=0, atol=1e-5 * np.abs(full).max())
    back = codec.loads(codec.dumps(r, dtype=np.float32), device=DEV)
    assert back.bond_sizes() == r.bond_sizes()
    a = objs[0]
    da = np.asarray(a.to_tensor(), np.float64)
    dot = float(np.sum(full * da)) / (np.linalg.norm(full) * np.linalg.norm(da))
    assert abs(compute_overlap(r, a) - dot) <= 1e-5


def test_operators():
    a = _make((30, 45, 20), "max_bond", F32, seed=1)
    b = _make((30, 45, 20), "compress", F32, seed=2)
    da, db = _dense(a), _dense(b)
    scale = float(a.norm_value) + float(b.norm_value)
    for got, want in [(a + b, da + db), (a - b, da - db), (-a, -da), (2.5 * a, 2.5 * da), (a * -3.0, -3.0 * da),
                      (a / 4.0, da / 4.0)]:
        assert np.linalg.norm(np.asarray(got.to_tensor(), np.float64) - want) <= 1e-5 * 4 * scale
    for s in (-a, 2.5 * a, a * -3.0, a / 4.0):
        assert s.bond_sizes() == a.bond_sizes()
    assert abs(float((2.5 * a).norm_value) - 2.5 * float(a.norm_value)) <= 1e-6 * float(a.norm_value)
    with pytest.raises(TypeError):
        a + 1.0
    with pytest.raises(TypeError):
        a * "x"
    with pytest.raises(TypeError):
        a * b


def test_errors():
    a = _make((30, 45, 20), "max_bond", F32, seed=1)
    with pytest.raises(ValueError):
        NDMPS.linear_combination([], [])
    with pytest.raises(ValueError):
        NDMPS.linear_combination([a, a], [1.0])
    with pytest.raises(ValueError):
        NDMPS.linear_combination([a], [float("nan")])
    with pytest.raises(ValueError):
        NDMPS.linear_combination([a], [1.0], cutoff=-1.0)
    with pytest.raises(ValueError):
        NDMPS.linear_combination([a], [1.0], max_bond=0)
    with pytest.raises(ValueError, match="shape"):
        NDMPS.linear_combination([a, _make((64, 64, 64), "max_bond", F32)], [1.0, 1.0])
    with pytest.raises(ValueError, match="mode"):
        NDMPS.linear_combination([a, _make((30, 45, 20), "max_bond", F32, "DCT")], [1.0, 1.0])
    with pytest.raises(ValueError, match="qubit_size"):
        c = _make((30, 45, 20), "max_bond", F32)
        c.qubit_size = np.asarray(c.qubit_size) * 2
        NDMPS.linear_combination([a, c], [1.0, 1.0])
    big = NDMPS.from_tensor(np.random.default_rng(0).standard_normal((64, 64, 64)).astype(np.float32), device=DEV)
    assert max(big.bond_sizes()) * 9 > 4096
    with pytest.raises(ValueError, match="recompress"):
        NDMPS.linear_combination([big] * 9, [1.0] * 9)


def test_memory_below_one_volume():
    objs = [NDMPS.from_tensor(synthetic_mri((256, 256, 256), seed=s), max_bond=32, device=DEV) for s in range(4)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = NDMPS.linear_combination(objs, [0.25] * 4)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20
    assert max(r.bond_sizes()) <= 128
