"""NDMPS.downsample / NDMPS.sum / NDMPS.mean on the MI355X (csrc/pool.hip, planner core/pool.py).

Reference: the object's own ``to_tensor()`` reshaped to ``(n0 / B0, B0, ...)`` and reduced over the block axes in
fp64 on the host.  Bars, and where they come from:

* Relative Frobenius error 1e-5 for fp32 cores and bf16 cores (which are widened to fp32 and contracted in fp32),
  1e-11 for fp64 cores, on the synthetic-MRI volumes.  Both sides contract a chain whose voxel errors are a few
  units of rounding of the storage type relative to the volume's scale (to_tensor: about 5e-7 relative in fp32, see
  tests/test_gpu_region.py, and about 1e-15 in fp64).  A block mean averages those errors and the site reduction
  adds a sum in fp64, so the reduced volumes differ by at most the same few units: 1e-5 leaves a factor of about
  20 over fp32 and 1e-11 four orders over fp64.  The volumes are nonnegative, so no reduction cancels and the
  Frobenius norm of the result is of the order of that of the volume's blocks.
* Signed volumes can cancel in a sum, so there the bar is per element: ``|got - want| <= tol * R(|to_tensor()|)``
  with ``R`` the same reduction, tol 1e-4 (fp32) and 1e-10 (fp64): an error of a few rounding units of every
  voxel's magnitude, summed over the block, cannot exceed the reduction of the magnitudes times those units.
* bf16 cores: ``to_tensor`` itself runs a bf16 chain, so against it the bar is BF16_TOL (tests/test_gpu_region.py);
  against ``to_tensor`` of the same cores widened to fp32 it is the fp32 bar.
* Against the oracle's reconstruction, reduced in fp64: the bars of test_gpu_region.py::test_region_matches_oracle.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.ndmps_oracle import OracleNDMPS  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
BF16_TOL = 1e-2  # tests/test_gpu_parity.py
SHAPES = [(64, 64, 64), (30, 45, 20), (512, 680), (16, 16, 8, 32)]  # tests/test_gpu_region.py
SHAPE_IDS = ["64c", "30x45x20", "512x680", "16x16x8x32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _make(shape, variant, storage, mode="Std", signed=False):
    x = synthetic_mri(shape, seed=17)
    if signed:
        x = x - np.float32(0.5) * x.max()
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
    else:
        raise AssertionError(variant)
    return obj.astype(BF16) if storage == BF16 else obj


def _reduce(vol, blocks, op):
    vol = np.asarray(vol, dtype=np.float64)
    inter = [v for n, b in zip(vol.shape, blocks) for v in (n // b, b)]
    r = vol.reshape(inter)
    odd = tuple(range(1, 2 * vol.ndim, 2))
    return r.mean(axis=odd) if op == "mean" else r.sum(axis=odd)


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300)


def _levels(shape, L):
    nd = len(shape)
    cases = [k for k in range(L + 1)]
    cases.append([min(L, 1 + a % 3) for a in range(nd)])
    cases.append([L] + [0] * (nd - 2) + [1])
    return cases


def _axes(nd):
    return [None, 0, -1, (0, nd - 1), tuple(range(1, nd))]


def _check_own(obj, shape, tol=None):
    """downsample / sum / mean against the object's own to_tensor, reduced in fp64."""
    tol = tol or (1e-11 if obj.mps.dtype == F64 else 1e-5)
    full = obj.to_tensor()
    wide = obj.astype(F32).to_tensor() if obj.mps.dtype == BF16 else full
    want_dtype = np.float64 if obj.mps.dtype == F64 else np.float32
    L = len(obj.mps.dims)
    for lev in _levels(shape, L):
        B = obj.block_shape(lev)
        for op in ("mean", "sum"):
            got = obj.downsample(lev, op=op)
            assert isinstance(got, np.ndarray) and got.dtype == want_dtype, (lev, op)
            assert got.shape == tuple(n // b for n, b in zip(shape, B)), (lev, got.shape)
            assert _rel(got, _reduce(wide, B, op)) <= tol, (lev, op, _rel(got, _reduce(wide, B, op)))
            if obj.mps.dtype == BF16:
                assert _rel(got, _reduce(full, B, op)) <= BF16_TOL, (lev, op)
    np.testing.assert_allclose(obj.downsample(0), wide, rtol=0, atol=tol * 10 * np.abs(wide).max())
    assert obj.downsample(L).shape == (1,) * len(shape)
    for axis in _axes(len(shape)):
        for keep in (False, True):
            for op in ("sum", "mean"):
                got = getattr(obj, op)(axis=axis, keepdims=keep)
                want = getattr(np.asarray(wide, dtype=np.float64), op)(axis=axis, keepdims=keep)
                assert np.shape(got) == np.shape(want), (axis, keep, op)
                assert _rel(got, want) <= tol, (axis, keep, op, _rel(got, want))
    s = obj.mean()
    assert isinstance(s, (np.floating,)) and np.ndim(s) == 0


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("variant", ["exact", "max_bond", "compress", "left"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_downsample_matches_own_to_tensor(shape, variant, storage):
    _check_own(_make(shape, variant, storage), shape)


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("variant", ["exact", "max_bond", "compress", "left"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_downsample_dct_mode_matches_own_to_tensor(shape, variant, storage):
    _check_own(_make(shape, variant, storage, mode="DCT"), shape)


def test_downsample_after_replace_tensordata():
    shape = (30, 45, 20)
    obj = _make(shape, "max_bond", F32)
    rng = np.random.default_rng(3)
    obj.replace_tensordata([np.abs(np.asarray(a)) * (1 + 0.1 * rng.random(a.shape)) for a in obj.mps.arrays])
    _check_own(obj, shape)


@pytest.mark.parametrize("mode", ["Std", "DCT"])
@pytest.mark.parametrize("storage,tol", [(F32, 1e-4), (F64, 1e-10)], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(30, 45, 20), (16, 16, 8, 32)], ids=["30x45x20", "16x16x8x32"])
def test_signed_volume_per_element(shape, storage, tol, mode):
    obj = _make(shape, "max_bond", storage, mode=mode, signed=True)
    full = np.asarray(obj.to_tensor(), dtype=np.float64)
    L = len(obj.mps.dims)
    for lev in _levels(shape, L):
        B = obj.block_shape(lev)
        for op in ("mean", "sum"):
            got = obj.downsample(lev, op=op)
            bound = tol * _reduce(np.abs(full), B, op)
            assert np.all(np.abs(got - _reduce(full, B, op)) <= bound), (lev, op)
    for axis in _axes(len(shape)):
        got = obj.sum(axis=axis, keepdims=True)
        assert np.all(np.abs(got - full.sum(axis=axis, keepdims=True)) <= tol * np.abs(full).sum(axis=axis, keepdims=True))


@pytest.mark.parametrize("storage,tol", [(F32, 5e-5), (F64, 1e-9), (BF16, BF16_TOL)], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_downsample_matches_oracle(shape, storage, tol):
    x = synthetic_mri(shape, seed=23)
    if storage == BF16:
        x = torch.from_numpy(x).to(BF16).float().numpy()  # the oracle sees the same bf16-rounded values
    obj = NDMPS.from_tensor(x, max_bond=8, device=DEV, dtype=F64 if storage == F64 else None)
    if storage == BF16:
        obj = obj.astype(BF16)
    rr = OracleNDMPS.from_tensor(x.astype(np.float64), max_bond=8).to_tensor()
    L = len(obj.mps.dims)
    for lev in _levels(shape, L):
        for op in ("mean", "sum"):
            assert _rel(obj.downsample(lev, op=op), _reduce(rr, obj.block_shape(lev), op)) <= tol, (lev, op)
    assert _rel(obj.mean(axis=0), rr.mean(axis=0)) <= tol
    assert _rel(obj.sum(), rr.sum()) <= tol


def test_wide_exact_sweep_collapse():
    """Exact sweep of 64^3: the middle bond is 512, so mean() collapses a 64 x 8 x 512 and a 512 x 8 x 64 site."""
    shape = (64, 64, 64)
    for storage in (F32, F64):
        obj = _make(shape, "exact", storage)
        assert max(obj.bond_sizes()) >= 512
        full = np.asarray(obj.to_tensor(), dtype=np.float64)
        tol = 1e-11 if storage == F64 else 1e-5
        assert _rel(obj.mean(), full.mean()) <= tol
        assert _rel(obj.sum(axis=(1, 2)), full.sum(axis=(1, 2))) <= tol
        assert _rel(obj.downsample([2, 6, 0]), _reduce(full, obj.block_shape([2, 6, 0]), "mean")) <= tol


def test_result_types():
    shape = (30, 45, 20)
    for storage, np_dt, t_dt in ((F32, np.float32, F32), (F64, np.float64, F64), (BF16, np.float32, BF16)):
        obj = _make(shape, "max_bond", storage)
        assert obj.downsample(1).dtype == np_dt and obj.sum(axis=1).dtype == np_dt
        t = obj.downsample(1, as_torch=True)
        assert t.is_cuda and t.dtype == t_dt and tuple(t.shape) == (6, 15, 4)
        assert obj.downsample(1, as_torch=True, dtype=torch.float16).dtype == torch.float16
        s = obj.mean(as_torch=True)
        assert s.is_cuda and s.dim() == 0
        assert isinstance(obj.sum(), np_dt)
        assert obj.mean(axis=(0, 2), keepdims=True).shape == (1, 45, 1)
    dct = _make(shape, "max_bond", BF16, mode="DCT")
    assert dct.downsample(1, as_torch=True).dtype == F32  # as decode_region: bf16 only for Std mode


def test_downsample_errors():
    shape = (30, 45, 20)
    obj = _make(shape, "max_bond", F32)
    L = len(obj.mps.dims)
    for bad in (1.5, "1", True, [1, 1, 1.0], [False, 0, 0], None):
        with pytest.raises(TypeError):
            obj.downsample(bad)
    for bad in (-1, L + 1, [1, 1], [0, 0, 0, 0], [0, L + 1, 0]):
        with pytest.raises(ValueError):
            obj.downsample(bad)
    with pytest.raises(ValueError):
        obj.downsample(1, op="max")
    with pytest.raises(TypeError):
        obj.block_shape(2.0)
    for bad in (1.0, True, (0, "1")):
        with pytest.raises(TypeError):
            obj.sum(axis=bad)
    for bad in (3, -4, (0, 5)):
        with pytest.raises(np.exceptions.AxisError):
            obj.mean(axis=bad)
    with pytest.raises(ValueError):
        obj.sum(axis=(0, -3))
    bare = NDMPS(obj.mps, obj.qubit_size, None, None, obj.norm, None, obj.mode, obj.dim)
    for call in (lambda: bare.downsample(1), lambda: bare.sum(), lambda: bare.mean(axis=0), lambda: bare.block_shape(1)):
        with pytest.raises(ValueError, match="the tensor shape is unknown"):
            call()
    obj.mode = "Other"
    assert obj.to_tensor() is None and obj.downsample(1) is None and obj.sum() is None and obj.mean(axis=0) is None


def test_lockstep_group_objects():
    shape = (16, 16, 8, 32)
    xs = [synthetic_mri(shape, seed=s) for s in (1, 2, 3)]
    objs = NDMPS.from_tensors(xs, max_bond=16, device=DEV)
    for o in objs:
        full = o.to_tensor()
        assert _rel(o.downsample(1), _reduce(full, o.block_shape(1), "mean")) <= 1e-5
        assert _rel(o.mean(axis=-1), full.astype(np.float64).mean(axis=-1)) <= 1e-5


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def test_memory_scales_with_the_coarse_volume():
    """256^3, chi = 64, fp32: downsample(1) writes 8 MiB of the volume's 64 and must raise the allocator's peak by
    less than a quarter of to_tensor's raise; mean() by less than 1 MiB."""
    shape = (256, 256, 256)
    obj = NDMPS.from_tensor(synthetic_mri(shape, seed=31), max_bond=64, device=DEV)
    full = obj.to_tensor(as_torch=True)
    ref1 = full.double().reshape(128, 2, 128, 2, 128, 2).mean(dim=(1, 3, 5))
    ref0 = float(full.double().mean())
    del full
    obj.downsample(1, as_torch=True)  # plans and tables of the coarse chain are cached from here on
    obj.mean(as_torch=True)
    got1, down_peak = _peak(lambda: obj.downsample(1, as_torch=True))
    got0, mean_peak = _peak(lambda: obj.mean(as_torch=True))
    _, full_peak = _peak(lambda: obj.to_tensor(as_torch=True))
    print(f"256^3 chi=64: downsample(1) peak {down_peak / 2**20:.2f} MiB, mean() peak {mean_peak / 2**20:.3f} MiB, "
          f"to_tensor peak {full_peak / 2**20:.2f} MiB")
    assert full_peak >= 64 * 2**20
    assert down_peak < full_peak / 4
    assert mean_peak < 2**20
    assert float((got1.double() - ref1).norm() / ref1.norm()) <= 1e-5
    assert abs(float(got0) - ref0) <= 1e-5 * abs(ref0)


def test_dct_mean_never_decodes_the_last_axis():
    shape = (256, 256, 256)
    obj = NDMPS.from_tensor(synthetic_mri(shape, seed=37), mode="DCT", max_bond=64, device=DEV)
    ref = float(obj.to_tensor(as_torch=True).double().mean())
    obj.mean(as_torch=True)
    got, peak = _peak(lambda: obj.mean(as_torch=True))
    print(f"256^3 chi=64 DCT: mean() peak {peak / 2**20:.3f} MiB")
    assert peak < 2**20
    assert abs(float(got) - ref) <= 1e-5 * abs(ref)
