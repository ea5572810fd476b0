"""NDMPS.decode_region / NDMPS.values_at on the MI355X (csrc/region.hip, planner core/region.py).

Against the object's own ``to_tensor()`` indexed with np.ix_ (same dtype and shape, relative Frobenius 1e-5 for
fp32, 1e-12 for fp64 storage), and against the CPU oracle at the class-level bars of the other GPU tests.
bf16 storage is contracted in fp32 here while ``to_tensor`` runs the bf16 chain (bf16 intermediates), so bf16 is
held to 1e-5 against ``to_tensor`` of the same cores widened to fp32, and to BF16_TOL against its own ``to_tensor``.
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
SHAPES = [(64, 64, 64), (30, 45, 20), (512, 680), (16, 16, 8, 32)]
SHAPE_IDS = ["64c", "30x45x20", "512x680", "16x16x8x32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _keys(shape):
    rng = np.random.default_rng(len(shape))
    D = len(shape)
    arr = [[int(v) for v in rng.integers(0, n, 7)] + [0, 0] for n in shape]  # unsorted, with repeats
    return [
        (),
        (Ellipsis,),
        (slice(5, min(37, shape[0])),),
        (slice(None, None, 3),) * D,
        (slice(None, None, -2),) + (1,) * (D - 1),
        tuple(arr),
        tuple(-1 - i for i in range(D)),
        (Ellipsis, np.array(arr[-1])),
        (arr[0], Ellipsis, -3),
        (3, slice(2, None, 5)) + (slice(None, 4),) * (D - 2),
    ]


def _ix(a, key, shape):
    """a[np.ix_(per-axis indices)] with int axes dropped: the outer-indexing meaning of `key`."""
    key = key if isinstance(key, tuple) else (key,)
    if any(k is Ellipsis for k in key):
        i = next(j for j, k in enumerate(key) if k is Ellipsis)
        key = key[:i] + (slice(None),) * (len(shape) - len(key) + 1) + key[i + 1:]
    key = key + (slice(None),) * (len(shape) - len(key))
    idx, out_shape = [], []
    for k, n in zip(key, shape):
        if isinstance(k, (int, np.integer)):
            idx.append(np.array([k % n]))
        elif isinstance(k, slice):
            idx.append(np.arange(*k.indices(n)))
            out_shape.append(idx[-1].size)
        else:
            idx.append(np.asarray(k) % n)
            out_shape.append(idx[-1].size)
    if isinstance(a, torch.Tensor):
        t = a
        for ax, i in enumerate(idx):
            t = t.index_select(ax, torch.from_numpy(i).to(t.device))
        return t.reshape(out_shape)
    return a[np.ix_(*idx)].reshape(out_shape)


def _rel(got, ref, vol):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    rms = np.linalg.norm(np.asarray(vol, dtype=np.float64)) / np.sqrt(np.asarray(vol).size)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), rms * np.sqrt(max(ref.size, 1)))


def _make(shape, variant, storage, mode="Std"):
    x = synthetic_mri(shape, seed=17)
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


def _check_against_own(obj, shape):
    tol = 1e-12 if obj.mps.dtype == F64 else 1e-5
    full = obj.to_tensor()
    full_t = obj.to_tensor(as_torch=True)
    wide = obj.astype(F32).to_tensor() if obj.mps.dtype == BF16 else full
    for key in _keys(shape):
        ref = _ix(full, key, shape)
        got = obj.decode_region(key)
        assert np.asarray(got).dtype == ref.dtype and np.shape(got) == ref.shape, (key, np.shape(got), ref.shape)
        assert _rel(got, _ix(wide, key, shape), full) <= tol, key
        if obj.mps.dtype == BF16:
            assert _rel(got, ref, full) <= BF16_TOL, key
        got_t = obj.decode_region(key, as_torch=True)
        ref_t = _ix(full_t, key, shape)
        assert got_t.dtype == ref_t.dtype and tuple(got_t.shape) == tuple(ref_t.shape) and got_t.is_cuda, key
        t_tol = BF16_TOL if got_t.dtype == BF16 else tol  # bf16 storage, Std: a bf16 tensor like to_tensor's
        assert _rel(got_t.float().cpu().numpy() if got_t.dtype == BF16 else got_t.cpu().numpy(),
                    _ix(wide, key, shape), full) <= t_tol, key
        got_h = obj.decode_region(key, as_torch=True, dtype=torch.float16)
        assert got_h.dtype == torch.float16 and tuple(got_h.shape) == tuple(ref_t.shape)


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("variant", ["exact", "max_bond", "compress", "left"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_region_matches_own_to_tensor(shape, variant, storage):
    _check_against_own(_make(shape, variant, storage), shape)


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("variant", ["exact", "max_bond", "compress", "left"])
def test_region_dct_mode_matches_own_to_tensor(variant, storage):
    shape = (16, 16, 8, 32)
    _check_against_own(_make(shape, variant, storage, mode="DCT"), shape)


def test_region_after_replace_tensordata():
    shape = (30, 45, 20)
    obj = _make(shape, "max_bond", F32)
    obj.replace_tensordata([np.asarray(a) * (1.0 + 0.1 * i) for i, a in enumerate(obj.mps.arrays)])
    _check_against_own(obj, shape)


@pytest.mark.parametrize("storage,tol", [(F32, 5e-5), (F64, 1e-9), (BF16, BF16_TOL)], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_region_matches_oracle(shape, storage, tol):
    x = synthetic_mri(shape, seed=23)
    if storage == BF16:
        x = torch.from_numpy(x).to(BF16).float().numpy()  # the oracle sees the same bf16-rounded values
    obj = NDMPS.from_tensor(x, max_bond=8, device=DEV, dtype=F64 if storage == F64 else None)
    if storage == BF16:
        obj = obj.astype(BF16)
    ref = OracleNDMPS.from_tensor(x.astype(np.float64), max_bond=8)
    rr = ref.to_tensor()
    for key in _keys(shape):
        assert _rel(obj.decode_region(key), _ix(rr, key, shape), rr) <= tol, key


@pytest.mark.parametrize("mode", ["Std", "DCT"])
@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
def test_values_at_random_points(mode, storage):
    for shape in SHAPES:
        obj = _make(shape, "max_bond", storage, mode=mode)
        full = obj.to_tensor()
        wide = obj.astype(F32).to_tensor() if storage == BF16 else full
        rng = np.random.default_rng(5)
        coords = np.stack([rng.integers(-n, n, 500) for n in shape], axis=1)  # negative indices included
        coords[7] = coords[3]
        got = obj.values_at(coords)
        ref = full[tuple(coords.T)]
        assert got.dtype == ref.dtype and got.shape == (500,)
        assert _rel(got, wide[tuple(coords.T)], full) <= (1e-12 if storage == F64 else 1e-5), shape
        got_t = obj.values_at(coords, as_torch=True)
        assert got_t.is_cuda and got_t.shape == (500,)
        assert obj.values_at(np.zeros((0, len(shape)), dtype=np.int64)).shape == (0,)


def test_region_errors():
    shape = (30, 45, 20)
    obj = _make(shape, "max_bond", F32)
    for key in [(30,), (0, -46), (0, 0, 0, 0), ([0, 30],), (Ellipsis, 0, Ellipsis)]:
        with pytest.raises(IndexError):
            obj.decode_region(key)
    for key in [(1.0,), (True,), (np.array([True, False]),), ([0.5],), (None,), (slice(0.5, 3),)]:
        with pytest.raises(TypeError):
            obj.decode_region(key)
    with pytest.raises(IndexError):
        obj.values_at([[0, 0]])
    with pytest.raises(IndexError):
        obj.values_at([[0, 0, 20]])
    with pytest.raises(TypeError):
        obj.values_at(np.zeros((2, 3)))
    # empty selections give empty results of the right shape
    assert obj.decode_region((slice(3, 3),)).shape == (0, 45, 20)
    bare = NDMPS(obj.mps, obj.qubit_size, None, None, obj.norm, None, obj.mode, obj.dim)
    with pytest.raises(ValueError, match="the tensor shape is unknown"):
        bare.decode_region((0,))
    with pytest.raises(ValueError, match="the tensor shape is unknown"):
        bare.values_at([[0, 0, 0]])
    obj.mode = "Other"
    assert obj.to_tensor() is None and obj.decode_region((0,)) is None and obj.values_at([[0, 0, 0]]) is None


def test_axial_slice_memory_scales_with_the_slice():
    """256^3, chi = 64, fp32: one axial slice must raise the allocator's peak by less than a quarter of the
    volume's 64 MiB (to_tensor needs all of it)."""
    shape = (256, 256, 256)
    obj = NDMPS.from_tensor(synthetic_mri(shape, seed=31), max_bond=64, device=DEV)
    torch.cuda.synchronize()
    full = obj.to_tensor(as_torch=True)
    ref = full[100].clone()
    del full
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = obj.decode_region((100,), as_torch=True)
    torch.cuda.synchronize()
    region_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base_full = torch.cuda.memory_allocated()
    obj.to_tensor(as_torch=True)
    torch.cuda.synchronize()
    full_peak = torch.cuda.max_memory_allocated() - base_full
    print(f"axial slice of 256^3 chi=64: region peak {region_peak / 2**20:.2f} MiB, to_tensor peak "
          f"{full_peak / 2**20:.2f} MiB")
    assert full_peak >= 64 * 2**20
    assert region_peak < 16 * 2**20
    assert float((got - ref).norm() / ref.norm()) <= 1e-5
