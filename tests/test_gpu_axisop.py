"""NDMPS.roll / shift / correlate1d / cumsum / flip on the MI355X (csrc/axisop.hip, core/axisop.py).

Bars, and where they come from:

* Kernel: ``oncore.axis_apply`` (the unrounded wide chain) against ``core.axisop.emulate`` in fp64 on the same cores.  roll,
  shift and flip have at most one term per output, so the device must return ``emulate``'s values exactly, absent
  entries as exact zeros.  Stencils and cumsum: per element ``(t + 1) u sum |M| |X|``, the standard bound of a sum of
  ``t`` products rounded once more into the work type (u = 2**-24 for fp32 work, 2**-53 for fp64; t = the largest
  number of non-zero entries of ``M_k`` along the summed digit).
* End to end: ``|op(obj).to_tensor() - numpy_op(obj.to_tensor())| <= tol * opnorm * norm_value`` (Frobenius), tol from
  tests/test_gpu_lincomb.py (1e-5 for fp32 / bf16 work, 1e-7 for fp64): the rounding drops directions below the
  storage floor ``1e-6 * opnorm * norm_value`` (1e-8 for fp64).
* ``max_bond``: the error against the exact operator result is at most ``(1 + 1e-3)`` times that of
  ``from_tensor(numpy_op(dense), max_bond)`` plus ``tol * scale``, the bar of ``recompress`` in test_gpu_lincomb.py.
* Memory: ``roll`` of a 256^3 object at chi = 64 raises the allocator peak by less than one decoded fp32 volume.
  Its cores are Gaussian with the bond weights 2**-b: with flat weights the rolled volume has the true bond 128 (the
  voxels that wrap span a second column space of the same weight), which no chain of bond 64 represents; graded weights
  put the 65th value of the rolled volume at 2**-32, below the storage floor, as a compressed image does.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import axisop as ax  # noqa: E402
from imgcompressionmps_amd.core import oncore  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.utils import core as _core  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

import sweep_cases as sc  # noqa: E402  (tests/ is on the path: rootdir conftest)

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
STORAGES = [F32, BF16, F64]
ST_IDS = ["f32", "bf16", "f64"]
KERNEL_SHAPES = [((12, 8, 18), 5), ((16, 16), 5), ((6, 20, 9, 4), 5), ((64, 64, 64), 16)]
KERNEL_IDS = ["12x8x18", "16x16", "6x20x9x4", "64c"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _tol(storage):
    return 1e-7 if storage == F64 else 1e-5


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


def _shift_zero(x, s, axis):
    out = np.zeros_like(x)
    n = x.shape[axis]
    src, dst = [slice(None)] * x.ndim, [slice(None)] * x.ndim
    if s >= 0:
        src[axis], dst[axis] = slice(0, n - s), slice(s, n)
    else:
        src[axis], dst[axis] = slice(-s, n), slice(0, n + s)
    out[tuple(dst)] = x[tuple(src)]
    return out


def _correlate(x, w, axis, mode, origin=0):
    """out[i] = sum_j w[j] x[i + j - len(w) // 2 - origin], zero or periodic outside (scipy.ndimage.correlate1d)."""
    out = np.zeros_like(x)
    for j, wj in enumerate(w):
        s = len(w) // 2 + origin - j
        out += wj * (np.roll(x, s, axis) if mode == "wrap" else _shift_zero(x, s, axis))
    return out


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("storage", STORAGES, ids=ST_IDS)
@pytest.mark.parametrize("shape,chi", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_kernel_against_emulate(shape, chi, storage):
    fa = _core.get_factorlist(shape)[0]
    dims = [int(d) for d in np.prod(fa, axis=1)]
    bonds = _bonds(dims, chi)
    rng = np.random.default_rng(len(shape) * 100 + chi)
    # multiples of 1/8 up to 8: exact in every storage type
    cores = [rng.integers(-64, 65, size=(bonds[k], dims[k], bonds[k + 1])).astype(np.float64) / 8 for k in range(len(dims))]
    obj = _object(cores, shape, storage)
    u = 2.0 ** -53 if storage == F64 else 2.0 ** -24
    worst = 0.0
    for axis in range(len(shape)):
        fs, n = fa[:, axis], shape[axis]
        single = [ax.roll_mpo(fs, 1), ax.roll_mpo(fs, -1), ax.roll_mpo(fs, 5), ax.roll_mpo(fs, n + 3), ax.shift_mpo(fs, 3),
                  ax.shift_mpo(fs, -2), ax.flip_mpo(fs)]
        for mpo in single:
            got = oncore.axis_apply(obj.mps, mpo, fa, axis)
            want = ax.emulate(cores, mpo, fa, axis)
            assert got.bonds == [d * b for d, b in zip(mpo.bonds, bonds)]
            for g, w in zip(got.cores, want):
                assert g.dtype == (F64 if storage == F64 else F32) and tuple(g.shape) == w.shape
                assert np.array_equal(g.to(F64).cpu().numpy(), w)
        trng = np.random.default_rng(axis)
        several = [ax.offsets_mpo(fs, {s: float(trng.standard_normal()) for s in range(-r, r + 1)}, mode)
                   for r in (1, 2, 4) if r < n for mode in ax.MODES] + [ax.cumsum_mpo(fs)]
        for mpo in several:
            got = oncore.axis_apply(obj.mps, mpo, fa, axis)
            want = ax.emulate(cores, mpo, fa, axis)
            mag = ax.emulate([np.abs(c) for c in cores], ax.AxisMPO([np.abs(m) for m in mpo.cores], mpo.opnorm), fa, axis)
            for g, w, a, m in zip(got.cores, want, mag, mpo.cores):
                t = int(np.count_nonzero(m, axis=2).max())
                err = np.abs(g.to(F64).cpu().numpy() - w)
                bound = (t + 1) * u * a
                assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
                assert not np.any(g.to(F64).cpu().numpy()[a == 0])  # absent entries are exact zeros
                worst = max(worst, float((err[a > 0] / bound[a > 0]).max()))
    print(f"\n[axisop] largest error / bound, {shape} {storage}: {worst:.3e}", end="")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("mode", ["Std", "DCT"])
@pytest.mark.parametrize("storage", STORAGES, ids=ST_IDS)
@pytest.mark.parametrize("shape", [(30, 45, 20), (64, 64, 64)], ids=["30x45x20", "64c"])
def test_end_to_end(shape, storage, mode):
    x = synthetic_mri(shape, seed=11)
    obj = NDMPS.from_tensor(x, mode=mode, max_bond=12, device=DEV, dtype=F64 if storage == F64 else None)
    assert max(obj.bond_sizes()) == 12  # the cap binds
    if storage == BF16:
        obj = obj.astype(BF16)
    dense = _dense(obj)
    nv, tol = float(obj.norm_value), _tol(storage)
    w3, w4 = [0.25, 0.5, 0.25], [-1.0, 3.0, -3.0, 1.0]
    for axis in range(len(shape) - (1 if mode == "DCT" else 0)):
        n = shape[axis]
        cases = [
            (obj.roll(7, axis), np.roll(dense, 7, axis), 1.0),
            (obj.roll(-1, axis), np.roll(dense, -1, axis), 1.0),
            (obj.shift(-3, axis), _shift_zero(dense, -3, axis), 1.0),
            (obj.correlate1d(w3, axis), _correlate(dense, w3, axis, "constant"), 1.0),
            (obj.correlate1d(w4, axis, mode="wrap", origin=-1), _correlate(dense, w4, axis, "wrap", -1), 8.0),
            (obj.cumsum(axis), np.cumsum(dense, axis), float(n)),
            (obj.flip(axis), np.flip(dense, axis), 1.0),
        ]
        for j, (r, want, opnorm) in enumerate(cases):
            got = _dense(r)  # flip keeps bf16 storage: widened first, like the input
            assert np.linalg.norm(got - want) <= tol * opnorm * nv, (axis, j, np.linalg.norm(got - want) / (opnorm * nv))
            assert r.mode == mode and r._shape == obj._shape
        r = cases[0][0]
        assert r.norm is False and r.mps.dtype == (F64 if storage == F64 else F32)
        assert r.sweep_spectra[0] is None and [len(s) for s in r.sweep_spectra[1:]] == r.bond_sizes()
        assert abs(float(r.norm_value) - nv) <= tol * nv
        assert cases[-1][0].mps.dtype == obj.mps.dtype and cases[-1][0].bond_sizes() == obj.bond_sizes()
    tup = obj.roll((3, -2), (0, 1))
    assert np.linalg.norm(np.asarray(tup.to_tensor(), np.float64) - np.roll(dense, (3, -2), (0, 1))) <= 2 * tol * nv
    if mode == "DCT":
        for call in (lambda: obj.roll(1, -1), lambda: obj.shift(1, len(shape) - 1), lambda: obj.cumsum(-1),
                     lambda: obj.flip(-1), lambda: obj.correlate1d(w3), lambda: obj.roll((1, 1), (0, -1))):
            with pytest.raises(ValueError, match="DCT"):
                call()


def test_dtype_argument_and_errors():
    x = synthetic_mri((30, 45, 20), seed=3)
    obj = NDMPS.from_tensor(x, max_bond=8, device=DEV)
    assert obj.roll(1, 0, dtype=BF16).mps.dtype == BF16
    assert obj.roll(1, 0, dtype=F64).mps.dtype == F64
    assert obj.cumsum(1, dtype=F32).mps.dtype == F32
    with pytest.raises(TypeError):
        obj.roll(1.5, 0)
    with pytest.raises(TypeError):
        obj.roll(1, None)
    with pytest.raises(TypeError):
        obj.shift(True, 0)
    with pytest.raises(ValueError):
        obj.roll(1, 3)
    with pytest.raises(ValueError):
        obj.roll((1, 2, 3), (0, 1))
    with pytest.raises(ValueError):
        obj.roll(1, 0, cutoff=-1.0)
    with pytest.raises(ValueError):
        obj.roll(1, 0, max_bond=0)
    with pytest.raises(ValueError):
        obj.roll(1, 0, dtype=torch.float16)
    with pytest.raises(ValueError):
        obj.correlate1d([], 0)
    with pytest.raises(ValueError):
        obj.correlate1d([1.0, float("nan")], 0)
    with pytest.raises(ValueError):
        obj.correlate1d([[1.0]], 0)
    with pytest.raises(ValueError):
        obj.correlate1d([1.0, 1.0, 1.0], 0, mode="reflect")
    with pytest.raises(ValueError, match="radius"):
        obj.correlate1d(np.ones(41), 2)  # radius 20 on the axis of 20


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("case,member", [("rank_eq_cap", 0), ("mixed3d", 1)])
def test_roll_and_back_keeps_the_planted_ranks(case, member, storage):
    x = sc.volumes(case)[member]
    planted = sc.CASES[case]["members"][member]["ranks"]
    obj = NDMPS.from_tensor(x, device=DEV, dtype=F64 if storage == F64 else None)
    assert obj.bond_sizes() == planted
    dims = obj.mps.dims
    caps = [int(min(np.prod(dims[:k]), np.prod(dims[k:]))) for k in range(1, len(dims))]
    nv = float(obj.norm_value)
    for axis in range(x.ndim):
        for s in (3, -1):
            there = obj.roll(s, axis)
            assert all(b <= min(2 * c, cap) for b, c, cap in zip(there.bond_sizes(), obj.bond_sizes(), caps))
            rolled = np.asarray(there.to_tensor(), np.float64)
            assert np.linalg.norm(rolled - np.roll(x, s, axis)) <= _tol(storage) * nv
            back = there.roll(-s, axis)
            assert back.bond_sizes() == planted, (axis, s, back.bond_sizes())
            assert np.linalg.norm(np.asarray(back.to_tensor(), np.float64) - x) <= _tol(storage) * nv


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_max_bond(storage):
    x = synthetic_mri((64, 64, 64), seed=5)
    dt = F64 if storage == F64 else None
    obj = NDMPS.from_tensor(x, max_bond=16, device=DEV, dtype=dt)
    dense = _dense(obj)
    scale = float(obj.norm_value)
    for axis, s, chi in ((0, 1, 8), (1, 5, 8), (2, -9, 4)):
        r = obj.roll(s, axis, max_bond=chi)
        assert max(r.bond_sizes()) <= chi
        want = np.roll(dense, s, axis)
        ft = NDMPS.from_tensor(want if storage == F64 else want.astype(np.float32), max_bond=chi, device=DEV, dtype=dt)
        e_r = np.linalg.norm(np.asarray(r.to_tensor(), np.float64) - want)
        e_f = np.linalg.norm(np.asarray(ft.to_tensor(), np.float64) - want)
        assert e_r <= (1 + 1e-3) * e_f + _tol(storage) * scale, (axis, e_r, e_f)
    w = [1.0, -2.0, 1.0]
    r = obj.correlate1d(w, 1, max_bond=8)
    assert max(r.bond_sizes()) <= 8
    want = _correlate(dense, w, 1, "constant")
    ft = NDMPS.from_tensor(want if storage == F64 else want.astype(np.float32), max_bond=8, device=DEV, dtype=dt)
    e_r = np.linalg.norm(np.asarray(r.to_tensor(), np.float64) - want)
    e_f = np.linalg.norm(np.asarray(ft.to_tensor(), np.float64) - want)
    assert e_r <= (1 + 1e-3) * e_f + _tol(storage) * 4.0 * scale, (e_r, e_f)


# ------------------------------------------------------------------------------------------------ zero and edge cases
@pytest.mark.parametrize("storage", STORAGES, ids=ST_IDS)
def test_zero_and_edge_cases(storage):
    shape = (30, 45, 20)
    obj = NDMPS.from_tensor(synthetic_mri(shape, seed=2), max_bond=10, device=DEV, dtype=F64 if storage == F64 else None)
    if storage == BF16:
        obj = obj.astype(BF16)
    dense, nv, L = _dense(obj), float(obj.norm_value), obj.mps.L
    for axis, n in enumerate(shape):
        for s in (n, -n, n + 4):
            z = obj.shift(s, axis)
            assert z.bond_sizes() == [1] * (L - 1)
            assert all(torch.isfinite(c).all().item() and not c.any().item() for c in z.mps.cores)
            assert float(z.norm_value) == 0.0
            assert [v.tolist() for v in z.sweep_spectra[1:]] == [[0.0]] * (L - 1)
            assert not np.asarray(z.to_tensor()).any()
        last = obj.shift(n - 1, axis)  # one plane survives
        assert np.linalg.norm(np.asarray(last.to_tensor(), np.float64) - _shift_zero(dense, n - 1, axis)) <= _tol(storage) * nv
        same = obj.roll(0, axis)
        assert np.linalg.norm(np.asarray(same.to_tensor(), np.float64) - dense) <= _tol(storage) * nv
        assert np.linalg.norm(np.asarray(obj.roll(n, axis).to_tensor(), np.float64) - dense) <= _tol(storage) * nv
        twice = obj.flip(axis).flip(axis)
        assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(twice.mps.cores, obj.mps.cores))
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(twice.mps.cores, obj.mps.cores))
        assert float(twice.norm_value) == nv and np.array_equal(twice.boundary_list, obj.boundary_list)


# ------------------------------------------------------------------------------------------------ no volume is formed
def test_roll_of_256_cubed_forms_no_volume():
    shape = (256, 256, 256)
    dims = [int(d) for d in _core.site_dims(shape)]
    bonds = _bonds(dims, 64)
    rng = np.random.default_rng(256)
    cores = [rng.standard_normal((bonds[k], dims[k], bonds[k + 1])) * (0.5 ** np.arange(bonds[k + 1]))[None, None, :]
             for k in range(len(dims))]
    obj = _object(cores, shape, F32)
    assert max(obj.bond_sizes()) == 64
    pts = np.stack([rng.integers(0, 256, size=1000) for _ in range(3)], axis=1)
    back = pts.copy()
    back[:, 0] = (back[:, 0] - 1) % 256
    want = np.asarray(obj.values_at(back), np.float64)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = obj.roll(1, 0, max_bond=64)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 64 << 20, peak
    assert max(r.bond_sizes()) <= 64
    got = np.asarray(r.values_at(pts), np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
