"""Host planner of the axis operators (core/axisop.py), without a GPU.

Exact TT cores of a random volume (oracle.mps.mps_from_dense on the site-order tensor) go through ``emulate``, the fp64
NumPy application of the operator that the device kernel is pinned to, are contracted and compared with the NumPy
operator on the volume to 1e-12 relative (fp64 throughout).  The shapes are mixed-radix: radices 2, 3, 4 and 5, an
L = 2 chain and the reversed odd axes.
"""
import numpy as np
import pytest

from imgcompressionmps_amd.core import axisop as ax
from imgcompressionmps_amd.utils import core as _core
from oracle.mps import mps_from_dense, mps_to_dense

SHAPES = [(12, 8, 18), (16, 16), (6, 20, 9, 4)]
CASES = [(s, a) for s in SHAPES for a in range(len(s))]
CASE_IDS = ["x".join(map(str, s)) + f"-ax{a}" for s, a in CASES]
RTOL = 1e-12

_EXACT = {}


def _exact(shape):
    """(volume, its exact cores, factor array, encoding map); computed once per shape, never modified."""
    if shape not in _EXACT:
        rng = np.random.default_rng(sum(shape))
        x = rng.standard_normal(shape)
        fa = _core.get_factorlist(shape)[0]
        dims, enc = _core.gen_encoding_map(shape)
        site = np.empty([int(d) for d in dims])
        site[tuple(enc)] = x
        cores, _ = mps_from_dense(site, dims)
        assert np.linalg.norm(mps_to_dense(cores)[tuple(enc)] - x) <= RTOL * np.linalg.norm(x)
        _EXACT[shape] = (x, cores, fa, enc)
    return _EXACT[shape]


def _apply(shape, axis, mpo):
    x, cores, fa, enc = _exact(shape)
    return mps_to_dense(ax.emulate(cores, mpo, fa, axis))[tuple(enc)]


def _close(got, want, scale):
    assert np.linalg.norm(got - want) <= RTOL * scale, np.linalg.norm(got - want) / scale


def _shift_zero(x, s, axis):
    out = np.zeros_like(x)
    n = x.shape[axis]
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    if s >= 0:
        src[axis], dst[axis] = slice(0, n - s), slice(s, n)
    else:
        src[axis], dst[axis] = slice(-s, n), slice(0, n + s)
    out[tuple(dst)] = x[tuple(src)]
    return out


def _stencil(x, taps, axis, mode):
    """y[o] = sum_s taps[s] x[o - s], written out."""
    out = np.zeros_like(x)
    for s, w in taps.items():
        out += w * (np.roll(x, s, axis) if mode == "wrap" else _shift_zero(x, s, axis))
    return out


@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_roll(shape, axis):
    x, _, fa, _ = _exact(shape)
    n = shape[axis]
    for s in (1, -1, 5, n - 1, n + 3):
        mpo = ax.roll_mpo(fa[:, axis], s)
        assert max(mpo.bonds) <= 2 and mpo.bonds[0] == mpo.bonds[-1] == 1 and mpo.opnorm == 1.0
        _close(_apply(shape, axis, mpo), np.roll(x, s, axis), np.linalg.norm(x))


@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_zero_filled_shift(shape, axis):
    x, _, fa, _ = _exact(shape)
    for s in (3, -2):
        mpo = ax.shift_mpo(fa[:, axis], s)
        assert max(mpo.bonds) <= 2
        _close(_apply(shape, axis, mpo), _shift_zero(x, s, axis), np.linalg.norm(x))
    n = shape[axis]
    for s in (n, -n, n + 2):  # everything is shifted out: the zero operator
        mpo = ax.shift_mpo(fa[:, axis], s)
        assert mpo.bonds == [1] * (fa.shape[0] + 1) and not any(m.any() for m in mpo.cores)


@pytest.mark.parametrize("mode", ax.MODES)
@pytest.mark.parametrize("radius", [1, 2, 4])
@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_stencil(shape, axis, radius, mode):
    x, _, fa, _ = _exact(shape)
    fs = fa[:, axis]
    rng = np.random.default_rng(radius)
    taps = {s: float(rng.standard_normal()) for s in range(-radius, radius + 1)}
    mpo = ax.offsets_mpo(fs, taps, mode)
    opnorm = sum(abs(w) for w in taps.values())
    assert mpo.opnorm == pytest.approx(opnorm, rel=1e-15)
    L = len(fs)
    finest = 2 * -(-radius // int(fs[-1])) + 1
    assert mpo.bonds[0] == mpo.bonds[L] == 1
    assert all(b <= 3 for b in mpo.bonds[1:L - 1])
    if L > 1:
        assert mpo.bonds[L - 1] <= finest
        if mode == "wrap":
            assert mpo.bonds[L - 1] == finest
    _close(_apply(shape, axis, mpo), _stencil(x, taps, axis, mode), opnorm * np.linalg.norm(x))


@pytest.mark.parametrize("mode", ax.MODES)
@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_correlate_taps_follow_scipy(shape, axis, mode):
    ndimage = pytest.importorskip("scipy.ndimage")
    x, _, fa, _ = _exact(shape)
    for w, origin in (([1.0, -2.0, 1.0], 0), ([0.5, 0.25, -1.0, 2.0], -1), ([1.0, 2.0, 3.0, 4.0, 5.0], 1), ([3.0], 0)):
        taps = ax.correlate_taps(w, origin, shape[axis])
        want = ndimage.correlate1d(x, w, axis=axis, mode=mode, cval=0.0, origin=origin)
        got = _apply(shape, axis, ax.offsets_mpo(fa[:, axis], taps, mode))
        _close(got, want, np.abs(w).sum() * np.linalg.norm(x))


@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_cumsum(shape, axis):
    x, _, fa, _ = _exact(shape)
    mpo = ax.cumsum_mpo(fa[:, axis])
    L = fa.shape[0]
    assert mpo.bonds == [1] + [2] * (L - 1) + [1] and mpo.opnorm == float(shape[axis])
    _close(_apply(shape, axis, mpo), np.cumsum(x, axis), mpo.opnorm * np.linalg.norm(x))
    tri = np.tril(np.ones((shape[axis], shape[axis])))
    assert np.linalg.norm(tri, 2) <= mpo.opnorm


@pytest.mark.parametrize("shape,axis", CASES, ids=CASE_IDS)
def test_flip(shape, axis):
    x, _, fa, _ = _exact(shape)
    mpo = ax.flip_mpo(fa[:, axis])
    assert mpo.bonds == [1] * (fa.shape[0] + 1) and mpo.opnorm == 1.0
    _close(_apply(shape, axis, mpo), np.flip(x, axis), np.linalg.norm(x))


def test_emulate_layout_is_carry_major():
    """The widened bond index is c * chi + a on both sides, and only the axis's digit moves inside the site index."""
    shape, axis = (12, 8, 18), 1
    fa = _core.get_factorlist(shape)[0]
    rng = np.random.default_rng(1)
    dims = np.prod(fa, axis=1)
    bonds = [1, 3, 4, 1]
    cores = [rng.standard_normal((bonds[k], int(dims[k]), bonds[k + 1])) for k in range(3)]
    mpo = ax.cumsum_mpo(fa[:, axis])
    wide = ax.emulate(cores, mpo, fa, axis)
    k = 1
    m, x = mpo.cores[k], cores[k]
    pre, f, post = ax.site_split(fa, axis)[k]
    assert (pre, f, post) == (int(fa[k, 0]), int(fa[k, 1]), int(fa[k, 2])) and pre * f * post == dims[k]
    for c, a, p, o, q, c2, a2 in [(0, 2, 1, 1, 2, 1, 3), (1, 0, 0, 0, 1, 1, 0), (1, 1, fa[k, 0] - 1, f - 1, post - 1, 0, 2)]:
        want = sum(m[c, o, i, c2] * x[a, (p * f + i) * post + q, a2] for i in range(f))
        assert wide[k][c * bonds[k] + a, (p * f + o) * post + q, c2 * bonds[k + 1] + a2] == pytest.approx(want, abs=1e-14)
    assert [w.shape for w in wide] == [(1, dims[0], 6), (6, dims[1], 8), (8, dims[2], 1)]


def test_rejected_arguments():
    fs = [2, 3, 2]
    for bad in (1.5, "1", None, True, np.float64(2.0)):
        with pytest.raises(TypeError):
            ax.check_shift(bad)
        with pytest.raises(TypeError):
            ax.normalize_axis(bad, 3)
    assert ax.check_shift(np.int64(-7)) == -7
    assert [ax.normalize_axis(a, 3) for a in (0, 2, -1, -3)] == [0, 2, 2, 0]
    for bad in (3, -4):
        with pytest.raises(ValueError):
            ax.normalize_axis(bad, 3)
    for bad in ([], [[1.0, 2.0]], 2.0, [1.0, float("nan")], [float("inf")], ["a"], None):
        with pytest.raises(ValueError):
            ax.check_taps(bad)
    for bad in ("reflect", "nearest", None, "Wrap"):
        with pytest.raises(ValueError):
            ax.check_mode(bad)
        with pytest.raises(ValueError):
            ax.offsets_mpo(fs, {1: 1.0}, bad)
    with pytest.raises(ValueError, match="radius"):
        ax.correlate_taps(np.ones(25), 0, 12)          # radius 12 on an axis of 12
    ax.correlate_taps(np.ones(23), 0, 12)               # radius 11 is fine
    with pytest.raises(ValueError, match="radius"):
        ax.correlate_taps([1.0, 1.0, 1.0], 0, 1)
    with pytest.raises(ValueError, match="origin"):
        ax.correlate_taps([1.0, 2.0, 3.0], 2, 12)
    with pytest.raises(ValueError, match="origin"):
        ax.correlate_taps([1.0, 2.0, 3.0, 4.0], 2, 12)
    with pytest.raises(TypeError):
        ax.correlate_taps([1.0, 2.0, 3.0], 0.5, 12)
    with pytest.raises(ValueError, match="DCT"):
        ax.check_data_axis("DCT", 2, 3)
    ax.check_data_axis("DCT", 1, 3)
    ax.check_data_axis("Std", 2, 3)
    with pytest.raises(ValueError, match="recompress"):
        ax.check_wide_bonds([1, 2, 3, 1], [1, 2048, 1366, 1])   # 3 * 1366 = 4098
    ax.check_wide_bonds([1, 2, 3, 1], [1, 2048, 1365, 1])       # 4096 and 4095; the outer bonds are not looked at
    with pytest.raises(TypeError):
        ax.offsets_mpo(fs, {0.5: 1.0})
    with pytest.raises(ValueError):
        ax.offsets_mpo(fs, {1: float("nan")})
    with pytest.raises(ValueError):
        ax.offsets_mpo([], {1: 1.0})
    with pytest.raises(ValueError):
        ax.offsets_mpo([2, 0], {1: 1.0})
    fa = _core.get_factorlist((12, 8, 18))[0]
    cores = [np.zeros((1, int(d), 1)) for d in np.prod(fa, axis=1)]
    with pytest.raises(ValueError, match="digits"):
        ax.emulate(cores, ax.flip_mpo(fa[:, 0]), fa, 1)
    with pytest.raises(ValueError, match="site dims"):
        ax.emulate(cores[::-1], ax.flip_mpo(fa[:, 0]), fa, 0)


def test_zero_weight_taps_are_dropped():
    fs = [2, 3, 2]
    a = ax.offsets_mpo(fs, {-1: 0.0, 0: 2.0, 1: 0.0}, "constant")
    assert a.bonds == [1, 1, 1, 1] and a.opnorm == 2.0
    z = ax.offsets_mpo(fs, {1: 0.0}, "wrap")
    assert z.opnorm == 0.0 and not any(m.any() for m in z.cores)
