"""SSIM and PSNR of csrc/metrics.hip on the MI355X at their tile, window and launch edges, on the cases of
tests/stream_cases.py, called through ``_lib`` with every argument under the test's control.

* SSIM: ``1e-12`` against ``oracle.metrics`` on the same fp32 values as float64, on shapes whose window-centre extent
  ends on a 16 x 32 tile or one past it, whose three slice orientations take different windows, on more than 65535
  slices (the tile kernel goes in launches of 65535) and with a slice that is constant after the clip (NaN exactly
  where the oracle gives NaN).  tests/test_stream_cases_host.py shows on the CPU that the bar rejects a wrong window,
  an omitted clip, a dropped tile row or column and the population covariance on every shape used here.
* PSNR: ``1e-9`` relative against ``oracle.metrics.compute_psnr`` on integer data at the lengths where the reduction's
  grid changes; infinite data as NumPy has it.

Every call is made twice and must give the same bits; a workspace one byte short must be refused with NDMPS_EWORKSPACE
and the output untouched.  ``WORST`` keeps the largest error over its bar per family.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import stream_cases as sc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402
from imgcompressionmps_amd.utils import metrics as dm  # noqa: E402

DEV = "cuda:0"
WORST = {}   # family -> the largest error / bar seen in this session


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A launch that faulted leaves the device in an error state: end the session instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


def sp():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    print("worst error / bar so far: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def _ssim(lib, a, b, short=0):
    """(rc, value) of one ndmps_ssim_f32 call on device tensors; ``short``: bytes taken off the workspace."""
    shape = _lib.i64_array(a.shape)
    nbytes = int(lib.ndmps_ssim_workspace_bytes(a.dim(), shape))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = C.c_double(sc.SENTINEL)
    rc = lib.ndmps_ssim_f32(a.data_ptr(), b.data_ptr(), a.dim(), shape, C.byref(out), ws.data_ptr(), nbytes - short, sp())
    return rc, out.value


def _slices(lib, a, b, axis, short=0):
    shape = _lib.i64_array(a.shape)
    nbytes = int(lib.ndmps_ssim_slices_workspace_bytes(shape, axis))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    n = int(a.shape[axis])
    out = (C.c_double * n)(*([sc.SENTINEL] * n))
    rc = lib.ndmps_ssim_slices_f32(a.data_ptr(), b.data_ptr(), shape, axis, out, ws.data_ptr(), nbytes - short, sp())
    return rc, np.array(out[:])


def _twice(run):
    (rc1, a), (rc2, b) = run(), run()
    assert rc1 == rc2 == _lib.OK, _lib.load().ndmps_last_error()
    assert np.array_equal(a, b, equal_nan=True), "two calls must give identical bits"
    return a


@pytest.mark.parametrize("shape", sc.SSIM_SHAPES)
def test_ssim_at_tile_and_window_edges(shape):
    lib = _lib.load()
    a, b = (dev(x) for x in sc.ssim_pair(shape))
    got = _twice(lambda: _ssim(lib, a, b))
    _note("ssim", sc.close(got, sc.ssim_expected(shape), sc.SSIM_BAR))
    rc, out = _ssim(lib, a, b, short=1)
    assert rc == _lib.EWORKSPACE and out == sc.SENTINEL, "a refused call wrote its result"
    with pytest.raises(_lib.NdmpsHipError, match="workspace"):
        _lib.check(rc)
    if len(shape) != 3:
        return
    for axis in range(3):
        got = _twice(lambda: _slices(lib, a, b, axis))
        _note("ssim slices", sc.close(got, sc.ssim_slices_expected(shape, axis), sc.SSIM_BAR))
        rc, out = _slices(lib, a, b, axis, short=1)
        assert rc == _lib.EWORKSPACE and np.all(out == sc.SENTINEL), "a refused call wrote its results"
        # the wrapper maps a negative axis onto the same call
        assert np.array_equal(np.array(dm.ssim_3d_axis(a, b, axis - 3)), got)
    with pytest.raises(ValueError):
        dm.ssim_3d_axis(a, b, 3)
    with pytest.raises(ValueError):
        dm.ssim_3d_axis(a, b, -4)
    assert dm.compute_ssim_by_dim(a, b) == _ssim(lib, a, b)[1]


def test_ssim_of_more_slices_than_one_launch_takes_4d():
    """(8, 8, 8, 8200): 65600 slices along every axis, so the tile kernel's second launch starts at slice 65535."""
    lib = _lib.load()
    a, b, want = sc.ssim_chunk_4d()
    a, b = dev(a), dev(b)
    got = _twice(lambda: _ssim(lib, a, b))
    _note("ssim chunks", sc.close(got, want, sc.SSIM_BAR))


def test_ssim_of_more_slices_than_one_launch_takes_3d_per_slice():
    """(65600, 8, 8) along axis 0: 41 distinct slices tiled, so every entry of the list is known; a launch that ignored
    its slice offset, or an index that wrapped, leaves the entries from 65535 on unwritten or wrong."""
    lib = _lib.load()
    a, b, want = sc.ssim_chunk_3d()
    a, b = dev(a), dev(b)
    got = _twice(lambda: _slices(lib, a, b, 0))
    _note("ssim chunks", sc.close(got, want, sc.SSIM_BAR))


def test_ssim_of_a_slice_that_is_constant_after_the_clip():
    """Slice 0 is zero in a and -1 in b: data range 0, 0 / 0 in every window.  NaN exactly where the oracle has NaN."""
    lib = _lib.load()
    a, b, per_slice, volume = sc.ssim_constant()
    a, b = dev(a), dev(b)
    got = _twice(lambda: _slices(lib, a, b, 0))
    assert np.isnan(got[0]) and np.isnan(per_slice[0])
    _note("ssim slices", sc.close(got, per_slice, sc.SSIM_BAR))
    for axis in (1, 2):      # the zero row or column of every other orientation is no constant slice
        rc, lst = _slices(lib, a, b, axis)
        assert rc == _lib.OK and not np.isnan(lst).any()
    assert np.isnan(volume) and np.isnan(_twice(lambda: _ssim(lib, a, b)))


# ----------------------------------------------------------------------------- PSNR
def _psnr(lib, a, b, short=0):
    nbytes = int(lib.ndmps_psnr_workspace_bytes())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = C.c_double(sc.SENTINEL)
    rc = lib.ndmps_psnr_f32(a.data_ptr(), b.data_ptr(), a.numel(), C.byref(out), ws.data_ptr(), nbytes - short, sp())
    return rc, out.value


def _agrees(got, want, rel):
    """NaN for NaN, an infinity for the same infinity, ``rel`` otherwise; returns the error over the bar."""
    if np.isnan(want) or np.isinf(want):
        assert np.array_equal(got, want, equal_nan=True), (got, want)
        return 0.0
    assert abs(got - want) <= rel * abs(want), (got, want)
    return abs(got - want) / (rel * abs(want))


@pytest.mark.parametrize("n", sc.RED_LENGTHS)
def test_psnr_on_integer_data(n):
    lib = _lib.load()
    for kind in sc.PSNR_KINDS:
        a, b = sc.psnr_pair(n, kind)
        want = sc.psnr_expected(a, b)
        assert (want == np.inf) == (kind == "equal")
        ta, tb = dev(a), dev(b)
        got = _twice(lambda: _psnr(lib, ta, tb))
        _note("psnr", _agrees(float(got), want, sc.PSNR_REL))
        assert dm.compute_psnr(ta, tb) == float(got)
    rc, out = _psnr(lib, ta, tb, short=1)
    assert rc == _lib.EWORKSPACE and out == sc.SENTINEL, "a refused call wrote its result"


@pytest.mark.parametrize("n,kind", sc.NONFINITE_CASES)
def test_psnr_of_infinite_data_is_numpys(n, kind):
    """Regression: the maximum was seeded with -FLT_MAX, so an original of nothing but -inf gave FLT_MAX**2 / inf -> -inf
    where NumPy's max is -inf and the ratio inf / inf is NaN."""
    lib = _lib.load()
    a = sc.nonfinite_data(n, kind)
    b = sc.red_data(n, 0).astype(np.float32)
    with np.errstate(all="ignore"):
        want = sc.psnr_expected(a, b)
    ta, tb = dev(a), dev(b)
    got = _twice(lambda: _psnr(lib, ta, tb))
    _agrees(float(got), want, sc.PSNR_REL)
