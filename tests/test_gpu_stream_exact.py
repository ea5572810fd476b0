"""Every streaming entry of csrc/reduce.hip on the MI355X, on the cases of tests/stream_cases.py.

The entries are called through ``_lib`` with every argument under the test's control.  Bars (tests/stream_cases.py has
the derivations, tests/test_stream_cases_host.py shows on the CPU that they reject a dropped element, block, slice or
pointer chunk, a shifted arena offset, the neighbouring arena row, a wrong cast, an FMA and fp32 arithmetic, and a wrong
twiddle on every case used here):

* reductions on integer data: equality with the exact (min, max, sum of squares);
* scale, quantise, dequantise: bit equality with the fp64 expression rounded once;
* infinities: NumPy's minimum and maximum, also for a tensor that is nothing but one infinity;
* DCT of impulses: ``dct_bar(n)`` per entry against SciPy's float64 transform, the ``_many`` entries bit for bit equal
  to the single calls, also with a member that is not 16-byte aligned.

Every call is made twice and must give the same bits (all of these kernels fold in a fixed order).  Outputs that live
on the device sit between 24 guard elements on both sides, which must survive; a workspace one byte short must be
refused with NDMPS_EWORKSPACE and the output untouched.  ``WORST`` keeps the largest error over its bar per family.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import stream_cases as sc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402
from imgcompressionmps_amd.utils import filetools as hft  # noqa: E402

DEV = "cuda:0"
G = sc.GUARD
FILL = {np.dtype(np.float32): sc.SENTINEL, np.dtype(np.float64): sc.SENTINEL, np.dtype(np.uint8): 0xA5,
        np.dtype(np.uint16): 0xA5A5}
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


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    print(f"worst error / bar so far: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


class Guarded:
    """``n`` elements of ``dtype`` on the device between 24 guard elements on both sides (-7.0, or the byte 0xA5)."""

    def __init__(self, dtype, n, data=None):
        self.dt, self.n = np.dtype(dtype), int(n)
        self.host = np.full(self.n + 2 * G, FILL[self.dt], dtype=self.dt)
        if data is not None:
            self.host[G:G + self.n] = data
        self.buf = torch.empty(self.host.nbytes, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr() + G * self.dt.itemsize
        self.fresh()

    def fresh(self):
        self.buf.copy_(torch.from_numpy(self.host.view(np.uint8)))

    def read(self):
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy().view(self.dt)
        fill = self.host[0]
        assert np.all(got[:G] == fill) and np.all(got[G + self.n:] == fill), "wrote outside its n elements"
        return got[G:G + self.n].copy()

    def untouched(self):
        return np.array_equal(self.read(), self.host[G:G + self.n])


def _twice(run):
    """``run()`` twice: the same bits; returns the first result."""
    a, b = run(), run()
    assert np.array_equal(a, b, equal_nan=True), "two calls must give identical bits"
    return a


def _red_ws(lib):
    nbytes = int(lib.ndmps_reduce_workspace_bytes())
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


# ----------------------------------------------------------------------------- single-tensor reductions
def _sumsq(lib, t, n, ws, nbytes):
    fn = lib.ndmps_sumsq_f64 if t.dtype == torch.float64 else lib.ndmps_sumsq_f32
    out = C.c_double(sc.SENTINEL)
    rc = fn(t.data_ptr(), n, C.byref(out), ws.data_ptr(), nbytes, sp())
    return rc, out.value


def _minmax(lib, t, n, ws, nbytes):
    lo, hi = C.c_float(sc.SENTINEL), C.c_float(sc.SENTINEL)
    rc = lib.ndmps_minmax_f32(t.data_ptr(), n, C.byref(lo), C.byref(hi), ws.data_ptr(), nbytes, sp())
    return rc, (lo.value, hi.value)


@pytest.mark.parametrize("n,turn", sc.RED_CASES)
def test_sumsq_and_minmax_on_integer_data(n, turn):
    lib = _lib.load()
    x = sc.red_data(n, turn)
    lo, hi, ss = sc.triple(x)
    ws, nbytes = _red_ws(lib)
    t32, t64 = dev(x, torch.float32), dev(x, torch.float64)

    def ok(rc, value):
        assert rc == _lib.OK
        return np.array(value)

    for t in (t32, t64):
        got = _twice(lambda: ok(*_sumsq(lib, t, n, ws, nbytes)))
        assert got == ss, (n, turn, t.dtype, float(got), ss)
    got = _twice(lambda: ok(*_minmax(lib, t32, n, ws, nbytes)))
    assert tuple(got) == (lo, hi), (n, turn, tuple(got), (lo, hi))


def test_reductions_refuse_a_short_workspace_and_take_an_empty_tensor():
    lib = _lib.load()
    ws, nbytes = _red_ws(lib)
    x = sc.red_data(257, 0)
    for t in (dev(x, torch.float32), dev(x, torch.float64)):
        rc, out = _sumsq(lib, t, 257, ws, nbytes - 1)
        assert rc == _lib.EWORKSPACE and out == sc.SENTINEL
        with pytest.raises(_lib.NdmpsHipError, match="workspace"):
            _lib.check(rc)
        rc, out = _sumsq(lib, t, 0, ws, nbytes)       # n = 0: the sum of nothing
        assert rc == _lib.OK and out == 0.0
    rc, out = _minmax(lib, dev(x, torch.float32), 257, ws, nbytes - 1)
    assert rc == _lib.EWORKSPACE and out == (sc.SENTINEL, sc.SENTINEL)
    rc, out = _minmax(lib, dev(x, torch.float32), 0, ws, nbytes)
    assert rc == _lib.EINVAL and out == (sc.SENTINEL, sc.SENTINEL)


# ----------------------------------------------------------------------------- many tensors
def _many(lib, ptrs, lens, f64=False, short=0):
    """(count, 3) of one minmax_many call on device addresses; ``short``: bytes taken off the workspace."""
    count = len(ptrs)
    nbytes = int(lib.ndmps_minmax_many_workspace_bytes(count))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = ((C.c_double if f64 else C.c_float) * (2 * count))(*([sc.SENTINEL] * (2 * count)))
    ss = (C.c_double * count)(*([sc.SENTINEL] * count))
    fn = lib.ndmps_minmax_many_f64 if f64 else lib.ndmps_minmax_many_f32
    rc = fn(count, (C.c_void_p * count)(*ptrs), _lib.i64_array(lens), out, ss, ws.data_ptr(), nbytes - short, sp())
    got = np.column_stack([np.array(out[0::2], dtype=np.float64), np.array(out[1::2], dtype=np.float64), np.array(ss[:])])
    if short:
        return rc, got
    _lib.check(rc)
    return got


@pytest.mark.parametrize("count", sc.MANY_COUNTS)
def test_minmax_many_on_mixed_lengths(count):
    lib = _lib.load()
    xs, want = sc.many_case(count)
    for dtype in (torch.float32, torch.float64):
        ts = [dev(x, dtype) for x in xs]
        got = _twice(lambda: _many(lib, [t.data_ptr() for t in ts], [t.numel() for t in ts], dtype == torch.float64))
        assert np.array_equal(got, want), (count, dtype, np.flatnonzero(np.any(got != want, axis=1))[:8])
        rc, got = _many(lib, [t.data_ptr() for t in ts], [t.numel() for t in ts], dtype == torch.float64, short=1)
        assert rc == _lib.EWORKSPACE and np.all(got == sc.SENTINEL), f"{dtype}: a refused call wrote its results"


def test_minmax_many_on_4100_spike_rows():
    """Row p is zero but for x[p, p] = 3: every element position of a length-4100 tensor, 129 chunks of the upload."""
    lib = _lib.load()
    t = dev(sc.spike_rows())
    ptrs = [t.data_ptr() + 4 * sc.SPIKE * p for p in range(sc.SPIKE)]
    got = _twice(lambda: _many(lib, ptrs, [sc.SPIKE] * sc.SPIKE))
    bad = np.flatnonzero(np.any(got != np.array([0.0, 3.0, 9.0]), axis=1))
    assert bad.size == 0, f"{bad.size} rows are not (0, 3, 9), first {bad[:8]}: {got[bad[:3]]}"


def test_minmax_many_wrapper_takes_strided_and_mixed_lists():
    """utils/filetools.minmax_many copies what is not contiguous fp32: a strided view, an fp64 and a bf16 tensor."""
    xs, want = sc.many_case(33)
    ts = []
    for i, x in enumerate(xs):
        if i % 4 == 0:      # every second element of a tensor twice as long
            wide = torch.full((2 * len(x),), 1e30, dtype=torch.float32, device=DEV)
            wide[::2] = dev(x, torch.float32)
            ts.append(wide[::2])
        else:
            ts.append(dev(x, (torch.float32, torch.float64, torch.bfloat16)[i % 3]))
    assert not ts[0].is_contiguous() or ts[0].numel() == 1
    mm, ss = hft.minmax_many(ts, with_sumsq=True)
    assert (mm, ss) == hft.minmax_many(ts, with_sumsq=True)
    assert np.array_equal(np.column_stack([np.array(mm), np.array(ss)]), want)
    t64 = [dev(x, torch.float64) for x in xs]
    mm, ss = hft.minmax_many(t64, with_sumsq=True)
    assert np.array_equal(np.column_stack([np.array(mm), np.array(ss)]), want)
    assert hft.minmax(t64[3]) == tuple(want[3, :2]) and hft.minmax(ts[1]) == tuple(want[1, :2])


# ----------------------------------------------------------------------------- arena
def _arena(lib, base_ptr, stride, batch, n_cores, offsets, lens, partial):
    rc = lib.ndmps_minmax_arena_launch_f32(base_ptr, stride, batch, n_cores,
                                           None if offsets is None else _lib.i64_array(offsets),
                                           None if lens is None else _lib.i64_array(lens), partial.data_ptr(), sp())
    return rc


def _collect(lib, count, partial):
    out = (C.c_float * (2 * count))()
    ss = (C.c_double * count)()
    _lib.check(lib.ndmps_minmax_collect(count, partial.data_ptr(), out, ss, sp()))
    return np.column_stack([np.array(out[0::2], dtype=np.float64), np.array(out[1::2], dtype=np.float64), np.array(ss[:])])


def _partials(lib, count):
    return torch.full((int(lib.ndmps_minmax_partials_bytes(count)) // 8 + G,), sc.SENTINEL, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("batch,n_cores", sc.ARENA_CASES)
def test_minmax_arena_reads_its_cores_and_nothing_else(batch, n_cores):
    lib = _lib.load()
    arena, offsets, lens, stride, want = sc.arena_case(batch, n_cores)
    t = dev(arena)
    count = batch * n_cores
    partial = _partials(lib, count)

    def run():
        partial.fill_(sc.SENTINEL)
        _lib.check(_arena(lib, t.data_ptr(), stride, batch, n_cores, offsets, lens, partial))
        got = _collect(lib, count, partial)
        assert bool((partial[-G:] == sc.SENTINEL).all()), "wrote behind the partials it asked for"
        return got

    got = _twice(run)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, f"(volume, core) {[(int(b) // n_cores, int(b) % n_cores) for b in bad[:6]]}: {got[bad[:3]]} != {want[bad[:3]]}"


def test_minmax_arena_refusals_write_nothing():
    lib = _lib.load()
    for name, batch, n_cores, offsets, lens, stride in sc.arena_refusals():
        count = batch * n_cores
        base = torch.zeros(batch * stride + 64, dtype=torch.float32, device=DEV)     # in bounds even if it were launched
        partial = _partials(lib, count)
        with pytest.raises(ValueError):
            _lib.check(_arena(lib, base.data_ptr(), stride, batch, n_cores, offsets, lens, partial))
        torch.cuda.synchronize()
        assert bool((partial == sc.SENTINEL).all()), name
    partial = _partials(lib, 2)
    for bad in (dict(base=None), dict(part=None)):
        rc = lib.ndmps_minmax_arena_launch_f32(None if "base" in bad else base.data_ptr(), 16, 1, 2, _lib.i64_array([0, 8]),
                                               _lib.i64_array([4, 4]), None if "part" in bad else partial.data_ptr(), sp())
        assert rc == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((partial == sc.SENTINEL).all())


# ----------------------------------------------------------------------------- infinities
@pytest.mark.parametrize("n,kind", sc.NONFINITE_CASES)
def test_reductions_return_numpys_extremes_of_infinite_data(n, kind):
    """Regression: the reductions were seeded with +-FLT_MAX (+-DBL_MAX), so a tensor of nothing but +inf came back with
    the minimum FLT_MAX and one of nothing but -inf with the maximum -FLT_MAX."""
    lib = _lib.load()
    x = sc.nonfinite_data(n, kind)
    want = (float(x.min()), float(x.max()))
    ws, nbytes = _red_ws(lib)
    t32, t64 = dev(x), dev(x, torch.float64)

    def minmax():
        rc, (lo, hi) = _minmax(lib, t32, n, ws, nbytes)
        return np.array([rc, lo, hi], dtype=np.float64)

    got = _twice(minmax)
    assert tuple(got) == (_lib.OK,) + want, ("minmax_f32", got, want)
    for t in (t32, t64):
        assert tuple(_twice(lambda: np.array(_sumsq(lib, t, n, ws, nbytes)))) == (_lib.OK, np.inf)
    finite = {False: dev(sc.red_data(257, 0), torch.float32), True: dev(sc.red_data(257, 0), torch.float64)}
    for t, f64 in ((t32, False), (t64, True)):      # beside a finite tensor, on both sides of it
        got = _twice(lambda: _many(lib, [t.data_ptr(), finite[f64].data_ptr(), t.data_ptr()], [n, 257, n], f64))
        assert tuple(got[0]) == tuple(got[2]) == want + (np.inf,), ("minmax_many", f64, got, want)
        assert tuple(got[1]) == sc.triple(sc.red_data(257, 0))
    arena = np.full((2, n + 8), -sc.ARENA_FILL, dtype=np.float32)
    arena[:, 3:3 + n] = x
    partial, d_arena = _partials(lib, 2), dev(arena)

    def run():
        partial.fill_(sc.SENTINEL)
        _lib.check(_arena(lib, d_arena.data_ptr(), n + 8, 2, 1, [3], [n], partial))
        return _collect(lib, 2, partial)

    got = _twice(run)
    assert tuple(got[0]) == tuple(got[1]) == want + (np.inf,), ("arena", got, want)


# ----------------------------------------------------------------------------- scale
@pytest.mark.parametrize("n", sc.STREAM_LENGTHS)
def test_scale_is_one_fp64_product_rounded_once(n):
    lib = _lib.load()
    for elem, fn in (("f32", lib.ndmps_scale_f32), ("f64", lib.ndmps_scale_f64)):
        x = sc.scale_data(n, elem)
        buf = Guarded(x.dtype, n, x)
        for f in sc.scale_factors(x):
            def run():
                buf.fresh()
                _lib.check(fn(buf.ptr, n, f, sp()))
                return buf.read()
            got = _twice(run)
            want = sc.scale_expected(x, f)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{elem} n={n} f={f}: {bad.size} elements differ, first {bad[:5]}"
        buf.fresh()
        _lib.check(fn(buf.ptr, 0, 2.0, sp()))       # n = 0 writes nothing
        assert buf.untouched()


@pytest.mark.parametrize("count,n", sc.SCALE_MANY)
def test_scale_many_gives_every_tensor_its_own_factor(count, n):
    lib = _lib.load()
    x, f = sc.scale_many_case(count, n)
    host = np.full((count, n + 2 * G), sc.SENTINEL, dtype=np.float32)
    host[:, G:G + n] = x
    buf = dev(host)
    ptrs = (C.c_void_p * count)(*[buf.data_ptr() + 4 * (r * (n + 2 * G) + G) for r in range(count)])

    def run():
        buf.copy_(torch.from_numpy(host))
        _lib.check(lib.ndmps_scale_many_f32(count, ptrs, n, _lib.f64_array(f), sp()))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[:, :G] == sc.SENTINEL) and np.all(got[:, G + n:] == sc.SENTINEL), "wrote outside a tensor"
        return got[:, G:G + n]

    got = _twice(run)
    want = sc.scale_many_expected(x, f)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (tensor, index) {bad[:5].tolist()}"


# ----------------------------------------------------------------------------- quantiser
def _quantise(lib, x, lo, hi, bits):
    """Codes of one quantise call into a guarded buffer, twice."""
    t = dev(x)
    fn = lib.ndmps_quantize_f64 if x.dtype == np.float64 else lib.ndmps_quantize_f32
    out = Guarded(sc.QDT[bits], len(x))

    def run():
        out.fresh()
        _lib.check(fn(t.data_ptr(), len(x), lo, hi, bits, out.ptr, sp()))
        return out.read()

    return _twice(run)


def _dequantise(lib, codes, lo, hi, bits, elem):
    t = dev(codes.view(np.int16) if bits == 16 else codes)
    fn = lib.ndmps_dequantize_f64 if elem == "f64" else lib.ndmps_dequantize_f32
    out = Guarded(sc.FDT[elem], len(codes))

    def run():
        out.fresh()
        _lib.check(fn(t.data_ptr(), len(codes), lo, hi, bits, out.ptr, sp()))
        return out.read()

    return _twice(run)


@pytest.mark.parametrize("r,bits,elem", sc.QUANT_CASES)
def test_quantiser_on_and_next_to_every_code(r, bits, elem):
    lib = _lib.load()
    x, lo, hi, want = sc.quant_case(r, bits, elem)
    got = _quantise(lib, x, lo, hi, bits)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} codes differ, first x={x[bad[:4]]}: {got[bad[:4]]} != {want[bad[:4]]}"
    # the wrapper finds lo and hi itself (they are in x)
    assert np.array_equal(hft.to_numpy_uint(hft.scale_to_dtype(dev(x), sc.QDT[bits]), sc.QDT[bits]), want)
    codes, lo, hi, back = sc.dequant_case(r, bits, elem)
    got = _dequantise(lib, codes, lo, hi, bits, elem)
    bad = np.flatnonzero(got != back)
    assert bad.size == 0, f"{bad.size} values differ, first codes {codes[bad[:4]]}: {got[bad[:4]]} != {back[bad[:4]]}"


@pytest.mark.parametrize("n", sc.STREAM_LENGTHS)
def test_quantiser_at_every_stream_grid_length(n):
    """quantize_kernel and dequantize_kernel have grid-stride loops of their own (four instantiations each): one
    element, around one block, around the 2048-workgroup cap and twice past it, both widths, both element types."""
    lib = _lib.load()
    for elem in ("f32", "f64"):
        for bits in (8, 16):
            x, lo, hi, codes, back = sc.quant_stream_case(n, bits, elem)
            got = _quantise(lib, x, lo, hi, bits)
            bad = np.flatnonzero(got != codes)
            assert bad.size == 0, f"{elem} {bits} bits: {bad.size} codes differ, first at {bad[:5]}: {got[bad[:5]]}"
            got = _dequantise(lib, codes, lo, hi, bits, elem)
            bad = np.flatnonzero(got != back)
            assert bad.size == 0, f"{elem} {bits} bits: {bad.size} values differ, first at {bad[:5]}: {got[bad[:5]]}"


@pytest.mark.parametrize("elem", ["f32", "f64"])
def test_quantiser_past_the_grid_cap_and_on_a_constant_tensor(elem):
    lib = _lib.load()
    x, lo, hi = sc.quant_large(elem)
    for bits in (8, 16):
        want = sc.quant_large_expected(x, bits)
        got = _quantise(lib, x, lo, hi, bits)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} codes differ, first at {bad[:5]}"
        back = _dequantise(lib, want, lo, hi, bits, elem)
        ref = sc.oft.scale_back(want, lo, hi, sc.QDT[bits]).astype(sc.FDT[elem])
        assert np.array_equal(back, ref)
        c = sc.quant_constant(elem)      # span = 0
        got = _quantise(lib, c, float(c[0]), float(c[0]), bits)
        assert not got.any(), "a constant tensor quantises to code 0, as in the oracle"


# ----------------------------------------------------------------------------- DCT
def _basis(lib, n):
    b = torch.empty((n, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_dct_basis_f32(b.data_ptr(), n, sp()))
    return b


def _dct(lib, src_ptr, dst_ptr, rows, n, basis, inverse=False):
    fn = lib.ndmps_idct_last_f32 if inverse else lib.ndmps_dct_last_f32
    _lib.check(fn(src_ptr, dst_ptr, rows, n, basis.data_ptr(), sp()))


def _dct_many(lib, src, dst, rows, n, basis, inverse=False):
    fn = lib.ndmps_idct_last_many_f32 if inverse else lib.ndmps_dct_last_many_f32
    count = len(src)
    _lib.check(fn(count, (C.c_void_p * count)(*src), (C.c_void_p * count)(*dst), rows, n, basis.data_ptr(), sp()))


@pytest.mark.parametrize("n", sc.DCT_N)
def test_dct_of_impulses_is_the_dct_matrix_at_fp32_accuracy(n):
    lib = _lib.load()
    want = sc.dct_matrix(n)
    basis = _basis(lib, n)
    eye = torch.eye(n, dtype=torch.float32, device=DEV)
    w32 = dev(want.astype(np.float32))
    y, back = torch.full_like(eye, sc.SENTINEL), torch.full_like(eye, sc.SENTINEL)

    def forward():
        y.fill_(sc.SENTINEL)
        _dct(lib, eye.data_ptr(), y.data_ptr(), n, n, basis)
        return y.cpu().numpy()

    def inverse():
        back.fill_(sc.SENTINEL)
        _dct(lib, w32.data_ptr(), back.data_ptr(), n, n, basis, inverse=True)
        return back.cpu().numpy()

    got, gotb = _twice(forward), _twice(inverse)
    err, errb = np.abs(got - want).max(), np.abs(gotb - np.eye(n)).max()
    print(f"n = {n}: forward {err:.3g} (bar {sc.dct_bar(n):.3g}), inverse {errb:.3g} (bar {sc.idct_bar(n):.3g})")
    _note("dct", err / sc.dct_bar(n))
    _note("idct", errb / sc.idct_bar(n))
    assert err <= sc.dct_bar(n), np.unravel_index(np.abs(got - want).argmax(), got.shape)
    assert errb <= sc.idct_bar(n), np.unravel_index(np.abs(gotb - np.eye(n)).argmax(), gotb.shape)

    # 33 volumes (the impulses and the matrix with their rows rolled by v) in one call: the bits of 33 single calls
    for inv, first in ((False, eye), (True, w32)):
        vols = torch.stack([torch.roll(first, v, dims=0) for v in range(sc.DCT_VOLS)])
        many, single, again = (torch.full_like(vols, sc.SENTINEL) for _ in range(3))
        for out in (many, again):
            _dct_many(lib, [vols[v].data_ptr() for v in range(sc.DCT_VOLS)], [out[v].data_ptr() for v in range(sc.DCT_VOLS)],
                      n, n, basis, inv)
        for v in range(sc.DCT_VOLS):
            _dct(lib, vols[v].data_ptr(), single[v].data_ptr(), n, n, basis, inv)
        torch.cuda.synchronize()
        assert torch.equal(many, again), "two calls must give identical bits"
        assert torch.equal(many, single), f"inverse={inv}: a volume of the group differs from its single call"
        assert torch.equal(many[0], y if not inv else back)
        assert torch.equal(many[5], torch.roll(many[0], 5, dims=0))


def _off_by_four_bytes(numel, data=None):
    """A (numel,) fp32 view that starts 4 bytes into its allocation."""
    buf = torch.full((numel + 1 + G,), sc.SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[1:1 + numel]
    assert view.data_ptr() % 16 == 4
    if data is not None:
        view.copy_(data.reshape(-1))
    return buf, view


@pytest.mark.parametrize("rows", [5, 64])
def test_dct_with_an_operand_off_its_16_byte_boundary(rows):
    """Four bytes into an allocation the FFT's 16-byte loads and stores are not possible: the basis product runs."""
    lib = _lib.load()
    n = 128
    x, ref = sc.dct_random(rows, n)
    basis = _basis(lib, n)
    bar = sc.DCT_LOOSE * max(1.0, np.abs(ref).max())
    tx, tref = dev(x), dev(ref.astype(np.float32))
    for inv, src, want, tol in ((False, tx, ref, bar), (True, tref, x.astype(np.float64), sc.DCT_LOOSE)):
        # the input off, then the output off
        _, s_off = _off_by_four_bytes(rows * n, src)
        out = torch.full((rows, n), sc.SENTINEL, dtype=torch.float32, device=DEV)

        def from_off():
            out.fill_(sc.SENTINEL)
            _dct(lib, s_off.data_ptr(), out.data_ptr(), rows, n, basis, inv)
            return out.cpu().numpy()

        err = np.abs(_twice(from_off) - want).max()
        _note("dct off boundary", err / tol)
        assert err <= tol, (inv, "input", err, tol)
        buf, o_off = _off_by_four_bytes(rows * n)

        def to_off():
            buf.fill_(sc.SENTINEL)
            _dct(lib, src.data_ptr(), o_off.data_ptr(), rows, n, basis, inv)
            torch.cuda.synchronize()
            assert float(buf[0]) == sc.SENTINEL and bool((buf[1 + rows * n:] == sc.SENTINEL).all()), "wrote outside the view"
            return o_off.cpu().numpy().reshape(rows, n)

        err = np.abs(_twice(to_off) - want).max()
        _note("dct off boundary", err / tol)
        assert err <= tol, (inv, "output", err, tol)


@pytest.mark.parametrize("rows", [5, 64])
def test_dct_many_routes_every_volume_by_its_own_alignment(rows):
    """Regression: one member off its 16-byte boundary sent the whole group through the basis product, so its aligned
    neighbours no longer had the bits of their single calls (which take the FFT)."""
    lib = _lib.load()
    n = 128
    basis = _basis(lib, n)
    for inv in (False, True):
        data = [sc.dct_random(rows + 100 * v, n) for v in range(3)]
        src = [dev((ref if inv else x)[:rows].astype(np.float32)) for x, ref in data]
        want = [(x.astype(np.float64) if inv else ref)[:rows] for x, ref in data]
        _, off = _off_by_four_bytes(rows * n, src[1])
        ins = [src[0].data_ptr(), off.data_ptr(), src[2].data_ptr()]
        many, many2, single, single2 = ([torch.full((rows, n), sc.SENTINEL, dtype=torch.float32, device=DEV)
                                         for _ in range(3)] for _ in range(4))
        for outs in (many, many2):
            _dct_many(lib, ins, [t.data_ptr() for t in outs], rows, n, basis, inv)
        for outs in (single, single2):
            for v in range(3):
                _dct(lib, ins[v], outs[v].data_ptr(), rows, n, basis, inv)
        torch.cuda.synchronize()
        for v in range(3):
            assert torch.equal(many[v], many2[v]) and torch.equal(single[v], single2[v]), "two calls: identical bits"
            assert torch.equal(many[v], single[v]), f"inverse={inv}: volume {v} differs from its single call"
            tol = sc.DCT_LOOSE * max(1.0, np.abs(want[v]).max())
            assert np.abs(many[v].cpu().numpy() - want[v]).max() <= tol
