"""Inputs and expected values for the streaming kernels (csrc/reduce.hip) and the device metrics (csrc/metrics.hip),
shared by tests/test_stream_cases_host.py (CPU: every bar rejects, on exactly these cases, the faults it exists for) and
tests/test_gpu_stream_exact.py / tests/test_gpu_metrics_edges.py (the kernels).  NumPy and SciPy only: no torch, no device.

Bars, and where they come from:

* Reductions (``sumsq``, ``minmax``, ``minmax_many``, the arena pair): integer data of magnitude at most 64.  Every sum
  of squares is an integer below 2**53 and the same in every order of summation, a minimum and a maximum are copies of
  an input: the bar is equality.  The unique minimum and maximum are planted (``planted``) where a block, a trip of the
  grid-stride loop or the tensor ends; every other value is a non-zero integer strictly between them, so dropping any
  non-empty set of elements changes the sum of squares.
* ``scale``: ``(x.astype(f64) * f).astype(f32)`` bit for bit (one fp64 product, one rounding to the element type).
* Quantiser: the codes of ``oracle.filetools.scale_to_dtype`` on the same values as float64, bit for bit; dequantiser:
  ``oracle.filetools.scale_back`` bit for bit in fp64 and its fp32 rounding for the fp32 kernel.
* DCT on impulses: ``dct_bar(n) = 8 (log2(n) / 2 + 3) 2**-24 sqrt(2 / n)`` per entry against SciPy's float64 transform.
  An impulse passes through at most ``ceil(log2(n / 2) / 2)`` twiddle multiplications, two post-twiddles and one scale,
  each an fp32 product with an fp32-rounded factor (at most 2 ulp each with the complex product's own sum); nothing
  cancels, and an entry is at most ``sqrt(2 / n)``.  The inverse of the fp32-rounded matrix is the identity within
  ``idct_bar(n)``, the same count at entry magnitude 1.
* SSIM: ``1e-12`` against ``oracle.metrics`` on the same fp32 values as float64 (the project's bar for this comparison;
  all inputs stay on the [0, 1] scale it was set on).  PSNR: ``1e-9`` relative against ``oracle.metrics.compute_psnr``.

Lengths name the kernel boundary they cross: ``RED_LENGTHS`` the ``ceil(n / 2048)``-block reductions capped at 1024
blocks (one block up to 2048, the cap from 2**21, a second trip of the grid-stride loop past it), ``STREAM_LENGTHS`` the
``stream_grid`` kernels capped at 2048 blocks of 256 (524288 elements), ``SLICE_LENGTHS`` the 16-slice kernels (one
trip up to 4096).
"""
import functools
import zlib

import numpy as np

from oracle import filetools as oft
from oracle import metrics as om

BLOCK = 256
RED_BLOCKS = 1024        # kRedBlocks, kPsnrBlocks
STREAM_BLOCKS = 2048     # stream_grid: 8 workgroups on each of 256 CUs
SLICES = 16              # kManySlices
CHUNK = 32               # kManyChunk, kScaleVols, kDctVols
ARENA_CORES = 64         # kArenaCores

RED_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 100003, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1,
               2 ** 21 + 2049, 3 * 2 ** 21 + 5)
STREAM_LENGTHS = (1, 255, 256, 257, 524287, 524288, 524289, 2 * 524288 + 3)
SLICE_LENGTHS = (1, 255, 256, 257, 4095, 4096, 4097, 8193)
SENTINEL, GUARD = -7.0, 24
ARENA_FILL = 1e30


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


# ----------------------------------------------------------------------------- integer data
def red_grid(n):
    """Workgroups of a single-tensor reduction (sumsq, minmax, PSNR)."""
    return min(max(-(-n // (8 * BLOCK)), 1), RED_BLOCKS)


def planted(n, grid):
    """Where a kernel with ``grid`` workgroups of 256 can lose an element: index 0, the last index, the last index of
    the first block, the first index of the last (partial) block, the first element of the second grid-stride trip."""
    c = [0, n - 1, min(BLOCK - 1, n - 1), (n - 1) // BLOCK * BLOCK, min(grid * BLOCK, n - 1)]
    return list(dict.fromkeys(c))


def integer_data(n, grid, turn, ident=0, key=()):
    """int8 data: non-zero values of magnitude at most 32, the unique minimum in [-64, -33] and the unique maximum in
    [33, 64] (both depend on ``ident``, so two tensors of one call differ in them) at the ``turn``-th and the next
    entry of ``planted``.  ``n = 1``: the one value is both."""
    rng = _rng("int", n, grid, turn, ident, *key)
    x = rng.integers(1, 33, size=n, dtype=np.int8)
    x *= rng.integers(0, 2, size=n, dtype=np.int8) * 2 - 1
    c = planted(n, grid)
    x[c[(turn + 1) % len(c)]] = 33 + (7 * ident) % 32
    x[c[turn % len(c)]] = -(33 + ident % 32)      # n = 1: the minimum wins
    return x


def triple(x):
    """(min, max, sum of squares) of integer data, exact."""
    xi = np.asarray(x, dtype=np.int64)
    return float(xi.min()), float(xi.max()), float(int(np.dot(xi, xi)))


# every length once, the planted pair moving on from case to case, and every pair at three lengths at which the five
# planted positions are distinct (3000: two workgroups, a second trip of both)
RED_ALL_TURNS = (3000, 100003, 2 ** 21 + 3000)
RED_CASES = tuple(dict.fromkeys([(n, i) for i, n in enumerate(RED_LENGTHS)] +
                                [(n, t) for n in RED_ALL_TURNS for t in range(5)]))


@functools.lru_cache(maxsize=None)
def red_data(n, turn):
    return integer_data(n, red_grid(n), turn)


# ----------------------------------------------------------------------------- many tensors in one call
SPIKE = 4100
MANY_COUNTS = (1, 31, 32, 33, 64, 65)


def spike_rows():
    """(P, n) with P = n = 4100: row p is zero but for x[p, p] = 3: every element position of a length-4100 tensor,
    and 129 chunks of the pointer upload.  Expected per row: (0, 3, 9)."""
    x = np.zeros((SPIKE, SPIKE), dtype=np.float32)
    np.fill_diagonal(x, 3.0)
    return x


def many_lengths(count):
    return [SLICE_LENGTHS[(3 * i + count) % len(SLICE_LENGTHS)] for i in range(count)]


@functools.lru_cache(maxsize=None)
def many_case(count):
    """``count`` tensors of mixed lengths; returns (list of int8 arrays, (count, 3) expected triples)."""
    xs = [integer_data(n, SLICES, i, ident=i, key=("many", count)) for i, n in enumerate(many_lengths(count))]
    return xs, np.array([triple(x) for x in xs])


# ----------------------------------------------------------------------------- arena
ARENA_CASES = tuple((b, c) for b in (1, 3) for c in (1, 7, 64))


def arena_layout(n_cores):
    """(offsets, lens, row_stride): a gap of 1 to 3 elements before every core (odd and even offsets), lengths from
    SLICE_LENGTHS, five elements of tail."""
    lens = [SLICE_LENGTHS[(5 * i + n_cores + 5) % len(SLICE_LENGTHS)] for i in range(n_cores)]
    offsets, off = [], 0
    for i, n in enumerate(lens):
        off += 1 + i % 3
        offsets.append(off)
        off += n
    return offsets, lens, off + 5


@functools.lru_cache(maxsize=None)
def arena_case(batch, n_cores):
    """(arena (batch, row_stride) fp32, offsets, lens, row_stride, expected (batch * n_cores, 3)).  Everything outside
    the cores holds +-1e30."""
    offsets, lens, stride = arena_layout(n_cores)
    arena = np.where(np.arange(batch * stride) % 2, ARENA_FILL, -ARENA_FILL).astype(np.float32).reshape(batch, stride)
    want = []
    for b in range(batch):
        for i, (o, n) in enumerate(zip(offsets, lens)):
            x = integer_data(n, SLICES, b + i, ident=b * (n_cores + 1) + i, key=("arena", batch, n_cores))
            arena[b, o:o + n] = x
            want.append(triple(x))
    return arena, offsets, lens, stride, np.array(want)


def arena_refusals():
    """(name, batch, n_cores, offsets, lens, row_stride) the library must refuse, writing nothing."""
    o65, l65 = [8 * i for i in range(65)], [4] * 65
    return [("65 cores", 1, 65, o65, l65, 1024),
            ("65536 tensors", 1024, 64, o65[:64], l65[:64], 1024),
            ("a core leaves its row", 1, 2, [0, 8], [4, 5], 12),
            ("an empty core", 1, 2, [0, 8], [4, 0], 16),
            ("no offsets", 1, 2, None, [4, 4], 16),
            ("no lengths", 1, 2, [0, 8], None, 16)]


# ----------------------------------------------------------------------------- scale
# The first and the last element of every scale tensor (no fp32 value does both for the factor 1 / 3).  SCALE_FIRST / 3
# in fp64 rounds up to fp32, so a truncating cast gives another value, and alone (n = 1) its product with
# 1 / sqrt(x^2) is 1 in fp64 and 1 - 2**-24 in fp32 arithmetic; SCALE_LAST / 3 differs from the fp32 product with
# fp32(1 / 3) (tests/test_stream_cases_host.py checks all three).
SCALE_FIRST, SCALE_LAST = np.float32(1.089), np.float32(1.7)
SCALE_MANY = ((1, 2 * 524288 + 3), (32, 524289), (33, 524287), (65, 257), (33, 1), (65, 255), (32, 256), (1, 524288),
              (2, 2048 * 2048 + 257))   # the last: past scale_many's own cap of 2048 workgroups of 2048 elements


@functools.lru_cache(maxsize=4)
def scale_data(n, elem="f32"):
    x = _rng("scale", n).standard_normal(n).astype(np.float32 if elem == "f32" else np.float64)
    x[-1] = SCALE_LAST
    x[0] = SCALE_FIRST
    return x


def scale_factors(x):
    x64 = x.astype(np.float64)
    return (1.0 / 3.0, 1.0 / float(np.sqrt(np.dot(x64, x64))), -0.25)


def scale_expected(x, f):
    return (x.astype(np.float64) * f).astype(x.dtype)


def scale_many_case(count, n):
    """((count, n) fp32 rows, factors (count,))."""
    x = _rng("scale_many", count, n).standard_normal((count, n)).astype(np.float32)
    x[:, -1] = SCALE_LAST
    x[:, 0] = SCALE_FIRST
    f = np.array([(-1.0) ** t / (3.0 + t) for t in range(count)])
    return x, f


def scale_many_expected(x, f):
    return (x.astype(np.float64) * f[:, None]).astype(np.float32)


# ----------------------------------------------------------------------------- quantiser
QRANGES = ((-0.1, 0.7), (0.0, 1.0), (-3e-3, 1e4))
QDT = {8: np.uint8, 16: np.uint16}
FDT = {"f32": np.float32, "f64": np.float64}
QUANT_CASES = tuple((r, bits, elem) for r in range(len(QRANGES)) for bits in (8, 16) for elem in ("f32", "f64"))
QUANT_LARGE = 2 * 524288 + 3


def qrange(r, elem):
    """The range as the kernel of ``elem`` can take it: fp32-representable bounds for the fp32 kernels."""
    lo, hi = QRANGES[r]
    return (float(np.float32(lo)), float(np.float32(hi))) if elem == "f32" else (lo, hi)


@functools.lru_cache(maxsize=None)
def quant_case(r, bits, elem):
    """(x, lo, hi, codes): for every code k the value lo + span k / qmax in the element type and its two neighbours,
    clipped into [lo, hi], with lo and hi themselves: where (x - lo) / span * qmax lands on or next to an integer."""
    lo, hi = qrange(r, elem)
    dt, qmax = FDT[elem], 2 ** bits - 1
    xk = (lo + (hi - lo) * np.arange(qmax + 1, dtype=np.float64) / qmax).astype(dt)
    inf = np.array(np.inf, dtype=dt)
    x = np.concatenate([[dt(lo)], xk, np.nextafter(xk, -inf), np.nextafter(xk, inf), [dt(hi)]]).astype(dt)
    x = np.clip(x, dt(lo), dt(hi))
    assert float(x.min()) == lo and float(x.max()) == hi
    return x, lo, hi, oft.scale_to_dtype(x.astype(np.float64), QDT[bits])


def dequant_case(r, bits, elem):
    """(codes 0 .. qmax, lo, hi, expected in the element type)."""
    lo, hi = qrange(r, elem)
    codes = np.arange(2 ** bits, dtype=QDT[bits])
    return codes, lo, hi, oft.scale_back(codes, lo, hi, QDT[bits]).astype(FDT[elem])


@functools.lru_cache(maxsize=2)
def quant_large(elem):
    """(x, lo, hi) of a random tensor past the 2048-workgroup cap of stream_grid, twice over."""
    lo, hi = QRANGES[0]
    x = _rng("quant", elem).uniform(lo, hi, QUANT_LARGE).astype(FDT[elem])
    return x, float(x.min()), float(x.max())


def quant_large_expected(x, bits):
    return oft.scale_to_dtype(x.astype(np.float64), QDT[bits])


QFILL = {8: 0xA5, 16: 0xA5A5}      # what a code buffer holds before the call (and its guard elements after it)


@functools.lru_cache(maxsize=None)
def _quant_large_codes(elem, bits):
    x, lo, hi = quant_large(elem)
    codes = quant_large_expected(x, bits)
    return codes, oft.scale_back(codes, lo, hi, QDT[bits]).astype(FDT[elem])


def quant_stream_case(n, bits, elem):
    """(x, lo, hi, codes, back) at a length of STREAM_LENGTHS: the first ``n`` elements of ``quant_large`` with the lo
    and hi of the whole tensor.  A code depends on its own element, lo and hi only, so the oracle's codes of the whole
    tensor, cut to ``n``, are the expectation; ``back`` is the oracle's ``scale_back`` of them in the element type."""
    x, lo, hi = quant_large(elem)
    codes, back = _quant_large_codes(elem, bits)
    return x[:n], lo, hi, codes[:n], back[:n]


def quant_constant(elem):
    """A constant tensor (span = 0): 0 / 0 is NaN, and the cast of NaN gives code 0, in the oracle as in the kernel."""
    return np.full(1000, 0.37, dtype=FDT[elem])


def oracle_constant_codes(x, bits):
    with np.errstate(all="ignore"):
        return oft.scale_to_dtype(x.astype(np.float64), QDT[bits])


# ----------------------------------------------------------------------------- infinities
NONFINITE_LENGTHS = (1, 257, 2049, 4097)
NONFINITE_KINDS = ("all +inf", "all -inf", "one +inf", "one -inf", "both")


def nonfinite_data(n, kind):
    """fp32 data with infinities (NaN is out of scope: fminf / fmaxf skip it); expected values are NumPy's."""
    if kind.startswith("all"):
        return np.full(n, np.inf if "+" in kind else -np.inf, dtype=np.float32)
    x = integer_data(n, SLICES, 1, key=("inf", kind)).astype(np.float32)
    if kind in ("one +inf", "both"):
        x[n // 2] = np.inf
    if kind in ("one -inf", "both"):
        x[(n // 3 + 1) % n] = -np.inf
    return x


NONFINITE_CASES = tuple((n, k) for n in NONFINITE_LENGTHS for k in NONFINITE_KINDS if n > 1 or k.startswith("all"))


# ----------------------------------------------------------------------------- DCT
DCT_N = (64, 128, 256, 512, 1024)
DCT_VOLS = 33
DCT_LOOSE = 3e-6    # the bar of test_dct_last_axis, times max(1, |ref|max)


def dct_bar(n):
    return 8 * (np.log2(n) / 2 + 3) * 2.0 ** -24 * np.sqrt(2.0 / n)


def idct_bar(n):
    return 8 * (np.log2(n) / 2 + 3) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def dct_matrix(n):
    """Row j: the orthonormal DCT-II of the impulse at j, in float64."""
    from scipy.fft import dct

    return dct(np.eye(n), type=2, norm="ortho", axis=-1)


def dct_random(rows, n):
    from scipy.fft import dct

    x = _rng("dct", rows, n).random((rows, n)).astype(np.float32)
    return x, dct(x.astype(np.float64), type=2, norm="ortho", axis=-1)


# ----------------------------------------------------------------------------- SSIM and PSNR
SSIM_BAR = 1e-12
PSNR_REL = 1e-9
SSIM_2D = ((3, 3), (4, 9), (7, 7), (8, 70), (22, 38), (23, 39), (38, 71), (39, 72))
SSIM_3D = ((40, 5, 33), (6, 6, 6), (3, 4, 9), (23, 39, 8))
SSIM_4D = ((3, 4, 9, 2), (9, 23, 39, 2))
SSIM_SHAPES = SSIM_2D + SSIM_3D + SSIM_4D
CHUNK_FRAMES, CHUNK_REPEAT = 41, 1600     # 41 * 1600 = 65600 slices: more than the 65535 of one launch


@functools.lru_cache(maxsize=None)
def ssim_pair(shape):
    """(a, b) fp32: a uniform in [0, 1), b = a + 0.05 N(0, 1) with its first element negative (so the clip of the
    second argument matters on every shape, also the 3 x 3 one)."""
    rng = _rng("ssim", *shape)
    a = rng.random(shape).astype(np.float32)
    b = (a + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    b.flat[0] = -abs(b.flat[0]) - np.float32(0.01)
    return a, b


def f64(*arrays):
    return tuple(x.astype(np.float64) for x in arrays)


@functools.lru_cache(maxsize=None)
def ssim_expected(shape):
    return float(om.compute_ssim_by_dim(*f64(*ssim_pair(shape))))


@functools.lru_cache(maxsize=None)
def ssim_slices_expected(shape, axis):
    return np.array(om.ssim_3d_axis(*f64(*ssim_pair(shape)), axis=axis))


@functools.lru_cache(maxsize=None)
def ssim_chunk_4d():
    """((8, 8, 8, 8200) pair, expected): 41 distinct frames 200 times; 8 * 8200 = 65600 slices per axis.  The mean over
    the repeated frames is the mean over the 41."""
    a, b = ssim_pair((8, 8, 8, CHUNK_FRAMES))
    rep = CHUNK_REPEAT // 8
    return np.tile(a, (1, 1, 1, rep)), np.tile(b, (1, 1, 1, rep)), float(om.compute_ssim_by_dim(*f64(a, b)))


@functools.lru_cache(maxsize=None)
def ssim_chunk_3d():
    """((65600, 8, 8) pair, expected list along axis 0): 41 distinct slices, tiled."""
    a, b = ssim_pair((CHUNK_FRAMES, 8, 8))
    want = np.array(om.ssim_3d_axis(*f64(a, b), axis=0))
    return np.tile(a, (CHUNK_REPEAT, 1, 1)), np.tile(b, (CHUNK_REPEAT, 1, 1)), np.tile(want, CHUNK_REPEAT)


@functools.lru_cache(maxsize=None)
def ssim_constant():
    """(a, b, per-slice list along axis 0, volume value): slice 0 is zero in a and -1 in b, so constant after the clip:
    data range 0, 0 / 0 in every window, NaN in the oracle."""
    a, b = (x.copy() for x in ssim_pair((12, 20, 16)))
    a[0], b[0] = 0.0, -1.0
    with np.errstate(all="ignore"):
        a64, b64 = f64(a, b)
        return a, b, np.array(om.ssim_3d_axis(a64, b64, axis=0)), float(om.compute_ssim_by_dim(a64, b64))


PSNR_KINDS = ("last", "negative", "equal")


def psnr_pair(n, kind):
    """fp32 (a, b) on integer data: b differs in the last element only; a entirely negative; a == b."""
    a = red_data(n, 1).astype(np.float32)
    if kind == "negative":
        a = -np.abs(a)
        b = a.copy()
        b[::3] += 1.0
        return a, b
    b = a.copy()
    if kind == "last":
        b[-1] += 3.0
    return a, b


def psnr_expected(a, b):
    return float(om.compute_psnr(*f64(a, b)))


def close(got, want, bar):
    """NaN exactly where the expectation is NaN, within ``bar`` elsewhere; returns the largest error over the bar."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where a number is due, or a number where NaN is due"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
    assert err <= bar, f"|got - want| = {err:.3g} > {bar:.3g}"
    return err / bar
