"""tests/stream_cases.py on the CPU: for every family a NumPy model of the faults a streaming kernel or a metric kernel
can have is applied to the case data, and the bar of tests/test_gpu_stream_exact.py / tests/test_gpu_metrics_edges.py
must reject it on every case the GPU tests use (where the fault changes what the kernel reads or computes at all: a
fault that is no fault on a case, such as a dropped partial block of a tensor that has none, is skipped there and must
apply somewhere).  A case its fault survives is repaired here, not on the GPU."""
from fractions import Fraction

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import stream_cases as sc
from oracle import filetools as oft
from oracle import metrics as om


def _same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))


def _triple_of(x):
    """What a reduction returns that read only ``x``: the seeds for nothing."""
    return sc.triple(x) if len(x) else (np.inf, -np.inf, 0.0)


# ----------------------------------------------------------------------------- reductions
def _reduction_faults(n, grid):
    """name -> boolean mask of the elements the faulty kernel still reads (None: the fault changes nothing here)."""
    i = np.arange(n)
    block = i // sc.BLOCK
    out = {"last element dropped": i < n - 1,
           "last partial block dropped": block < (n - 1) // sc.BLOCK if n % sc.BLOCK else None,
           "second trip dropped": block < grid if n > grid * sc.BLOCK else None}
    return out


def test_integer_data_is_what_the_bars_assume():
    for n, turn in sc.RED_CASES:
        x = sc.red_data(n, turn).astype(np.int64)
        lo, hi, ss = sc.triple(x)
        assert np.all(x != 0) and np.abs(x).max() <= 64 and ss < 2.0 ** 53
        assert np.count_nonzero(x == lo) == 1 and (n == 1 or np.count_nonzero(x == hi) == 1)
        c = sc.planted(n, sc.red_grid(n))
        assert int(np.argmin(x)) == c[turn % len(c)] and (n == 1 or int(np.argmax(x)) == c[(turn + 1) % len(c)])
        # fp32 holds every value, fp64 every partial sum of squares: the same bits in every order
        assert np.array_equal(x.astype(np.float32).astype(np.int64), x)
    # every planted position is used as the minimum and as the maximum at the three lengths that take all turns
    for n in sc.RED_ALL_TURNS:
        c = sc.planted(n, sc.red_grid(n))
        assert len(c) == 5 and c[4] == sc.red_grid(n) * sc.BLOCK
        assert {int(np.argmin(sc.red_data(n, t))) for t in range(5)} == set(c)


def test_reduction_bars_reject_dropped_elements():
    applied = set()
    for n, turn in sc.RED_CASES:
        x = sc.red_data(n, turn)
        want = sc.triple(x)
        for name, keep in _reduction_faults(n, sc.red_grid(n)).items():
            if keep is None:
                continue
            applied.add(name)
            got = _triple_of(x[keep])
            assert got[2] != want[2], (n, turn, name)          # the sum of squares alone tells
    assert applied == {"last element dropped", "last partial block dropped", "second trip dropped"}
    # the planted extremes tell too, wherever the fault drops one of them
    x = sc.red_data(3000, 0)
    assert _triple_of(x[:-1])[1] != sc.triple(x)[1]


def _many_faults(n):
    i = np.arange(n)
    block = i // sc.BLOCK
    out = _reduction_faults(n, sc.SLICES)
    for s in range(sc.SLICES):
        out[f"slice {s} skipped"] = (block % sc.SLICES != s) if n > s * sc.BLOCK else None
    return out


def test_many_bars_reject_dropped_elements_slices_and_chunks():
    applied = set()
    for count in sc.MANY_COUNTS:
        xs, want = sc.many_case(count)
        assert want.shape == (count, 3) and sorted(set(sc.many_lengths(count))) == sorted(set(len(x) for x in xs))
        for x, w in zip(xs, want):
            for name, keep in _many_faults(len(x)).items():
                if keep is None:
                    continue
                applied.add(name)
                assert not _same(_triple_of(x[keep]), w), (count, len(x), name)
        # a chunk of 32 pointers that was not uploaded: its tensors read as empty
        for base in range(0, count, sc.CHUNK):
            got = want.copy()
            got[base:base + sc.CHUNK] = _triple_of(xs[0][:0])
            assert not _same(got, want)
    assert applied >= {f"slice {s} skipped" for s in range(sc.SLICES)}
    assert {len(x) for c in sc.MANY_COUNTS for x in sc.many_case(c)[0]} == set(sc.SLICE_LENGTHS)
    # the spike rows: every row (0, 3, 9); a lost element p, a lost slice or a lost chunk zeroes a row's maximum
    assert -(-sc.SPIKE // sc.CHUNK) == 129 and sc.SPIKE > 128 * sc.CHUNK      # 128 full chunks and a 129th of 4
    assert sc.SPIKE > sc.SLICES * sc.BLOCK                                     # a second trip of slice 0
    row = np.zeros(sc.SPIKE, dtype=np.float32)
    row[sc.SPIKE - 1] = 3.0
    assert _triple_of(row.astype(np.int64)) == (0.0, 3.0, 9.0) and _triple_of(row[:-1].astype(np.int64)) != (0.0, 3.0, 9.0)


def test_arena_bars_reject_shifted_offsets_and_the_neighbouring_row():
    for batch, n_cores in sc.ARENA_CASES:
        arena, offsets, lens, stride, want = sc.arena_case(batch, n_cores)
        assert want.shape == (batch * n_cores, 3) and arena.shape == (batch, stride)
        assert stride > offsets[-1] + lens[-1] and any(o % 2 for o in offsets) and offsets[0] >= 1
        assert all(offsets[i] + lens[i] < offsets[i + 1] for i in range(n_cores - 1))      # gaps
        inside = np.zeros(stride, dtype=bool)
        for o, n in zip(offsets, lens):
            inside[o:o + n] = True
        assert np.all(np.abs(arena[:, ~inside]) == np.float32(sc.ARENA_FILL)) and np.all(np.abs(arena[:, inside]) <= 64)

        def read(shift=0, row=0):
            out = []
            for b in range(batch):
                for o, n in zip(offsets, lens):
                    x = arena[(b + row) % batch, o + shift:o + shift + n].astype(np.float64)
                    out.append((x.min(), x.max(), float(np.dot(x, x))))
            return np.array(out)

        assert _same(read(), want)
        for shift in (-1, 1):
            got = read(shift=shift)
            assert np.all(np.any(got != want, axis=1)), (batch, n_cores, shift)      # every tensor tells
        if batch > 1:
            for row in (-1, 1):
                assert np.all(np.any(read(row=row) != want, axis=1)), (batch, n_cores, row)
    for name, batch, n_cores, offsets, lens, stride in sc.arena_refusals():
        bad = (n_cores > sc.ARENA_CORES or batch * n_cores > 65535 or offsets is None or lens is None
               or any(n <= 0 or o + n > stride for o, n in zip(offsets, lens)))
        assert bad, name


# ----------------------------------------------------------------------------- scale
def _toward_zero(y64, dt):
    """fp64 -> dt with a truncating cast."""
    y = y64.astype(dt)
    over = np.abs(y.astype(np.float64)) > np.abs(y64)
    return np.where(over, np.nextafter(y, dt(0)), y)


def test_scale_bar_rejects_a_truncating_cast_and_fp32_arithmetic():
    third = 1.0 / 3.0
    first, last = np.array([sc.SCALE_FIRST]), np.array([sc.SCALE_LAST])
    assert not np.array_equal(_toward_zero(first.astype(np.float64) * third, np.float32), sc.scale_expected(first, third))
    assert not np.array_equal(last * np.float32(third), sc.scale_expected(last, third))
    alone = sc.scale_factors(first)[1]
    assert not np.array_equal(first * np.float32(alone), sc.scale_expected(first, alone))
    for n in sc.STREAM_LENGTHS:
        x = sc.scale_data(n)
        assert x[0] == sc.SCALE_FIRST and (n == 1 or x[-1] == sc.SCALE_LAST)
        f3, fn, fq = sc.scale_factors(x)
        assert (f3, fq) == (third, -0.25)
        # -0.25 is a power of two: exact in every arithmetic, it checks the sign and the indexing, not the rounding
        assert np.array_equal(x * np.float32(fq), sc.scale_expected(x, fq))
        for f in (f3, fn):
            want = sc.scale_expected(x, f)
            if n > 1 or f == f3:      # n = 1: x / |x| is 1, which no cast changes
                assert not np.array_equal(_toward_zero(x.astype(np.float64) * f, np.float32), want), (n, f)
            if n > 1 or f == fn:      # n = 1: SCALE_FIRST tells fp32 arithmetic by the norm factor only
                assert not np.array_equal(x * np.float32(f), want), (n, f)
            # a kernel that stops one element short leaves the last one unscaled
            assert want[-1] != x[-1] and want[0] != x[0]
    for count, n in ((33, 1), (65, 257)):
        x, f = sc.scale_many_case(count, n)
        want = sc.scale_many_expected(x, f)
        assert len(set(f)) == count
        assert not np.array_equal((x * f.astype(np.float32)[:, None]).astype(np.float32), want)
        # tensor t scaled by the factor of tensor t + 1 (a chunk of 32 read from the wrong base): every row tells
        assert np.all(np.any(sc.scale_many_expected(x, np.roll(f, 1)) != want, axis=1))


# ----------------------------------------------------------------------------- quantiser
def _codes(x, lo, hi, bits, rounding):
    u = (x.astype(np.float64) - lo) / (hi - lo) * (2 ** bits - 1)
    return (np.rint(u) if rounding else np.trunc(u)).astype(sc.QDT[bits])


@pytest.mark.parametrize("r,bits,elem", sc.QUANT_CASES)
def test_quantiser_cases_reject_a_rounding_cast(r, bits, elem):
    x, lo, hi, want = sc.quant_case(r, bits, elem)
    assert x.dtype == sc.FDT[elem] and want.dtype == sc.QDT[bits] and len(x) == 3 * 2 ** bits + 2
    assert want[0] == 0 and want[-1] == 2 ** bits - 1 and len(np.unique(want)) > 0.9 * 2 ** bits
    assert np.array_equal(_codes(x, lo, hi, bits, rounding=False), want)       # the model is the oracle
    wrong = _codes(x, lo, hi, bits, rounding=True) != want
    assert wrong.mean() > 0.2, "a rounding cast must be wrong next to most codes"
    # fp32 arithmetic in the kernel where fp64 is due
    u32 = ((x.astype(np.float32) - np.float32(lo)) / np.float32(hi - lo) * np.float32(2 ** bits - 1)).astype(sc.QDT[bits])
    assert r == 1 or not np.array_equal(u32, want)      # lo = 0, span = 1: only the product with qmax rounds


def test_quantiser_large_and_constant_cases():
    for elem in ("f32", "f64"):
        x, lo, hi = sc.quant_large(elem)
        assert len(x) > 2 * sc.STREAM_BLOCKS * sc.BLOCK and x.dtype == sc.FDT[elem]
        for bits in (8, 16):
            want = sc.quant_large_expected(x, bits)
            assert np.array_equal(_codes(x, lo, hi, bits, rounding=False), want)
            assert not np.array_equal(_codes(x, lo, hi, bits, rounding=True), want)
            assert want[-1] != 0 or want[-2] != 0                    # a tail that was not written shows
            # span = 0: no rounding happens, only 0 / 0 -> NaN -> code 0; what the oracle yields
            assert not sc.oracle_constant_codes(sc.quant_constant(elem), bits).any()


@pytest.mark.parametrize("elem", ["f32", "f64"])
@pytest.mark.parametrize("bits", [8, 16])
def test_quantiser_at_the_stream_lengths_tells_a_dropped_tail(bits, elem):
    """quantise and dequantise have loops of their own over stream_grid: at every length a kernel that stops an
    element, a block or a grid-stride trip short leaves what the output buffer held, which the expectation is not."""
    qmax, fill = 2 ** bits - 1, sc.QFILL[bits]
    for n in sc.STREAM_LENGTHS:
        x, lo, hi, codes, back = sc.quant_stream_case(n, bits, elem)
        assert len(x) == len(codes) == len(back) == n and x.dtype == back.dtype == sc.FDT[elem]
        assert lo <= x.min() and x.max() <= hi
        assert np.array_equal(_codes(x, lo, hi, bits, rounding=False), codes)      # the oracle's codes, element by element
        assert np.array_equal(back, ((codes / qmax) * (hi - lo) + lo).astype(sc.FDT[elem]))
        assert n < 255 or not np.array_equal(_codes(x, lo, hi, bits, rounding=True), codes)
        tails = [n - 1, (n - 1) // sc.BLOCK * sc.BLOCK]                            # last element, last block
        if n > sc.STREAM_BLOCKS * sc.BLOCK:
            tails.append(sc.STREAM_BLOCKS * sc.BLOCK)                              # second trip
        for first in tails:
            assert np.any(codes[first:] != fill) and np.all(back[first:] != sc.SENTINEL), (n, first)
        assert codes[-1] != fill


def _fma_dequant(code, lo, hi, qmax):
    """(code / qmax) * span + lo with one rounding after the sum, through exact fractions."""
    unit = float(code) / qmax
    return float(Fraction(unit) * Fraction(hi - lo) + Fraction(lo))


@pytest.mark.parametrize("bits", [8, 16])
def test_dequantiser_bar_rejects_an_fma(bits):
    qmax = 2 ** bits - 1
    told = set()
    for r in range(len(sc.QRANGES)):
        codes, lo, hi, want = sc.dequant_case(r, bits, "f64")
        assert np.array_equal(want, (codes / qmax) * (hi - lo) + lo) and want[0] == lo
        pick = range(0, qmax + 1, max(1, qmax // 255))      # a handful of codes: 256 of them
        if any(_fma_dequant(codes[k], lo, hi, qmax) != want[k] for k in pick):
            told.add(r)
        c32, lo32, hi32, w32 = sc.dequant_case(r, bits, "f32")
        assert w32.dtype == np.float32 and np.array_equal(w32, oft.scale_back(c32, lo32, hi32, sc.QDT[bits]).astype(np.float32))
        # a dequantiser in fp32 arithmetic
        wrong = (c32.astype(np.float32) / np.float32(qmax)) * np.float32(hi32 - lo32) + np.float32(lo32)
        assert r == 1 or not np.array_equal(wrong, w32), (r, bits)
    # lo = 0, span = 1 leaves the sum nothing to round; the two other ranges tell an FMA from two roundings
    assert told == {0, 2}


# ----------------------------------------------------------------------------- infinities
def test_infinity_cases_tell_a_finite_seed():
    flt_max = float(np.finfo(np.float32).max)
    for n, kind in sc.NONFINITE_CASES:
        x = sc.nonfinite_data(n, kind)
        assert x.dtype == np.float32 and not np.isnan(x).any() and np.isinf(x).any()
        seeded = (min(flt_max, float(x.min())), max(-flt_max, float(x.max())))
        if kind.startswith("all"):
            assert seeded != (float(x.min()), float(x.max())), (n, kind)
    assert {k for _, k in sc.NONFINITE_CASES} == set(sc.NONFINITE_KINDS)


# ----------------------------------------------------------------------------- DCT
def _model_dct(x, fft_fault=None, post_fault=None):
    """Makhoul's DCT-II through an N-point radix-2 FFT with explicit twiddle tables, in fp64.  ``fft_fault = j`` reads
    entry j + 1 of the FFT's table where j is due, ``post_fault = k`` the same in the post-twiddle table."""
    n = x.shape[-1]
    tw = np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n)
    wq = np.exp(-1j * np.pi * np.arange(n + 1) / (2 * n))
    if fft_fault is not None:
        tw[fft_fault] = tw[fft_fault + 1]
    if post_fault is not None:
        wq[post_fault] = wq[post_fault + 1]
    v = np.concatenate([x[..., ::2], x[..., ::-1][..., ::2]], axis=-1).astype(np.complex128)
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])
    a = v[..., rev]
    m = 2
    while m <= n:
        half = m // 2
        a = a.reshape(x.shape[:-1] + (n // m, m))
        odd = a[..., half:] * tw[np.arange(half) * (n // m)]
        a = np.concatenate([a[..., :half] + odd, a[..., :half] - odd], axis=-1).reshape(x.shape)
        m *= 2
    s = np.full(n, np.sqrt(2.0 / n))
    s[0] = np.sqrt(1.0 / n)
    return (a * wq[:n]).real * s


@pytest.mark.parametrize("n", sc.DCT_N)
def test_dct_bar_sits_between_fp32_rounding_and_a_wrong_twiddle(n):
    from scipy.fft import dct

    want = sc.dct_matrix(n)
    bar = sc.dct_bar(n)
    assert np.abs(want).max() <= np.sqrt(2.0 / n) * (1 + 1e-15)
    # SciPy's own float32 transform of the same impulses: the bar is at least 4 times its error (about 15 times here:
    # n = 64: 3.3e-8 against 5.1e-7, n = 1024: 1.5e-8 against 1.7e-7), and at most 1e-4 of an entry's scale
    err32 = np.abs(dct(np.eye(n, dtype=np.float32), type=2, norm="ortho", axis=-1).astype(np.float64) - want).max()
    print(f"n = {n}: fp32 pocketfft error {err32:.3g}, bar {bar:.3g}")
    assert 4 * err32 <= bar <= 1e-4 * np.sqrt(2.0 / n)
    eye = np.eye(n)
    assert np.abs(_model_dct(eye) - want).max() <= 1e-14
    for fault in (dict(fft_fault=1), dict(fft_fault=n // 4), dict(post_fault=1), dict(post_fault=n - 2)):
        assert np.abs(_model_dct(eye, **fault) - want).max() > 100 * bar, fault
    # the inverse: the fp32-rounded matrix times its transpose is the identity far inside the bar, a wrong twiddle is not
    w32 = want.astype(np.float32).astype(np.float64)
    assert np.abs(w32 @ want.T - eye).max() <= 0.1 * sc.idct_bar(n)
    assert np.abs(_model_dct(eye, fft_fault=1) @ want.T - eye).max() > 4 * sc.idct_bar(n)
    assert sc.DCT_VOLS > sc.CHUNK


# ----------------------------------------------------------------------------- SSIM and PSNR
def _win_for(h, w):
    win = min(7, h, w)
    return win - 1 if win % 2 == 0 else win


def _model_ssim_2d(a, b, win=None, clip=True, sample=True, drop=None):
    """The kernel's arithmetic on one slice: box sums over win x win windows, one tile of 16 x 32 window centres per
    workgroup.  ``drop``: the last row ("row") or column ("col") of the first tile is left out of the sum."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    if clip:
        b = np.clip(b, 0, None)
    rng = max(a.max(), b.max()) - min(a.min(), b.min())
    w = win or _win_for(*a.shape)
    wa, wb = sliding_window_view(a, (w, w)), sliding_window_view(b, (w, w))
    npix = w * w
    norm = npix / (npix - 1.0) if sample else 1.0
    ux, uy = wa.mean(axis=(2, 3)), wb.mean(axis=(2, 3))
    vx = norm * ((wa * wa).mean(axis=(2, 3)) - ux * ux)
    vy = norm * ((wb * wb).mean(axis=(2, 3)) - uy * uy)
    vxy = norm * ((wa * wb).mean(axis=(2, 3)) - ux * uy)
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    th, tw = min(16, s.shape[0]), min(32, s.shape[1])
    if drop == "row":
        s[th - 1, :tw] = 0.0
    if drop == "col":
        s[:th, tw - 1] = 0.0
    return s.sum() / s.size


def _model_ssim(a, b, one_window=False, shrink=False, **kw):
    """The window faults.  The issue's "window 7 where 5 is due" cannot be evaluated inside a slice: a window below 7
    is due exactly where an extent is below 7, so the larger window does not fit the slice it is wrong for (a kernel
    doing that reads past the slice).  What a kernel can get wrong in bounds is modelled instead: ``one_window`` takes
    one window for all three orientations of a volume, that of its smallest extent (5 where 7 is due; no fault, and
    asserted to be none, on volumes whose orientations share a window), and ``shrink`` takes the next smaller odd
    window on every slice (5 where 7 is due, 3 where 5 is; not applicable where 3 is due)."""
    if a.ndim == 2:
        win = _win_for(*a.shape) - 2 if shrink else None
        return _model_ssim_2d(a, b, win=win, **kw)
    if a.ndim == 4:
        return np.mean([_model_ssim(a[..., t], b[..., t], one_window=one_window, shrink=shrink, **kw)
                        for t in range(a.shape[3])])
    total = []
    for ax in range(3):
        h, w = [s for j, s in enumerate(a.shape) if j != ax]
        win = _win_for(min(a.shape), min(a.shape)) if one_window else _win_for(h, w) - 2 if shrink else None
        total.append(np.mean([_model_ssim_2d(np.take(a, i, axis=ax), np.take(b, i, axis=ax), win=win, **kw)
                              for i in range(a.shape[ax])]))
    return np.mean(total)


@pytest.mark.parametrize("shape", sc.SSIM_SHAPES)
def test_ssim_bar_rejects_the_faults_of_a_tile_kernel(shape):
    a, b = sc.ssim_pair(shape)
    want = sc.ssim_expected(shape)
    assert a.dtype == b.dtype == np.float32 and b.min() < 0 and 0 <= a.min() and a.max() < 1
    assert abs(_model_ssim(a, b) - want) <= 0.01 * sc.SSIM_BAR          # the model is the oracle
    for fault in (dict(clip=False), dict(sample=False), dict(drop="row"), dict(drop="col")):
        assert abs(_model_ssim(a, b, **fault) - want) > 1e6 * sc.SSIM_BAR, fault
    if min(shape[:3] if len(shape) >= 3 else shape) >= 5:      # every slice's window is at least 5: a smaller one fits
        assert abs(_model_ssim(a, b, shrink=True) - want) > 1e6 * sc.SSIM_BAR
    if len(shape) >= 3:
        wins = {_win_for(*[s for j, s in enumerate(shape[:3]) if j != ax]) for ax in range(3)}
        if len(wins) > 1:      # one window for all three orientations: 5 where 7 is due
            assert abs(_model_ssim(a, b, one_window=True) - want) > 1e6 * sc.SSIM_BAR
        else:
            assert abs(_model_ssim(a, b, one_window=True) - want) <= 0.01 * sc.SSIM_BAR
    if len(shape) == 3:
        for ax in range(3):
            got = sc.ssim_slices_expected(shape, ax)
            assert got.shape == (shape[ax],) and not np.isnan(got).any()
        # the volume's value is the mean of the three lists' means
        assert abs(np.mean([sc.ssim_slices_expected(shape, ax).mean() for ax in range(3)]) - want) <= 0.01 * sc.SSIM_BAR


def test_ssim_shapes_sit_on_the_edges_they_are_named_for():
    centre = {s: (s[0] - _win_for(*s) + 1, s[1] - _win_for(*s) + 1) for s in sc.SSIM_2D}
    assert centre[(22, 38)] == (16, 32) and centre[(23, 39)] == (17, 33)            # one tile; one past it
    assert centre[(38, 71)] == (32, 65) and centre[(39, 72)] == (33, 66)
    assert centre[(3, 3)] == (1, 1) and _win_for(4, 9) == 3 and _win_for(8, 70) == 7
    wins = [_win_for(*[s for j, s in enumerate((40, 5, 33)) if j != ax]) for ax in range(3)]
    assert wins == [5, 7, 5]


def test_ssim_chunk_and_constant_cases():
    a, b, want = sc.ssim_chunk_4d()
    assert a.shape == (8, 8, 8, 8200) and a.shape[0] * a.shape[3] > 65535
    assert np.array_equal(a[..., 41 * 7 + 3], a[..., 3]) and not np.array_equal(a[..., 0], a[..., 1])
    # the same mean: every frame 200 times
    assert abs(np.mean(np.tile([_model_ssim(a[..., t], b[..., t]) for t in range(41)], 200)) - want) <= 0.01 * sc.SSIM_BAR
    a3, b3, lst = sc.ssim_chunk_3d()
    assert a3.shape == (65600, 8, 8) and lst.shape == (65600,) and np.array_equal(a3[41 * 5 + 2], a3[2])
    assert len(set(lst[:41])) == 41
    # a launch that ignored its slice offset, or an index that wrapped at 65535, leaves the tail unwritten or repeats
    # the head: both tell
    got = lst.copy()
    got[65535:] = 0.0
    assert np.abs(got - lst).max() > 1e6 * sc.SSIM_BAR
    got = lst.copy()
    got[65535:] = lst[:65]
    assert np.abs(got - lst).max() > 1e6 * sc.SSIM_BAR       # 65535 is no multiple of 41
    ac, bc, per_slice, volume = sc.ssim_constant()
    assert not ac[0].any() and np.all(bc[0] == -1) and ac.shape == (12, 20, 16)
    assert np.isnan(per_slice[0]) and not np.isnan(per_slice[1:]).any() and np.isnan(volume)
    with pytest.raises(AssertionError):
        sc.close(np.nan_to_num(per_slice), per_slice, sc.SSIM_BAR)
    sc.close(per_slice, per_slice, sc.SSIM_BAR)


def test_psnr_cases_reject_a_dropped_element_and_a_wrong_maximum():
    for n, _ in sc.RED_CASES[:len(sc.RED_LENGTHS)]:
        a, b = sc.psnr_pair(n, "equal")
        assert sc.psnr_expected(a, b) == np.inf
        a, b = sc.psnr_pair(n, "last")
        want = sc.psnr_expected(a, b)
        assert np.isfinite(want) and np.count_nonzero(a != b) == 1
        assert n == 1 or om.compute_psnr(*sc.f64(a[:-1], b[:-1])) == np.inf    # the last element dropped
        a, b = sc.psnr_pair(n, "negative")
        want = sc.psnr_expected(a, b)
        assert a.max() < 0 and np.isfinite(want)
        # a maximum that starts from 0 instead of the smallest value
        wrong = 10 * np.log10(max(0.0, float(a.max())) ** 2 / np.mean((a.astype(np.float64) - b) ** 2) + 1e-300)
        assert abs(wrong - want) > sc.PSNR_REL * abs(want)
        if n > 2:      # max |a| where max a is due (n = 2: both elements are -33)
            wrong = 10 * np.log10(float(np.abs(a).max()) ** 2 / np.mean((a.astype(np.float64) - b) ** 2))
            assert abs(wrong - want) > sc.PSNR_REL * abs(want)
