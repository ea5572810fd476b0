"""The bars of tests/dct_decode_cases.py checked on the CPU, before any kernel is held to them.

* sound: a NumPy / SciPy restatement of the two stages in the work type -- the chain contracted right to left in
  float32 (float64 for fp64 storage; bf16 intermediates for ``to_tensor`` of bf16 cores), then ``scipy.fft.idct`` on
  float32 where the device takes the FFT, a matmul with the rounded basis elsewhere, a matmul with the kernel's pooled
  basis for a partial reduction, fp64 site sums for the rest -- stays within a quarter of every bar, on every case
  the GPU test uses;
* teeth: seven deliberate mistakes in that restatement each put an element outside the bar they are aimed at;
* the kernel's formula for the pooled basis, evaluated in float64 on the CPU, stays within a quarter of the basis bar;
* SciPy's float32 ``idct`` stays below 0.03 of the FFT term and a float32 matmul with the rounded basis below 0.23 of
  the product term (the ratios the bars were chosen with).

The relative Frobenius change that fault 1 makes on a smooth, library-encoded volume is printed, not asserted.
"""
import functools

import numpy as np
import pytest
from scipy.fft import idct

import dct_decode_cases as dc
from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle import index_map as im
from oracle.metrics import synthetic_mri
from oracle.ndmps_oracle import OracleNDMPS

MARGIN = 4.0
CASES = [(s, f, t) for s in dc.SHAPES for f in dc.FAMILIES for t in dc.STORAGES]
CASE_IDS = [f"{'x'.join(map(str, s))}-{f}-{t}" for s, f, t in CASES]
F32_UNIFORM = [(s, "uniform", "f32") for s in dc.SHAPES]


# ------------------------------------------------------------------------------------------------ restatement
def restate_y(cs, call):
    """The coefficient tensor as the device forms it for ``call`` ("to_tensor" / "wide"), in volume order."""
    bf16_chain = cs.storage == "bf16" and call == "to_tensor"
    dt = np.float64 if cs.storage == "f64" else np.float32
    store = (lambda a: cc.round_bf16(a)) if bf16_chain else (lambda a: a)
    t = np.ones((1, 1), dtype=dt)
    for c in reversed(cs.cores):  # right to left: another association than the reference's
        chi_l, d, chi_r = c.shape
        t = store(c.astype(dt).reshape(chi_l * d, chi_r) @ t.reshape(chi_r, -1)).reshape(chi_l, -1)
        assert t.dtype == dt
    dest = im.flat_destination(cs.shape).reshape(-1)
    return cb.to_volume(t.reshape(-1), dest).reshape(cs.shape)


@functools.lru_cache(maxsize=None)
def _model_basis(n):
    c = np.ascontiguousarray(dc.kernel_model_basis(n, 1, 1.0, False).T)
    assert np.allclose(c, dc.basis(n), rtol=0, atol=1e-14)
    c.setflags(write=False)
    return c


def rounded_basis(n, work, dc_scale=None):
    """The basis as the device holds it: the formula of dct_basis_kernel (csrc/reduce.hip) evaluated in float64 --
    the pooled basis with blocks of one row -- and rounded to the work type.  ``dc_scale``: fault 2, s_0 taken as s_k."""
    c = np.array(_model_basis(n))
    if dc_scale:
        c[0] *= dc_scale
    return c.astype(np.float32 if work == "f32" else np.float64)


def transform(y, work, drop_last=False, dc_wrong=False):
    """Stage two on rows ``y`` in the work type: float32 FFT (scipy) or a matmul with the rounded basis."""
    n = y.shape[-1]
    y = np.array(y, dtype=np.float32 if work == "f32" else np.float64)
    if drop_last:
        y[..., n - 1] = 0                      # fault 1
    if dc.fft_route(n, work):
        if dc_wrong:
            y[..., 0] *= np.float32(np.sqrt(2.0))
        out = idct(y, type=2, norm="ortho", axis=-1)
    else:
        out = y @ rounded_basis(n, work, np.sqrt(2.0) if dc_wrong else None)
    assert out.dtype == y.dtype
    return out


def ratio(got, ref, bar):
    got, ref, bar = (np.asarray(a, dtype=np.float64) for a in (got, ref, bar))
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    err = np.abs(got - ref)
    assert np.all(err[bar == 0] == 0)
    pos = bar > 0
    return float(np.max(err[pos] / bar[pos])) if pos.any() else 0.0


def restate_pooled(cs, levels, op, pick_weight=None, first=0, transposed=False):
    """``downsample(levels, op)`` restated: fp64 block sums of the work-type coefficient tensor over the other axes
    (the device sums on the cores in fp64), then the transform, the pooled-basis product or the pick."""
    shape, n = cs.shape, cs.n
    L = dc.factor_array(shape).shape[0]
    lev = dc.normalize_levels(shape, levels)
    blocks = dc.block_shape(shape, lev)
    work = dc.work_of(cs.storage)
    dt = np.float32 if work == "f32" else np.float64
    y_r = dc.block_reduce(restate_y(cs, "wide"), blocks[:-1] + (1,), op).astype(dt)
    if lev[-1] == L:
        w = pick_weight if pick_weight is not None else (1.0 / np.sqrt(n) if op == "mean" else np.sqrt(float(n)))
        return (w * y_r[..., :1].astype(np.float64)).astype(dt)
    if lev[-1] == 0:
        return transform(y_r, work)
    Bk = blocks[-1]
    W = dc.kernel_model_basis(n, Bk, 1.0 / Bk if op == "mean" else 1.0, work == "f32", first=first).astype(dt)
    Wt = W.reshape(n, n // Bk) if transposed else W.T  # fault 7: the (n / Bk, n) buffer read as (n, n / Bk)
    return y_r @ Wt


# ------------------------------------------------------------------------------------------------ the cases
def test_shapes_have_the_sites_factors_and_routes_of_the_table():
    for shape, (L, factors, n, route) in dc.TABLE.items():
        fa = dc.factor_array(shape)
        assert fa.shape[0] == L and tuple(int(v) for v in fa[:, -1]) == factors and shape[-1] == n
        assert dc.fft_route(n, "f32") == (route == "fft") and not dc.fft_route(n, "f64")
        assert max(dc.capped_bonds(shape)) <= dc.MAX_BOND
    assert max(int(np.prod(s)) for s in dc.SHAPES) == 348160
    for n, Bk in dc.BASIS_CASES:
        assert n % Bk == 0


def test_reference_transform_is_the_orthonormal_inverse_dct():
    for n in (20, 64):
        c = dc.basis(n)
        assert np.allclose(c @ c.T, np.eye(n), atol=1e-14)
        k, m = np.arange(n)[:, None], np.arange(n)[None, :]
        want = np.where(k == 0, np.sqrt(1 / n), np.sqrt(2 / n)) * np.cos(np.pi * (2 * m + 1) * k / (2 * n))
        assert np.allclose(c, want, atol=1e-14)
        assert np.allclose(c.sum(axis=1), np.sqrt(n) * (np.arange(n) == 0), atol=1e-13)


@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_restated_decode_is_within_a_quarter_of_the_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    for c in cs.cores:
        assert np.array_equal(cc.to_storage(c, storage), c)
    work = dc.work_of(storage)
    worst = {}
    for call in ("to_tensor", "wide"):
        y = restate_y(cs, call)
        if cs.factor(call) == 0.0:
            assert family == "integer" and np.array_equal(y.astype(np.float64), cs.y)  # stage 1 is exact
        worst[call] = ratio(transform(y, work), cs.x, cs.decode_bar(call))
    print(f"[dct-host] {cs.label}: error / bar  to_tensor {worst['to_tensor']:.3f}  region {worst['wide']:.3f}")
    assert max(worst.values()) <= 1 / MARGIN, worst


@pytest.mark.parametrize("cap", [7, 9])
@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_restated_series_frames_are_within_a_quarter_of_the_bar(shape, family, storage, cap):
    """The frames of the GPU test's series: bonds capped at 7 and 9, other draws."""
    cs = dc.case(shape, family, storage, bonds=tuple(dc.capped_bonds(shape, cap)), salt=3 + cap)
    assert max(cs.bonds) == cap
    y = restate_y(cs, "wide")
    assert ratio(transform(y, dc.work_of(storage)), cs.x, cs.decode_bar("wide")) <= 1 / MARGIN
    # in a series with an fp64 frame the cores are widened exactly and both stages run in fp64
    # in a series with an fp64 frame the cores are widened exactly and both stages run in fp64.  At fp64 and small n
    # the float64 reference's own rounding is of the size of what the margin measures (0.12 of the bar at n = 20 on
    # integer cores, against 0.2 for the product): each is measured against the transform formed in extended
    # precision, and the product is still inside the bar against the float64 reference itself
    wide = dc.case(shape, family, "f64", bonds=tuple(cs.bonds), salt=3 + cap)  # any fp64 chain restates that stage
    for c, y in ((wide, restate_y(wide, "wide")), (cs, cs.y)):
        got, bar = y @ rounded_basis(cs.n, "f64"), c.decode_bar("f64")
        assert ratio(got, c.x, bar) <= 1.0
        truth = _extended_x(c)
        assert ratio(got, truth, bar) <= 1 / MARGIN and ratio(c.x, truth, bar) <= 1 / MARGIN


def _extended_x(cs):
    """``y C`` in extended precision for n <= 32 (where long double is wider than double), else the reference."""
    if cs.n > 32 or np.finfo(np.longdouble).nmant < 63:
        return cs.x
    C = dc.pooled_basis(cs.n, 1, 1.0).T.astype(np.longdouble)  # blocks of one row: the basis itself, (k, m)
    return np.asarray(cs.y.astype(np.longdouble) @ C, dtype=np.float64)


@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_restated_pooled_decode_is_within_a_quarter_of_the_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    worst = {"pooled": 0.0, "pick": 0.0}
    levels = dc.level_list(shape) + [dc.axis_levels(shape, a) for a in dc.axis_list(shape)]
    for lev in levels:
        for op in ("mean", "sum"):
            kind, ref, bar = dc.pooled(cs, lev, op)
            r = ratio(restate_pooled(cs, lev, op), ref, bar)
            if kind == "pick" and family == "integer" and ref.size == 1:
                assert r <= 1.0, (lev, op, r)  # the bar IS one rounding into the result type: no margin to ask for
                continue
            assert r <= 1 / MARGIN, (lev, op, kind, r)
            worst[kind] = max(worst[kind], r)
    print(f"[dct-host] {cs.label}: error / bar  pooled {worst['pooled']:.3f}  pick {worst['pick']:.3f}")


@pytest.mark.parametrize("n,Bk", dc.BASIS_CASES)
def test_kernel_formula_of_the_pooled_basis_is_within_a_quarter_of_its_bar(n, Bk):
    for w in (1.0, 1.0 / Bk):
        W = dc.pooled_basis(n, Bk, w)
        wt, _ = dc.pooled_weights(n, Bk, w)
        assert np.allclose(W, wt.T, rtol=0, atol=1e-13 * Bk * w)  # the same matrix as the SciPy basis, block-summed
        bar64 = dc.basis_bar(n, Bk, w, False)
        for f32 in (False, True):
            # the fp32 kernel's one rounding of the result has no margin to ask for: the factor is on the fp64 part
            bar = bar64 + MARGIN * (dc.basis_bar(n, Bk, w, True) - bar64) if f32 else bar64
            r = ratio(dc.kernel_model_basis(n, Bk, w, f32), W, bar)
            print(f"[dct-host] pooled basis n={n} Bk={Bk} w={w:.4g} {'f32' if f32 else 'f64'}: error / bar {r:.3f}")
            assert r <= 1 / MARGIN, (n, Bk, w, f32, r)


def test_float32_transforms_reproduce_the_ratios_the_bars_were_chosen_with():
    rng = np.random.default_rng(11)
    for n in (64, 128, 256, 512, 1024):
        y32 = rng.uniform(-1, 1, (64, n)).astype(np.float32)
        y64 = y32.astype(np.float64)
        r = ratio(idct(y32, norm="ortho", axis=-1), idct(y64, norm="ortho", axis=-1), dc.transform_term(y64, "f32"))
        print(f"[dct-host] float32 FFT n={n}: error / FFT term {r:.4f}")
        assert dc.fft_route(n, "f32") and r < 0.03
    for n in (9, 20, 32, 100, 333, 680):
        y = rng.uniform(-1, 1, (64, n)).astype(np.float32)
        got = y @ rounded_basis(n, "f32")
        r = ratio(got, y.astype(np.float64) @ dc.basis(n), dc.transform_term(y.astype(np.float64), "f32"))
        print(f"[dct-host] float32 basis product n={n}: error / product term {r:.4f}")
        assert not dc.fft_route(n, "f32") and r < 0.23


# ------------------------------------------------------------------------------------------------ teeth
def _outside(got, ref, bar):
    got, ref, bar = (np.asarray(a, dtype=np.float64) for a in (got, ref, bar))
    assert got.shape == ref.shape == bar.shape
    return int(np.count_nonzero(np.abs(got - ref) > bar))


@pytest.mark.parametrize("shape,family,storage", F32_UNIFORM + [(s, "integer", "f64") for s in dc.SHAPES],
                         ids=[i for i in CASE_IDS if i.endswith("uniform-f32") or i.endswith("integer-f64")])
def test_fault_1_dropped_last_coefficient_and_fault_2_dc_scale_leave_the_decode_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    y, work = restate_y(cs, "wide"), dc.work_of(storage)
    assert _outside(transform(y, work), cs.x, cs.decode_bar("wide")) == 0
    assert _outside(transform(y, work, drop_last=True), cs.x, cs.decode_bar("wide")) >= 1
    assert _outside(transform(y, work, dc_wrong=True), cs.x, cs.decode_bar("wide")) >= 1


@pytest.mark.parametrize("shape,family,storage", F32_UNIFORM, ids=dc.SHAPE_IDS)
def test_fault_3_indexing_before_the_transform_leaves_the_region_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    y = restate_y(cs, "wide")
    for key in dc.extra_region_keys(shape)[:3]:
        good = dc.ix(transform(y, "f32"), key, shape)
        assert _outside(good, dc.ix(cs.x, key, shape), dc.ix(cs.decode_bar("wide"), key, shape)) == 0
        early = dc.ix(y, key, shape)  # the coefficients indexed, then transformed at their own length
        wrong = idct(early.astype(np.float32), type=2, norm="ortho", axis=-1)
        assert _outside(wrong, dc.ix(cs.x, key, shape), dc.ix(cs.decode_bar("wide"), key, shape)) >= 1, key


@pytest.mark.parametrize("shape,family,storage", F32_UNIFORM, ids=dc.SHAPE_IDS)
def test_fault_4_points_read_from_the_first_decoded_row_leave_the_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    n = cs.n
    pts = dc.points(shape) % np.array(shape)
    row_key = np.ravel_multi_index(tuple(pts[:, :-1].T), shape[:-1])
    uniq, inv = np.unique(row_key, return_inverse=True)
    assert uniq.size > 1 and np.count_nonzero(row_key == row_key[2]) >= 58 and np.array_equal(pts[0], pts[1])
    rows = restate_y(cs, "wide").reshape(-1, n)[uniq]
    rec = transform(rows, "f32").reshape(-1)
    ref, bar = cs.x[tuple(pts.T)], cs.decode_bar("wide")[tuple(pts.T)]
    assert _outside(rec[inv.ravel() * n + pts[:, -1]], ref, bar) == 0
    assert _outside(rec[pts[:, -1]], ref, bar) >= 1  # ``sel`` without ``inv * n``
    one = dc.points_one_row(shape) % np.array(shape)
    assert np.unique(np.ravel_multi_index(tuple(one[:, :-1].T), shape[:-1])).size == 1


@pytest.mark.parametrize("shape,family,storage", F32_UNIFORM + [(s, "integer", "f32") for s in dc.SHAPES],
                         ids=[i for i in CASE_IDS if i.endswith("-f32")])
def test_fault_5_pick_weighted_one_over_f_leaves_the_pick_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    L, nd = dc.factor_array(shape).shape
    # the mean of a whole uniform volume cancels to far below its bound, which no weight can leave: all levels L is
    # asked of the integer family only, whose bar there is one rounding of the result
    for lev in ([0] * (nd - 1) + [L],) + ((L,) if family == "integer" else ()):
        kind, ref, bar = dc.pooled(cs, lev, "mean")
        assert kind == "pick" and _outside(restate_pooled(cs, lev, "mean"), ref, bar) == 0
        assert _outside(restate_pooled(cs, lev, "mean", pick_weight=1.0 / cs.n), ref, bar) >= 1, lev


@pytest.mark.parametrize("shape,family,storage", F32_UNIFORM, ids=dc.SHAPE_IDS)
def test_fault_6_late_block_and_fault_7_transposed_basis_leave_the_pooled_bar(shape, family, storage):
    cs = dc.case(shape, family, storage)
    L, nd = dc.factor_array(shape).shape
    for lev in ([0] * (nd - 1) + [1], [1] * (nd - 1) + [L - 1]):
        for op in ("mean", "sum"):
            kind, ref, bar = dc.pooled(cs, lev, op)
            assert kind == "pooled" and ref.shape[-1] not in (1, cs.n)
            assert _outside(restate_pooled(cs, lev, op), ref, bar) == 0
            assert _outside(restate_pooled(cs, lev, op, first=1), ref, bar) >= 1, (lev, op)
            assert _outside(restate_pooled(cs, lev, op, transposed=True), ref, bar) >= 1, (lev, op)


@pytest.mark.parametrize("n,Bk", dc.BASIS_CASES)
def test_fault_6_late_block_leaves_the_basis_bar(n, Bk):
    for w in (1.0, 1.0 / Bk):
        for f32 in (False, True):
            bar = dc.basis_bar(n, Bk, w, f32)
            W = dc.pooled_basis(n, Bk, w)
            assert _outside(dc.kernel_model_basis(n, Bk, w, f32), W, bar) == 0
            assert _outside(dc.kernel_model_basis(n, Bk, w, f32, first=1), W, bar) >= 1
            if n // Bk != n and Bk != n:
                wrong = dc.kernel_model_basis(n, Bk, w, f32).T.reshape(n // Bk, n)  # filled as (n, n / Bk)
                assert _outside(wrong, W, bar) >= 1


def test_frobenius_change_of_fault_1_on_a_smooth_volume_is_reported():
    """What the existing relative-Frobenius bars see of a dropped last coefficient: printed, not asserted."""
    shape = (64, 64, 64)
    x = synthetic_mri(shape)
    obj = OracleNDMPS.from_tensor(x, mode="DCT", max_bond=12)
    rec = obj.to_tensor()
    obj.mode = "Std"
    y = obj.to_tensor()
    y[..., -1] = 0.0
    wrong = idct(y, type=2, norm="ortho", axis=-1)
    change = np.linalg.norm(wrong - rec) / np.linalg.norm(rec)
    print(f"[dct-host] fault 1 on synthetic_mri{shape} max_bond=12 DCT: relative Frobenius change {change:.3e} "
          f"(the existing bars are 1e-5 at fp32 / bf16, 1e-11 or 1e-12 at fp64)")
    assert np.isfinite(change)
