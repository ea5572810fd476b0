"""Pair statistics per label from the cores, on the host (no GPU): the six-exponent scale rule, the workspace, the
refusals the C entries make before their first launch, the host side's arithmetic, and the cases and bars of
tests/labelpair_cases.py.

* ndmps_labelpair_scales equals the rule stated in Python integers (labelpair_cases.scale_rule) on a grid of
  magnitudes including 0, subnormals and values near 1.79e308, and with its exponents no sum of numel terms can leave
  62 bits.
* every exponent is at least 0 on every integer pair in both storages (the exact bar needs it); the smallest is 15.
* ndmps_labelpair_workspace_bytes is the pair query (or the single-chain query) plus the documented table.
* the bars accept the reference and reject every modelled fault on every case where the fault changes the result.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import labelpair_cases as lpc
import labelstat_cases as lc
import pairstat_cases as pc
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import labelpair as lp
from imgcompressionmps_amd.core import pairstat as ps
from oracle import chain_cases as cc


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except ImportError:
        pytest.skip("the library is not built")


# ------------------------------------------------------------------------------------------------ the scale rule
TOP = 1.7976931348623157e308
MAGNITUDES = [float(v) for v in (0.0, 5e-324, 2.2250738585072014e-308 / 4, 2.2250738585072014e-308, 1e-160, 2.0 ** -30, np.nextafter(1.0, 0.0),
              1.0, np.nextafter(1.0, 2.0), 3.0, 5457.0, 2.0 ** 30, 1e154, 1.4e154, 1e300, TOP / 2, np.nextafter(TOP, 0.0), TOP)]
NUMELS = [1, 2, 2520, 2 ** 21, 2 ** 21 + 1, 2 ** 40]


def test_scales_equal_the_rule_in_python_integers(lib):
    assert lpc.scale_rule(5457.0, 3.0, 5460.0, 2 ** 21) == dict(s_a=27, s2_a=15, s_b=38, s2_b=36, s_ab=26, s2_d=15)  # 5457 * 3 < 2**14
    assert set(lpc.scale_rule(0.0, 0.0, 0.0, 8).values()) == {0}
    for numel in NUMELS:
        for max_a in MAGNITUDES:
            for max_b in MAGNITUDES:
                for max_d in (0.0, abs(max_a - max_b), min(max_a + max_b, TOP)):
                    out = (C.c_int * 6)(*[-7] * 6)
                    assert lib.ndmps_labelpair_scales(max_a, max_b, max_d, numel, out) == _lib.OK
                    want = lpc.scale_rule(max_a, max_b, max_d, numel)
                    where = (max_a, max_b, max_d, numel)
                    assert tuple(out) == tuple(want[k] for k in lpc.SCALES) == lp.scales(*where), where
                    # the exponents of a, of b and of d are the single-volume rule's
                    assert (want["s_a"], want["s2_a"]) == lc.scale_rule(max_a, numel)
                    assert (want["s_b"], want["s2_b"]) == lc.scale_rule(max_b, numel)
                    assert want["s2_d"] == lc.scale_rule(max_d, numel)[1]
                    # every |q| <= |a b| 2**s_ab + 1/2 with |a b| <= max_a max_b: numel of them stay below 2**62
                    if want["s_ab"] > -1000:
                        bound = Fraction(float(max_a)) * Fraction(float(max_b)) * Fraction(2) ** want["s_ab"]
                        assert numel * (bound + 1) < 2 ** 62, where
    out = (C.c_int * 6)()
    for bad in (-1.0, math.inf, math.nan):
        for at in range(3):
            args = [1.0, 1.0, 1.0]
            args[at] = bad
            assert lib.ndmps_labelpair_scales(*args, 8, out) == _lib.EINVAL
    assert lib.ndmps_labelpair_scales(1.0, 1.0, 1.0, 0, out) == _lib.EINVAL
    assert lib.ndmps_labelpair_scales(1.0, 1.0, 1.0, 8, None) == _lib.EINVAL


@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.INT_NAMES)
def test_integer_pairs_have_exponents_that_keep_integers_exact(name, storage):
    p = pc.pair(name, "integer", storage)
    scales = lpc.ref_scales(p.a.ref, p.b.ref)
    print(f"[labelpair] {name}/{storage}: max |a| {np.abs(p.a.ref).max()}, max |b| {np.abs(p.b.ref).max()}, "
          f"max |a - b| {np.abs(p.a.ref - p.b.ref).max()}, n {p.n}, scales {scales}")
    assert min(scales.values()) >= 15, scales
    if name == "int_8x7":
        assert scales["s2_a"] == 15 and scales["s2_d"] == 15 and min(scales.values()) == 15
    assert (scales["s_a"], scales["s2_a"]) == lc.ref_scales(p.a.ref)
    assert (scales["s_b"], scales["s2_b"]) == lc.ref_scales(p.b.ref)


# ------------------------------------------------------------------------------------------------ the workspace
def _table_bytes(n_labels):
    # thirteen 64-bit slots per label, then outside, overflow, six exponents, the flag and five extremes
    return -(-(8 * (13 * n_labels + 14)) // 256) * 256


@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("name", pc.REAL_NAMES + pc.INT_NAMES)
def test_workspace_is_the_pair_or_the_single_workspace_plus_the_table(lib, name, elem_bytes):
    dims, bonds_a = pc.CHAINS[name]
    bonds_b = (pc.INT_PAIRS if name in pc.INT_PAIRS else pc.REAL_PAIRS)[name]
    L, d, ba, bb = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a), _lib.i64_array(bonds_b)
    pair = lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, elem_bytes, 0, 0)
    single = lib.ndmps_valstat_workspace_bytes(L, d, ba, elem_bytes, 0)
    assert pair > 0 and pair % 256 == 0 and single > 0 and single % 256 == 0
    for n_labels in (1, 2, 7, 27, 512, 513, 1030, 4096):
        assert lib.ndmps_labelpair_workspace_bytes(L, d, ba, bb, elem_bytes, n_labels) == pair + _table_bytes(n_labels), n_labels
        assert lib.ndmps_labelpair_workspace_bytes(L, d, ba, None, elem_bytes, n_labels) == single + _table_bytes(n_labels)
    for bad in (0, -1, 4097):
        assert lib.ndmps_labelpair_workspace_bytes(L, d, ba, bb, elem_bytes, bad) == 0
        assert lib.ndmps_labelpair_workspace_bytes(L, d, ba, None, elem_bytes, bad) == 0
    assert lib.ndmps_labelpair_workspace_bytes(L, d, ba, bb, 2, 7) == 0
    assert lib.ndmps_labelpair_workspace_bytes(0, d, ba, bb, elem_bytes, 7) == 0
    assert lib.ndmps_labelpair_workspace_bytes(L, d, None, bb, elem_bytes, 7) == 0


def test_window_fits_in_64_kib_of_lds_without_opt_in():
    """512 labels of 7 64-bit words, 4 keys and 2 counters each, 8 bytes of outside / overflow, and the two staging
    tiles (2 x k-tile x 68 elements): under 64 KiB in both element types."""
    for elem, k_tile in ((4, 16), (8, 8)):
        per_label = 7 * 8 + 4 * elem + 2 * 4
        assert per_label == (80 if elem == 4 else 96)
        total = lpc.WINDOW * per_label + 8 + 2 * k_tile * 68 * elem
        assert total <= 65536, (elem, total)
    assert -(-4096 // lpc.WINDOW) == 8 and -(-1030 // lpc.WINDOW) == 3


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    bonds_b = pc.REAL_PAIRS["L4_tail_last"]
    L, d, b, b2 = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds), _lib.i64_array(bonds_b)
    fake = (C.c_void_p * L)(*[256] * L)
    p = 256
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    host = np.zeros(5 * 4096, dtype=np.int64).ctypes.data
    for suffix, eb in (("f32", 4), ("f64", 8)):
        pair_entry = getattr(lib, f"ndmps_labelpair_{suffix}")
        orig_entry = getattr(lib, f"ndmps_labelpair_original_{suffix}")

        def pair_call(n_labels=7, lab_bytes=2, lab=p, row=p, col=p, perm=p, cols=n_cols, ws=p, nbytes=1 << 30, sums=host,
                      bonds_=b2, cores=fake):
            return pair_entry(L, d, b, bonds_, fake, cores, lab, lab_bytes, row, col, perm, cols, n_labels, sums, host, host,
                              host, host, host, ws, nbytes, None)

        def orig_call(n_labels=7, lab_bytes=2, lab=p, row=p, col=p, perm=p, cols=n_cols, ws=p, nbytes=1 << 30, sums=host,
                      bonds_=b, cores=fake, ref=p):
            return orig_entry(L, d, bonds_, cores, ref, lab, lab_bytes, row, col, perm, cols, n_labels, sums, host, host, host,
                              host, host, ws, nbytes, None)

        for call, need in ((pair_call, lib.ndmps_labelpair_workspace_bytes(L, d, b, b2, eb, 7)),
                           (orig_call, lib.ndmps_labelpair_workspace_bytes(L, d, b, None, eb, 7))):
            for n_labels in (0, -3, 4097):
                assert call(n_labels=n_labels) == _lib.EINVAL and b"labels" in lib.ndmps_last_error(), n_labels
            for lab_bytes in (0, 3, 8):
                assert call(lab_bytes=lab_bytes) == _lib.EINVAL and b"bytes" in lib.ndmps_last_error(), lab_bytes
            for missing in ("lab", "row", "col", "perm"):
                assert call(**{missing: None}) == _lib.EINVAL, missing
            assert call(sums=None) == _lib.EINVAL
            assert call(cores=None) == _lib.EINVAL
            assert call(cols=n_cols * dims[-2]) == _lib.EINVAL and b"columns" in lib.ndmps_last_error()
            assert call(bonds_=_lib.i64_array([1, 4, 13, 13, 1])) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error()
            assert call(ws=264) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error()
            assert call(ws=None) == _lib.EWORKSPACE
            assert call(nbytes=need - 1) == _lib.EWORKSPACE
            assert call(nbytes=need - _table_bytes(7)) == _lib.EWORKSPACE  # room for the chains and the records only
            assert b"labelpair workspace" in lib.ndmps_last_error()
        assert orig_call(ref=None) == _lib.EINVAL and b"NULL" in lib.ndmps_last_error()


# ------------------------------------------------------------------------------------------------ the host side
def test_result_dict_is_ldexp_of_the_exact_integers_and_derive_is_pairstat_s():
    n = 5
    rng = np.random.default_rng(3)
    sums = np.concatenate([[0, 3, -5, 2 ** 53 + 1, -(2 ** 60) - 1], rng.integers(-2 ** 40, 2 ** 40, 2 * n)]).astype(np.int64)
    sums[[5, 10]] = 0
    sumsq = np.concatenate([[0, 9, 25, 2 ** 53 + 3, 2 ** 63 + 2 ** 11 + 1], rng.integers(1, 2 ** 50, 2 * n)]).astype(np.uint64)
    sumsq[[5, 10]] = 0
    counts = np.array([0, 1, 2, 3, 4] + [2, 0, 0, 0, 1], dtype=np.int64)
    ext = np.tile(np.array([np.nan, 1, 2, 3, 4], dtype=np.float64), 5)
    whole = np.arange(5, dtype=np.float64)
    for exps in ((0,) * 6, (27, 15, 38, 36, 25, 15), (-3, -7, 2, 0, -1, 5)):
        info = np.array([6, *exps, 99], dtype=np.int64)
        got = lp._finish((sums, sumsq, counts, ext, info, whole))
        assert set(got) == set(lp.ARRAYS) | {"outside", "scales"}
        assert got["outside"] == 6 and got["scales"] == dict(zip(lp.SCALES, exps))
        for i, (key, scale) in enumerate(lp.SUMS):
            assert lc.same_bits(got[key], np.array([math.ldexp(int(q), -got["scales"][scale]) for q in sums[i * n:(i + 1) * n]]))
        for i, (key, scale) in enumerate(lp.SQUARES):
            assert lc.same_bits(got[key], np.array([math.ldexp(int(q), -got["scales"][scale]) for q in sumsq[i * n:(i + 1) * n]]))
        for l in range(n):  # the derived fields are pairstat.derive's, label by label, bit for bit
            one = ps.derive({k: (int(got[k][l]) if k in lp.COUNTS else float(got[k][l])) for k in lp.COUNTS + ps.RAW_FIELDS})
            for key in lp.DERIVED:
                assert lc.same_bits(np.float64(got[key][l]), np.float64(one[key])), (key, l, got[key][l], one[key])
        assert all(np.isnan(got[key][0]) for key in lp.DERIVED + lp.EXTREMES)
        assert all(got[key][0] == 0 for key, _ in lp.SUMS + lp.SQUARES)


# ------------------------------------------------------------------------------------------------ the bars
def _reject(bar, fault, label):
    try:
        bar(fault)
    except AssertionError:
        return
    pytest.fail(f"the bar accepted the fault {label}")


ALWAYS = {"site_order_labels", "site_order_original", "b_tile_shifted", "swapped", "tile_left_out", "run_not_flushed"}


@pytest.mark.parametrize("name", pc.INT_NAMES)
def test_exact_bar_on_the_reference_and_on_modelled_faults(name):
    p = pc.pair(name, "integer", "f64")
    ra, rb = p.a.ref, p.b.ref
    seen = set()
    for kind in lc.kinds_for(name, p.n):
        lab, n_labels = lc.labels(p.a, kind)
        truth = lpc.ref_stats(ra, rb, lab, n_labels)
        lpc.exact_stats(truth, ra, rb, lab, n_labels)
        assert int(truth["count"].sum()) + truth["outside"] == p.n
        faults = lpc.faults(p, lab, n_labels)
        expected = set(ALWAYS)
        if kind in ("window", "max"):
            expected.add("windows_folded")
        if kind == "outside":
            expected |= {"outside_to_first", "outside_to_last"}
        if kind == "one":
            expected.discard("site_order_labels")  # one label: the address of the label does not matter
        if p.a.identity:
            expected -= {"site_order_labels", "site_order_original"}
        if truth["scales"]["s2_a"] != truth["scales"]["s_ab"] and np.any(truth["sum_ab"] != 0):
            expected.add("sum_ab_scaled_with_s2_a")
        assert expected <= set(faults), (kind, sorted(expected - set(faults)))
        seen |= set(faults)
        for label, fault in faults.items():
            _reject(lambda f: lpc.exact_stats(f, ra, rb, lab, n_labels, truth), fault, f"{name}/{kind}/{label}")
    # NaN planted in a core of b only: counted per label, apart
    _, rb_nan = vc.with_nan(p.b)
    for kind in ("blocks", "scatter"):
        lab, n_labels = lc.labels(p.a, kind)
        lpc.exact_stats(lpc.ref_stats(ra, rb_nan, lab, n_labels), ra, rb_nan, lab, n_labels)
        fault = lpc.fault_nan_of_b_ignored(ra, rb_nan, lab, n_labels)
        assert fault is not None
        _reject(lambda f: lpc.exact_stats(f, ra, rb_nan, lab, n_labels), fault, f"{name}/{kind}/nan_of_b_ignored")
    print(f"[labelpair] {name}: faults rejected {sorted(seen)}")


def test_padding_fault_occurs_on_some_integer_case():
    hit = [name for name in pc.INT_NAMES
           if lpc.fault_padding_counted(pc.pair(name, "integer", "f64"), *lc.labels(pc.pair(name, "integer", "f64").a, "blocks"))]
    assert hit, "no integer pair has padded tiles"


@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.REAL_NAMES)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, storage):
    p = pc.pair(name, "uniform", storage)
    ra, ba, rb, bb = p.a.ref, p.a.bound, p.b.ref, p.b.bound
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(p.a, kind)
        truth = lpc.ref_stats(ra, rb, lab, n_labels)
        lpc.sandwich_stats(truth, ra, ba, rb, bb, lab, n_labels)
        faults = lpc.faults(p, lab, n_labels)
        expected = {"swapped", "tile_left_out", "run_not_flushed"}
        if p.m * p.cols > 64 * 64:
            expected.add("b_tile_shifted")
        if not p.a.identity:
            expected |= {"site_order_labels", "site_order_original"}
        assert expected <= set(faults), (kind, sorted(expected - set(faults)))
        for label, fault in faults.items():
            _reject(lambda f: lpc.sandwich_stats(f, ra, ba, rb, bb, lab, n_labels), fault, f"{name}/{kind}/{label}")
