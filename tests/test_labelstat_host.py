"""Statistics per label from the cores, on the host (no GPU): the scale rule, the workspace, the refusals, and the
cases and bars of tests/labelstat_cases.py.

* ndmps_labelstat_scales equals the rule stated in Python integers (labelstat_cases.scale_rule), and with its s no
  sum of numel terms can leave 62 bits.
* ndmps_labelstat_workspace_bytes is the value statistics' workspace plus the documented table.
* the refusals the C entry makes before its first launch (with pointers that are never dereferenced) and the ones
  core/labelstat.py makes before it touches the device.
* the bars accept the reference and reject every modelled fault (labels read in site order, a tile left out, padding
  counted as label 0, a held run never flushed, windows folded, NaN counted, outside voxels added to a label) on every
  case where the fault changes the result.
* the fixed-point sums in integers alone reproduce NumPy's fp64 sums on the integer cases, whose scales are not
  negative.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import labelstat_cases as lc
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import labelstat as ls
from oracle import chain_cases as cc


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the scale rule
def _ulp_neighbours(x):
    return [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]


MAXABS = [0.0, 1.0, 5457.0, 1e300] + [float(v) for k in range(-30, 31) for v in _ulp_neighbours(2.0 ** k)]
NUMELS = [1, 2, 2520, 2 ** 21, 2 ** 21 + 1, 2 ** 40]


def test_scales_equal_the_rule_in_python_integers(lib):
    assert lc.scale_rule(5457.0, 2 ** 21) == (27, 15)
    assert lc.scale_rule(0.0, 2 ** 21) == (0, 0)
    for numel in NUMELS:
        nb = (numel - 1).bit_length()
        assert 2 ** nb >= numel and (nb == 0 or 2 ** (nb - 1) < numel)
        for maxabs in MAXABS:
            s, s2 = C.c_int(-7), C.c_int(-7)
            assert lib.ndmps_labelstat_scales(maxabs, numel, C.byref(s), C.byref(s2)) == _lib.OK
            assert (s.value, s2.value) == lc.scale_rule(maxabs, numel) == ls.scales(maxabs, numel), (maxabs, numel)
            # every |q| <= maxabs 2**s + 1/2, so the sum of numel of them stays below 2**62
            assert numel * (Fraction(maxabs) * Fraction(2) ** s.value + 1) < 2 ** 62, (maxabs, numel)
            sq = Fraction(maxabs * maxabs) if maxabs * maxabs < math.inf else None
            if sq is not None and s2.value > -1000:
                assert numel * (sq * Fraction(2) ** s2.value + 1) < 2 ** 62, (maxabs, numel)
    s = C.c_int()
    for bad in (-1.0, math.inf, math.nan):
        assert lib.ndmps_labelstat_scales(bad, 8, C.byref(s), C.byref(s)) == _lib.EINVAL
    assert lib.ndmps_labelstat_scales(1.0, 0, C.byref(s), C.byref(s)) == _lib.EINVAL
    assert lib.ndmps_labelstat_scales(1.0, 8, None, C.byref(s)) == _lib.EINVAL


@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_integer_cases_have_scales_that_keep_integers_exact(name):
    c = vc.case(name, "integer", "f64")
    s, s2 = lc.ref_scales(c.ref)
    print(f"[labelstat] {name}: maxabs {np.abs(c.ref).max()}, n {c.n}, s {s}, s2 {s2}")
    assert 27 <= s <= 44 and 15 <= s2 <= 40
    if name == "int_8x7":
        assert (np.abs(c.ref).max(), c.n, s, s2) == (5457, 2 ** 21, 27, 15)


# ------------------------------------------------------------------------------------------------ the workspace
@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("name", sorted(vc.ALL_CHAINS))
def test_workspace_is_the_valstat_workspace_plus_the_table(lib, name, elem_bytes):
    dims, bonds = vc.ALL_CHAINS[name]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    base = lib.ndmps_valstat_workspace_bytes(L, d, b, elem_bytes, 0)
    assert base > 0 and base % 256 == 0
    last = 0
    for n_labels in (1, 2, 7, 27, 1001, 1024, 1025, 4096):
        got = lib.ndmps_labelstat_workspace_bytes(L, d, b, elem_bytes, n_labels)
        # six 64-bit slots per label, then outside, overflow, s, s2 and the flag
        assert got == base + -(-(8 * (6 * n_labels + 5)) // 256) * 256, n_labels
        assert got >= last
        last = got
    for bad in (0, -1, 4097):
        assert lib.ndmps_labelstat_workspace_bytes(L, d, b, elem_bytes, bad) == 0
    assert lib.ndmps_labelstat_workspace_bytes(L, d, b, 2, 7) == 0
    assert lib.ndmps_labelstat_workspace_bytes(0, d, b, elem_bytes, 7) == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[256] * L)
    p = 256
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    host = np.zeros(2 * 4096, dtype=np.int64).ctypes.data
    for suffix, eb in (("f32", 4), ("f64", 8)):
        entry = getattr(lib, f"ndmps_labelstat_{suffix}")

        def call(n_labels=7, lab_bytes=2, lab=p, row=p, col=p, perm=p, cols=n_cols, ws=p, nbytes=1 << 30, sums=host,
                 bonds_=b, cores=fake):
            return entry(L, d, bonds_, cores, lab, lab_bytes, row, col, perm, cols, n_labels, sums, host, host, host, host,
                         ws, nbytes, None)

        for n_labels in (0, -3, 4097):
            assert call(n_labels=n_labels) == _lib.EINVAL and b"labels" in lib.ndmps_last_error(), n_labels
        for lab_bytes in (0, 3, 8):
            assert call(lab_bytes=lab_bytes) == _lib.EINVAL and b"bytes" in lib.ndmps_last_error(), lab_bytes
        for missing in ("lab", "row", "col", "perm"):
            assert call(**{missing: None}) == _lib.EINVAL and b"NULL" in lib.ndmps_last_error(), missing
        assert call(sums=None) == _lib.EINVAL
        assert call(cores=None) == _lib.EINVAL
        assert call(cols=n_cols * dims[-2]) == _lib.EINVAL and b"columns" in lib.ndmps_last_error()
        assert call(bonds_=_lib.i64_array([1, 4, 13, 13, 1])) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error()
        assert call(ws=264) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error()
        assert call(ws=None) == _lib.EWORKSPACE
        need = lib.ndmps_labelstat_workspace_bytes(L, d, b, eb, 7)
        assert call(nbytes=need - 1) == _lib.EWORKSPACE
        # room for the chain and the records but not for the table
        assert call(nbytes=lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)) == _lib.EWORKSPACE
        assert b"labelstat workspace" in lib.ndmps_last_error()


def test_python_refusals_before_the_device():
    shape = (6, 10)
    good = np.arange(60).reshape(shape) % 5
    lab, n = ls.check_labels(good, shape)
    assert n == 5 and lab.dtype == np.int32 and np.array_equal(lab, good)
    for dtype in (np.uint8, np.int16, np.int32):
        lab, n = ls.check_labels(good.astype(dtype), shape, 9)
        assert n == 9 and lab.dtype == dtype
    lab, n = ls.check_labels(good > 2, shape)
    assert n == 2 and lab.dtype == np.uint8 and np.array_equal(lab, (good > 2).astype(np.uint8))
    assert ls.check_labels(np.zeros(shape, dtype=np.int64), shape)[1] == 1
    assert ls.check_labels(np.full(shape, -1, dtype=np.int8), shape)[1] == 1  # at least one label
    lab, n = ls.check_labels(np.array([[-2 ** 31, 2 ** 31 - 1]], dtype=np.int64), (1, 2), 3)
    assert lab.dtype == np.int32 and lab.tolist() == [[-2 ** 31, 2 ** 31 - 1]]
    for dtype in (np.float32, np.float64, np.float16, np.complex64):
        with pytest.raises(TypeError, match="integers"):
            ls.check_labels(good.astype(dtype), shape)
    with pytest.raises(ValueError, match="shape"):
        ls.check_labels(good.reshape(10, 6), shape)
    with pytest.raises(ValueError, match="shape"):
        ls.check_labels(good.reshape(-1), shape)
    for value in (2 ** 31, -2 ** 31 - 1):
        big = good.astype(np.int64)
        big[3, 3] = value
        with pytest.raises(ValueError, match="int32"):
            ls.check_labels(big, shape, 5)
    with pytest.raises(ValueError, match="int32"):
        ls.check_labels(np.full(shape, 2 ** 32 - 1, dtype=np.uint32), shape, 5)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        ls.check_labels(good, shape, 4097)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        ls.check_labels(good * 1024, shape)  # max(labels) + 1 = 4097
    with pytest.raises(ValueError, match="at least 1"):
        ls.check_labels(good, shape, 0)


def test_result_dict_is_ldexp_of_the_exact_integers():
    """The host side turns the raw arrays into the dict: sums are math.ldexp(int, -s), rounded once; an empty label has
    sum = sumsq = 0 and NaN for the rest."""
    sums = np.array([0, 3, -5, 2 ** 53 + 1, -(2 ** 60) - 1, 2 ** 62 - 1, 0], dtype=np.int64)
    sumsq = np.array([0, 9, 25, 2 ** 53 + 3, 2 ** 63 + 2 ** 11 + 1, 2 ** 64 - 1, 0], dtype=np.uint64)
    n = sums.size
    counts = np.array([0, 1, 2, 3, 4, 5, 0] + [2, 0, 0, 0, 0, 0, 0], dtype=np.int64)
    minmax = np.array([np.nan, 1, 2, 3, 4, 5, np.nan] * 2, dtype=np.float64)
    for s, s2 in ((0, 0), (27, 15), (-3, -7), (44, 40)):
        got = ls._finish(sums, sumsq, counts, minmax, np.array([6, s, s2, 99], dtype=np.int64))
        assert (got["outside"], got["s"], got["s2"]) == (6, s, s2)
        assert lc.same_bits(got["sum"], np.array([math.ldexp(int(q), -s) for q in sums]))
        assert lc.same_bits(got["sumsq"], np.array([math.ldexp(int(q), -s2) for q in sumsq]))
        assert np.array_equal(got["count"], counts[:n]) and np.array_equal(got["n_nan"], counts[n:])
        filled = counts[:n] > 0
        assert lc.same_bits(got["mean"][filled], got["sum"][filled] / counts[:n][filled])
        for key in ("mean", "std", "min", "max"):
            assert np.isnan(got[key][~filled]).all(), key
        assert np.all(got["sum"][~filled] == 0) and np.all(got["sumsq"][~filled] == 0)
        assert np.all(got["std"][filled] >= 0)


# ------------------------------------------------------------------------------------------------ the bars
def _reject(bar, fault, label):
    try:
        bar(fault)
    except AssertionError:
        return
    pytest.fail(f"the bar accepted the fault {label}")


@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_exact_bar_on_the_reference_and_on_modelled_faults(name):
    c = vc.case(name, "integer", "f64")
    assert not c.identity
    s, s2 = lc.ref_scales(c.ref)
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        truth = lc.ref_stats(c.ref, lab, n_labels)
        lc.exact_stats(truth, c.ref, lab, n_labels)
        assert int(truth["count"].sum()) + truth["outside"] == c.n
        assert (truth["outside"] == 3) == (kind == "outside") and truth["outside"] in (0, 3)
        assert ((truth["count"] == 0).sum() == 2) == (kind == "empty")
        faults = lc.faults(c, lab, n_labels)
        expected = {"site_order_labels", "tile_left_out", "run_not_flushed"}
        if kind in ("window", "max"):
            expected.add("windows_folded")
        if kind == "outside":
            expected |= {"outside_to_first", "outside_to_last"}
        if kind == "one":
            expected.discard("site_order_labels")  # one label: the address does not matter
        assert expected <= set(faults), (kind, sorted(faults))
        for label, fault in faults.items():
            _reject(lambda f: lc.exact_stats(f, c.ref, lab, n_labels), fault, f"{name}/{kind}/{label}")
        # the kernel's sums in integers alone
        total, squares = lc.fixed_point_sums(c.ref, lab, n_labels, s, s2)
        assert lc.same_bits(total, truth["sum"]) and lc.same_bits(squares, truth["sumsq"]), kind
    # NaN planted in a core: counted per label, apart
    _, ref_nan = vc.with_nan(c)
    for kind in ("blocks", "scatter"):
        lab, n_labels = lc.labels(c, kind)
        lc.exact_stats(lc.ref_stats(ref_nan, lab, n_labels), ref_nan, lab, n_labels)
        fault = lc.fault_nan_counted(ref_nan, lab, n_labels)
        assert fault is not None
        _reject(lambda f: lc.exact_stats(f, ref_nan, lab, n_labels), fault, f"{name}/{kind}/nan_counted")


def test_padding_fault_occurs_on_some_integer_case():
    hit = [name for name in sorted(vc.INT_CHAINS)
           if lc.fault_padding_counted(vc.case(name, "integer", "f64"), *lc.labels(vc.case(name, "integer", "f64"), "blocks"))]
    assert hit, "no integer case has padded tiles"


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, family, storage):
    c = vc.case(name, family, storage)
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(c, kind)
        truth = lc.ref_stats(c.ref, lab, n_labels)
        lc.sandwich_stats(truth, c.ref, c.bound, lab, n_labels)
        faults = lc.faults(c, lab, n_labels)
        assert {"tile_left_out", "run_not_flushed"} <= set(faults), (kind, sorted(faults))
        assert c.identity or "site_order_labels" in faults
        for label, fault in faults.items():
            _reject(lambda f: lc.sandwich_stats(f, c.ref, c.bound, lab, n_labels), fault, f"{name}/{kind}/{label}")
