"""Voxels selected by value from the cores, on the host (no GPU): the bars, the refusals, the host logic of topk.

* both bars of tests/select_cases.py accept the reference and reject the modelled faults: a 64 x 64 tile left out,
  padding taken as data, an open right bound, site-order instead of C-order indices, NaN selected by ``invert``, a
  duplicated slot, an unsorted result.  A fault that a case cannot show (no padding, an identity index map, ...) is
  skipped for that case by a condition stated here.
* the refusals of core/select.py and of the NDMPS methods that need no device.
* ``core.select.topk_select`` (the bracketing and the tie rule) on a NumPy stand-in for the passes.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import select_cases as sc
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import select as sel
from oracle import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_TILE = (slice(0, sc.TILE), slice(0, sc.TILE))


def _rejects(bar, *args, **kw):
    with pytest.raises(AssertionError):
        bar(*args, **kw)


# ------------------------------------------------------------------------------------------------ the exact bar
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sc.INT_NAMES)
def test_exact_bar_accepts_the_reference_and_rejects_the_modelled_faults(name, storage):
    c = sc.int_case(name, storage)
    assert np.array_equal(c.ref, np.round(c.ref)) and np.abs(c.ref).max() < 2 ** 24
    identity = np.array_equal(c.dest.reshape(-1), np.arange(c.ref.size))
    padded = bool(c.m % sc.TILE or c.n % sc.TILE)
    intervals = sc.int_intervals(c.ref)
    if name == "int_wrap":
        assert c.tiles == 1024 and c.ref.size == 4 ** 11
        intervals = {k: intervals[k] for k in ("closed_ends", "max_only", "invert")}
    for key, (lo, hi, invert) in intervals.items():
        index, values = sc.emulate(c, lo, hi, invert)
        sc.exact_find(index, values, c.ref, lo, hi, invert)
        assert index.size == sc.ref_count(c.ref, lo, hi, invert)
        if key == "empty":
            assert index.size == 0
            continue
        if key == "everything":
            assert np.array_equal(index, np.arange(c.ref.size))
        if index.size > 1:
            _rejects(sc.exact_find, *sc.emulate(c, lo, hi, invert, duplicate=True), c.ref, lo, hi, invert)
            _rejects(sc.exact_find, *sc.emulate(c, lo, hi, invert, unsorted=True), c.ref, lo, hi, invert)
        if not identity:
            _rejects(sc.exact_find, *sc.emulate(c, lo, hi, invert, site_order=True), c.ref, lo, hi, invert)
        if hi is not None and not invert:  # the right end is a voxel value: an open bound loses those voxels
            assert (c.ref == hi).any()
            _rejects(sc.exact_find, *sc.emulate(c, lo, hi, invert, open_right=True), c.ref, lo, hi, invert)
    # a tile left out, where the first tile holds a match: everything selected
    _rejects(sc.exact_find, *sc.emulate(c, skip=FIRST_TILE), c.ref)
    # padding taken as data shows wherever 0 is selected; the two signed chains have no 0 among their voxels
    if padded:
        _rejects(sc.exact_find, *sc.emulate(c, -1.0, 1.0, padding=True), c.ref, -1.0, 1.0)
    if name == "int_positive":
        assert 64 <= c.ref.min() and c.ref.max() <= 2048 and padded
        assert sc.ref_count(c.ref, -1.0, 1.0) == 0 and sc.emulate(c, -1.0, 1.0, padding=True)[0].size > 0
    if name == "int_negative":
        assert sc.ref_count(c.ref, -4096.0, -1.0, invert=True) == 0
        assert sc.emulate(c, -4096.0, -1.0, invert=True, padding=True)[0].size > 0


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_is_listed_by_find_nan_only_and_a_nan_selected_by_invert_is_rejected(name, storage):
    c = sc.int_case(name, storage).with_nan()
    n_nan = int(np.isnan(c.ref).sum())
    assert 0 < n_nan < c.ref.size
    sc.exact_nan(sc.emulate(c, nan=True)[0], c.ref)
    assert sc.ref_find_nan(c.ref).size == n_nan
    index, values = sc.emulate(c)
    sc.exact_find(index, values, c.ref)
    assert index.size == c.ref.size - n_nan and not np.isnan(values).any()
    lo, hi, _ = sc.int_intervals(c.ref)["closed_ends"]
    sc.exact_find(*sc.emulate(c, lo, hi, invert=True), c.ref, lo, hi, True)
    _rejects(sc.exact_find, *sc.emulate(c, lo, hi, invert=True, nan_by_invert=True), c.ref, lo, hi, True)
    with pytest.raises(AssertionError):
        sc.exact_nan(sc.emulate(c, nan=True)[0][1:], c.ref)


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sc.SMALL_INT_NAMES + ("int_8x7",))
def test_topk_reference_and_bar(name, storage):
    c = sc.int_case(name, storage)
    flat = c.ref.reshape(-1)
    for largest in (True, False):
        for k in (1, 7, 100):
            index, values = sc.ref_topk(c.ref, k, largest)
            assert index.size == min(k, flat.size) and np.array_equal(flat[index], values)
            s = -1.0 if largest else 1.0
            assert np.all(np.diff(s * values) >= 0)
            same = np.diff(values) == 0
            assert np.all(np.diff(index)[same] > 0), "equal values do not ascend in their index"
            rest = np.delete(flat, index)
            assert rest.size == 0 or (s * rest).min() >= (s * values).max()
            sc.exact_topk(index, values, c.ref, k, largest)
            if k > 1 and same.any():  # the last of the ties instead of the first
                i = int(np.flatnonzero(same)[0])
                swapped = index.copy()
                swapped[[i, i + 1]] = swapped[[i + 1, i]]
                _rejects(sc.exact_topk, swapped, values, c.ref, k, largest)


# ------------------------------------------------------------------------------------------------ the sandwich bar
def test_the_real_cases_are_those_that_meet_the_cap():
    assert set(sc.REAL_CASES) | set(sc.DROPPED) == set(vc.REAL_CASES) and not set(sc.REAL_CASES) & set(sc.DROPPED)
    assert len(sc.REAL_CASES) >= 15


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", sc.REAL_CASES, ids=sc.REAL_IDS)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, family, storage):
    c = sc.real_case(name, family, storage)  # asserts the cap: at most 10 % ambiguous per certain voxel
    identity = np.array_equal(np.asarray(c.dest).reshape(-1), np.arange(c.ref.size))
    padded = bool(c.m % sc.TILE or c.n % sc.TILE)
    for key, (lo, hi) in c.intervals.items():
        must, certainly_not = sc.certain(c.ref, c.bound, lo, hi)
        share = sc.ambiguous_share(c.ref, c.bound, lo, hi)
        print(f"[select] {name}/{family}/{storage} {key}: {int(must.sum())} certain, {share:.4f} ambiguous per certain")
        index, values = sc.emulate(c, lo, hi)
        assert sc.sandwich_find(index, values, c.ref, c.bound, lo, hi) <= int((~must & ~certainly_not).sum())
        if index.size > 1:
            _rejects(sc.sandwich_find, *sc.emulate(c, lo, hi, duplicate=True), c.ref, c.bound, lo, hi)
            _rejects(sc.sandwich_find, *sc.emulate(c, lo, hi, unsorted=True), c.ref, c.bound, lo, hi)
        if not identity and must.sum() > 1:
            _rejects(sc.sandwich_find, *sc.emulate(c, lo, hi, site_order=True), c.ref, c.bound, lo, hi)
    # the tile that holds the largest voxel of the product, which the top interval certainly selects
    lo, hi = c.intervals["top"]
    perm = c.tables[2]
    r, col = np.unravel_index(np.argmax(c.site[:, perm]), c.site.shape)
    tile = (slice(r // sc.TILE * sc.TILE, r // sc.TILE * sc.TILE + sc.TILE),
            slice(col // sc.TILE * sc.TILE, col // sc.TILE * sc.TILE + sc.TILE))
    _rejects(sc.sandwich_find, *sc.emulate(c, lo, hi, skip=tile), c.ref, c.bound, lo, hi)
    # a padded zero lies in the band where the band holds 0 beyond every bound
    lo, hi = c.intervals["band"]
    if padded and lo < 0 < hi:
        _rejects(sc.sandwich_find, *sc.emulate(c, lo, hi, padding=True), c.ref, c.bound, lo, hi)


# ------------------------------------------------------------------------------------------------ the refusals
def _obj(dims, bonds, mode="Std", dtype=None, shape=None):
    torch = pytest.importorskip("torch")
    from imgcompressionmps_amd import NDMPS
    from imgcompressionmps_amd.core.mps import DeviceMPS

    cores = [torch.full((bonds[j], d, bonds[j + 1]), 0.5, dtype=dtype or torch.float32) for j, d in enumerate(dims)]
    obj = NDMPS(DeviceMPS(cores), np.array(dims), None, None, False, None, mode, len(shape or (1,)))
    obj._shape = shape
    return obj


def test_refusals_need_no_device():
    torch = pytest.importorskip("torch")
    dims, shape = [4, 4, 4], (8, 8)
    a = _obj(dims, [1, 2, 2, 1], shape=shape)
    calls = (lambda o: o.count_between(0.0, 1.0), lambda o: o.find(0.0, 1.0), lambda o: o.find_nan(), lambda o: o.topk(3))
    for call in calls:
        with pytest.raises(ValueError, match="DCT"):
            call(_obj(dims, [1, 2, 2, 1], mode="DCT", shape=shape))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(_obj(dims, [1, 2, 2, 1], dtype=torch.bfloat16, shape=shape))
    for call in calls[1:]:
        with pytest.raises(ValueError, match="shape is unknown"):
            call(_obj(dims, [1, 2, 2, 1]))
    for k in (0, -3):
        with pytest.raises(ValueError, match="k must be at least 1"):
            a.topk(k)
    with pytest.raises(TypeError):
        a.topk(2.5)
    for call in (lambda lo, hi: a.count_between(lo, hi), lambda lo, hi: a.find(lo, hi),
                 lambda lo, hi: a.find(lo, hi, invert=True)):
        with pytest.raises(ValueError, match="lo = .* > hi"):
            call(2.0, 1.0)
        with pytest.raises(ValueError, match="NaN"):
            call(np.nan, 1.0)
        with pytest.raises(ValueError, match="NaN"):
            call(None, float("nan"))
    for call in (lambda n: a.find(0.0, 1.0, max_count=n), lambda n: a.find_nan(max_count=n), lambda n: a.topk(3, max_count=n)):
        with pytest.raises(ValueError, match="max_count must not be negative"):
            call(-1)
    # the bounds are cast to the element type before anything else
    lo, hi = sel.bounds(0.1, None, np.float32)
    assert lo.dtype == np.float32 and lo == np.float32(0.1) and hi == np.inf
    assert sel.bounds(None, 1e300, np.float32) == (-np.inf, np.inf)
    with pytest.raises(ValueError):
        sel.bounds(np.nextafter(np.float32(1), np.float32(2)), 1.0, np.float32)
    assert sel.bounds(1.0 + 2.0 ** -40, 1.0, np.float32) == (1.0, 1.0)  # equal once cast


def test_header_binding_and_library_agree():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("ndmps_select_"))
    assert names == ["ndmps_select_f32", "ndmps_select_f64"]
    for name in names:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, f"{name} is not declared in include/ndmps_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)


def test_entry_refusals_before_any_launch():
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    lib = _lib.load()
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[256] * L)
    p = C.c_void_p(256)
    total = C.c_int64()
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    big = 1 << 30
    for suffix, eb in (("f32", 4), ("f64", 8)):
        need = lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)
        entry = getattr(lib, f"ndmps_select_{suffix}")

        def call(mode=0, lo=0.0, hi=1.0, cols=n_cols, capacity=4, index=p, values=p, out=C.byref(total), ws=p, nbytes=big,
                 bonds_=b, cores=fake, row=p):
            return entry(L, d, bonds_, cores, mode, lo, hi, row, p, p, cols, capacity, index, values, out, ws, nbytes, None)

        assert call(nbytes=need - 1) == _lib.EWORKSPACE
        assert call(ws=None) == _lib.EWORKSPACE
        assert call(ws=C.c_void_p(264)) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error()
        for mode in (-1, 3):
            assert call(mode=mode) == _lib.EINVAL and b"neither" in lib.ndmps_last_error()
        for lo, hi in ((2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
            assert call(lo=lo, hi=hi) == _lib.EINVAL and b"lo <= hi" in lib.ndmps_last_error()
            assert call(mode=1, lo=lo, hi=hi) == _lib.EINVAL
        assert call(capacity=-1) == _lib.EINVAL and b"slots" in lib.ndmps_last_error()
        assert call(index=None) == _lib.EINVAL and call(values=None) == _lib.EINVAL
        assert call(out=None) == _lib.EINVAL
        assert call(row=None) == _lib.EINVAL
        assert call(cols=n_cols * dims[-2]) == _lib.EINVAL and b"columns" in lib.ndmps_last_error()
        assert call(bonds_=_lib.i64_array([1, 4, 13, 13, 1])) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error()
        assert call(cores=None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ topk on the host
def _volume(kind, np_type):
    rng = np.random.default_rng(7)
    if kind == "ties":        # integers with heavy ties
        v = rng.integers(-5, 6, size=5000).astype(np_type)
    elif kind == "real":
        v = rng.standard_normal(20000).astype(np_type)
    elif kind == "spread":    # twelve decades, both signs, the two zeros, infinities
        v = (rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 7, size=20000)).astype(np_type)
        v[:4] = [0.0, -0.0, np.inf, -np.inf]
    elif kind == "dense":     # neighbouring numbers of the element type: brackets with no edge inside
        v = (np_type(1) + np.finfo(np_type).eps * rng.integers(0, 3, size=4000).astype(np_type)).astype(np_type)
    else:                     # "nan": NaN among the voxels
        v = rng.integers(-3, 4, size=3000).astype(np_type)
        v[::7] = np.nan
    return v


@pytest.mark.parametrize("np_type", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["ties", "real", "spread", "dense", "nan"])
def test_topk_select_brackets_to_numpy_s_order(kind, np_type):
    v = _volume(kind, np_type)
    n = int((~np.isnan(v)).sum())
    for largest in (True, False):
        for k, max_count in ((1, 1 << 20), (7, 1 << 20), (100, 1 << 20), (100, 150), (7, 7), (1, 1), (n + 5, 1 << 20)):
            be = sc.NumpyBackend(v, max_count)
            try:
                index, values = sel.topk_select(be, k, largest, max_count, np_type)
            except ValueError as e:  # only the ties at the k-th value may refuse; checked below
                want_index, want_values = sc.ref_topk(v, k, largest)
                ties = int((v == want_values[-1]).sum())
                assert "tie" in str(e) and ties > max_count, (kind, k, max_count, str(e))
                continue
            sc.exact_topk(index, values, v, k, largest, np_type)
            assert be.widest <= max_count and be.calls["moments"] == 1
            assert be.calls["bin_counts"] + be.calls["count"] <= 12, be.calls
            if max_count >= n:
                assert be.calls["bin_counts"] == 0 and be.calls["find"] == 1  # everything fits: one find


def test_topk_select_completes_ties_and_refuses_too_many():
    v = np.zeros(1000, dtype=np.float32)
    v[[5, 400, 999]] = [3.0, 2.0, 3.0]
    v[[17, 600]] = -1.0
    # the 10 largest with room for the 995 zeros that tie at the k-th value: the three strictly better voxels from one
    # find, then the first seven zeros in C order from another
    be = sc.NumpyBackend(v, 995)
    index, values = sel.topk_select(be, 10, True, 995, np.float32)
    sc.exact_topk(index, values, v, 10, True, np.float32)
    assert list(index[:3]) == [5, 999, 400] and list(index[3:]) == [0, 1, 2, 3, 4, 6, 7]
    assert be.calls["find"] == 2 and be.widest == 995
    # the smallest: two strictly better, then zeros
    be = sc.NumpyBackend(v, 995)
    index, values = sel.topk_select(be, 4, False, 995, np.float32)
    sc.exact_topk(index, values, v, 4, False, np.float32)
    assert list(index) == [17, 600, 0, 1] and be.calls["find"] == 2
    # no strictly better voxel: one find of the ties
    be = sc.NumpyBackend(np.ones(500, dtype=np.float64), 499)
    with pytest.raises(ValueError, match="500 voxels tie at the k-th value 1.0"):
        sel.topk_select(be, 3, True, 499, np.float64)
    with pytest.raises(ValueError, match="995 voxels tie"):
        sel.topk_select(sc.NumpyBackend(v, 994), 10, True, 994, np.float32)
    with pytest.raises(ValueError, match="k = 20 voxels are more than max_count = 19"):
        sel.topk_select(sc.NumpyBackend(v, 19), 20, True, 19, np.float32)
    # fewer than k voxels are not NaN: all of them; none: nothing
    w = np.array([np.nan, 2.0, np.nan, -1.0], dtype=np.float32)
    index, values = sel.topk_select(sc.NumpyBackend(w, 10), 9, True, 10, np.float32)
    assert list(index) == [1, 3] and list(values) == [2.0, -1.0]
    index, values = sel.topk_select(sc.NumpyBackend(np.full(3, np.nan, dtype=np.float32), 10), 2, True, 10, np.float32)
    assert index.size == 0 and values.size == 0
