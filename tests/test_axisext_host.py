"""Extremes along axes from the cores, on the host (no GPU): the planner, the key encoding, the bars, the refusals.

* core/axisext.host_tables on the split tables of the oracle's index map: scattering the site-order reference through
  ``row_out[r] + col_out[c]`` and ``row_idx[r] + col_idx[c]`` (tests/axisext_cases.emulate, the epilogue in NumPy)
  gives NumPy's max, min, argmax and argmin for every axis and pair of axes; columns that share a cell are adjacent.
* a Python model of the order-preserving key: monotone from -inf over the denormals and the two zeros to +inf, never
  0, and the packed key prefers the smaller index.
* both bars accept the reference and reject modelled faults: a 64 x 64 tile left out (the first one on the integer
  cases, the one that holds the extreme of the product on the real ones), padding counted, the last
  occurrence instead of the first, ``col_idx`` dropped, the columns left unpermuted under permuted tables, NaN winning.
  A fault is rejected when the bar fails for at least one axis set and operation of the case.
* the refusals the C entries make before their first launch, with pointers that are never dereferenced.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import axisext_cases as ac
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import axisext as ax
from oracle import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_TILE = (slice(0, ac.TILE), slice(0, ac.TILE))


def _tables(c, axes):
    return ax.host_tables(*c.tables, c.shape, axes)


def _run_bar(c, exact, **fault):
    """The whole bar of a case on what the emulated epilogue returns under ``fault``."""
    for axes in ac.axis_sets(len(c.shape)):
        t = _tables(c, axes)
        for op in ac.OPS:
            values = ac.emulate(c.site, t, op, col_perm0=c.tables[2], **fault)
            (ac.exact_values if exact else ac.sandwich_values)(values, c.ref, *(() if exact else (c.bound,)), axes, op)
            if len(axes) == 1:
                where, again = ac.emulate(c.site, t, op, index=True, col_perm0=c.tables[2], **fault)
                assert np.array_equal(again, values, equal_nan=True)
                if exact:
                    ac.exact_index(where, c.ref, axes[0], op)
                else:
                    ac.sandwich_index(where, c.ref, c.bound, axes[0], op)


def _rejects(c, exact, **fault):
    with pytest.raises(AssertionError):
        _run_bar(c, exact, **fault)


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ac.SIGNED_NAMES)
def test_planner_tables_reproduce_numpy_and_the_exact_bar_has_teeth(name, storage):
    c = ac.int_case(name, storage)
    assert np.array_equal(c.ref, np.round(c.ref)) and np.abs(c.ref).max() < 2 ** 24
    row_off, col_off, perm = c.tables
    permuted = False
    for axes in ac.axis_sets(3):
        t = _tables(c, axes)
        assert t.out_shape == tuple(s for a, s in enumerate(c.shape) if a not in axes)
        assert t.row_out.dtype == t.col_out.dtype == np.int64 and t.col_perm.dtype == np.int32
        assert sorted(t.col_perm.tolist()) == list(range(c.n))
        # the columns of one cell are adjacent, and ascend in their coordinate
        assert np.all(np.diff(t.col_out) >= 0), "col_out is not sorted, so its runs are not contiguous"
        if len(axes) == 1:
            assert t.row_idx.dtype == t.col_idx.dtype == np.int32
            same = np.diff(t.col_out) == 0
            assert np.all(np.diff(t.col_idx)[same] > 0)
            at = (t.row_out[:, None] + t.col_out[None, :]).reshape(-1)
            idx = (t.row_idx[:, None] + t.col_idx[None, :]).reshape(-1)
            assert np.unique(at * c.shape[axes[0]] + idx).size == c.m * c.n, "two elements share a cell and a coordinate"
            assert idx.min() == 0 and idx.max() == c.shape[axes[0]] - 1
        else:
            assert t.row_idx is None and t.col_idx is None
        assert (t.row_out[:, None] + t.col_out[None, :]).min() == 0
        assert (t.row_out[:, None] + t.col_out[None, :]).max() == t.out_numel - 1
        permuted |= not np.array_equal(t.col_perm, perm)
    _run_bar(c, True)
    for op in ac.OPS:
        i, v = ac.ref_flat(c.ref, op)
        ac.exact_flat(i, v, c.ref, op)
        with pytest.raises(AssertionError):
            ties = np.flatnonzero(c.ref.reshape(-1) == v)  # the last of the tied places, or the place next to the only one
            ac.exact_flat(int(ties[-1]) if ties.size > 1 else (i + 1) % c.ref.size, v, c.ref, op)
    # the faults
    _rejects(c, True, skip=FIRST_TILE)
    _rejects(c, True, drop_col_idx=True)
    # the last site of int_tail_last lies wholly on axis 0: its 41 columns are in the planner's order as they come
    assert permuted == (name != "int_tail_last"), "which projections reorder the columns has changed"
    if permuted:
        _rejects(c, True, unpermuted=True)
    if max(ac.tied_share(c.ref, a, op) for a in range(3) for op in ac.OPS) > 0:
        _rejects(c, True, last=True)
    if name in ("int_positive", "int_negative"):
        lo, hi = (64, 2048) if name == "int_positive" else (-2048, -64)
        assert lo <= c.ref.min() and c.ref.max() <= hi and (c.m % ac.TILE or c.n % ac.TILE)
        _rejects(c, True, padding=True)


def test_the_integer_cases_are_what_the_issue_describes():
    shapes = {"int_8x7": ((128,) * 3, (512, 4096)), "int_wide": ((60, 16, 12), (8, 1440)),
              "int_tail_last": ((164, 30, 5), (600, 41)), "int_no_tail": ((48, 32, 64), (12, 8192)),
              "int_tail_all": ((10, 42, 6), (5, 504)), "int_positive": ((10, 42, 6), (5, 504))}
    assert set(shapes) == set(ac.INT_NAMES)
    tied = 0
    for name, (shape, mn) in shapes.items():
        c = ac.int_case(name, "f32")
        assert (c.shape, (c.m, c.n)) == (shape, mn), name
        share = max(ac.tied_share(c.ref, a, op) for a in range(3) for op in ac.OPS)
        tied += share >= 0.05
    assert tied >= 4, "the first-occurrence rule needs tied rays"
    c = ac.int_case("int_no_tail", "f32")
    i, v = ac.ref_flat(c.ref, "max")
    assert i == 2 and int((c.ref == v).sum()) == 8126


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_takes_no_part_and_a_nan_that_wins_is_rejected(name, storage):
    c = ac.int_case(name, storage).with_nan()
    nan = np.isnan(c.ref)
    assert any(nan.all(axis=a).any() for a in range(3)), "no ray of NaN only"
    assert any((nan.any(axis=a) & ~nan.all(axis=a)).any() for a in range(3)), "no partly NaN ray"
    _run_bar(c, True)
    for a in range(3):
        assert np.array_equal(ac.ref_index(c.ref, a, "max") == -1, nan.all(axis=a))
    _rejects(c, True, nan_wins=True)


# ------------------------------------------------------------------------------------------------ the keys
@pytest.mark.parametrize("bits", [32, 64])
def test_key_model_is_monotone_and_never_zero(bits):
    f = np.float32 if bits == 32 else np.float64
    tiny, small, big = np.finfo(f).smallest_subnormal, np.finfo(f).tiny, np.finfo(f).max
    ladder = [-np.inf, -big, -1.5, -1.0, -small, -tiny, 0.0, tiny, small, 1.0, 1.5, big, np.inf]
    up = [ac.key_of(v, "max", bits) for v in ladder]
    down = [ac.key_of(v, "min", bits) for v in ladder]
    assert all(a < b for a, b in zip(up, up[1:])) and all(a > b for a, b in zip(down, down[1:]))
    assert min(up + down) > 0 and max(up + down) < 2 ** bits
    assert ac.key_of(np.nan, "max", bits) == ac.key_of(-np.nan, "min", bits) == 0
    for op in ac.OPS:
        assert ac.key_of(-0.0, op, bits) == ac.key_of(0.0, op, bits)
        for v in ladder:
            assert ac.value_of(ac.key_of(v, op, bits), op, bits) == f(v)
        assert np.isnan(ac.value_of(0, op, bits))
    assert not np.signbit(ac.value_of(ac.key_of(-0.0, "max", bits), "max", bits))


def test_packed_key_prefers_the_larger_value_then_the_smaller_index():
    for op, better, worse in (("max", 2.0, 1.0), ("min", -3.0, 0.5)):
        assert ac.packed_key(better, 900, op) > ac.packed_key(worse, 0, op)
        assert ac.packed_key(better, 3, op) > ac.packed_key(better, 4, op) > ac.packed_key(better, 2 ** 31 - 1, op) > 0
        assert ac.packed_key(-0.0, 1, op) > ac.packed_key(0.0, 2, op)  # the zeros tie: the smaller index
        assert ac.packed_key(np.nan, 0, op) == 0


# ------------------------------------------------------------------------------------------------ the sandwich bar
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, family, storage):
    c = ac.real_case(name, family, storage)  # asserts the condition: at most 10 % of the rays are ambiguous
    shares = [ac.ambiguous_share(c.ref, c.bound, a, op) for a in range(2) for op in ac.OPS]
    print(f"[axisext] {name}/{family}/{storage}: shape {c.shape}, ambiguous rays {max(shares):.4f}")
    if storage == "f64":
        assert max(shares) == 0
    _run_bar(c, False)
    # a ray notices a missing tile only if its extreme sat there: leave out the tile of the extreme of the product
    _rejects(c, False, skip="extreme")
    if any(not np.array_equal(_tables(c, (a,)).col_perm, c.tables[2]) for a in range(2)):
        _rejects(c, False, unpermuted=True)
    if any(_tables(c, (a,)).col_idx.any() for a in range(2)):
        _rejects(c, False, drop_col_idx=True)


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_binding_and_library_agree():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("ndmps_axisext_", "ndmps_argext_")))
    assert names == ["ndmps_argext_f32", "ndmps_argext_f64", "ndmps_axisext_f32", "ndmps_axisext_f64"]
    for name in names:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, f"{name} is not declared in include/ndmps_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)


def test_refusals_before_any_launch():
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    lib = _lib.load()
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[256] * L)
    p = C.c_void_p(256)
    value, flat = C.c_double(), C.c_int64()
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    big = 1 << 30
    for suffix, eb in (("f32", 4), ("f64", 8)):
        need = lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)
        axis = getattr(lib, f"ndmps_axisext_{suffix}")
        arg = getattr(lib, f"ndmps_argext_{suffix}")

        def call_axis(bonds_=b, ws=p, nbytes=big, op=0, cols=n_cols, ridx=p, cidx=p, index=p, cores=fake, values=p):
            return axis(L, d, bonds_, cores, op, p, p, p, cols, ridx, cidx, 1755, values, index, ws, nbytes, None)

        def call_values(**kw):
            return call_axis(ridx=None, cidx=None, index=None, **kw)

        def call_arg(bonds_=b, ws=p, nbytes=big, op=0, cols=n_cols, cores=fake):
            return arg(L, d, bonds_, cores, op, p, p, p, cols, C.byref(value), C.byref(flat), ws, nbytes, None)

        for what, call in (("axis", call_axis), ("values", call_values), ("arg", call_arg)):
            assert call(nbytes=need - 1) == _lib.EWORKSPACE, what
            assert call(ws=None) == _lib.EWORKSPACE, what
            assert call(ws=C.c_void_p(264)) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error(), what
            for bad in ([1, 4, 13, 13, 1], [1, 3, 13, 65, 1], [1, 3, 0, 13, 1]):
                assert call(bonds_=_lib.i64_array(bad)) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error(), (what, bad)
            for bad in ([2, 3, 13, 13, 1], [1, 3, 13, 13, 2]):
                assert call(bonds_=_lib.i64_array(bad)) == _lib.EINVAL and b"boundary" in lib.ndmps_last_error(), (what, bad)
            assert call(cols=n_cols * dims[-2]) == _lib.EINVAL and b"columns" in lib.ndmps_last_error(), what
            for op in (-1, 2):
                assert call(op=op) == _lib.EINVAL and b"neither" in lib.ndmps_last_error(), (what, op)
            assert call(cores=None) == _lib.EINVAL, what
        # the index tables and d_index are given together or not at all
        for kw in (dict(index=None), dict(ridx=None), dict(cidx=None), dict(ridx=None, cidx=None),
                   dict(ridx=None, index=None), dict(cidx=None, index=None)):
            assert call_axis(**kw) == _lib.EINVAL and b"together" in lib.ndmps_last_error(), kw
        assert call_axis(values=None) == _lib.EINVAL
        assert axis(L, d, b, fake, 0, p, p, p, n_cols, None, None, 0, p, None, p, big, None) == _lib.EINVAL
        assert axis(L, d, b, fake, 0, None, p, p, n_cols, None, None, 9, p, None, p, big, None) == _lib.EINVAL
        assert arg(L, d, b, fake, 0, p, None, p, n_cols, C.byref(value), C.byref(flat), p, big, None) == _lib.EINVAL
        assert arg(L, d, b, fake, 0, p, p, p, n_cols, None, C.byref(flat), p, big, None) == _lib.EINVAL
        assert arg(0, d, b, fake, 0, p, p, p, n_cols, C.byref(value), C.byref(flat), p, big, None) == _lib.EINVAL
