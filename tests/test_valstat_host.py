"""Value statistics from the cores, on the host (no GPU): the plan, the cases and the bars of tests/valstat_cases.py.

* chain_stats_plan (csrc/valstat_plan.h) through ndmps_valstat_plan_query: the products and order of chain_plan, the
  two differences (the last product has no destination, the output's turns as an intermediate go to the second left
  buffer), no product writes a buffer it reads, the workspace is the sum of its parts.
* the condition of the sandwich bar, from the reference alone: at most 1 % of the voxels lie within their bound of
  one of the edges the cases use (64 uniform bins over the reference's range; fewer where 64 break the condition).
* the bars accept the reference and reject every modelled fault (a tile left out, padding counted, the last bin open,
  bins shifted by one, the original read in site order, NaN in a bin) on every case the fault can occur on.  Two of
  them are applied on the integer cases only.  NaN in a bin needs NaN voxels, and only the integer cases plant one.
  The open last bin needs a voxel ON the last edge: on the real cases that is the largest voxel alone, whose computed
  value may lie a bound above the edge anyway, so the sandwich cannot tell an open bin from roundoff there (and the
  chains small enough for bound 0 have their range widened, so no voxel sits on an edge); the exact bar, whose
  edge sets end on the maximum, rejects it.
* the refusals the entries make before their first launch, with pointers that are never dereferenced.
* pinned answers: code and whole message of every such refusal of the six single-chain entries (value statistics,
  extremes, label statistics), and the workspace and plan of every chain, as literals.
"""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import valstat_cases as vc
from imgcompressionmps_amd import _lib
from oracle import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS_LEFT, WS_TAIL0, WS_TAIL1, OUT, NONE, WS_LEFT2, UNIT = -1, -2, -3, -4, -5, -6, -7
ELEMS = {"f32": 0, "f64": 2}
HEAD = ("j0", "tail_cols", "n_products", "left_elems", "tail_elems", "decode_bytes", "left2_bytes", "reduce_bytes", "bytes")
ROW = ("kind", "m", "n", "k", "a", "b", "c", "spare")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _decode_plan(lib, dims, bonds, elem):
    L = len(dims)
    out = (C.c_int64 * (6 + 8 * (L - 1)))()
    assert lib.ndmps_chain_plan_query(ELEMS[elem], L, _lib.i64_array(dims), _lib.i64_array(bonds), out) == _lib.OK
    return list(out[:6]), [dict(zip(ROW, out[6 + 8 * q:14 + 8 * q])) for q in range(out[2])]


def _stats_plan(lib, dims, bonds, elem, n_bins=0):
    L = len(dims)
    out = (C.c_int64 * (9 + 8 * L))()
    assert lib.ndmps_valstat_plan_query(ELEMS[elem], L, _lib.i64_array(dims), _lib.i64_array(bonds), n_bins, out) == _lib.OK
    head = dict(zip(HEAD, out[:9]))
    rows = [dict(zip(ROW, out[9 + 8 * q:17 + 8 * q])) for q in range(head["n_products"] + 1)]
    return head, rows[:-1], rows[-1]


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("elem", sorted(ELEMS))
@pytest.mark.parametrize("name", sorted(vc.ALL_CHAINS))
def test_stats_plan_is_the_decode_plan_with_two_differences(lib, name, elem):
    dims, bonds = vc.ALL_CHAINS[name]
    L = len(dims)
    dhead, dprod = _decode_plan(lib, dims, bonds, elem)
    head, prod, reduced = _stats_plan(lib, dims, bonds, elem)
    assert [head[k] for k in HEAD[:6]] == dhead
    assert len(prod) == len(dprod) == L - 1
    for q, (s, d) in enumerate(zip(prod, dprod)):
        last = q == L - 2
        assert (s["kind"], s["m"], s["n"], s["k"], s["b"], s["spare"]) == (d["kind"], d["m"], d["n"], d["k"], d["b"], d["spare"])
        assert s["a"] == (WS_LEFT2 if d["a"] == OUT else d["a"])
        assert s["c"] == (NONE if last else WS_LEFT2 if d["c"] == OUT else d["c"])
        assert not last or d["c"] == OUT
    if L == 1:
        assert (reduced["m"], reduced["n"], reduced["k"], reduced["a"], reduced["b"], reduced["c"]) == (1, dims[0], 1, UNIT, 0, NONE)
    else:
        assert reduced == prod[-1] and reduced["c"] == NONE
    assert (reduced["m"], reduced["n"]) == vc.last_product_shape(dims)

    # no product writes a buffer it reads, every operand was written, every destination has room
    capacity = {WS_LEFT: head["left_elems"], WS_LEFT2: head["left_elems"], WS_TAIL0: head["tail_elems"],
                WS_TAIL1: head["tail_elems"]}
    written = set(range(L)) | {UNIT}
    for q, p in enumerate(prod + ([reduced] if L == 1 else [])):
        assert p["a"] in written and p["b"] in written, f"product {q} reads a buffer nothing wrote"
        assert p["c"] not in (p["a"], p["b"], OUT), f"product {q} writes a buffer it reads, or the output"
        if p["c"] != NONE:
            assert p["m"] * p["n"] <= capacity[p["c"]], f"product {q} does not fit its destination"
            written.add(p["c"])
    if reduced["spare"] != NONE:
        assert reduced["spare"] in (WS_TAIL0, WS_TAIL1) and reduced["spare"] != reduced["b"]
        assert reduced["k"] * reduced["n"] <= head["tail_elems"]


@pytest.mark.parametrize("n_bins", [0, 1, 256, 4096])
@pytest.mark.parametrize("elem", sorted(ELEMS))
@pytest.mark.parametrize("name", sorted(vc.ALL_CHAINS))
def test_workspace_query_is_the_sum_of_its_parts(lib, name, elem, n_bins):
    dims, bonds = vc.ALL_CHAINS[name]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    eb = 8 if elem == "f64" else 4
    head, _, _ = _stats_plan(lib, dims, bonds, elem, n_bins)
    decode = (lib.ndmps_chain_workspace_bytes_f64 if elem == "f64" else lib.ndmps_chain_workspace_bytes)(L, d, b)
    assert head["decode_bytes"] == decode
    assert head["left2_bytes"] == -(-head["left_elems"] // 64) * 64 * eb
    # the unit operand, 512 partial records and the result, then the counters and the edges of the histogram
    r256 = lambda x: -(-x // 256) * 256  # noqa: E731
    assert head["reduce_bytes"] == 256 + 512 * 64 + 256 + r256((n_bins + 3) * 8) + r256((n_bins + 1) * eb)
    assert head["bytes"] == head["decode_bytes"] + head["left2_bytes"] + head["reduce_bytes"]
    assert lib.ndmps_valstat_workspace_bytes(L, d, b, eb, n_bins) == head["bytes"]


def test_workspace_of_the_two_million_voxel_case_is_a_fraction_of_the_volume(lib):
    dims, bonds = vc.INT_EXTRA["int_8x7"]
    numel = int(np.prod(dims))
    assert numel == 2 ** 21 and int(np.prod(bonds)) == 4194304 < 2 ** 24
    got = lib.ndmps_valstat_workspace_bytes(len(dims), _lib.i64_array(dims), _lib.i64_array(bonds), 4, 4096)
    assert 0 < got < numel * 4 // 4


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("ndmps_valstat_"))
    assert len(names) == 8
    for name in names:
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, f"{name} is not declared in include/ndmps_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)


def test_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[256] * L)
    p = C.c_void_p(256)
    stats, counts = (C.c_double * 4)(), (C.c_int64 * 4100)()
    inf = float("inf")
    for suffix, eb, arr in (("f32", 4, C.c_float), ("f64", 8, C.c_double)):
        need = lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)
        need_h = lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 4)
        assert need_h >= need > 0
        mom = getattr(lib, f"ndmps_valstat_moments_{suffix}")
        hist = getattr(lib, f"ndmps_valstat_histogram_{suffix}")
        err = getattr(lib, f"ndmps_valstat_error_{suffix}")
        edges = (arr * 5)(0, 1, 2, 3, 4)
        n_cols = lib.ndmps_chain_tail_columns(L, d)
        calls = {
            "moments": lambda bonds_, ws, nbytes: mom(L, d, bonds_, fake, -inf, inf, stats, counts, ws, nbytes, None),
            "histogram": lambda bonds_, ws, nbytes: hist(L, d, bonds_, fake, edges, 4, counts, ws, nbytes, None),
            "error": lambda bonds_, ws, nbytes: err(L, d, bonds_, fake, p, p, p, p, n_cols, stats, counts, ws, nbytes, None),
        }
        for what, call in calls.items():
            assert call(b, p, (need_h if what == "histogram" else need) - 1) == _lib.EWORKSPACE, what
            assert call(b, None, 1 << 30) == _lib.EWORKSPACE, what
            assert call(b, C.c_void_p(264), 1 << 30) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error(), what
            for bad in ([1, 4, 13, 13, 1], [1, 3, 13, 65, 1], [1, 3, 0, 13, 1]):
                assert call(_lib.i64_array(bad), p, 1 << 30) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error(), (what, bad)
            for bad in ([2, 3, 13, 13, 1], [1, 3, 13, 13, 2]):
                assert call(_lib.i64_array(bad), p, 1 << 30) == _lib.EINVAL and b"boundary" in lib.ndmps_last_error(), (what, bad)
        assert mom(L, d, b, None, -inf, inf, stats, counts, p, 1 << 30, None) == _lib.EINVAL
        assert mom(L, d, b, fake, float("nan"), inf, stats, counts, p, 1 << 30, None) == _lib.EINVAL
        assert mom(0, d, b, fake, -inf, inf, stats, counts, p, 1 << 30, None) == _lib.EINVAL
        # the histogram's edges: too many, too few, descending, NaN
        assert hist(L, d, b, fake, edges, 4097, counts, p, 1 << 30, None) == _lib.EINVAL and b"bins" in lib.ndmps_last_error()
        assert hist(L, d, b, fake, edges, 0, counts, p, 1 << 30, None) == _lib.EINVAL
        assert hist(L, d, b, fake, (arr * 5)(0, 1, 3, 2, 4), 4, counts, p, 1 << 30, None) == _lib.EINVAL
        assert b"ascending" in lib.ndmps_last_error()
        assert hist(L, d, b, fake, (arr * 5)(0, 1, float("nan"), 3, 4), 4, counts, p, 1 << 30, None) == _lib.EINVAL
        assert hist(L, d, b, fake, None, 4, counts, p, 1 << 30, None) == _lib.EINVAL
        # the error's tables: another split of the sites, a missing table, a missing original
        assert err(L, d, b, fake, p, p, p, p, n_cols * dims[-2], stats, counts, p, 1 << 30, None) == _lib.EINVAL
        assert b"columns" in lib.ndmps_last_error()
        assert err(L, d, b, fake, p, None, p, p, n_cols, stats, counts, p, 1 << 30, None) == _lib.EINVAL
        assert err(L, d, b, fake, None, p, p, p, n_cols, stats, counts, p, 1 << 30, None) == _lib.EINVAL
    assert lib.ndmps_valstat_workspace_bytes(L, d, b, 2, 0) == 0
    assert lib.ndmps_valstat_workspace_bytes(L, d, b, 4, 4097) == 0
    out = (C.c_int64 * (9 + 8 * L))()
    assert lib.ndmps_valstat_plan_query(1, L, d, b, 0, out) == _lib.EINVAL  # bf16 has no statistics entry
    assert lib.ndmps_valstat_plan_query(0, L, d, b, 0, None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ pinned answers
# What the single-chain entries (moments, histogram, error, the extremes along axes, the place of the global extreme,
# the label statistics) answer before their first HIP call, as literals: return code and the whole message, in the
# order the checks are made (where two faults compete, the one checked first wins), and the sizes and plans of every
# chain.  Taken from the build before the family got its shared host prologue; a change of any of them is a change
# of behaviour.
def _digest(values):
    return hashlib.sha256(np.asarray(list(values), dtype=np.int64).tobytes()).hexdigest()[:16]


def refusal_calls(lib, suffix):
    """name -> call, each refused before the first HIP call (the pointers are fakes)."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    eb, arr = (4, C.c_float) if suffix == "f32" else (8, C.c_double)
    fake = (C.c_void_p * L)(*[256] * L)
    hole = (C.c_void_p * L)(256, 256, None, 256)
    p, big = 256, 1 << 30
    stats, counts = (C.c_double * 4)(), (C.c_int64 * 4100)()
    value, flat = C.c_double(), C.c_int64()
    host = np.zeros(2 * 4096, dtype=np.int64)
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    need = lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)
    up, nan, inf = _lib.i64_array([1, 4, 13, 13, 1]), float("nan"), float("inf")
    edges, down, hurt = (arr * 5)(0, 1, 2, 3, 4), (arr * 5)(0, 1, 3, 2, 4), (arr * 5)(0, 1, nan, 3, 4)
    entry = lambda name: getattr(lib, f"ndmps_{name}_{suffix}")  # noqa: E731

    def mom(L=L, d=d, b=b, cores=fake, lo=-inf, hi=inf, stats=stats, ws=p, nbytes=big):
        return entry("valstat_moments")(L, d, b, cores, lo, hi, stats, counts, ws, nbytes, None)

    def hist(L=L, b=b, cores=fake, e=edges, bins=4, out=counts, ws=p, nbytes=big):
        return entry("valstat_histogram")(L, d, b, cores, e, bins, out, ws, nbytes, None)

    def err(L=L, b=b, cores=fake, ref=p, row=p, col=p, perm=p, cols=n_cols, ws=p, nbytes=big):
        return entry("valstat_error")(L, d, b, cores, ref, row, col, perm, cols, stats, counts, ws, nbytes, None)

    def axis(L=L, b=b, cores=fake, op=0, row=p, col=p, perm=p, cols=n_cols, ridx=None, cidx=None, numel=64, values=p,
             index=None, ws=p, nbytes=big):
        return entry("axisext")(L, d, b, cores, op, row, col, perm, cols, ridx, cidx, numel, values, index, ws, nbytes, None)

    def arg(L=L, b=b, cores=fake, op=0, row=p, col=p, perm=p, cols=n_cols, value=C.byref(value), ws=p, nbytes=big):
        return entry("argext")(L, d, b, cores, op, row, col, perm, cols, value, C.byref(flat), ws, nbytes, None)

    def lab(L=L, b=b, cores=fake, labels=p, width=2, row=p, col=p, perm=p, cols=n_cols, n_labels=7, sums=host.ctypes.data,
            ws=p, nbytes=big):
        h = host.ctypes.data
        return entry("labelstat")(L, d, b, cores, labels, width, row, col, perm, cols, n_labels, sums, h, h, h, h, ws, nbytes, None)

    calls = {}
    for name, f in (("moments", mom), ("histogram", hist), ("error", err), ("axisext", axis), ("argext", arg), ("labelstat", lab)):
        calls.update({  # the chain and the workspace, as every entry checks them
            f"{name}/no_sites": lambda f=f: f(L=0),
            f"{name}/no_bonds": lambda f=f: f(b=None),
            f"{name}/no_cores": lambda f=f: f(cores=None),
            f"{name}/core_2_null": lambda f=f: f(cores=hole),
            f"{name}/boundary": lambda f=f: f(b=_lib.i64_array([1, 3, 13, 13, 2])),
            f"{name}/bond_exceeds": lambda f=f: f(b=up),
            f"{name}/bond_zero": lambda f=f: f(b=_lib.i64_array([1, 3, 0, 13, 1])),
            f"{name}/workspace_null": lambda f=f: f(ws=None),
            f"{name}/workspace_short": lambda f=f: f(nbytes=need - 1),
            f"{name}/workspace_misaligned": lambda f=f: f(ws=264),
            f"{name}/bond_exceeds_and_workspace_short": lambda f=f: f(b=up, nbytes=1),
            f"{name}/workspace_short_and_misaligned": lambda f=f: f(ws=264, nbytes=1),
        })
    calls.update({
        "moments/no_dims": lambda: mom(d=None),
        "moments/no_result": lambda: mom(stats=None),
        "moments/clip_nan": lambda: mom(lo=nan),
        "moments/clip_nan_and_no_sites": lambda: mom(L=0, hi=nan),
        "moments/clip_nan_and_bond_exceeds": lambda: mom(hi=nan, b=up),
        "histogram/no_edges": lambda: hist(e=None),
        "histogram/no_counts": lambda: hist(out=None),
        "histogram/no_bins": lambda: hist(bins=0),
        "histogram/too_many_bins": lambda: hist(bins=4097),
        "histogram/edges_descend": lambda: hist(e=down),
        "histogram/edge_nan": lambda: hist(e=hurt),
        "histogram/too_many_bins_and_workspace_short": lambda: hist(bins=4097, nbytes=1),
        "histogram/edges_descend_and_bond_exceeds": lambda: hist(e=down, b=up),
        "error/no_original": lambda: err(ref=None),
        "error/no_row_table": lambda: err(row=None),
        "error/no_col_table": lambda: err(col=None),
        "error/no_col_perm": lambda: err(perm=None),
        "error/other_columns": lambda: err(cols=n_cols * dims[-2]),
        "error/no_table_and_other_columns": lambda: err(col=None, cols=n_cols + 1),
        "error/other_columns_and_workspace_short": lambda: err(cols=n_cols + 1, nbytes=1),
        "error/no_table_and_misaligned": lambda: err(row=None, ws=264),
        "axisext/op": lambda: axis(op=2),
        "axisext/no_row_table": lambda: axis(row=None),
        "axisext/no_col_perm": lambda: axis(perm=None),
        "axisext/no_values": lambda: axis(values=None),
        "axisext/empty_result": lambda: axis(numel=0),
        "axisext/index_without_tables": lambda: axis(index=p),
        "axisext/tables_without_index": lambda: axis(ridx=p, cidx=p),
        "axisext/one_index_table": lambda: axis(ridx=p, index=p),
        "axisext/other_columns": lambda: axis(cols=n_cols + 1),
        "axisext/op_and_no_table": lambda: axis(op=-1, col=None),
        "axisext/no_table_and_other_columns": lambda: axis(perm=None, cols=n_cols + 1),
        "axisext/index_without_tables_and_workspace_short": lambda: axis(index=p, nbytes=1),
        "axisext/other_columns_and_workspace_short": lambda: axis(cols=n_cols + 1, nbytes=1),
        "argext/op": lambda: arg(op=2),
        "argext/no_value": lambda: arg(value=None),
        "argext/no_row_table": lambda: arg(row=None),
        "argext/no_col_table": lambda: arg(col=None),
        "argext/no_col_perm": lambda: arg(perm=None),
        "argext/other_columns": lambda: arg(cols=n_cols + 1),
        "argext/op_and_bond_exceeds": lambda: arg(op=7, b=up),
        "argext/no_table_and_other_columns": lambda: arg(col=None, cols=n_cols + 1),
        "argext/other_columns_and_workspace_short": lambda: arg(cols=n_cols + 1, nbytes=1),
        "labelstat/no_result": lambda: lab(sums=None),
        "labelstat/no_labels_at_all": lambda: lab(n_labels=0),
        "labelstat/too_many_labels": lambda: lab(n_labels=4097),
        "labelstat/label_width": lambda: lab(width=3),
        "labelstat/too_many_labels_and_label_width": lambda: lab(n_labels=4097, width=8),
        "labelstat/label_width_and_bond_exceeds": lambda: lab(width=0, b=up),
        "labelstat/no_label_volume": lambda: lab(labels=None),
        "labelstat/no_col_perm": lambda: lab(perm=None),
        "labelstat/other_columns": lambda: lab(cols=n_cols + 1),
        "labelstat/no_table_and_other_columns": lambda: lab(row=None, cols=n_cols + 1),
        "labelstat/room_for_the_chain_not_the_table": lambda: lab(nbytes=need),
        "labelstat/other_columns_and_no_room_for_the_table": lambda: lab(cols=n_cols + 1, nbytes=need),
        "labelstat/workspace_short_and_other_columns": lambda: lab(cols=n_cols + 1, nbytes=need - 1),
    })
    return calls


def refusals(lib):
    out = {}
    for suffix in ("f32", "f64"):
        for name, call in refusal_calls(lib, suffix).items():
            rc = call()
            out[f"{name}/{suffix}"] = (rc, lib.ndmps_last_error().decode() if rc != _lib.OK else "")
    return out


def sizes(lib):
    """name -> per element type: the workspace at 0 and 4096 bins, the label statistics' at 1500 labels, and a digest
    of the plan query's answer at 0 and at 256 bins."""
    out = {}
    for name, (dims, bonds) in sorted(vc.ALL_CHAINS.items()):
        L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
        row = []
        for elem, eb in (("f32", 4), ("f64", 8)):
            row += [lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0), lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 4096),
                    lib.ndmps_labelstat_workspace_bytes(L, d, b, eb, 1500)]
            for n_bins in (0, 256):
                plan = (C.c_int64 * (9 + 8 * L))()
                assert lib.ndmps_valstat_plan_query(ELEMS[elem], L, d, b, n_bins, plan) == _lib.OK
                row.append(_digest(plan))
        out[name] = tuple(row)
    return out


REFUSED = {'moments/no_sites/f32': (-1, 'bad valstat argument'),
 'moments/no_bonds/f32': (-1, 'bad valstat argument'),
 'moments/no_cores/f32': (-1, 'bad valstat argument'),
 'moments/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'moments/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'moments/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'moments/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'moments/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'moments/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'moments/bond_exceeds_and_workspace_short/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'histogram/no_sites/f32': (-1, 'bad valstat argument'),
 'histogram/no_bonds/f32': (-1, 'bad valstat argument'),
 'histogram/no_cores/f32': (-1, 'bad valstat argument'),
 'histogram/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'histogram/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'histogram/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'histogram/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'histogram/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'histogram/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'histogram/bond_exceeds_and_workspace_short/f32': (-1,
                                                    'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'error/no_sites/f32': (-1, 'bad valstat argument'),
 'error/no_bonds/f32': (-1, 'bad valstat argument'),
 'error/no_cores/f32': (-1, 'bad valstat argument'),
 'error/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'error/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'error/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'error/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'error/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'error/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'error/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'error/bond_exceeds_and_workspace_short/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'error/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'axisext/no_sites/f32': (-1, 'bad axisext argument'),
 'axisext/no_bonds/f32': (-1, 'bad axisext argument'),
 'axisext/no_cores/f32': (-1, 'bad valstat argument'),
 'axisext/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'axisext/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'axisext/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'axisext/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'axisext/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'axisext/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'axisext/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'axisext/bond_exceeds_and_workspace_short/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'axisext/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'argext/no_sites/f32': (-1, 'bad argext argument'),
 'argext/no_bonds/f32': (-1, 'bad argext argument'),
 'argext/no_cores/f32': (-1, 'bad valstat argument'),
 'argext/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'argext/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'argext/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'argext/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'argext/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'argext/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'argext/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'argext/bond_exceeds_and_workspace_short/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'argext/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'labelstat/no_sites/f32': (-1, 'bad labelstat argument'),
 'labelstat/no_bonds/f32': (-1, 'bad labelstat argument'),
 'labelstat/no_cores/f32': (-1, 'bad valstat argument'),
 'labelstat/core_2_null/f32': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'labelstat/boundary/f32': (-1, 'open boundary bonds must be 1'),
 'labelstat/bond_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'labelstat/bond_zero/f32': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'labelstat/workspace_null/f32': (-4, 'valstat workspace too small: 1073741824 < 246272'),
 'labelstat/workspace_short/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'labelstat/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'labelstat/bond_exceeds_and_workspace_short/f32': (-1,
                                                    'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'labelstat/workspace_short_and_misaligned/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'moments/no_dims/f32': (-1, 'bad valstat argument'),
 'moments/no_result/f32': (-1, 'bad valstat argument'),
 'moments/clip_nan/f32': (-1, 'moments: the clip range must not be NaN'),
 'moments/clip_nan_and_no_sites/f32': (-1, 'bad valstat argument'),
 'moments/clip_nan_and_bond_exceeds/f32': (-1, 'moments: the clip range must not be NaN'),
 'histogram/no_edges/f32': (-1, 'bad valstat argument'),
 'histogram/no_counts/f32': (-1, 'bad valstat argument'),
 'histogram/no_bins/f32': (-1, 'histogram: 0 bins outside [1, 4096]'),
 'histogram/too_many_bins/f32': (-1, 'histogram: 4097 bins outside [1, 4096]'),
 'histogram/edges_descend/f32': (-1, 'histogram: edges must be ascending and not NaN (edge 3)'),
 'histogram/edge_nan/f32': (-1, 'histogram: edges must be ascending and not NaN (edge 2)'),
 'histogram/too_many_bins_and_workspace_short/f32': (-1, 'histogram: 4097 bins outside [1, 4096]'),
 'histogram/edges_descend_and_bond_exceeds/f32': (-1, 'histogram: edges must be ascending and not NaN (edge 3)'),
 'error/no_original/f32': (-1, 'NULL original or offset table'),
 'error/no_row_table/f32': (-1, 'NULL original or offset table'),
 'error/no_col_table/f32': (-1, 'NULL original or offset table'),
 'error/no_col_perm/f32': (-1, 'NULL original or offset table'),
 'error/other_columns/f32': (-1, 'offset tables are for 4160 columns, the last product has 64'),
 'error/no_table_and_other_columns/f32': (-1, 'NULL original or offset table'),
 'error/other_columns_and_workspace_short/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'error/no_table_and_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'axisext/op/f32': (-1, 'axisext: op 2 is neither 0 (max) nor 1 (min)'),
 'axisext/no_row_table/f32': (-1, 'axisext: NULL table or result'),
 'axisext/no_col_perm/f32': (-1, 'axisext: NULL table or result'),
 'axisext/no_values/f32': (-1, 'axisext: NULL table or result'),
 'axisext/empty_result/f32': (-1, 'axisext: NULL table or result'),
 'axisext/index_without_tables/f32': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/tables_without_index/f32': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/one_index_table/f32': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/other_columns/f32': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'axisext/op_and_no_table/f32': (-1, 'axisext: op -1 is neither 0 (max) nor 1 (min)'),
 'axisext/no_table_and_other_columns/f32': (-1, 'axisext: NULL table or result'),
 'axisext/index_without_tables_and_workspace_short/f32': (-1,
                                                          'axisext: the index tables and d_index are given together or not '
                                                          'at all'),
 'axisext/other_columns_and_workspace_short/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'argext/op/f32': (-1, 'argext: op 2 is neither 0 (max) nor 1 (min)'),
 'argext/no_value/f32': (-1, 'bad argext argument'),
 'argext/no_row_table/f32': (-1, 'NULL original or offset table'),
 'argext/no_col_table/f32': (-1, 'NULL original or offset table'),
 'argext/no_col_perm/f32': (-1, 'NULL original or offset table'),
 'argext/other_columns/f32': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'argext/op_and_bond_exceeds/f32': (-1, 'argext: op 7 is neither 0 (max) nor 1 (min)'),
 'argext/no_table_and_other_columns/f32': (-1, 'NULL original or offset table'),
 'argext/other_columns_and_workspace_short/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'labelstat/no_result/f32': (-1, 'bad labelstat argument'),
 'labelstat/no_labels_at_all/f32': (-1, 'label statistics take 1 to 4096 labels, got 0'),
 'labelstat/too_many_labels/f32': (-1, 'label statistics take 1 to 4096 labels, got 4097'),
 'labelstat/label_width/f32': (-1, 'labels are uint8, int16 or int32 (1, 2 or 4 bytes), got 3 bytes'),
 'labelstat/too_many_labels_and_label_width/f32': (-1, 'label statistics take 1 to 4096 labels, got 4097'),
 'labelstat/label_width_and_bond_exceeds/f32': (-1, 'labels are uint8, int16 or int32 (1, 2 or 4 bytes), got 0 bytes'),
 'labelstat/no_label_volume/f32': (-1, 'NULL original or offset table'),
 'labelstat/no_col_perm/f32': (-1, 'NULL original or offset table'),
 'labelstat/other_columns/f32': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'labelstat/no_table_and_other_columns/f32': (-1, 'NULL original or offset table'),
 'labelstat/room_for_the_chain_not_the_table/f32': (-4, 'labelstat workspace too small: 246272 < 246784'),
 'labelstat/other_columns_and_no_room_for_the_table/f32': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'labelstat/workspace_short_and_other_columns/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'moments/no_sites/f64': (-1, 'bad valstat argument'),
 'moments/no_bonds/f64': (-1, 'bad valstat argument'),
 'moments/no_cores/f64': (-1, 'bad valstat argument'),
 'moments/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'moments/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'moments/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'moments/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'moments/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'moments/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'moments/bond_exceeds_and_workspace_short/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'histogram/no_sites/f64': (-1, 'bad valstat argument'),
 'histogram/no_bonds/f64': (-1, 'bad valstat argument'),
 'histogram/no_cores/f64': (-1, 'bad valstat argument'),
 'histogram/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'histogram/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'histogram/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'histogram/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'histogram/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'histogram/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'histogram/bond_exceeds_and_workspace_short/f64': (-1,
                                                    'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'error/no_sites/f64': (-1, 'bad valstat argument'),
 'error/no_bonds/f64': (-1, 'bad valstat argument'),
 'error/no_cores/f64': (-1, 'bad valstat argument'),
 'error/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'error/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'error/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'error/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'error/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'error/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'error/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'error/bond_exceeds_and_workspace_short/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'error/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'axisext/no_sites/f64': (-1, 'bad axisext argument'),
 'axisext/no_bonds/f64': (-1, 'bad axisext argument'),
 'axisext/no_cores/f64': (-1, 'bad valstat argument'),
 'axisext/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'axisext/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'axisext/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'axisext/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'axisext/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'axisext/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'axisext/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'axisext/bond_exceeds_and_workspace_short/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'axisext/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'argext/no_sites/f64': (-1, 'bad argext argument'),
 'argext/no_bonds/f64': (-1, 'bad argext argument'),
 'argext/no_cores/f64': (-1, 'bad valstat argument'),
 'argext/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'argext/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'argext/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'argext/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'argext/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'argext/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'argext/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'argext/bond_exceeds_and_workspace_short/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'argext/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'labelstat/no_sites/f64': (-1, 'bad labelstat argument'),
 'labelstat/no_bonds/f64': (-1, 'bad labelstat argument'),
 'labelstat/no_cores/f64': (-1, 'bad valstat argument'),
 'labelstat/core_2_null/f64': (-1, 'dims[2] must be positive and core 2 non-NULL'),
 'labelstat/boundary/f64': (-1, 'open boundary bonds must be 1'),
 'labelstat/bond_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'labelstat/bond_zero/f64': (-1, 'bond 2 = 0 exceeds min(27, 4160), the rank any unfolding can have'),
 'labelstat/workspace_null/f64': (-4, 'valstat workspace too small: 1073741824 < 435712'),
 'labelstat/workspace_short/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'labelstat/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'labelstat/bond_exceeds_and_workspace_short/f64': (-1,
                                                    'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'labelstat/workspace_short_and_misaligned/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'moments/no_dims/f64': (-1, 'bad valstat argument'),
 'moments/no_result/f64': (-1, 'bad valstat argument'),
 'moments/clip_nan/f64': (-1, 'moments: the clip range must not be NaN'),
 'moments/clip_nan_and_no_sites/f64': (-1, 'bad valstat argument'),
 'moments/clip_nan_and_bond_exceeds/f64': (-1, 'moments: the clip range must not be NaN'),
 'histogram/no_edges/f64': (-1, 'bad valstat argument'),
 'histogram/no_counts/f64': (-1, 'bad valstat argument'),
 'histogram/no_bins/f64': (-1, 'histogram: 0 bins outside [1, 4096]'),
 'histogram/too_many_bins/f64': (-1, 'histogram: 4097 bins outside [1, 4096]'),
 'histogram/edges_descend/f64': (-1, 'histogram: edges must be ascending and not NaN (edge 3)'),
 'histogram/edge_nan/f64': (-1, 'histogram: edges must be ascending and not NaN (edge 2)'),
 'histogram/too_many_bins_and_workspace_short/f64': (-1, 'histogram: 4097 bins outside [1, 4096]'),
 'histogram/edges_descend_and_bond_exceeds/f64': (-1, 'histogram: edges must be ascending and not NaN (edge 3)'),
 'error/no_original/f64': (-1, 'NULL original or offset table'),
 'error/no_row_table/f64': (-1, 'NULL original or offset table'),
 'error/no_col_table/f64': (-1, 'NULL original or offset table'),
 'error/no_col_perm/f64': (-1, 'NULL original or offset table'),
 'error/other_columns/f64': (-1, 'offset tables are for 4160 columns, the last product has 64'),
 'error/no_table_and_other_columns/f64': (-1, 'NULL original or offset table'),
 'error/other_columns_and_workspace_short/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'error/no_table_and_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'axisext/op/f64': (-1, 'axisext: op 2 is neither 0 (max) nor 1 (min)'),
 'axisext/no_row_table/f64': (-1, 'axisext: NULL table or result'),
 'axisext/no_col_perm/f64': (-1, 'axisext: NULL table or result'),
 'axisext/no_values/f64': (-1, 'axisext: NULL table or result'),
 'axisext/empty_result/f64': (-1, 'axisext: NULL table or result'),
 'axisext/index_without_tables/f64': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/tables_without_index/f64': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/one_index_table/f64': (-1, 'axisext: the index tables and d_index are given together or not at all'),
 'axisext/other_columns/f64': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'axisext/op_and_no_table/f64': (-1, 'axisext: op -1 is neither 0 (max) nor 1 (min)'),
 'axisext/no_table_and_other_columns/f64': (-1, 'axisext: NULL table or result'),
 'axisext/index_without_tables_and_workspace_short/f64': (-1,
                                                          'axisext: the index tables and d_index are given together or not '
                                                          'at all'),
 'axisext/other_columns_and_workspace_short/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'argext/op/f64': (-1, 'argext: op 2 is neither 0 (max) nor 1 (min)'),
 'argext/no_value/f64': (-1, 'bad argext argument'),
 'argext/no_row_table/f64': (-1, 'NULL original or offset table'),
 'argext/no_col_table/f64': (-1, 'NULL original or offset table'),
 'argext/no_col_perm/f64': (-1, 'NULL original or offset table'),
 'argext/other_columns/f64': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'argext/op_and_bond_exceeds/f64': (-1, 'argext: op 7 is neither 0 (max) nor 1 (min)'),
 'argext/no_table_and_other_columns/f64': (-1, 'NULL original or offset table'),
 'argext/other_columns_and_workspace_short/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'labelstat/no_result/f64': (-1, 'bad labelstat argument'),
 'labelstat/no_labels_at_all/f64': (-1, 'label statistics take 1 to 4096 labels, got 0'),
 'labelstat/too_many_labels/f64': (-1, 'label statistics take 1 to 4096 labels, got 4097'),
 'labelstat/label_width/f64': (-1, 'labels are uint8, int16 or int32 (1, 2 or 4 bytes), got 3 bytes'),
 'labelstat/too_many_labels_and_label_width/f64': (-1, 'label statistics take 1 to 4096 labels, got 4097'),
 'labelstat/label_width_and_bond_exceeds/f64': (-1, 'labels are uint8, int16 or int32 (1, 2 or 4 bytes), got 0 bytes'),
 'labelstat/no_label_volume/f64': (-1, 'NULL original or offset table'),
 'labelstat/no_col_perm/f64': (-1, 'NULL original or offset table'),
 'labelstat/other_columns/f64': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'labelstat/no_table_and_other_columns/f64': (-1, 'NULL original or offset table'),
 'labelstat/room_for_the_chain_not_the_table/f64': (-4, 'labelstat workspace too small: 435712 < 436224'),
 'labelstat/other_columns_and_no_room_for_the_table/f64': (-1, 'offset tables are for 65 columns, the last product has 64'),
 'labelstat/workspace_short_and_other_columns/f64': (-4, 'valstat workspace too small: 435711 < 435712')}
SIZES = {'L1': (35584, 84736, 107776, '9a8aba3065151f64', '35398ed30e90fa61', 36096, 101632, 108288, '544ff19030c90a67',
        '50cd7686096cbf5c'),
 'L2_maxbond': (65792, 114944, 137984, 'a179925bb5b85c90', '89afb1077a413b2a', 92416, 157952, 164608, '54876c6d1f44fd06',
                '3507f8f54e7ae212'),
 'L2_no_tail': (362496, 411648, 434688, '5575fa02e451781c', '93f9bb1d17a85086', 624640, 690176, 696832, 'cb7a6f4a50c0c357',
                'e61eafe88af78b7f'),
 'L3_no_tail': (1263616, 1312768, 1335808, 'ed6167d07b3f3ee8', '8036d1b46bcd85bf', 2246656, 2312192, 2318848,
                '0e791668494c50ac', '17298ea533c848bf'),
 'L3_tail_all': (39936, 89088, 112128, '992199d66676b1bb', 'e408519a923ec437', 44032, 109568, 116224, '9463f9731b571140',
                 'ed07ccc6c91c416f'),
 'L3_tail_last': (237824, 286976, 310016, 'f278b90c2b4ef69a', 'f08c615efaf0560a', 407808, 473344, 480000,
                  '2722415ea1ae6282', 'c490642fe640b6b8'),
 'L4_large': (132914688, 132963840, 132986880, '43ded77df130ba4f', 'a8d74c7a016cb435', 264737792, 264803328, 264809984,
              '208971f3ef348fe7', '3a56b5e2b7c29f89'),
 'L4_no_tail': (935936, 985088, 1008128, 'dfa4ae31095399cc', '390cb907ddd6fe40', 1722368, 1787904, 1794560,
                '5509015b15682a89', 'd67de1d66f2a18ce'),
 'L4_tail_4096': (692224, 741376, 764416, 'a89c274789fe169d', 'c4f0a3d8cb1d1ba3', 1218560, 1284096, 1290752,
                  '8cfc59d6ebc810b7', '54e0181964f46ae7'),
 'L4_tail_last': (246272, 295424, 318464, '57c8978c61bf816e', 'ec3f74d3011c17f4', 435712, 501248, 507904,
                  'd8e8e218ce254b66', 'dc82e4bddb0eefc2'),
 'L5_mid_tail_129': (5496832, 5545984, 5569024, 'c7dd2f545d1a724d', '31e70633a3bd746a', 9918464, 9984000, 9990656,
                     'cf2ad32053daf27f', '58e697db2aa04332'),
 'L5_mid_tail_65': (1197568, 1246720, 1269760, 'b76f2d28de2b4f4c', 'b97c28843fc1ba92', 2137088, 2202624, 2209280,
                    '439074447b153336', '6babbd4a753ed774'),
 'L5_nonmonotone': (1660928, 1710080, 1733120, 'a4967ef2f21e30e5', 'e770410d4b6f5bab', 2964480, 3030016, 3036672,
                    'd9e7d66532bd5da4', '093d092cdb2f76c6'),
 'L5_primes_maxbond': (59136, 108288, 131328, 'fab84a516101e232', '3da5fb2d1a7726f8', 78592, 144128, 150784,
                       '7453bdbcdaeecd3c', '3df5cf86995ef739'),
 'L5_ragged': (128256, 177408, 200448, '86c5df7700b045d3', 'ef412094e54d194d', 203008, 268544, 275200, '0b920bb2436e7e05',
               '7167795b44834249'),
 'L5_tail_last': (1111552, 1160704, 1183744, '87abafec239ed896', '52cac4da636a9216', 2158080, 2223616, 2230272,
                  '14a8cbf37db7735f', '0689ad66dc039f45'),
 'L5_unit_dims': (38656, 87808, 110848, '0b7e7607c51b8207', '2a1b86213ca6889f', 41728, 107264, 113920, '0bb59223d95b8805',
                  'bb38d2422d3ba7c7'),
 'L6_bonds_one': (69888, 119040, 142080, '423bd5bca15c5df5', 'aaed56d898d3c271', 98048, 163584, 170240, 'a39fafb1b84aa85c',
                  'c60fde25d26739f9'),
 'L6_tail_all': (139008, 188160, 211200, '95ae321af37eecf1', '341652781e56aeea', 222464, 288000, 294656, 'cd18128acf1f6a49',
                 '44a8a51ff5b422f5'),
 'L6_tail_last': (1320448, 1369600, 1392640, 'ebe96cb64b3d7140', 'e00b637a9752a76c', 2532352, 2597888, 2604544,
                  'c08c8894a2b4ca37', '55f6b8d2b27f1034'),
 'L7_tail_all': (42496, 91648, 114688, '11057a2b632468a8', 'fd11178c570724be', 48640, 114176, 120832, '9fac600bdb804886',
                 '0f36bc470c241940'),
 'L7_tail_last': (1343488, 1392640, 1415680, '4c01f09908f51681', '1bf7eddd611f04fb', 2596352, 2661888, 2668544,
                  'd3ab15339a3aae4c', 'cd0dfb8dc5d939ee'),
 'int_8x7': (755712, 804864, 827904, 'efb2839eeb679d5a', 'a6e54c750b7fba90', 1345536, 1411072, 1417728, '9374cb1221e31eba',
             'c110bd49414c35e5'),
 'int_no_tail': (854016, 903168, 926208, 'd8cfc43e3138e0a4', '7cbccc42e2f2c2c2', 1640448, 1705984, 1712640,
                 '0711cd2c15be1826', '780ef010505d03f2'),
 'int_tail_all': (45568, 94720, 117760, '55b334ce007e82bf', 'cb5ff1c92b262fb9', 54272, 119808, 126464, 'b31ebc44f2a89546',
                  'c7d679ccc33b598f'),
 'int_tail_last': (64000, 113152, 136192, '66f12de5e673570e', '4142794505b0c8e3', 90112, 155648, 162304, 'b9ed69653f11dc27',
                   'e9ff9b826f315bfd'),
 'int_wide': (150528, 199680, 222720, '86168390fce3aa67', 'd99c7935b7f18bf3', 243200, 308736, 315392, '4df8252cc6af0cb0',
              'abeb4b40ea93bd39')}


def test_every_refusal_is_pinned(lib):
    got = refusals(lib)
    assert sorted(got) == sorted(REFUSED)
    for name, answer in got.items():
        assert answer[0] < 0, f"{name} was not refused"
        assert answer == REFUSED[name], (name, answer, REFUSED[name])


def test_sizes_and_plans_are_pinned(lib):
    got = sizes(lib)
    assert sorted(got) == sorted(SIZES)
    for name, answer in got.items():
        assert answer == SIZES[name], (name, answer, SIZES[name])


# ------------------------------------------------------------------------------------------------ the cases
def test_the_cases_are_what_the_bars_assume():
    assert "L4_large" not in dict(vc.REAL_CASES) and len(vc.REAL_CASES) == len(cc.CHAINS) - 1 + len(cc.GRADED)
    assert set(vc.INT_CHAINS) == set(cc.INTEGER_CHAINS) | {"int_8x7"}
    for name, (dims, bonds) in vc.ALL_CHAINS.items():
        if name != "L4_large":
            assert int(np.prod(dims, dtype=np.int64)) <= 2 ** 21 + 2 ** 18, name
    for name, (dims, bonds) in vc.INT_CHAINS.items():
        assert int(np.prod(bonds, dtype=np.int64)) < 2 ** 24, name
    # a chain whose decode permutation is not the identity exists among the integer and among the real cases
    assert not vc.case("int_wide", "integer", "f32").identity
    assert not vc.case("L5_ragged", "uniform", "f32").identity


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, family, storage):
    c = vc.case(name, family, storage)
    edges = c.edges64()
    # the condition: few voxels sit within their bound of an edge, so the sandwich is tight almost everywhere
    share = vc.near_edge_fraction(c.ref, c.bound, edges)
    print(f"[valstat] {name}/{family}/{storage}: {edges.size - 1} bins, {share:.2e} of the voxels within their bound of an edge")
    assert edges.size - 1 in (64, 32, 16, 8, 4)
    assert share <= 0.01
    # the reference passes its own bar
    counts, out = vc.ref_histogram(c.ref, edges)
    vc.sandwich_moments(vc.ref_moments(c.ref), c.ref, c.bound)
    vc.sandwich_histogram(counts, out, c.ref, c.bound, edges)
    y = c.original()
    vc.sandwich_error(vc.ref_error(c.ref, y), c.ref, c.bound, y)
    # the faults
    m, n = vc.last_product_shape(c.dims)
    some = vc.fault_tile_left_out(c)
    with pytest.raises(AssertionError):
        vc.sandwich_moments(vc.ref_moments(some), c.ref, c.bound)
    with pytest.raises(AssertionError):
        vc.sandwich_histogram(*vc.values_histogram(some, edges), c.ref, c.bound, edges)
    padded = vc.fault_padding_counted(c)
    assert (padded is None) == (m % vc.TILE == 0 and n % vc.TILE == 0)
    if padded is not None:
        with pytest.raises(AssertionError):
            vc.sandwich_moments(vc.ref_moments(padded), c.ref, c.bound)
        with pytest.raises(AssertionError):
            vc.sandwich_histogram(*vc.values_histogram(padded, edges), c.ref, c.bound, edges)
    with pytest.raises(AssertionError):
        vc.sandwich_histogram(*vc.fault_bins_shifted(c.ref, edges), c.ref, c.bound, edges)
    if not c.identity:
        with pytest.raises(AssertionError):
            vc.sandwich_error(vc.fault_site_order_original(c, y), c.ref, c.bound, y)


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_exact_bar_on_the_reference_and_on_modelled_faults(name, storage):
    c = vc.case(name, "integer", storage)
    assert np.array_equal(c.ref, np.round(c.ref)) and np.abs(c.ref).max() < 2 ** 24
    vc.exact_moments(vc.ref_moments(c.ref), c.ref)
    y = c.original()
    assert y[0] != c.ref[0] and y[-1] != c.ref[-1]
    vc.exact_error(vc.ref_error(c.ref, y), c.ref, y)
    if not c.identity:
        with pytest.raises(AssertionError):
            vc.exact_error(vc.fault_site_order_original(c, y), c.ref, y)
    some, padded = vc.fault_tile_left_out(c), vc.fault_padding_counted(c)
    with pytest.raises(AssertionError):
        vc.exact_moments(vc.ref_moments(some), c.ref)
    if padded is not None:
        with pytest.raises(AssertionError):
            vc.exact_moments(vc.ref_moments(padded), c.ref)
    sets = vc.integer_edge_sets(c.ref, vc.NP_TYPE[storage])
    assert sets["bins_4096"].size == 4097 and sets["one_bin"].size == 2
    assert float(sets["last_edge_is_max"][-1]) == c.ref.max()
    for label, edges in sets.items():
        assert np.all(np.diff(edges.astype(np.float64)) >= 0), label
        vc.exact_histogram(*vc.ref_histogram(c.ref, edges), c.ref, edges)
        with pytest.raises(AssertionError):
            vc.exact_histogram(*vc.values_histogram(some, edges), c.ref, edges)
        if padded is not None:
            with pytest.raises(AssertionError):
                vc.exact_histogram(*vc.values_histogram(padded, edges), c.ref, edges)
        with pytest.raises(AssertionError):
            vc.exact_histogram(*vc.fault_bins_shifted(c.ref, edges), c.ref, edges)
    # the open last bin can occur where a voxel equals the last edge
    for label in ("last_edge_is_max", "one_bin"):
        opened = vc.fault_last_bin_open(c.ref, sets[label])
        assert opened is not None, label
        with pytest.raises(AssertionError):
            vc.exact_histogram(*opened, c.ref, sets[label])
    below, above, _ = vc.ref_histogram(c.ref, sets["range_excludes"])[1]
    assert below > 0 and above > 0, "the excluding range excludes nothing"
    # NaN planted in a core entry: counted apart, in no bin
    _, ref_nan = vc.with_nan(c)
    k = int(np.isnan(ref_nan).sum())
    assert 0 < k < c.n
    edges = sets["half_integers"]
    vc.exact_histogram(*vc.ref_histogram(ref_nan, edges), ref_nan, edges)
    with pytest.raises(AssertionError):
        vc.exact_histogram(*vc.fault_nan_in_a_bin(ref_nan, edges), ref_nan, edges)


def test_psnr_formula_at_its_edges():
    from imgcompressionmps_amd.core import valstat as vs

    assert vs.psnr_from(dict(mse=0.0, ref_max=3.0)) == np.inf
    assert vs.psnr_from(dict(mse=0.25, ref_max=0.0)) == -np.inf  # numpy's 10 * log10(0 / mse)
    assert vs.psnr_from(dict(mse=0.25, ref_max=-2.0)) == 10 * np.log10(16.0)

