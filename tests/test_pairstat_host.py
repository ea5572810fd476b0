"""Statistics of two chains from the cores, on the host (no GPU).

* chain_pair_plan (csrc/pairstat_plan.h) through ndmps_pairstat_plan_query / _workspace_bytes against a Python
  restatement of the layout, on every pair of tests/pairstat_cases.py.
* what is refused before any launch: more than 16384 cells, an axis above 1024 bins, and the chain checks of the
  single-chain entries on either chain, with pointers that are never dereferenced.  The C entries take ONE dims array,
  and chain_plan splits by the dims alone, so two last products that differ in rows or columns cannot be handed to
  them; that refusal is made where two chains meet, in core/pairstat.py, and tested there.
* pinned answers: code and whole message of every such refusal, and the workspace and plan of every pair, as literals.
* mutual information from planted count tables.
* the preconditions of the NDMPS methods, on objects built without a device.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pairstat_cases as pc
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import pairstat as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = {"f32": 0, "f64": 2}
SLOTS = ("m", "n", "k_a", "k_b", "bytes_a", "bytes_b", "off_b", "off_partials", "off_result", "off_counts", "off_edges_a",
         "off_edges_b", "pair_bytes", "bytes")
ALL_PAIRS = dict(pc.REAL_PAIRS, **pc.INT_PAIRS)
r256 = lambda x: -(-x // 256) * 256  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _plan(lib, dims, bonds_a, bonds_b, elem, bins_a=0, bins_b=0):
    out = (C.c_int64 * len(SLOTS))()
    rc = lib.ndmps_pairstat_plan_query(ELEMS[elem], len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a),
                                       _lib.i64_array(bonds_b), bins_a, bins_b, out)
    assert rc == _lib.OK, lib.ndmps_last_error()
    return dict(zip(SLOTS, out))


@pytest.mark.parametrize("bins", [(0, 0), (1, 1), (64, 64), (1, 1024), (1024, 16), (128, 128)])
@pytest.mark.parametrize("elem", sorted(ELEMS))
@pytest.mark.parametrize("name", sorted(ALL_PAIRS))
def test_plan_is_two_stats_plans_and_the_pair_scratch(lib, name, elem, bins):
    dims, bonds_a = pc.CHAINS[name]
    bonds_b = ALL_PAIRS[name]
    L, d = len(dims), _lib.i64_array(dims)
    eb = 8 if elem == "f64" else 4
    p = _plan(lib, dims, bonds_a, bonds_b, elem, *bins)
    assert (p["m"], p["n"]) == vc.last_product_shape(dims)
    assert (p["k_a"], p["k_b"]) == (pc.last_k(dims, bonds_a), pc.last_k(dims, bonds_b))
    # the two single-chain workspaces (no bins of their own), back to back
    assert p["bytes_a"] == lib.ndmps_valstat_workspace_bytes(L, d, _lib.i64_array(bonds_a), eb, 0)
    assert p["bytes_b"] == lib.ndmps_valstat_workspace_bytes(L, d, _lib.i64_array(bonds_b), eb, 0)
    assert p["off_b"] == r256(p["bytes_a"]) and p["off_partials"] == r256(p["off_b"] + p["bytes_b"])
    # 512 partial records of 128 bytes, the result, then for a histogram the counters and the two edge tables
    assert p["off_result"] == p["off_partials"] + 512 * 128
    assert p["off_counts"] == p["off_result"] + 256
    cells = bins[0] * bins[1]
    hist = cells > 0
    assert p["off_edges_a"] == p["off_counts"] + (r256((cells + 2) * 8) if hist else 0)
    assert p["off_edges_b"] == p["off_edges_a"] + (r256((bins[0] + 1) * eb) if hist else 0)
    assert p["bytes"] == p["off_edges_b"] + (r256((bins[1] + 1) * eb) if hist else 0)
    assert p["pair_bytes"] == p["bytes"] - p["off_partials"]
    assert all(p[k] % 256 == 0 for k in SLOTS if k.startswith("off_"))
    assert lib.ndmps_pairstat_workspace_bytes(L, d, _lib.i64_array(bonds_a), _lib.i64_array(bonds_b), eb, *bins) == p["bytes"]


def test_workspace_of_the_two_million_voxel_pair_is_a_fraction_of_one_volume(lib):
    dims, bonds_a = vc.INT_EXTRA["int_8x7"]
    got = lib.ndmps_pairstat_workspace_bytes(len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a),
                                             _lib.i64_array(pc.INT_PAIRS["int_8x7"]), 4, 128, 128)
    assert 0 < got < int(np.prod(dims)) * 4 // 4


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("ndmps_pairstat_"))
    assert len(names) == 6
    for name in names:
        decl = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, f"{name} is not declared in include/ndmps_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert f"#define NDMPS_PAIRSTAT_PLAN_SLOTS {len(SLOTS)}" in header


def test_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    dims, bonds_a = vc.ALL_CHAINS["L4_tail_last"]
    bonds_b = pc.REAL_PAIRS["L4_tail_last"]
    L, d, ba, bb = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a), _lib.i64_array(bonds_b)
    fake = (C.c_void_p * L)(*[256] * L)
    p = C.c_void_p(256)
    stats, counts = (C.c_double * 11)(), (C.c_int64 * 16386)()
    out = (C.c_int64 * len(SLOTS))()
    big = 1 << 40
    for suffix, eb, arr in (("f32", 4, C.c_float), ("f64", 8, C.c_double)):
        need = lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 0, 0)
        need_h = lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 4, 2)
        assert need_h > need > 0
        mom = getattr(lib, f"ndmps_pairstat_moments_{suffix}")
        hist = getattr(lib, f"ndmps_pairstat_histogram_{suffix}")
        e4, e2 = (arr * 5)(0, 1, 2, 3, 4), (arr * 3)(0, 1, 2)
        calls = {
            "moments": lambda a_, b_, ws, nbytes: mom(L, d, a_, b_, fake, fake, stats, counts, ws, nbytes, None),
            "histogram": lambda a_, b_, ws, nbytes: hist(L, d, a_, b_, fake, fake, e4, 4, e2, 2, counts, ws, nbytes, None),
        }
        for what, call in calls.items():
            assert call(ba, bb, p, (need_h if what == "histogram" else need) - 1) == _lib.EWORKSPACE, what
            assert call(ba, bb, None, big) == _lib.EWORKSPACE, what
            assert call(ba, bb, C.c_void_p(264), big) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error(), what
            for bad in ([1, 4, 13, 13, 1], [1, 3, 13, 65, 1], [1, 3, 0, 13, 1]):  # either chain
                assert call(_lib.i64_array(bad), bb, p, big) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error(), (what, bad)
                assert call(ba, _lib.i64_array(bad), p, big) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error(), (what, bad)
            for bad in ([2, 3, 13, 13, 1], [1, 3, 13, 13, 2]):
                assert call(ba, _lib.i64_array(bad), p, big) == _lib.EINVAL and b"boundary" in lib.ndmps_last_error(), (what, bad)
            assert call(None, bb, p, big) == _lib.EINVAL and call(ba, None, p, big) == _lib.EINVAL, what
        assert mom(L, d, ba, bb, None, fake, stats, counts, p, big, None) == _lib.EINVAL
        assert mom(L, d, ba, bb, fake, None, stats, counts, p, big, None) == _lib.EINVAL
        assert mom(0, d, ba, bb, fake, fake, stats, counts, p, big, None) == _lib.EINVAL
        # the histogram's limits: an axis above 1024, more than 16384 cells, no bins; then its edges
        wide = (arr * 1026)(*range(1026))
        assert hist(L, d, ba, bb, fake, fake, wide, 1025, e2, 1, counts, p, big, None) == _lib.EINVAL
        assert b"an axis takes 1 to 1024" in lib.ndmps_last_error()
        assert hist(L, d, ba, bb, fake, fake, e2, 1, wide, 1025, counts, p, big, None) == _lib.EINVAL
        assert hist(L, d, ba, bb, fake, fake, wide, 1024, wide, 17, counts, p, big, None) == _lib.EINVAL
        assert b"more than 16384 cells" in lib.ndmps_last_error()
        assert hist(L, d, ba, bb, fake, fake, wide, 1024, wide, 16, counts, p, 1, None) == _lib.EWORKSPACE  # the limit itself passes
        assert hist(L, d, ba, bb, fake, fake, e4, 0, e2, 2, counts, p, big, None) == _lib.EINVAL
        assert hist(L, d, ba, bb, fake, fake, (arr * 5)(0, 1, 3, 2, 4), 4, e2, 2, counts, p, big, None) == _lib.EINVAL
        assert b"ascending" in lib.ndmps_last_error() and b"of a" in lib.ndmps_last_error()
        assert hist(L, d, ba, bb, fake, fake, e4, 4, (arr * 3)(0, float("nan"), 2), 2, counts, p, big, None) == _lib.EINVAL
        assert b"of b" in lib.ndmps_last_error()
        assert hist(L, d, ba, bb, fake, fake, None, 4, e2, 2, counts, p, big, None) == _lib.EINVAL
        assert lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 1025, 1) == 0
        assert lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 1024, 17) == 0
        assert lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 4, 0) == 0
    assert lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, 2, 0, 0) == 0
    assert lib.ndmps_pairstat_plan_query(0, L, d, ba, bb, 1025, 1, out) == _lib.EINVAL and b"1024" in lib.ndmps_last_error()
    assert lib.ndmps_pairstat_plan_query(0, L, d, ba, bb, 1024, 17, out) == _lib.EINVAL and b"16384" in lib.ndmps_last_error()
    assert lib.ndmps_pairstat_plan_query(1, L, d, ba, bb, 0, 0, out) == _lib.EINVAL  # bf16 has no statistics entry
    assert lib.ndmps_pairstat_plan_query(0, L, d, ba, bb, 0, 0, None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ pinned answers
# What the two pair entries answer before their first HIP call, as literals (return code and the whole message, in the
# order the checks are made), and the workspace and the plan of every pair.  Taken from the build before the
# statistics family got its shared host prologue; a change of any of them is a change of behaviour.
def refusal_calls(lib, suffix):
    """name -> call, each refused before the first HIP call (the pointers are fakes)."""
    dims, bonds_a = vc.ALL_CHAINS["L4_tail_last"]
    L, d, ba, bb = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a), _lib.i64_array(pc.REAL_PAIRS["L4_tail_last"])
    eb, arr = (4, C.c_float) if suffix == "f32" else (8, C.c_double)
    fake = (C.c_void_p * L)(*[256] * L)
    hole = (C.c_void_p * L)(256, None, 256, 256)
    p, big = 256, 1 << 40
    stats, counts = (C.c_double * 11)(), (C.c_int64 * 16386)()
    need = lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 0, 0)
    need_a = lib.ndmps_valstat_workspace_bytes(L, d, ba, eb, 0)
    up = _lib.i64_array([1, 4, 13, 13, 1])
    e4, e2, wide = (arr * 5)(0, 1, 2, 3, 4), (arr * 3)(0, 1, 2), (arr * 1026)(*range(1026))
    down, hurt = (arr * 5)(0, 1, 3, 2, 4), (arr * 3)(0, float("nan"), 2)

    def mom(L=L, d=d, a=ba, b=bb, cores_a=fake, cores_b=fake, stats=stats, ws=p, nbytes=big):
        return getattr(lib, f"ndmps_pairstat_moments_{suffix}")(L, d, a, b, cores_a, cores_b, stats, counts, ws, nbytes, None)

    def hist(L=L, d=d, a=ba, b=bb, cores_a=fake, cores_b=fake, ea=e4, na=4, eb_=e2, nb=2, ws=p, nbytes=big):
        return getattr(lib, f"ndmps_pairstat_histogram_{suffix}")(L, d, a, b, cores_a, cores_b, ea, na, eb_, nb, counts, ws,
                                                                 nbytes, None)

    calls = {}
    for name, f in (("moments", mom), ("histogram", hist)):
        calls.update({
            f"{name}/no_sites": lambda f=f: f(L=0),
            f"{name}/no_dims": lambda f=f: f(d=None),
            f"{name}/no_bonds_of_b": lambda f=f: f(b=None),
            f"{name}/no_cores_of_a": lambda f=f: f(cores_a=None),
            f"{name}/no_cores_of_b": lambda f=f: f(cores_b=None),
            f"{name}/core_1_of_b_null": lambda f=f: f(cores_b=hole),
            f"{name}/boundary_of_b": lambda f=f: f(b=_lib.i64_array([2, 3, 13, 13, 1])),
            f"{name}/bond_of_a_exceeds": lambda f=f: f(a=up),
            f"{name}/bond_of_b_exceeds": lambda f=f: f(b=up),
            f"{name}/both_bonds_exceed": lambda f=f: f(a=up, b=_lib.i64_array([1, 3, 28, 13, 1])),
            f"{name}/workspace_null": lambda f=f: f(ws=None),
            f"{name}/workspace_short_for_a": lambda f=f: f(nbytes=need_a - 1),
            f"{name}/workspace_short_for_b": lambda f=f: f(nbytes=need_a + 256),
            f"{name}/workspace_short_for_the_pair": lambda f=f: f(nbytes=need - 1),
            f"{name}/workspace_misaligned": lambda f=f: f(ws=264),
            f"{name}/bond_of_b_exceeds_and_workspace_short_for_a": lambda f=f: f(b=up, nbytes=1),
        })
    calls.update({
        "moments/no_result": lambda: mom(stats=None),
        "histogram/no_edges_of_b": lambda: hist(eb_=None),
        "histogram/axis_a_too_wide": lambda: hist(ea=wide, na=1025, nb=1),
        "histogram/axis_b_too_wide": lambda: hist(na=1, eb_=wide, nb=1025),
        "histogram/no_bins_on_a": lambda: hist(na=0),
        "histogram/too_many_cells": lambda: hist(ea=wide, na=1024, eb_=wide, nb=17),
        "histogram/edges_of_a_descend": lambda: hist(ea=down),
        "histogram/edge_of_b_nan": lambda: hist(eb_=hurt),
        "histogram/both_edge_tables_bad": lambda: hist(ea=down, eb_=hurt),
        "histogram/too_many_cells_and_edges_descend": lambda: hist(ea=down, na=1024, eb_=wide, nb=17),
        "histogram/edges_descend_and_bond_exceeds": lambda: hist(ea=down, a=up),
        "histogram/edge_nan_and_workspace_short": lambda: hist(eb_=hurt, nbytes=1),
        "histogram/workspace_short_for_the_cells": lambda: hist(nbytes=need),
        "histogram/the_limit_itself_with_no_room": lambda: hist(ea=wide, na=1024, eb_=wide, nb=16, nbytes=1),
    })
    return calls


def refusals(lib):
    out = {}
    for suffix in ("f32", "f64"):
        for name, call in refusal_calls(lib, suffix).items():
            rc = call()
            out[f"{name}/{suffix}"] = (rc, lib.ndmps_last_error().decode() if rc != _lib.OK else "")
    out["query/axis"] = (lib.ndmps_pairstat_plan_query(0, 2, _lib.i64_array([4, 4]), _lib.i64_array([1, 2, 1]),
                                                       _lib.i64_array([1, 3, 1]), 1025, 1, (C.c_int64 * len(SLOTS))()),
                         lib.ndmps_last_error().decode())
    out["query/cells"] = (lib.ndmps_pairstat_plan_query(2, 2, _lib.i64_array([4, 4]), _lib.i64_array([1, 2, 1]),
                                                        _lib.i64_array([1, 3, 1]), 1024, 17, (C.c_int64 * len(SLOTS))()),
                          lib.ndmps_last_error().decode())
    out["query/one_axis_without_bins"] = (lib.ndmps_pairstat_plan_query(0, 2, _lib.i64_array([4, 4]), _lib.i64_array([1, 2, 1]),
                                                                        _lib.i64_array([1, 3, 1]), 4, 0, (C.c_int64 * len(SLOTS))()),
                                          lib.ndmps_last_error().decode())
    out["query/element"] = (lib.ndmps_pairstat_plan_query(1, 2, _lib.i64_array([4, 4]), _lib.i64_array([1, 2, 1]),
                                                          _lib.i64_array([1, 3, 1]), 0, 0, (C.c_int64 * len(SLOTS))()),
                            lib.ndmps_last_error().decode())
    return out


def sizes(lib):
    """name -> per element type: the workspace of the moments and of 128 x 128 cells, then the plan query's fourteen
    slots at 64 x 16 bins."""
    out = {}
    for name in sorted(ALL_PAIRS):
        dims, bonds_a = pc.CHAINS[name]
        L, d, ba, bb = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds_a), _lib.i64_array(ALL_PAIRS[name])
        row = []
        for elem, eb in (("f32", 4), ("f64", 8)):
            row += [lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 0, 0),
                    lib.ndmps_pairstat_workspace_bytes(L, d, ba, bb, eb, 128, 128)]
            row.append(tuple(_plan(lib, dims, bonds_a, ALL_PAIRS[name], elem, 64, 16)[k] for k in SLOTS))
        out[name] = tuple(row)
    return out


REFUSED = {'moments/no_sites/f32': (-1, 'bad pairstat argument'),
 'moments/no_dims/f32': (-1, 'bad pairstat argument'),
 'moments/no_bonds_of_b/f32': (-1, 'bad pairstat argument'),
 'moments/no_cores_of_a/f32': (-1, 'bad valstat argument'),
 'moments/no_cores_of_b/f32': (-1, 'bad valstat argument'),
 'moments/core_1_of_b_null/f32': (-1, 'dims[1] must be positive and core 1 non-NULL'),
 'moments/boundary_of_b/f32': (-1, 'open boundary bonds must be 1'),
 'moments/bond_of_a_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/bond_of_b_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/both_bonds_exceed/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/workspace_null/f32': (-4, 'valstat workspace too small: 1099511627776 < 246272'),
 'moments/workspace_short_for_a/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'moments/workspace_short_for_b/f32': (-4, 'valstat workspace too small: 256 < 684800'),
 'moments/workspace_short_for_the_pair/f32': (-4, 'pairstat workspace too small: 996863 < 996864'),
 'moments/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'moments/bond_of_b_exceeds_and_workspace_short_for_a/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'histogram/no_sites/f32': (-1, 'bad pairstat argument'),
 'histogram/no_dims/f32': (-1, 'bad pairstat argument'),
 'histogram/no_bonds_of_b/f32': (-1, 'bad pairstat argument'),
 'histogram/no_cores_of_a/f32': (-1, 'bad valstat argument'),
 'histogram/no_cores_of_b/f32': (-1, 'bad valstat argument'),
 'histogram/core_1_of_b_null/f32': (-1, 'dims[1] must be positive and core 1 non-NULL'),
 'histogram/boundary_of_b/f32': (-1, 'open boundary bonds must be 1'),
 'histogram/bond_of_a_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/bond_of_b_exceeds/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/both_bonds_exceed/f32': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/workspace_null/f32': (-4, 'valstat workspace too small: 1099511627776 < 246272'),
 'histogram/workspace_short_for_a/f32': (-4, 'valstat workspace too small: 246271 < 246272'),
 'histogram/workspace_short_for_b/f32': (-4, 'valstat workspace too small: 256 < 684800'),
 'histogram/workspace_short_for_the_pair/f32': (-4, 'pairstat workspace too small: 996863 < 997632'),
 'histogram/workspace_misaligned/f32': (-1, 'valstat workspace must be 256-byte aligned'),
 'histogram/bond_of_b_exceeds_and_workspace_short_for_a/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'moments/no_result/f32': (-1, 'bad pairstat argument'),
 'histogram/no_edges_of_b/f32': (-1, 'bad pairstat argument'),
 'histogram/axis_a_too_wide/f32': (-1, 'joint histogram: 1025 x 1 bins, an axis takes 1 to 1024'),
 'histogram/axis_b_too_wide/f32': (-1, 'joint histogram: 1 x 1025 bins, an axis takes 1 to 1024'),
 'histogram/no_bins_on_a/f32': (-1, 'joint histogram: 0 x 2 bins, an axis takes 1 to 1024'),
 'histogram/too_many_cells/f32': (-1, 'joint histogram: 1024 x 17 bins are more than 16384 cells'),
 'histogram/edges_of_a_descend/f32': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/edge_of_b_nan/f32': (-1, 'joint histogram: edges of b must be ascending and not NaN (edge 1)'),
 'histogram/both_edge_tables_bad/f32': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/too_many_cells_and_edges_descend/f32': (-1, 'joint histogram: 1024 x 17 bins are more than 16384 cells'),
 'histogram/edges_descend_and_bond_exceeds/f32': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/edge_nan_and_workspace_short/f32': (-1, 'joint histogram: edges of b must be ascending and not NaN (edge 1)'),
 'histogram/workspace_short_for_the_cells/f32': (-4, 'pairstat workspace too small: 996864 < 997632'),
 'histogram/the_limit_itself_with_no_room/f32': (-4, 'valstat workspace too small: 1 < 246272'),
 'moments/no_sites/f64': (-1, 'bad pairstat argument'),
 'moments/no_dims/f64': (-1, 'bad pairstat argument'),
 'moments/no_bonds_of_b/f64': (-1, 'bad pairstat argument'),
 'moments/no_cores_of_a/f64': (-1, 'bad valstat argument'),
 'moments/no_cores_of_b/f64': (-1, 'bad valstat argument'),
 'moments/core_1_of_b_null/f64': (-1, 'dims[1] must be positive and core 1 non-NULL'),
 'moments/boundary_of_b/f64': (-1, 'open boundary bonds must be 1'),
 'moments/bond_of_a_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/bond_of_b_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/both_bonds_exceed/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'moments/workspace_null/f64': (-4, 'valstat workspace too small: 1099511627776 < 435712'),
 'moments/workspace_short_for_a/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'moments/workspace_short_for_b/f64': (-4, 'valstat workspace too small: 256 < 1266944'),
 'moments/workspace_short_for_the_pair/f64': (-4, 'pairstat workspace too small: 1768447 < 1768448'),
 'moments/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'moments/bond_of_b_exceeds_and_workspace_short_for_a/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'histogram/no_sites/f64': (-1, 'bad pairstat argument'),
 'histogram/no_dims/f64': (-1, 'bad pairstat argument'),
 'histogram/no_bonds_of_b/f64': (-1, 'bad pairstat argument'),
 'histogram/no_cores_of_a/f64': (-1, 'bad valstat argument'),
 'histogram/no_cores_of_b/f64': (-1, 'bad valstat argument'),
 'histogram/core_1_of_b_null/f64': (-1, 'dims[1] must be positive and core 1 non-NULL'),
 'histogram/boundary_of_b/f64': (-1, 'open boundary bonds must be 1'),
 'histogram/bond_of_a_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/bond_of_b_exceeds/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/both_bonds_exceed/f64': (-1, 'bond 1 = 4 exceeds min(3, 37440), the rank any unfolding can have'),
 'histogram/workspace_null/f64': (-4, 'valstat workspace too small: 1099511627776 < 435712'),
 'histogram/workspace_short_for_a/f64': (-4, 'valstat workspace too small: 435711 < 435712'),
 'histogram/workspace_short_for_b/f64': (-4, 'valstat workspace too small: 256 < 1266944'),
 'histogram/workspace_short_for_the_pair/f64': (-4, 'pairstat workspace too small: 1768447 < 1769216'),
 'histogram/workspace_misaligned/f64': (-1, 'valstat workspace must be 256-byte aligned'),
 'histogram/bond_of_b_exceeds_and_workspace_short_for_a/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'moments/no_result/f64': (-1, 'bad pairstat argument'),
 'histogram/no_edges_of_b/f64': (-1, 'bad pairstat argument'),
 'histogram/axis_a_too_wide/f64': (-1, 'joint histogram: 1025 x 1 bins, an axis takes 1 to 1024'),
 'histogram/axis_b_too_wide/f64': (-1, 'joint histogram: 1 x 1025 bins, an axis takes 1 to 1024'),
 'histogram/no_bins_on_a/f64': (-1, 'joint histogram: 0 x 2 bins, an axis takes 1 to 1024'),
 'histogram/too_many_cells/f64': (-1, 'joint histogram: 1024 x 17 bins are more than 16384 cells'),
 'histogram/edges_of_a_descend/f64': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/edge_of_b_nan/f64': (-1, 'joint histogram: edges of b must be ascending and not NaN (edge 1)'),
 'histogram/both_edge_tables_bad/f64': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/too_many_cells_and_edges_descend/f64': (-1, 'joint histogram: 1024 x 17 bins are more than 16384 cells'),
 'histogram/edges_descend_and_bond_exceeds/f64': (-1, 'joint histogram: edges of a must be ascending and not NaN (edge 3)'),
 'histogram/edge_nan_and_workspace_short/f64': (-1, 'joint histogram: edges of b must be ascending and not NaN (edge 1)'),
 'histogram/workspace_short_for_the_cells/f64': (-4, 'pairstat workspace too small: 1768448 < 1769216'),
 'histogram/the_limit_itself_with_no_room/f64': (-4, 'valstat workspace too small: 1 < 435712'),
 'query/axis': (-1, 'joint histogram: 1025 x 1 bins, an axis takes 1 to 1024'),
 'query/cells': (-1, 'joint histogram: 1024 x 17 bins are more than 16384 cells'),
 'query/one_axis_without_bins': (-1, 'joint histogram: 4 x 0 bins: both at least 1, or both 0 for the moments'),
 'query/element': (-1, 'bad pairstat plan query (elem=1)')}
SIZES = {'L1': (136960, 269824, (1, 37, 1, 1, 35584, 35584, 35584, 71168, 136704, 136960, 145408, 145920, 75008, 146176), 137984,
        271872, (1, 37, 1, 1, 36096, 36096, 36096, 72192, 137728, 137984, 146432, 147200, 75264, 147456)),
 'L2_maxbond': (171776, 304640, (33, 65, 33, 5, 65792, 40192, 65792, 105984, 171520, 171776, 180224, 180736, 75008, 180992),
                203008, 336896,
                (33, 65, 33, 5, 92416, 44800, 92416, 137216, 202752, 203008, 211456, 212224, 75264, 212480)),
 'L4_no_tail': (2019584, 2152448,
                (12, 8192, 7, 12, 935936, 1017856, 935936, 1953792, 2019328, 2019584, 2028032, 2028544, 75008, 2028800),
                3592448, 3726336,
                (12, 8192, 7, 12, 1722368, 1804288, 1722368, 3526656, 3592192, 3592448, 3600896, 3601664, 75264, 3601920)),
 'L4_tail_4096': (1163008, 1295872,
                  (16, 4096, 16, 9, 692224, 404992, 692224, 1097216, 1162752, 1163008, 1171456, 1171968, 75008, 1172224),
                  1985792, 2119680,
                  (16, 4096, 16, 9, 1218560, 701440, 1218560, 1920000, 1985536, 1985792, 1994240, 1995008, 75264, 1995264)),
 'L4_tail_last': (996864, 1129728,
                  (1755, 64, 13, 40, 246272, 684800, 246272, 931072, 996608, 996864, 1005312, 1005824, 75008, 1006080),
                  1768448, 1902336,
                  (1755, 64, 13, 40, 435712, 1266944, 435712, 1702656, 1768192, 1768448, 1776896, 1777664, 75264, 1777920)),
 'L5_mid_tail_65': (2014208, 2147072,
                    (90, 1716, 65, 40, 1197568, 750848, 1197568, 1948416, 2013952, 2014208, 2022656, 2023168, 75008,
                     2023424),
                    3532288, 3666176,
                    (90, 1716, 65, 40, 2137088, 1329408, 2137088, 3466496, 3532032, 3532288, 3540736, 3541504, 75264,
                     3541760)),
 'L5_ragged': (295936, 428800,
               (7, 1320, 7, 5, 128256, 101888, 128256, 230144, 295680, 295936, 304384, 304896, 75008, 305152), 424448,
               558336, (7, 1320, 7, 5, 203008, 155648, 203008, 358656, 424192, 424448, 432896, 433664, 75264, 433920)),
 'L5_tail_last': (1734144, 1867008,
                  (3900, 64, 33, 16, 1111552, 556800, 1111552, 1668352, 1733888, 1734144, 1742592, 1743104, 75008, 1743360),
                  3288064, 3421952,
                  (3900, 64, 33, 16, 2158080, 1064192, 2158080, 3222272, 3287808, 3288064, 3296512, 3297280, 75264,
                   3297536)),
 'L6_tail_all': (274688, 407552,
                 (4, 3456, 3, 1, 139008, 69888, 139008, 208896, 274432, 274688, 283136, 283648, 75008, 283904), 386304,
                 520192, (4, 3456, 3, 1, 222464, 98048, 222464, 320512, 386048, 386304, 394752, 395520, 75264, 395776)),
 'int_8x7': (1216768, 1349632,
             (512, 4096, 16, 8, 755712, 395264, 755712, 1150976, 1216512, 1216768, 1225216, 1225728, 75008, 1225984),
             2101504, 2235392,
             (512, 4096, 16, 8, 1345536, 690176, 1345536, 2035712, 2101248, 2101504, 2109952, 2110720, 75264, 2110976)),
 'int_many_tiles': (1736960, 1869824,
                    (2, 40010, 2, 2, 835584, 835584, 835584, 1671168, 1736704, 1736960, 1745408, 1745920, 75008, 1746176),
                    3017984, 3151872,
                    (2, 40010, 2, 2, 1476096, 1476096, 1476096, 2952192, 3017728, 3017984, 3026432, 3027200, 75264,
                     3027456)),
 'int_no_tail': (1806592, 1939456,
                 (12, 8192, 2, 4, 854016, 886784, 854016, 1740800, 1806336, 1806592, 1815040, 1815552, 75008, 1815808),
                 3379456, 3513344,
                 (12, 8192, 2, 4, 1640448, 1673216, 1640448, 3313664, 3379200, 3379456, 3387904, 3388672, 75264, 3388928)),
 'int_tail_all': (162048, 294912, (5, 504, 2, 3, 45568, 50688, 45568, 96256, 161792, 162048, 170496, 171008, 75008, 171264),
                  183552, 317440,
                  (5, 504, 2, 3, 54272, 63488, 54272, 117760, 183296, 183552, 192000, 192768, 75264, 193024)),
 'int_tail_last': (177408, 310272,
                   (600, 41, 5, 2, 64000, 47616, 64000, 111616, 177152, 177408, 185856, 186368, 75008, 186624), 214272,
                   348160, (600, 41, 5, 2, 90112, 58368, 90112, 148480, 214016, 214272, 222720, 223488, 75264, 223744)),
 'int_wide': (309248, 442112, (8, 1440, 8, 4, 150528, 92928, 150528, 243456, 308992, 309248, 317696, 318208, 75008, 318464),
              448512, 582400,
              (8, 1440, 8, 4, 243200, 139520, 243200, 382720, 448256, 448512, 456960, 457728, 75264, 457984))}


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


# ------------------------------------------------------------------------------------------------ mutual information
def test_mutual_information_of_planted_tables():
    mi = ps.mutual_information_from_counts
    rows, cols = np.array([3, 5, 2, 7]), np.array([4, 1, 6])
    independent = np.outer(rows, cols)  # n_ij N = r_i c_j in integers: every logarithm is ln 1
    assert mi(independent) == 0.0
    h = lambda c: float(-(c / c.sum() * np.log(c / c.sum())).sum())  # noqa: E731
    # normalized: (H(a) + H(b)) / H(a, b) with H(a, b) = H(a) + H(b) for independent marginals; a few roundings
    assert abs(mi(independent, normalized=True) - 1.0) <= 8 * np.finfo(np.float64).eps
    diagonal = np.diag(rows)
    assert abs(mi(diagonal) - h(rows)) <= 8 * np.finfo(np.float64).eps * h(rows)
    assert abs(mi(diagonal, normalized=True) - 2.0) <= 8 * np.finfo(np.float64).eps
    assert mi(np.zeros((4, 3), dtype=np.int64)) == 0.0 and mi(np.zeros((4, 3), dtype=np.int64), normalized=True) == 1.0
    one_cell = np.zeros((4, 3), dtype=np.int64)
    one_cell[2, 1] = 9
    assert mi(one_cell) == 0.0 and mi(one_cell, normalized=True) == 1.0  # H(a, b) == 0
    # a permutation table is as informative as the diagonal; empty rows and columns change nothing; nats
    permuted = np.zeros((4, 5), dtype=np.int64)
    permuted[[0, 1, 2, 3], [3, 0, 4, 1]] = rows
    assert abs(mi(permuted) - h(rows)) <= 8 * np.finfo(np.float64).eps * h(rows)
    assert abs(mi(np.eye(2, dtype=np.int64)) - math.log(2)) <= 4 * np.finfo(np.float64).eps
    # against the definition on probabilities, on a table with empty cells
    rng = np.random.default_rng(5)
    table = rng.integers(0, 50, size=(7, 9)) * (rng.random((7, 9)) < 0.7)
    pij = table / table.sum()
    pi, pj = pij.sum(axis=1, keepdims=True), pij.sum(axis=0, keepdims=True)
    nz = pij > 0
    assert abs(mi(table) - float((pij[nz] * np.log(pij[nz] / (pi * pj)[nz])).sum())) <= 1e-13


def test_bins_and_limits_need_no_device():
    assert ps.split_bins(64) == (64, 64) and ps.split_bins((16, 8)) == (16, 8)
    e = np.linspace(0, 1, 5)
    assert ps.split_bins((e, 3))[1] == 3 and ps.split_bins([e, e])[0] is e
    for bad in ((1, 2, 3), "ab"[:1], None, 2.5):
        with pytest.raises(ValueError):
            ps.split_bins(bad)
    ps.check_bins(1024, 16)
    ps.check_bins(128, 128)
    with pytest.raises(ValueError, match="1024 bins per axis"):
        ps.check_bins(1025, 1)
    with pytest.raises(ValueError, match="16384 cells"):
        ps.check_bins(1024, 17)
    with pytest.raises(ValueError, match="at least 1"):
        ps.check_bins(4, 0)


# ------------------------------------------------------------------------------------------------ the methods
def _obj(dims, bonds, mode="Std", dtype=None, shape=None):
    torch = pytest.importorskip("torch")
    from imgcompressionmps_amd import NDMPS
    from imgcompressionmps_amd.core.mps import DeviceMPS

    cores = [torch.full((bonds[j], d, bonds[j + 1]), 0.5, dtype=dtype or torch.float32) for j, d in enumerate(dims)]
    obj = NDMPS(DeviceMPS(cores), np.array(dims), None, None, False, None, mode, len(shape or (1,)))
    obj._shape = shape
    return obj


def test_preconditions_of_the_methods_need_no_device():
    torch = pytest.importorskip("torch")
    from imgcompressionmps_amd import NDMPS

    dims, shape = [4, 4, 4], (8, 8)
    a = _obj(dims, [1, 2, 2, 1], shape=shape)
    calls = (lambda x, y: x.pair_stats(y), lambda x, y: x.joint_histogram(y), lambda x, y: x.mutual_information(y),
             lambda x, y: NDMPS.mutual_information_many([x], y))
    for call in calls:
        with pytest.raises(TypeError, match="NDMPS"):
            call(a, np.zeros(shape))
        with pytest.raises(ValueError, match="DCT"):
            call(a, _obj(dims, [1, 2, 2, 1], mode="DCT", shape=shape))
        with pytest.raises(ValueError, match="DCT"):
            call(_obj(dims, [1, 2, 2, 1], mode="DCT", shape=shape), a)
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(a, _obj(dims, [1, 3, 2, 1], dtype=torch.bfloat16, shape=shape))
        with pytest.raises(ValueError, match="shape is unknown"):
            call(a, _obj(dims, [1, 2, 2, 1]))
        with pytest.raises(ValueError, match="in shape"):
            call(a, _obj(dims, [1, 2, 2, 1], shape=(4, 16)))
        with pytest.raises(ValueError, match="site dims|qubit_size"):
            call(a, _obj([8, 2, 4], [1, 2, 2, 1], shape=shape))
    with pytest.raises(TypeError, match="NDMPS"):
        NDMPS.mutual_information_many([a, 3], a)
    # chains whose last products would differ in rows or columns are refused where two chains meet
    from imgcompressionmps_amd.core.mps import DeviceMPS

    other = DeviceMPS([torch.zeros((1, 8, 2)), torch.zeros((2, 8, 1))])
    with pytest.raises(ValueError, match="site dims.*rows or columns"):
        ps.pair_chains(a.mps, other)
    with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
        ps.pair_chains(a.mps, _obj(dims, [1, 2, 2, 1], dtype=torch.bfloat16, shape=shape).mps)
    # one fp32 and one fp64 chain make an fp64 pair; two of a kind are taken as they are
    b64 = _obj(dims, [1, 3, 2, 1], dtype=torch.float64, shape=shape).mps
    wa, wb = ps.pair_chains(a.mps, b64)
    assert wa.dtype == wb.dtype == torch.float64 and wb is b64 and list(wa.bonds) == list(a.mps.bonds)
    assert all(torch.equal(x.to(torch.float64), y) for x, y in zip(a.mps.cores, wa.cores))
    sa, sb = ps.pair_chains(a.mps, a.mps)
    assert sa is a.mps and sb is a.mps
