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
"""
import ctypes as C
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

