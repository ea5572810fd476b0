"""Histograms and quantiles per label from the cores, on the host (no GPU): the window rule, the refusals, the exported
names, and the cases and bars of tests/labelhist_cases.py.

* ndmps_labelhist_plan_query equals the window rule stated in Python integers (labelhist_cases.window_rule) and refuses
  what needs more than 64 launches; the workspace is the value statistics' plus the table and the edge rows.
* the refusals the C entries make before their first launch (with pointers that are never dereferenced) and the ones
  core/labelhist.py makes before it touches the device.
* header, ``_lib.SIGNATURES`` and the library's exports agree on the ``ndmps_labelhist_`` names.
* the bars accept the reference and reject every modelled fault (labels read in site order, a tile left out, padding
  counted into label 0, windows folded, the shared edge row used for per-label rows, the last bin open on the right,
  NaN in a bin, outside voxels added to the first or the last label, a voxel on a repeated last edge lost) on every case
  where the fault can occur.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import labelhist_cases as hc
import labelstat_cases as lc
import valstat_cases as vc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import labelhist as lh
from oracle import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndmps_labelhist_workspace_bytes", "ndmps_labelhist_plan_query", "ndmps_labelhist_f32", "ndmps_labelhist_f64")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the names
def test_header_signatures_and_exports_agree(lib):
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    declared = set(re.findall(r"\b(ndmps_labelhist_\w+)\s*\(", header))
    assert declared == set(NAMES)
    assert {n for n in _lib.SIGNATURES if n.startswith("ndmps_labelhist_")} == declared
    for name in NAMES:
        assert hasattr(lib, name), name


# ------------------------------------------------------------------------------------------------ the window rule
@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("per_label", [False, True])
def test_plan_query_is_the_window_rule(lib, elem_bytes, per_label):
    refused = []
    for bins in (1, 64, 1000, 4096):
        for n_labels in (1, 7, 1030, 4096):
            want = hc.window_rule(elem_bytes, n_labels, bins, per_label)
            out = (C.c_int64 * 4)(-1, -1, -1, -1)
            status = lib.ndmps_labelhist_plan_query(elem_bytes, n_labels, bins, int(per_label), out)
            if want is None:
                refused.append((bins, n_labels))
                assert status == _lib.EINVAL and list(out) == [-1] * 4
                message = lib.ndmps_last_error()
                assert b"fewer bins" in message and b"split the atlas" in message and b"64" in message, message
                with pytest.raises(ValueError, match="fewer bins or split the atlas"):
                    lh.plan_query(np.float32 if elem_bytes == 4 else np.float64, n_labels, bins, per_label)
                continue
            assert status == _lib.OK
            got = dict(zip(("window", "launches", "lds_bytes", "table_bytes"), out))
            assert got == want == lh.plan_query(np.float32 if elem_bytes == 4 else np.float64, n_labels, bins, per_label)
            # the largest window that fits: one label more would not (or there is none)
            assert got["lds_bytes"] <= 65536 and 1 <= got["window"] <= n_labels
            rows = got["window"] if per_label else 1
            assert got["lds_bytes"] == elem_bytes * (rows * (bins + 1) + 2 * got["window"]) + 4 * got["window"] * (bins + 3)
            if got["window"] < n_labels:
                w = got["window"] + 1
                assert elem_bytes * ((w if per_label else 1) * (bins + 1) + 2 * w) + 4 * w * (bins + 3) > 65536
    assert (4096, 1030) in refused and (4096, 4096) in refused and (1000, 4096) in refused
    assert (4096, 7) not in refused and (64, 4096) not in refused and (1, 4096) not in refused
    # a window of one label always fits
    assert hc.window_rule(8, 1, 4096, True)["lds_bytes"] == 49188
    out = (C.c_int64 * 4)()
    for bad in ((2, 7, 64), (4, 0, 64), (4, 4097, 64), (4, 7, 0), (4, 7, 4097)):
        assert lib.ndmps_labelhist_plan_query(*bad, int(per_label), out) == _lib.EINVAL, bad
    assert lib.ndmps_labelhist_plan_query(4, 7, 64, int(per_label), None) == _lib.EINVAL


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_workspace_is_the_valstat_workspace_plus_table_and_edges(lib, elem_bytes):
    for name in sorted(vc.ALL_CHAINS):
        dims, bonds = vc.ALL_CHAINS[name]
        L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
        base = lib.ndmps_valstat_workspace_bytes(L, d, b, elem_bytes, 0)
        for n_labels, bins, per_label in ((1, 1, 0), (7, 64, 0), (7, 64, 1), (7, 4096, 1), (1030, 256, 0), (4096, 64, 1)):
            table = hc.window_rule(elem_bytes, n_labels, bins, bool(per_label))["table_bytes"]
            edges = -(-((n_labels if per_label else 1) * (bins + 1) * elem_bytes) // 256) * 256
            assert lib.ndmps_labelhist_workspace_bytes(L, d, b, elem_bytes, n_labels, bins, per_label) == base + table + edges
        for n_labels, bins in ((0, 64), (4097, 64), (7, 0), (7, 4097), (4096, 4096)):
            assert lib.ndmps_labelhist_workspace_bytes(L, d, b, elem_bytes, n_labels, bins, 0) == 0
        assert lib.ndmps_labelhist_workspace_bytes(L, d, b, 2, 7, 64, 0) == 0
        assert lib.ndmps_labelhist_workspace_bytes(0, d, b, elem_bytes, 7, 64, 0) == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the device pointers are fakes."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[256] * L)
    p = 256
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    counts = np.zeros(4096 * 8, dtype=np.int64).ctypes.data
    minmax = np.zeros(2 * 4096, dtype=np.float64).ctypes.data
    info = np.zeros(2, dtype=np.int64).ctypes.data
    for suffix, eb, np_type in (("f32", 4, np.float32), ("f64", 8, np.float64)):
        entry = getattr(lib, f"ndmps_labelhist_{suffix}")
        shared = np.linspace(-1, 1, 5).astype(np_type)
        rows = np.tile(shared, (7, 1))

        def call(n_labels=7, lab_bytes=2, lab=p, row=p, col=p, perm=p, cols=n_cols, ws=p, nbytes=1 << 30, edges=shared,
                 bins=4, per_label=0, out=counts, bonds_=b, cores=fake):
            keep = None if edges is None else np.ascontiguousarray(edges)
            return entry(L, d, bonds_, cores, lab, lab_bytes, row, col, perm, cols, n_labels,
                         None if keep is None else keep.ctypes.data, bins, per_label, out, minmax, info, ws, nbytes, None)

        for n_labels in (0, -3, 4097):
            assert call(n_labels=n_labels) == _lib.EINVAL and b"labels" in lib.ndmps_last_error(), n_labels
        for bins in (0, -1, 4097):
            assert call(bins=bins) == _lib.EINVAL and b"bins" in lib.ndmps_last_error(), bins
        for lab_bytes in (0, 3, 8):
            assert call(lab_bytes=lab_bytes) == _lib.EINVAL and b"bytes" in lib.ndmps_last_error(), lab_bytes
        for missing in ("lab", "row", "col", "perm"):
            assert call(**{missing: None}) == _lib.EINVAL and b"NULL" in lib.ndmps_last_error(), missing
        assert call(edges=None) == _lib.EINVAL
        assert call(out=None) == _lib.EINVAL
        assert call(cores=None) == _lib.EINVAL
        # a descending or a NaN edge row, in row 0 and in a later row; a row that repeats an edge is legal
        for bad in ([-1, 0.5, 0, 1, 2], [-1, 0, np.nan, 1, 2]):
            assert call(edges=np.array(bad, dtype=np_type)) == _lib.EINVAL and b"ascending" in lib.ndmps_last_error()
            for r in (0, 3, 6):
                broken = rows.copy()
                broken[r] = bad
                assert call(edges=broken, per_label=1) == _lib.EINVAL and b"ascending" in lib.ndmps_last_error(), r
        padded = rows.copy()
        padded[:, 2:] = padded[:, 2:3]
        need = lib.ndmps_labelhist_workspace_bytes(L, d, b, eb, 7, 4, 1)
        assert need > 0
        assert call(edges=padded, per_label=1, nbytes=need - 1) == _lib.EWORKSPACE  # legal rows: the next check refuses
        assert call(n_labels=4096, bins=4096, edges=np.zeros(4097, dtype=np_type)) == _lib.EINVAL
        assert b"fewer bins" in lib.ndmps_last_error()
        assert call(cols=n_cols * dims[-2]) == _lib.EINVAL and b"columns" in lib.ndmps_last_error()
        assert call(bonds_=_lib.i64_array([1, 4, 13, 13, 1])) == _lib.EINVAL and b"exceeds" in lib.ndmps_last_error()
        assert call(ws=264) == _lib.EINVAL and b"aligned" in lib.ndmps_last_error()
        assert call(ws=None) == _lib.EWORKSPACE
        need = lib.ndmps_labelhist_workspace_bytes(L, d, b, eb, 7, 4, 0)
        assert call(nbytes=need - 1) == _lib.EWORKSPACE and b"labelhist workspace" in lib.ndmps_last_error()
        # room for the chain and the records but not for the table
        assert call(nbytes=lib.ndmps_valstat_workspace_bytes(L, d, b, eb, 0)) == _lib.EWORKSPACE


def test_python_refusals_before_the_device():
    shape = (6, 10)
    good = np.arange(60).reshape(shape) % 3
    inside = lh.mask_labels(good)
    assert inside.dtype == np.bool_ and np.array_equal(inside, good != 0)
    assert np.array_equal(lh.mask_labels(good > 1), good > 1)
    assert np.array_equal(lh.mask_labels(good.astype(np.uint8) * 200), good != 0)
    for dtype in (np.float32, np.float64, np.complex64):
        with pytest.raises(TypeError, match="bool or integer"):
            lh.mask_labels(good.astype(dtype))
    with pytest.raises(ValueError, match="fewer bins or split the atlas"):
        lh.plan_query(np.float32, 4096, 4096, False)
    with pytest.raises(ValueError, match="labels"):
        lh.plan_query(np.float32, 4097, 4, False)
    with pytest.raises(ValueError, match="bins"):
        lh.plan_query(np.float64, 7, 4097, True)


# ------------------------------------------------------------------------------------------------ the bars
def _reject(bar, fault, label):
    try:
        bar(fault)
    except AssertionError:
        return
    pytest.fail(f"the bar accepted the fault {label}")


@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_one_pass_references_equal_numpy_label_by_label(name):
    """``hist_of`` and ``quantiles_of`` are ``vc.ref_histogram`` and ``np.quantile(..., method="inverted_cdf")`` of each
    label's voxels, on the reference and with NaN planted, for shared and per-label rows."""
    c = vc.case(name, "integer", "f64")
    _, ref_nan = vc.with_nan(c)
    for ref in (c.ref, ref_nan):
        for kind in ("one", "scatter", "outside", "empty") if c.n < 2 ** 18 else ("outside",):
            lab, n_labels = lc.labels(c, kind)
            tables = dict(vc.integer_edge_sets(ref, np.float64), rows=hc.per_label_rows(ref, lab, n_labels, 16, np.float64))
            for label, edges in tables.items():
                assert hc.same_result(hc.hist_of(ref, lab, n_labels, edges), hc.hist_of_by_numpy(ref, lab, n_labels, edges)), \
                    (kind, label)
            fast = hc.quantiles_of(ref, lab, n_labels, hc.QS + (0.1, 0.999))
            for j, q in enumerate(hc.QS + (0.1, 0.999)):
                assert lc.same_bits(fast[:, j], hc.quantile_of_by_numpy(ref, lab, n_labels, q)), (kind, q)


def _edge_sets(c, n_labels):
    """The integer edge tables a call with ``n_labels`` labels is not refused for (fp64, the wider element)."""
    sets = vc.integer_edge_sets(c.ref, np.float64)
    return {k: e for k, e in sets.items() if hc.window_rule(8, n_labels, e.size - 1, False) is not None}


@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_exact_bar_on_the_reference_and_on_modelled_faults(name):
    c = vc.case(name, "integer", "f64")
    assert not c.identity
    found = {}  # the places of the voxels in a table, shared by the label volumes
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        sets = _edge_sets(c, n_labels)
        assert {"one_bin", "one_bin_inside", "range_excludes"} <= set(sets) and (n_labels > 9 or len(sets) == 7), sorted(sets)
        for label, edges in sets.items():
            plan = hc.window_rule(8, n_labels, edges.size - 1, False)
            truth = hc.hist_of(c.ref, lab, n_labels, edges)
            hc.exact_histogram(truth, c.ref, lab, n_labels, edges)
            faults = hc.histogram_faults(c, c.ref, lab, n_labels, edges, plan["window"], found.setdefault(label, {}))
            expected = {"tile_left_out"}
            if kind != "one" and label != "one_bin":  # one label, or one bin that holds every voxel: the address is moot
                expected.add("site_order_labels")
            if n_labels > plan["window"]:
                expected.add("windows_folded")
            if kind == "outside":
                expected |= {"outside_to_first", "outside_to_last"}
            if label in ("last_edge_is_max", "one_bin"):
                expected.add("last_bin_open")
            assert expected <= set(faults), (kind, label, sorted(faults))
            for what, fault in faults.items():
                _reject(lambda f: hc.exact_histogram(f, c.ref, lab, n_labels, edges, truth), fault,
                        f"{name}/{kind}/{label}/{what}")
            if label == "bins_4096" and n_labels == 7:
                assert plan["window"] == 1 and plan["launches"] == 7
                assert hc.window_rule(4, 7, 4096, False)["window"] == 2
    # one row per label, short rows padded with their last edge
    for kind in ("blocks", "scatter", "outside"):
        lab, n_labels = lc.labels(c, kind)
        rows = hc.per_label_rows(c.ref, lab, n_labels, 16, np.float64)
        truth = hc.hist_of(c.ref, lab, n_labels, rows)
        hc.exact_histogram(truth, c.ref, lab, n_labels, rows)
        faults = hc.histogram_faults(c, c.ref, lab, n_labels, rows)
        assert "shared_row_used" in faults or np.all(rows == rows[0]), (kind, sorted(faults))
        if np.any(rows[:, -2] == rows[:, -1]):
            assert "padded_edge_lost" in faults, (kind, sorted(faults))
        for what, fault in faults.items():
            _reject(lambda f: hc.exact_histogram(f, c.ref, lab, n_labels, rows), fault, f"{name}/{kind}/rows/{what}")
    # NaN planted in a core: counted per label, in no bin
    _, ref_nan = vc.with_nan(c)
    for kind in ("blocks", "scatter"):
        lab, n_labels = lc.labels(c, kind)
        edges = vc.integer_edge_sets(ref_nan, np.float64)["half_integers"]
        hc.exact_histogram(hc.hist_of(ref_nan, lab, n_labels, edges), ref_nan, lab, n_labels, edges)
        faults = hc.histogram_faults(c, ref_nan, lab, n_labels, edges)
        assert "nan_in_a_bin" in faults
        for what, fault in faults.items():
            _reject(lambda f: hc.exact_histogram(f, ref_nan, lab, n_labels, edges), fault, f"{name}/{kind}/nan/{what}")


def test_padding_and_padded_edge_faults_occur_on_some_integer_case():
    padded, lost = [], []
    for name in sorted(vc.INT_CHAINS):
        c = vc.case(name, "integer", "f64")
        lab, n_labels = lc.labels(c, "blocks")
        edges = vc.integer_edge_sets(c.ref, np.float64)["range_excludes"]
        if "padding_counted" in hc.histogram_faults(c, c.ref, lab, n_labels, edges):
            padded.append(name)
        rows = hc.per_label_rows(c.ref, lab, n_labels, 16, np.float64)
        if "padded_edge_lost" in hc.histogram_faults(c, c.ref, lab, n_labels, rows):
            lost.append(name)
    assert padded, "no integer case has padded tiles"
    assert lost, "no integer case has a voxel on a repeated last edge"


@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_exact_quantile_bar_on_the_reference_and_on_modelled_faults(name):
    c = vc.case(name, "integer", "f64")
    span = int(c.ref.max() - c.ref.min()) + 1
    for bins in (4, 64):
        passes = hc.passes_for(c.ref, bins)
        assert bins ** passes >= span and (passes == 1 or bins ** (passes - 1) < span)
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        plan = hc.window_rule(8, n_labels, 64, True)
        assert plan is not None, "label_quantile's default bins serve 4096 labels"
        truth = hc.quantile_truth(c.ref, lab, n_labels, hc.QS)
        for q in hc.QS:
            hc.exact_quantile(truth[q], c.ref, lab, n_labels, q)
        faults = hc.quantile_faults(c, lab, n_labels, hc.QS, plan["window"])
        assert set(faults["tile_left_out"]) == set(hc.QS)  # the count changes: every q differs
        if n_labels > plan["window"]:
            assert "windows_folded" in faults
        if kind == "outside":
            assert {"outside_to_first", "outside_to_last"} <= set(faults)
        for what, by_q in faults.items():
            for q, fault in by_q.items():
                _reject(lambda f: hc.exact_quantile(f, c.ref, lab, n_labels, q), fault, f"{name}/{kind}/q{q}/{what}")


SANDWICH_MUST_REJECT = ("site_order_labels", "tile_left_out", "padding_counted", "outside_to_first", "outside_to_last")


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, family, storage):
    c = vc.case(name, family, storage)
    edges = c.edges64()
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(c, kind)
        truth = hc.hist_of(c.ref, lab, n_labels, edges)
        hc.sandwich_histogram(truth, c.ref, c.bound, lab, n_labels, edges)
        faults = hc.histogram_faults(c, c.ref, lab, n_labels, edges)
        assert "tile_left_out" in faults and (c.identity or "site_order_labels" in faults), (kind, sorted(faults))
        for what in SANDWICH_MUST_REJECT:  # the faults that move whole voxels: an open last bin hides inside the bound
            if what in faults:
                _reject(lambda f: hc.sandwich_histogram(f, c.ref, c.bound, lab, n_labels, edges), faults[what],
                        f"{name}/{kind}/{what}")
        qs = (0.0, 0.5, 1.0)
        truth = hc.quantile_truth(c.ref, lab, n_labels, qs)
        wrong = hc.quantile_faults(c, lab, n_labels, qs)
        for q in qs:
            hc.sandwich_quantile(truth[q], c.ref, c.bound, lab, n_labels, q)
            for what in ("tile_left_out", "outside_to_first", "outside_to_last"):  # they change a label's count
                if q in wrong.get(what, {}):
                    _reject(lambda f: hc.sandwich_quantile(f, c.ref, c.bound, lab, n_labels, q), wrong[what][q],
                            f"{name}/{kind}/q{q}/{what}")
