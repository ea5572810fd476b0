"""Statistics of two chains from the cores, on the host (no GPU).

* chain_pair_plan (csrc/pairstat_plan.h) through ndmps_pairstat_plan_query / _workspace_bytes against a Python
  restatement of the layout, on every pair of tests/pairstat_cases.py.
* what is refused before any launch: more than 16384 cells, an axis above 1024 bins, and the chain checks of the
  single-chain entries on either chain, with pointers that are never dereferenced.  The C entries take ONE dims array,
  and chain_plan splits by the dims alone, so two last products that differ in rows or columns cannot be handed to
  them; that refusal is made where two chains meet, in core/pairstat.py, and tested there.
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
