"""The Gram family's size queries, pinned (no GPU).  Every launcher lays its partial tiles out by the plan the query
was answered from, and callers allocate by the query: a changed number here is a changed workspace layout.  The table
was recorded from the build before the queries were moved onto the plan; it hits every route and every boundary
between two routes (n = 8/9, 16/17, 32/33, 63/64/65, 127/128; m = 255/256; one matrix / two; the 48/49 matrices of a
launch of the 128-wide kernel; more than 64 matrices of the 64-wide ones)."""
import ctypes as C

import numpy as np
import pytest

import sweep_cases as sc
from imgcompressionmps_amd import _lib

SWITCHES = ("NDMPS_GRAM_XCD", "NDMPS_GRAM64_TILES", "NDMPS_GRAM_NO_TURN", "NDMPS_GRAM_GENERAL")

# (query, batch, m, n, bytes)
PINNED = [
    ('f32', 1, 1, 1, 73984), ('f32', 1, 64, 8, 73984), ('f32', 1, 200001, 8, 73984), ('f32', 1, 2097152, 8, 73984),
    ('f32', 1, 1000, 9, 39168), ('f32', 1, 16, 16, 6400), ('f32', 1, 4096, 16, 143616), ('f32', 1, 300, 17, 57600),
    ('f32', 1, 777, 32, 123136), ('f32', 1, 777, 33, 491776), ('f32', 1, 32768, 48, 17891584),
    ('f32', 1, 255, 63, 196864), ('f32', 1, 256, 63, 196864), ('f32', 1, 255, 64, 196864),
    ('f32', 1, 256, 64, 131328), ('f32', 1, 4096, 64, 1179904), ('f32', 1, 2097152, 64, 17891584),
    ('f32', 1, 255, 65, 590080), ('f32', 1, 256, 65, 393472), ('f32', 1, 4099, 96, 3637504),
    ('f32', 1, 255, 127, 590080), ('f32', 1, 256, 127, 393472), ('f32', 1, 255, 128, 590080),
    ('f32', 1, 256, 128, 262400), ('f32', 1, 300, 128, 262400), ('f32', 1, 257, 131, 786688),
    ('f32', 1, 5000, 130, 9437440), ('f32', 1, 1001, 136, 1966336), ('f32', 1, 100, 257, 1966336),
    ('f32', 1, 4096, 512, 35127552), ('f32', 1, 200001, 512, 67109120), ('f32', 1, 333, 680, 5505280),
    ('f32', 1, 32768, 2048, 69206272), ('f64', 1, 1, 1, 6400), ('f64', 1, 1000, 8, 39168),
    ('f64', 1, 1000, 9, 39168), ('f64', 1, 4096, 16, 143616), ('f64', 1, 300, 17, 57600),
    ('f64', 1, 777, 33, 491776), ('f64', 1, 256, 64, 196864), ('f64', 1, 4096, 64, 2294016),
    ('f64', 1, 256, 128, 590080), ('f64', 1, 5000, 130, 16711936), ('f64', 1, 200001, 512, 18874624),
    ('f64', 1, 333, 680, 17301760), ('batched', 1, 256, 128, 262400), ('batched', 1, 4096, 512, 35127552),
    ('batched', 2, 256, 128, 262400), ('batched', 2, 255, 128, 0), ('batched', 1, 256, 127, 0),
    ('batched', 2, 256, 127, 393472), ('batched', 2, 255, 127, 0), ('batched', 1, 4096, 64, 0),
    ('batched', 2, 4096, 64, 2097408), ('batched', 2, 256, 64, 131328), ('batched', 2, 255, 64, 0),
    ('batched', 2, 4096, 63, 0), ('batched', 2, 4096, 65, 6291712), ('batched', 3, 1000, 200, 1179904),
    ('batched', 5, 300, 128, 655616), ('batched', 32, 512, 512, 41943296), ('batched', 2, 20000, 384, 47186176),
    ('batched', 4, 257, 131, 1573120), ('batched', 32, 32768, 64, 49283328), ('batched', 3, 5000, 64, 3932416),
    ('batched', 2, 300, 100, 590080), ('batched', 70, 700, 96, 41287936), ('batched', 2, 4099, 64, 2162944),
    ('batched', 66, 260, 64, 6488320), ('batched', 48, 4096, 512, 427819264),
    ('batched', 49, 4096, 512, 436732160), ('batched', 48, 1024, 128, 12583168),
    ('batched', 49, 1024, 128, 12845312), ('batched', 64, 2097152, 64, 50331904),
    ('batched', 32, 200001, 2048, 570425600),
]


@pytest.fixture
def lib(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def _query(lib, which, batch, m, n):
    if which == "batched":
        return lib.ndmps_gram_batched_workspace_bytes(batch, m, n)
    return (lib.ndmps_gram_f64_workspace_bytes if which == "f64" else lib.ndmps_gram_workspace_bytes)(m, n)


def test_gram_size_queries_are_pinned(lib):
    assert len(PINNED) >= 60
    got = [(which, batch, m, n, _query(lib, which, batch, m, n)) for which, batch, m, n, _ in PINNED]
    assert got == PINNED


def test_plan_query_reports_the_size_the_size_queries_return(lib):
    """ndmps_gram_plan_query answers from the same GramPlan: slot 13 is the size query's number on every pinned row
    (fp32 and bf16 share a plan), and the route slot is 0 exactly where there is nothing to run."""
    for which, batch, m, n, nbytes in PINNED:
        for elem in ((2,) if which == "f64" else (0, 1)):
            out = (C.c_int64 * 14)()
            assert lib.ndmps_gram_plan_query(elem, batch, m, n, 0, int(which == "batched"), out) == 0
            assert out[13] == nbytes, (which, elem, batch, m, n)
            assert (out[0] == 0) == (nbytes == 0)
            assert 0 <= out[0] <= 6
    assert lib.ndmps_gram_plan_query(3, 1, 64, 8, 0, 0, out) == _lib.EINVAL
    assert lib.ndmps_gram_plan_query(0, 1, 64, 8, 0, 0, None) == _lib.EINVAL


def test_shapes_without_a_route_need_no_workspace(lib):
    """What test_gram_batched_fp64 asserts on the GPU: narrower matrices and a lone 64-column matrix have no batched
    route (the caller loops over ndmps_gram_f32); nor have short ones, empty ones and an empty batch."""
    for m in (300, 512, 1000, 4096, 4099, 5000, 20000, 32768, 700, 257, 260):
        assert lib.ndmps_gram_batched_workspace_bytes(3, m, 48) == 0
        assert lib.ndmps_gram_batched_workspace_bytes(1, m, 64) == 0
    for batch, m, n in [(0, 4096, 512), (-1, 4096, 512), (4, 255, 512), (4, 0, 512), (4, 4096, 0), (4, 4096, 8)]:
        assert lib.ndmps_gram_batched_workspace_bytes(batch, m, n) == 0
    for m, n in [(0, 64), (64, 0), (-3, 8), (8, -3)]:
        assert lib.ndmps_gram_workspace_bytes(m, n) == 0 and lib.ndmps_gram_f64_workspace_bytes(m, n) == 0


def test_the_switches_move_only_the_plans_they_name(lib, monkeypatch):
    """NDMPS_GRAM64_TILES sends a batch of 64-column matrices to the tile kernel (shorter slabs, more partial tiles);
    NDMPS_GRAM_XCD regroups big batched launches of the 128-wide kernel; both are read per call."""
    base = {k: _query(lib, *k) for k in [("batched", 32, 32768, 64), ("batched", 32, 4096, 512), ("f32", 1, 4096, 512),
                                         ("batched", 70, 700, 96), ("f32", 1, 4096, 64)]}
    monkeypatch.setenv("NDMPS_GRAM64_TILES", "1")
    assert _query(lib, "batched", 32, 32768, 64) > base[("batched", 32, 32768, 64)]
    assert all(_query(lib, *k) == v for k, v in base.items() if k != ("batched", 32, 32768, 64))
    monkeypatch.delenv("NDMPS_GRAM64_TILES")
    monkeypatch.setenv("NDMPS_GRAM_XCD", "1")
    assert _query(lib, "batched", 32, 4096, 512) != base[("batched", 32, 4096, 512)]
    assert all(_query(lib, *k) == v for k, v in base.items() if k != ("batched", 32, 4096, 512))
    monkeypatch.delenv("NDMPS_GRAM_XCD")
    assert all(_query(lib, *k) == v for k, v in base.items())


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_sweep_workspace_covers_every_gram_it_can_reach(lib, name):
    """The sweep sizes its Gram workspace before it knows the bonds it will find (gram_ws_bound): at every site whose
    Gram is taken of the columns (n <= m), for every bond up to the cap, and for the raw Gram of the merged trailing
    run, the sweep's workspace is at least what the Gram entry it calls asks for."""
    case = sc.CASES[name]
    dims = sc.site_dims(case["shape"])
    L, cap, batch = len(dims), case["cap"] or 0, len(case["members"])
    cd = _lib.i64_array(dims)
    sweep = {"f32": lib.ndmps_tt_sweep_batched_workspace_bytes(batch, L, cd, cap),
             "f64": lib.ndmps_tt_sweep_batched_workspace_bytes_f64(batch, L, cd, cap)}
    assert min(sweep.values()) > 0
    reach = []  # (m, n') of every Gram the sweep can ask for
    for i in range(1, L):
        m, right = int(np.prod(dims[:i])), int(np.prod(dims[i + 1:]))
        chi_max = min(int(np.prod(dims[:i + 1])), right, cap or right)
        reach += [(m, dims[i] * chi) for chi in range(1, chi_max + 1) if dims[i] * chi <= m]
    start = sc.merge_start(dims, cap)
    if start < L:
        merge_n = int(np.prod(dims[start:]))
        reach.append((int(np.prod(dims)) // merge_n, merge_n))
    assert reach
    for m, n in reach:
        assert sweep["f32"] >= lib.ndmps_gram_workspace_bytes(m, n), (m, n)
        assert sweep["f64"] >= lib.ndmps_gram_f64_workspace_bytes(m, n), (m, n)
        assert sweep["f32"] >= lib.ndmps_gram_batched_workspace_bytes(batch, m, n), (batch, m, n)
