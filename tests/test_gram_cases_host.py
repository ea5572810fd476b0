"""tests/gram_cases.py on the CPU: every case reaches the route and the edge it was chosen for (through
ndmps_gram_plan_query, no GPU call), the integer data is exact in fp64 in any order of summation, and the two
assertions of tests/test_gpu_gram_routes.py reject, on exactly these cases, the errors a Gram kernel can make without
the old max-norm bar noticing."""
import numpy as np
import pytest

import gram_cases as gc
from imgcompressionmps_amd import _lib

TILE_EDGE = {"Small": 8, "Tiles64": 64, "Tiles64Batched": 64, "Stream64": 64, "Tiles128": 128}


@pytest.fixture
def lib(monkeypatch):
    gc.set_switch(monkeypatch, None)
    return _lib.load()


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name,switch", gc.variants(), ids=lambda v: str(v))
def test_case_takes_the_route_and_geometry_it_exists_for(lib, monkeypatch, name, switch):
    case = gc.CASES[name]
    gc.set_switch(monkeypatch, switch)
    plan = gc.plan_of(lib, case)
    facts = gc.facts_of(case, plan, switch)
    want = dict(case["facts"], **(case["switches"][switch] if switch else {}))
    assert {k: facts.get(k) for k in want} == want
    # the plan's size is the size query's, under the switch as well
    if gc.is_batched(case):
        assert plan["workspace_bytes"] == lib.ndmps_gram_batched_workspace_bytes(case["batch"], case["m"], case["n"]) > 0
    elif case["elem"] == "f64":
        assert plan["workspace_bytes"] == lib.ndmps_gram_f64_workspace_bytes(case["m"], case["n"]) > 0
    else:
        assert plan["workspace_bytes"] == lib.ndmps_gram_workspace_bytes(case["m"], case["n"]) > 0


def test_the_table_covers_what_it_claims(lib, monkeypatch):
    """Every route, both fetch arms of every staged kernel, every mode of the 128-wide one, both XCD orders engaged
    (mode 1's odd last off-diagonal slab among them) and not engaged, a second launch chunk on every batched route."""
    seen = set()
    for name, switch in gc.variants():
        case = gc.CASES[name]
        gc.set_switch(monkeypatch, switch)
        f = gc.facts_of(case, gc.plan_of(lib, case), switch)
        seen.add((f["route"], case["elem"]))
        seen.add((f["route"], "vec_ok", f["vec_ok"]))
        seen.add((f["route"], "launches", f.get("launches")))
        seen.add((f["route"], "gathered", gc.is_gathered(case)))
        if f["route"] == "Tiles128":
            seen.add(("mode", f["mode"], "xcd", f["xcd"]))
            if f["xcd"] == 1 and f["slabs_off"] % 2 == 1:
                seen.add("xcd 1, odd last slab")
            if case["batch"] > 48 and f["xcd"]:
                seen.add("xcd in the second chunk")
    for route in ("Small", "Tiles16", "Tiles64", "Tiles128", "Tiles64Batched", "Stream64"):
        assert (route, "f32") in seen and (route, "bf16") in seen
    assert ("Tiles16", "f64") in seen
    for route in ("Small", "Tiles64", "Tiles128"):
        assert (route, "vec_ok", 0) in seen and (route, "vec_ok", 1) in seen
    for route in ("Tiles128", "Tiles64Batched", "Stream64"):
        assert (route, "launches", 2) in seen and (route, "gathered", True) in seen
    assert ("Tiles64", "gathered", True) in seen
    for mode in (0, 1, 2):
        for xcd in (0, 1, 2):
            assert ("mode", mode, "xcd", xcd) in seen
    assert "xcd 1, odd last slab" in seen and "xcd in the second chunk" in seen


@pytest.mark.parametrize("name", list(gc.CASES))
def test_integer_data_is_exact_and_the_assertions_have_teeth(lib, name):
    case = gc.CASES[name]
    m, n, elem = case["m"], case["n"], case["elem"]
    plan = gc.plan_of(lib, case)
    imax = gc.IMAX[elem] if case["imax"] is None else case["imax"]
    assert m * imax * imax < 2 ** 53
    a, exact = gc.data(name, "integer")[0]
    assert np.abs(a).max() <= imax and np.array_equal(gc.cc.to_storage(a, elem), a)
    ai = a.astype(np.int64)
    assert exact.dtype == np.int64 and np.array_equal(ai[:, -3:].T @ ai, exact[-3:])
    g_ref = exact.astype(np.float64)
    gc.check_integer(g_ref, exact)

    # summed slab by slab in fp64, as the kernels do: the same integers
    rows = gc.slab_rows(plan)
    g = np.zeros((n, n))
    for r0 in range(0, m, rows):
        g = g + a[r0:r0 + rows].T @ a[r0:r0 + rows]
    gc.check_integer(g, exact)

    ag, ref64, absg = gc.data(name, "graded")[0]
    gc.check_graded(ref64, ref64, absg, m)
    for mat, good, check, args in ((a, g_ref, gc.check_integer, (exact,)), (ag, ref64, gc.check_graded, (ref64, absg, m))):
        integer = check is gc.check_integer
        # an fp32 accumulator
        a32 = mat.astype(np.float32)
        wrong = (a32.T @ a32).astype(np.float64)
        if integer:
            assert exact.max() > 2 ** 24 or elem == "bf16"   # bf16: 255^2 m / 3 reaches 2^24 from 775 rows on
        if not integer or exact.max() > 2 ** 24:
            assert _rejects(check, wrong, *args), "fp32 accumulation"
        # the last row of the first slab missing from the last diagonal tile
        edge = TILE_EDGE.get(gc.ROUTES[plan["route"]], 16 * plan["T"])
        j0 = (n - 1) // edge * edge
        r = min(m, rows) - 1
        assert np.count_nonzero(mat[r, j0:]) > 0
        wrong = good.copy()
        wrong[j0:, j0:] -= np.outer(mat[r, j0:], mat[r, j0:])
        assert _rejects(check, wrong, *args), "dropped row"
        # the last two columns swapped
        p = np.arange(n)
        p[[n - 2, n - 1]] = n - 1, n - 2
        assert _rejects(check, good[np.ix_(p, p)], *args), "swapped columns"
        # an element that is not the matrix's read as one: the rows taken n apart instead of lda, or one row too many;
        # a gathered operand's column offsets taken as 0 .. n - 1
        if gc.is_gathered(case):
            row_off, col_off, perm, base_len = gc.gather_tables(m, n, 0)
            base = gc.gathered_base(mat, row_off, col_off, perm, base_len)
            right = base[row_off[:, None] + col_off[None, :]]
            back = np.empty((n, n))
            back[np.ix_(perm, perm)] = right.T @ right
            assert np.array_equal(back, good) or not integer
            assert np.count_nonzero(np.isnan(base)) == base_len - m * n
            seen = base[row_off[:, None] + np.arange(n)[None, :]]
        else:
            flat = gc.poisoned(mat, case["lda"], 3, case["offset"])
            assert np.count_nonzero(np.isnan(flat)) == flat.size - m * n
            rows_seen = m if case["lda"] > n else m + 1
            seen = flat[case["offset"]:][:rows_seen * n].reshape(rows_seen, n)
        assert _rejects(check, seen.T @ seen, *args), "pad element"


@pytest.mark.parametrize("name", list(gc.CASES))
def test_componentwise_bar_sees_what_the_max_norm_bar_did_not(name):
    """1e-9 relative in the entry of the smallest scale: far outside bar(m) |A|^T |A|, far inside 1e-13 max|ref|."""
    case = gc.CASES[name]
    _, ref64, absg = gc.data(name, "graded")[0]
    n = case["n"]
    assert gc.bar(case["m"]) < 2e-10
    wrong = ref64.copy()
    wrong[n - 1, n - 1] *= 1.0 + 1e-9
    assert np.abs(wrong - ref64).max() <= 1e-13 * np.abs(ref64).max()
    assert _rejects(gc.check_graded, wrong, ref64, absg, case["m"])
