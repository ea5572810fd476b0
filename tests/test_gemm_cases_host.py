"""tests/gemm_cases.py on the CPU: every case takes the tile, the staging and the fetch paths it was chosen for
(through ndmps_gemm_plan_query, no GPU call), the table reaches every variant the kernels have, the integer data is
exact in the accumulator in any order of summation, and the two assertions of tests/test_gpu_gemm_cases.py reject, on
exactly these cases, the errors a product kernel can make without a norm bound noticing."""
import ctypes

import numpy as np
import pytest

import gemm_cases as gm
from imgcompressionmps_amd import _lib

SENTINEL = -7.0


@pytest.fixture
def lib():
    return _lib.load()


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _want(case, facts):
    return {k: facts.get(k) for k in case["facts"]}


# ----------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", list(gm.CASES))
def test_case_takes_the_tile_and_the_fetch_it_exists_for(lib, name):
    case = gm.CASES[name]
    plan = gm.plan_of(lib, case)
    assert _want(case, gm.facts_of(case, plan)) == case["facts"]
    if case["elem"] != "bf16":
        va, vb = gm.TILES[case["elem"]][plan["bm"], plan["bn"]]
        assert (plan["va"], plan["vb"]) == (plan["vec"] * va, plan["vec"] * vb)
        assert (plan["grid_x"], plan["grid_y"]) == (-(-case["m"] // plan["bm"]), -(-case["n"] // plan["bn"]))
        assert plan["vec_in"] == plan["vec_out"] == plan["transposes"] == 0 and plan["launches"] == 1
    # a base pointer that is off, or a stride that is not tight, changes how the operands are fetched and nothing else
    if case["same_as"]:
        base = gm.plan_of(lib, gm.CASES[case["same_as"]])
        for slot in ("bm", "bn", "grid_x", "grid_y", "transposes", "launches"):
            assert plan[slot] == base[slot]
    if case["guarded"]:
        under = gm.plan_of(lib, case, guarded=True)
        assert under == dict(plan, inner_a=0, inner_b=0)
        f = gm.facts_of(case, under)
        assert "inner" not in f["paths_a"] | f["paths_b"]
        assert ("guarded" in f["paths_a"]) == bool(plan["va"]) and ("guarded" in f["paths_b"]) == bool(plan["vb"])


def test_the_table_covers_what_it_claims(lib):
    """Every (elem, tile, ta, tb) with every (va, vb) the tile has, each operand on the straight-line, the guarded and
    the element-wise fetch wherever the tile stages it in quads at all; both values of vec_in, vec_out and
    transposes, a k that is no whole chunk with and without 16-byte loads, and a second launch for bf16; the vector
    shape of every tile also under the switch."""
    seen = set()
    for name, case in gm.CASES.items():
        plan = gm.plan_of(lib, case)
        f = gm.facts_of(case, plan)
        if case["elem"] == "bf16":
            seen.add(("bf16", "vec_in", f["vec_in"], "vec_out", f["vec_out"]))
            seen.add(("bf16", "transposes", f["transposes"], "vec_in", f["vec_in"]))
            seen.add(("bf16", "launches", f["launches"]))
            seen.add(("bf16", "tail", case["k"] % 8 != 0, "vec_in", f["vec_in"]))
            seen.add(("bf16", "ktiles", -(-case["k"] // 64)))
            continue
        key = (case["elem"], plan["bm"], plan["bn"], case["ta"], case["tb"])
        seen.add(key + (plan["va"], plan["vb"]))
        for p in f["paths_a"]:
            seen.add(key + ("a", p))
        for p in f["paths_b"]:
            seen.add(key + ("b", p))
        if case["guarded"] and plan["vec"]:
            seen.add(key + ("switch",))
        if case["entry"] == "batched":
            seen.add((case["elem"], "batched", case["batch"], plan["vec"]))
    for elem, tiles in gm.TILES.items():
        for (bm, bn), (va, vb) in tiles.items():
            for ta in (0, 1):
                for tb in (0, 1):
                    key = (elem, bm, bn, ta, tb)
                    assert key + (va, vb) in seen and key + (0, 0) in seen and key + ("switch",) in seen
                    for x, v in (("a", va), ("b", vb)):
                        assert key + (x, "scalar") in seen
                        if v:
                            assert key + (x, "inner") in seen and key + (x, "guarded") in seen
        for batch in (1, 3, 64):
            assert (elem, "batched", batch, 1) in seen
        assert (elem, "batched", 3, 0) in seen
    for vi in (0, 1):
        for vo in (0, 1):
            assert ("bf16", "vec_in", vi, "vec_out", vo) in seen
        for t in (0, 1):
            assert ("bf16", "transposes", t, "vec_in", vi) in seen
        assert ("bf16", "tail", True, "vec_in", vi) in seen
    assert ("bf16", "launches", 1) in seen and ("bf16", "launches", 2) in seen
    assert {("bf16", "ktiles", t) for t in (1, 2, 3)} <= seen


def _query(lib, elem, ta, tb, m, n, k, lda, ldb, ldc, mis=(0, 0, 0), guarded=0, out=True):
    buf = (ctypes.c_int64 * len(gm.PLAN_SLOTS))()
    rc = lib.ndmps_gemm_plan_query(gm.ELEMS[elem] if isinstance(elem, str) else elem, ta, tb, m, n, k, lda, ldb, ldc, *mis,
                                   guarded, buf if out else None)
    return rc, dict(zip(gm.PLAN_SLOTS, list(buf)))


def test_the_query_refuses_what_the_entries_refuse(lib):
    ok = ("f32", 0, 0, 8, 12, 16, 16, 12, 12)
    assert _query(lib, *ok)[0] == _lib.OK
    assert _query(lib, 3, *ok[1:])[0] == _lib.EINVAL and _query(lib, -1, *ok[1:])[0] == _lib.EINVAL
    assert _query(lib, *ok, out=False)[0] == _lib.EINVAL
    assert _query(lib, *ok, mis=(-1, 0, 0))[0] == _lib.EINVAL
    for elem in ("f32", "f64"):
        for ta in (0, 1):
            for tb in (0, 1):
                m, n, k = 8, 12, 16
                lda, ldb, ldc = (m if ta else k), (k if tb else n), n
                assert _query(lib, elem, ta, tb, m, n, k, lda, ldb, ldc)[0] == _lib.OK
                # a leading dimension one below the row length, for each operand
                assert _query(lib, elem, ta, tb, m, n, k, lda - 1, ldb, ldc)[0] == _lib.EINVAL
                assert _query(lib, elem, ta, tb, m, n, k, lda, ldb - 1, ldc)[0] == _lib.EINVAL
                assert _query(lib, elem, ta, tb, m, n, k, lda, ldb, ldc - 1)[0] == _lib.EINVAL
                for bad in ((-1, n, k), (m, -1, k), (m, n, -1)):
                    assert _query(lib, elem, ta, tb, *bad, 64, 64, 64)[0] == _lib.EINVAL
        # an empty product is accepted and launches nothing; k = 0 launches (C = 0)
        for shape in ((0, 12, 16), (8, 0, 16)):
            rc, plan = _query(lib, elem, 0, 0, *shape, 16, 12, 12)
            assert rc == _lib.OK and plan["launches"] == plan["grid_x"] == plan["grid_y"] == 0
        rc, plan = _query(lib, elem, 0, 0, 8, 12, 0, 4, 12, 12)
        assert rc == _lib.OK and plan["launches"] == 1
    for tb in (0, 1):
        m, n, k = 8, 16, 24
        ldb = k if tb else n
        assert _query(lib, "bf16", 0, tb, m, n, k, k, ldb, n)[0] == _lib.OK
        assert _query(lib, "bf16", 1, tb, m, n, k, k, ldb, n)[0] == _lib.EINVAL       # no transposed left operand
        assert _query(lib, "bf16", 0, tb, m, n, k, k - 1, ldb, n)[0] == _lib.EINVAL
        assert _query(lib, "bf16", 0, tb, m, n, k, k, ldb - 1, n)[0] == _lib.EINVAL
        assert _query(lib, "bf16", 0, tb, m, n, k, k, ldb, n - 1)[0] == _lib.EINVAL
        for bad in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
            assert _query(lib, "bf16", 0, tb, *bad, 64, 64, 64)[0] == _lib.EINVAL


def test_what_the_switch_and_the_alignment_change(lib):
    """NDMPS_GEMM_GUARDED takes the straight-line fetch away and nothing else; 16 bytes (fp64: 32) decide vec."""
    shape = (0, 0, 260, 132, 36, 36, 132, 132)
    for elem, al in (("f32", 16), ("f64", 32)):
        _, plain = _query(lib, elem, *shape)
        _, under = _query(lib, elem, *shape, guarded=1)
        assert plain["vec"] == plain["va"] == plain["vb"] == 1 and plain["inner_a"] > 0 and plain["inner_b"] > 0
        assert under == dict(plain, inner_a=0, inner_b=0)
        for mis in range(0, 64, 4):
            for which in range(2):
                _, p = _query(lib, elem, *shape, mis=tuple(mis if w == which else 0 for w in range(3)))
                assert p["vec"] == int(mis % al == 0)
            assert _query(lib, elem, *shape, mis=(0, 0, mis))[1] == plain   # C is stored element by element
    for mis in range(0, 64, 2):
        _, p = _query(lib, "bf16", 0, 1, 300, 8, 64, 64, 64, 8, mis=(mis, 0, 0))
        assert (p["vec_in"], p["vec_out"]) == (int(mis % 16 == 0), 1)
        _, p = _query(lib, "bf16", 0, 1, 300, 8, 64, 64, 64, 8, mis=(0, 0, mis))
        assert (p["vec_in"], p["vec_out"]) == (1, int(mis % 16 == 0))


# ----------------------------------------------------------------------------- the data and the assertions
def _buffers(case, a, b):
    """The operands as the entry sees them: flat poisoned buffers (tests/test_gpu_gemm_cases.py builds the same)."""
    lda, ldb, _ = gm.lds(case)
    return (gm.poisoned(gm.stored(a, case["ta"]), lda, 3, case["off_a"]),
            gm.poisoned(gm.stored(b, case["tb"]), ldb, 3, case["off_b"]))


def _read(flat, off, ld, trans, rows, cols):
    """op(X) (rows, cols) as a kernel reads it: element (r, c) at off + r ld + c, or off + c ld + r under the flag;
    what lies behind the buffer reads as NaN."""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    idx = off + (c * ld + r if trans else r * ld + c)
    return np.where(idx < flat.size, flat[np.minimum(idx, flat.size - 1)], np.nan)


def _bf16_truncated(x):
    bits = np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64)


def _stand_ins(case, a, b):
    """{mutation: the C (fp64, before it is stored) of a kernel that is wrong in that way}."""
    m, n, k, ta, tb = case["m"], case["n"], case["k"], case["ta"], case["tb"]
    lda, ldb, _ = gm.lds(case)
    fa, fb = _buffers(case, a, b)
    oa, ob = case["off_a"], case["off_b"]
    assert np.array_equal(_read(fa, oa, lda, ta, m, k), a) and np.array_equal(_read(fb, ob, ldb, tb, k, n), b)
    assert np.count_nonzero(np.isnan(fa)) == fa.size - m * k and np.count_nonzero(np.isnan(fb)) == fb.size - k * n
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        # one element behind the k range read as data: a pad column, the neighbouring row or a trailing row
        out["pad element"] = _read(fa, oa, lda, ta, m, k + 1) @ _read(fb, ob, ldb, tb, k + 1, n)
        if k == 0:
            out["C not written"] = np.full((m, n), SENTINEL)
            return out
        out["dropped k term"] = a[:, :k - 1] @ b[:k - 1]
        chunk = 8 if case["elem"] == "bf16" else 16
        kk = (k - 1) // chunk * chunk
        out["last partial k-tile dropped"] = a[:, :kk] @ b[:kk]
        # a vector with unit stride reads the same under either flag: there the flag cannot be wrong
        a_flip, b_flip = _read(fa, oa, lda, 1 - ta, m, k), _read(fb, ob, ldb, 1 - tb, k, n)
        a_same, b_same = np.array_equal(a_flip, a), np.array_equal(b_flip, b)
        assert (not a_same or lda == 1) and (not b_same or ldb == 1)
        if not a_same:
            out["op(A) flag flipped"] = a_flip @ b
        if ta != tb and not (a_same and b_same):
            out["flags swapped"] = a_flip @ b_flip
        elif not b_same:
            out["op(B) flag flipped"] = a @ b_flip
        h = (k + 1) // 2
        out["fp16 partial sum"] = (a[:, :h] @ b[:h]).astype(np.float16).astype(np.float64) + a[:, h:] @ b[h:]
    return out


def _store(c, elem):
    with np.errstate(invalid="ignore", over="ignore"):
        return gm.cc.to_storage(c, elem)


# mutations the graded bar of bf16 (2**-8 of |A||B|: one rounding of the result) cannot see by construction: they
# are the integer assertion's to catch
_INTEGER_ONLY = {"bf16": ("fp16 partial sum", "truncated to bf16")}


@pytest.mark.parametrize("name", gm.small_cases())
def test_integer_data_is_exact_and_the_assertions_have_teeth(name):
    case = gm.CASES[name]
    elem, k = case["elem"], case["k"]
    imax = gm.imax_of(case)
    if elem == "f64":
        assert imax == 2 ** 19 and k <= 2 ** 13
    else:
        assert k * imax * imax < 2 ** 24 and imax <= (255 if elem == "bf16" else 2047)
    a, b, exact = gm.data(name, "integer")[0]
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) <= imax
    assert np.array_equal(gm.cc.to_storage(a, elem), a) and np.array_equal(gm.cc.to_storage(b, elem), b)
    # any order of summation: k-tile by k-tile in the accumulator's type gives the same integers
    acc_t = np.float64 if elem == "f64" else np.float32
    acc = np.zeros((case["m"], case["n"]), dtype=acc_t)
    for k0 in range(0, k, gm.BK[elem]):
        acc = acc + (a[:, k0:k0 + gm.BK[elem]].astype(acc_t) @ b[k0:k0 + gm.BK[elem]].astype(acc_t))
    gm.check_integer(_store(acc.astype(np.float64), elem), exact)
    if case["m"] == case["n"] and k > 0:
        assert not np.array_equal(exact, exact.T)   # a transposed accumulator map shows

    ag, bg, ref, bound = gm.data(name, "graded")[0]
    good = _store(ag @ bg, elem)
    gm.check_graded(good, ref, bound)
    for kind, (x, y), check, args in (("integer", (a, b), gm.check_integer, (exact,)),
                                      ("graded", (ag, bg), gm.check_graded, (ref, bound))):
        wrong = _stand_ins(case, x, y)
        if elem == "bf16":
            wrong["truncated to bf16"] = None
        for what, c in wrong.items():
            c = _bf16_truncated(x @ y) if c is None else _store(c, elem)
            if kind == "graded" and what in _INTEGER_ONLY.get(elem, ()):
                continue
            assert _rejects(check, c, *args), f"{what} passes the {kind} assertion"


def test_no_graded_bar_is_vacuous():
    """bar / |ref| is below 1 somewhere in every case (an entry the bar would let be anything tests nothing); the
    largest of these per-case minima is asserted here and stated in DESIGN.md."""
    worst = {}
    for name in gm.small_cases():
        case = gm.CASES[name]
        if case["k"] == 0:
            continue   # the bar is 0: equality
        _, _, ref, bound = gm.data(name, "graded")[0]
        with np.errstate(divide="ignore"):
            least = float((bound / np.abs(ref).astype(np.float64)).min())
        worst[case["elem"]] = max(worst.get(case["elem"], 0.0), least)
    print({e: f"{v:.3g}" for e, v in worst.items()})
    assert worst["f32"] < 1e-5 and worst["f64"] < 1e-13 and worst["bf16"] < 0.05


@pytest.mark.parametrize("name", [n for n in gm.small_cases() if gm.CASES[n]["elem"] == "f32" and
                                  min(gm.CASES[n]["m"], gm.CASES[n]["n"], gm.CASES[n]["k"]) >= 16])
def test_componentwise_bar_sees_what_the_norm_bar_did_not(name):
    """100 bars of error in the entry with the smallest bar: rejected, and a thousand times inside the norm bound
    ``4e-7 * max row sum of |A| * max|B| * sqrt(k)`` that the products were held to before."""
    case = gm.CASES[name]
    a, b, ref, bound = gm.data(name, "graded")[0]
    i = np.unravel_index(np.argmin(bound), bound.shape)
    wrong = ref.copy()
    wrong[i] += 100.0 * bound[i]
    assert _rejects(gm.check_graded, wrong, ref, bound)
    assert np.abs(wrong - ref).max() <= 1e-3 * 4e-7 * np.abs(a).sum(axis=1).max() * np.abs(b).max() * np.sqrt(case["k"])


# ----------------------------------------------------------------------------- the fold
def test_the_fold_case_and_its_checks():
    case = gm.CASES[gm.FOLD]
    assert case["k"] * gm.imax_of(case) ** 2 < 256          # exact in bf16's 8 bits: no rounding at all
    assert case["m"] * 8 * (2 + 2 + 1) < 0.5e9   # on the device: A and C as bf16, A's int8 staging copy
    rows = gm.fold_checked_rows()
    assert rows[-1] == case["m"] - 1 and gm.FOLD_ROWS - 1 in rows and gm.FOLD_ROWS in rows
    a, b = gm.fold_rows(rows), gm.fold_b()
    assert np.abs(a).max() == 5 and np.abs(b).max() == 5 and a.min() == -5
    right = a.astype(np.int64) @ b.astype(np.int64).T
    # a second launch that starts one tile early, or that never runs, shows in the compared rows
    early = gm.fold_rows(rows - 128 * (rows >= gm.FOLD_ROWS)).astype(np.int64) @ b.astype(np.int64).T
    assert not np.array_equal(early[-1], right[-1]) and early[-1].sum() != right[-1].sum()
    assert np.count_nonzero(right[-1]) > 0
    # rows are distinct enough that a shifted block cannot pass: no two compared rows agree
    assert len({tuple(r) for r in a}) > len(rows) // 2
