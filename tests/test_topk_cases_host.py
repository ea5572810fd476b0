"""tests/topk_cases.py held to its own claims, on the CPU: the exact eigenvectors are eigenvectors, the straddling
family crosses the columns it is meant to cross, LAPACK truncated to k passes every bar with a margin of 10 on every
case, every bar rejects the fault it exists for, every (case, cutoff) pair the GPU suite uses passes the guard, and the
route table is what trd_route plans for the MI355X's resident-slot counts (ndmps_syevd_topk_route_query with h_slots
given makes no GPU call)."""
import numpy as np
import pytest

import eig_routes as er
import topk_cases as tc
from imgcompressionmps_amd import _lib

CASES = tc.all_cases()


def _k_of(case):
    """The rank a case is judged at here: 128 (inside a cluster of the straddling family), or every pair of a smaller one."""
    return min(case.n, 128)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_claims(case):
    assert np.array_equal(case.S, case.S.T) and np.all(np.diff(case.lam) <= 0) and case.lam.size == case.n
    assert np.array_equal(0.5 * (case.G + case.G.T), case.S)
    if case.family == "skew":
        assert not np.array_equal(case.G, case.G.T)
    ref = np.linalg.eigvalsh(case.S)[::-1]
    assert np.abs(ref - case.lam).max() <= tc.E(case.n) * case.scale / 10 + 0.0
    v = tc.vectors_of(case)
    if v is not None:
        n = case.n
        assert np.abs(v.T @ v - np.eye(n)).max() <= 1e-14
        assert np.abs(case.S @ v - v * case.lam[None, :]).max() <= 1e-13 * max(case.scale, 1.0)


@pytest.mark.parametrize("n", [1024, 300])
def test_straddling_family_crosses_the_block_columns(n):
    case = tc.straddle(n)
    ends = [b for _, b, _ in tc.clusters(case.lam)][:5]
    assert tuple(ends) == tc.STRADDLE_ENDS
    sizes = np.diff((0,) + tc.STRADDLE_ENDS)
    assert sizes.min() >= 20 and sizes.max() <= 40
    for col in list(range(16, 129, 16)) + [100, 128]:    # inverse-iteration blocks of 16, ortho blocks of 64, the ranks
        assert case.lam[col - 1] == case.lam[col], col
    assert set(np.unique(case.lam)) == {0.0, 1.0, 2.0, 3.0, 8.0, 9.0, 10.0, 11.0, 12.0}
    assert np.array_equal(case.S * tc.jc.hadamard_m(n), np.round(case.S * tc.jc.hadamard_m(n)))   # multiples of 1 / m


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_lapack_passes_every_bar_with_a_margin_of_ten(case):
    full = tc.jc.lapack(case)
    for k, k_max in {(_k_of(case), _k_of(case)), (max(_k_of(case) // 2, 1), _k_of(case)), (min(case.n, 100), 128)}:
        w, v = tc.lapack_topk(case, k, k_max, full)
        assert not tc.failures(case, w, v, k_max, margin=10.0), (k, k_max)
    if case.n <= 300:      # every eigenpair, the chip-wide route of more than 128 vectors
        w, v = tc.lapack_topk(case, case.n, case.n, full)
        assert not tc.failures(case, w, v, case.n, margin=10.0)


def test_no_bar_exceeds_the_factor_of_its_regime():
    for case in CASES:
        for k in (1, 64, 65, 128, 129, 200):
            f = tc.factor(case, min(k, case.n))
            assert f == (1.0 if case.family in ("laplace", "graded") else 8.0 if 65 <= min(k, case.n) <= 128 else 4.0)
            assert f <= 8.0


# ------------------------------------------------------------------------------------- planted faults
def _fails(case, w, v, k_max, name):
    bad = tc.failures(case, w, v, k_max)
    assert name in bad, f"{case.name}: the fault went unnoticed by '{name}' ({bad})"


@pytest.mark.parametrize("case", [tc.laplace(130), tc.graded(257), tc.hadamard(129, "b"), tc.straddle(300),
                                  tc.deficient(130, 7)], ids=repr)
def test_bars_reject_planted_faults(case):
    k, k_max = 100, 128
    kv = min(k_max, case.n)
    w, v = tc.lapack_topk(case, k, k_max)
    assert not tc.failures(case, w, v, k_max)
    e = tc.factor(case, k) * tc.E(case.n)
    # two swapped columns (of different eigenvalues)
    j = next(i for i in range(1, k) if case.lam[i] != case.lam[0])
    sw = v.copy()
    sw[:, [0, j]] = sw[:, [j, 0]]
    _fails(case, w, sw, k_max, "resid")
    # one vector perturbed by 100 x its bar
    pv = v.copy()
    pv[np.argmax(np.abs(pv[:, 3])), 3] *= 1 + 100 * e / np.abs(pv[:, 3]).max()
    _fails(case, w, pv, k_max, "orth")
    # one eigenvalue off by 100 x its bar
    pw = w.copy()
    pw[3] += 100 * e * case.scale
    _fails(case, pw, v, k_max, "values")
    # a flipped sign
    fs = v.copy()
    fs[:, 5] = -fs[:, 5]
    _fails(case, w, fs, k_max, "sign")
    # two eigenvalues out of order
    j = next(i for i in range(1, kv) if case.lam[i] != case.lam[i - 1])
    ow = w.copy()
    ow[[j - 1, j]] = ow[[j, j - 1]]
    _fails(case, ow, v, k_max, "order")
    # a non-zero behind the leading kv values
    tw = w.copy()
    tw[kv] = 1e-300
    _fails(case, tw, v, k_max, "tail")
    if case.family == "laplace":      # a vector rotated towards its neighbour by 100 x the bar on vectors
        rv = v.copy()
        t = 100 * e * case.scale / tc.gaps(case.lam)[7]
        rv[:, 7] = np.cos(t) * v[:, 7] + np.sin(t) * v[:, 8]
        rv[:, 8] = np.cos(t) * v[:, 8] - np.sin(t) * v[:, 7]
        _fails(case, w, rv, k_max, "vectors")


@pytest.mark.parametrize("case,k", [(tc.straddle(300), 114), (tc.straddle(1024), 74), (tc.hadamard(129, "a"), 32)], ids=repr)
def test_subspace_bar_rejects_a_column_rotated_out_of_the_kept_set(case, k):
    """A column of a cluster that ends at the kept rank, rotated towards an eigenvector of another cluster by 100 x the
    bar (orthonormality is kept by rotating the pair; only the kept one is delivered)."""
    ends = [b for _, b, _ in tc.clusters(case.lam)]
    if k not in ends:
        k = next(b for b in ends if b >= k)
    w, vfull = tc.jc.lapack(case)
    wt = np.zeros(case.n)
    wt[:k] = w[:k]
    assert not tc.failures(case, wt, vfull[:, :k], k)
    a, b, gap = next(c for c in tc.clusters(case.lam) if c[1] == k)
    t = 100 * tc.factor(case, k) * tc.E(case.n) * case.scale / gap
    v = vfull[:, :k].copy()
    v[:, k - 1] = np.cos(t) * vfull[:, k - 1] + np.sin(t) * vfull[:, k]
    v = tc.sign_normalise(v)
    _fails(case, wt, v, k, "subspace")
    # rotated INSIDE its cluster: the same subspace, no fault
    if b - a >= 2:
        v = vfull[:, :k].copy()
        v[:, k - 1] = np.cos(0.3) * vfull[:, k - 1] + np.sin(0.3) * vfull[:, k - 2]
        v[:, k - 2] = np.cos(0.3) * vfull[:, k - 2] - np.sin(0.3) * vfull[:, k - 1]
        assert not tc.failures(case, wt, tc.sign_normalise(v), k)


# ------------------------------------------------------------------------------------- rank model and guard
def _auto_pairs():
    pairs = []
    for case in CASES:
        if case.indefinite or case.scale == 0.0 or case.n == 1:
            continue
        pairs.append((case, tc.auto_cutoff(case)))
    return pairs


@pytest.mark.parametrize("case,cutoff", _auto_pairs(), ids=repr)
def test_every_cutoff_in_use_passes_the_guard(case, cutoff):
    assert 0.0 < cutoff < 1.0
    assert tc.admitted(case, cutoff), tc.guard_distance(case, cutoff)
    for k_cap in (64, 100, 128):
        want = tc.rank_exact(case.lam, cutoff, k_cap)
        assert 1 <= want <= min(k_cap, case.n)
        # LAPACK's rounding does not move the rank
        w, _ = tc.lapack_topk(case, 1, k_cap)
        assert tc.rank_from(w, cutoff, k_cap) == want
    if case.family == "deficient":
        assert tc.rank_exact(case.lam, cutoff, 128) == min(case.rank, 128) and abs(cutoff - 1e-3) < 1e-12
        assert not tc.admitted(case, 1e-6 * 1e-3) or case.rank == case.n   # the floor is not: zeros sit at the threshold


def _batches():
    rows = [(r, m) for r in tc.ROUTES if r["k"] <= tc.MAX_K for m in tc.row_cases(r)]
    return rows + [(r, tc.mixed_cases(r)) for r in tc.MIXED]


@pytest.mark.parametrize("row,members", _batches(), ids=lambda x: tc.route_id(x) if isinstance(x, dict) else "")
def test_every_batch_has_one_cutoff_all_members_admit(row, members):
    assert [c.n for c in members] == list(row["orders"])
    cutoff = tc.common_cutoff(members)
    assert 0.0 < cutoff < 1.0 and all(tc.admitted(c, cutoff) and not c.indefinite for c in members)
    ranks = [tc.rank_exact(c.lam, cutoff, row["k"]) for c in members]
    assert all(1 <= r <= min(row["k"], c.n) for r, c in zip(ranks, members))


def test_rank_model_edges_and_faults():
    lam = np.array([9.0, 4.0, 1.0, 0.0, -1.0])
    assert tc.rank_exact(lam, 0.0, 128) == 3                 # sqrt(max(., 0)) > 0: the positive ones
    assert tc.rank_exact(lam, 0.5, 128) == 2                 # strict: 2 > 1.5, 1 > 1.5 is false
    assert tc.rank_exact(lam, 1.0, 128) == 1 and tc.rank_exact(lam, 7.0, 128) == 1
    assert tc.rank_exact(lam, 0.0, 2) == 2
    assert tc.rank_exact(np.zeros(4), 0.0, 128) == 1 and tc.rank_exact(np.zeros(4), 0.3, 2) == 1
    assert tc.rank_exact(np.array([-1.0, -2.0]), 0.0, 5) == 1      # nothing positive: one pair all the same
    case = tc.straddle(300)
    cutoff = tc.auto_cutoff(case)
    want = tc.rank_exact(case.lam, cutoff, 128)
    w, _ = tc.lapack_topk(case, 1, 128)
    assert tc.rank_from(w, cutoff, 128) == want
    assert not tc.admitted(case, float(np.sqrt(9.0 / 12.0)))          # on an eigenvalue
    assert not tc.admitted(case, float(np.sqrt((9.0 + 1e-10) / 12.0)))  # within 100 E scale of one
    assert tc.admitted(case, float(np.sqrt(9.5 / 12.0)))
    assert np.array_equal(tc.spectra_from(np.array([4.0, 1.0, -1e-18, 0.0]), 3), np.array([2.0, 1.0, 0.0]))


def _auto_result(case, k_cap, rank):
    """What the auto entry leaves for ``case`` if it keeps ``rank``, made of LAPACK's pairs: (w, the n x n block of V
    in a sentinel, the stride of spectra in a sentinel)."""
    n, kk = case.n, min(k_cap, case.n)
    w, v = tc.lapack_topk(case, rank, k_cap)
    block = np.full((n, n), tc.SENTINEL)
    block[:, :rank] = v
    block[:, rank:kk] = 0.0
    spectra = np.full(k_cap + 5, tc.SENTINEL)
    spectra[:kk] = np.sqrt(np.maximum(w[:kk], 0.0))
    return w, block, spectra


@pytest.mark.parametrize("case,k_cap", [(tc.hadamard(129, "a"), 128), (tc.straddle(300), 128), (tc.laplace(40), 64),
                                        (tc.deficient(130, 7), 128)], ids=repr)
def test_auto_contract_check_rejects_planted_faults(case, k_cap):
    """topk_cases.auto_failures is what the GPU driver holds every member of an auto call to.  A faithful result
    passes; a rank off by one (with V filled to match), a denormal in a fill column, a write behind min(k_cap, n), a
    spectrum one ulp off, a spectrum written behind min(k_cap, n) and a kept column never written are each reported,
    and nothing else with them."""
    cutoff = tc.auto_cutoff(case)
    assert tc.admitted(case, cutoff)
    n, kk = case.n, min(k_cap, case.n)
    k = tc.rank_exact(case.lam, cutoff, k_cap)
    assert 1 < k < kk - 1

    def check(w, block, rank, spectra):
        return tc.auto_failures(w, block, rank, spectra, cutoff, k_cap, exact=k)

    w, block, spectra = _auto_result(case, k_cap, k)
    assert check(w, block, k, spectra) == [] and check(w, block, k, None) == []
    for off in (-1, 1):                                 # a rank off by one, everything else consistent with it
        assert check(*_auto_result(case, k_cap, k + off)[:2], k + off, spectra) == ["rank", "rank_exact"]
        assert tc.auto_failures(*_auto_result(case, k_cap, k + off)[:2], k + off, spectra, cutoff, k_cap) == ["rank"]
    for rank in (0, kk + 1):
        assert "range" in check(w, block, rank, spectra)
    for col in (k, kk - 1):                             # a non-zero in a fill column, however small
        bad = block.copy()
        bad[n // 2, col] = 5e-324
        assert check(w, bad, k, spectra) == ["fill"]
    if kk < n:                                          # a write behind min(k_cap, n), even of a zero
        for col in (kk, n - 1):
            bad = block.copy()
            bad[0, col] = 0.0
            assert check(w, bad, k, spectra) == ["extent"]
    bad = block.copy()                                  # a kept column that was never written
    bad[:, k - 1] = tc.SENTINEL
    assert check(w, bad, k, spectra) == ["kept"]
    for j in (0, k, kk - 1):                            # a spectrum one ulp off
        bad = spectra.copy()
        bad[j] = np.nextafter(bad[j], np.inf)
        assert check(w, block, k, bad) == ["spectra"]
    for j in (kk, k_cap + 4):                           # a spectrum written behind min(k_cap, n)
        bad = spectra.copy()
        bad[j] = 0.0
        assert check(w, block, k, bad) == ["spectra_extent"]


# ------------------------------------------------------------------------------------- routes
@pytest.fixture
def lib(monkeypatch):
    for name in tc.SWITCHES + ("NDMPS_INVIT_DBG",):
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def test_route_numbers_are_those_of_eig_routes():
    assert (tc.WIDE_AUTO, tc.WIDE, tc.SMALL, tc.BLOCKS, tc.COLUMNS) == (er.ORTHO_WIDE_AUTO, er.ORTHO_WIDE, er.ORTHO_SMALL,
                                                                        er.ORTHO_BLOCKS, er.ORTHO_COLUMNS)
    assert (tc.LANES, tc.ROWS, tc.BACK_WIDE) == (er.BACK_LANES, er.BACK_ROWS, er.BACK_WIDE)


@pytest.mark.parametrize("row", tc.ROUTES + tc.MIXED, ids=tc.route_id)
def test_route_table_is_what_the_solver_plans(lib, monkeypatch, row):
    for item in row["env"].split():
        monkeypatch.setenv(*item.split("="))
    r = er.route(lib, row["orders"], row["k"], 1, 0, er.MI355X_TEAM_SLOTS)
    assert {f: r[f] for f in tc.route_fields(row)} == tc.route_fields(row)
    assert r["invit_dbg"] == 0


def test_route_table_reaches_every_phase_two_regime():
    rows = tc.ROUTES
    assert {r["ortho"] for r in rows} == set(range(5))
    assert {r["back"] for r in rows} == set(range(3))
    assert {r["lane_class"] for r in rows if r["back"] == tc.LANES} == set(range(6))
    assert {r["invit_cb"] for r in rows} == {16, 128}
    assert {r["t_factors"] for r in rows} == {0, 1, 2}
    by = {(r["orders"], r["k"], r["env"]): r for r in rows}
    # either side of every switch of the lane-dealt kernel that the table can reach with one to three matrices
    assert by[((128,), 64, "")]["lane_class"] == 0 and by[((129,), 64, "")]["lane_class"] == 1
    assert by[((256,), 64, "")]["lane_class"] == 1 and by[((257,), 64, "")]["lane_class"] == 2
    assert by[((512,), 64, "")]["lane_class"] == 2 and by[((513,) * 3, 64, "")]["lane_class"] == 3
    assert by[((1024,) * 3, 128, "")]["lane_class"] == 3 and by[((1025,), 128, tc.NARROW)]["lane_class"] == 4
    assert by[((2049,), 128, tc.NARROW)]["lane_class"] == 5
    assert max(max(r["orders"]) for r in rows) == 2049
    # mixed batches: orders below the cap in each, and one on the chip-wide route
    assert all(min(r["orders"]) < r["k"] for r in tc.MIXED)
    assert any(r["back"] == tc.ROWS for r in tc.MIXED)
