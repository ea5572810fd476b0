"""tests/trd_cases.py on the host (no GPU): the model of the tridiagonalisation and LAPACK's dsytrd pass every bar on every
case of the route table with a margin of 10; every planted fault is reported by exactly the items that exist for it and
nothing is reported without one; the table of phase-1 routes is what trd_route plans with the MI355X's slot counts and
reaches every kind, every resident kernel and both tails; ndmps_syevd_topk_reduction_offsets is the layout's."""
import ctypes as C

import numpy as np
import pytest

import eig_routes as er
import trd_cases as td
from imgcompressionmps_amd import _lib

S = er.MI355X_TEAM_SLOTS
CASES = td.all_cases()


@pytest.fixture
def lib(monkeypatch):
    for name in td.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def _setenv(monkeypatch, env):
    for item in env.split():
        monkeypatch.setenv(*item.split("="))


# ------------------------------------------------------------------------------------- the cases
def test_the_cases_are_what_they_claim():
    names = {c.family for c in CASES}
    assert {"laplace", "graded", "hadamard", "straddle", "deficient", "skew", "diag", "blocks", "arrow", "rank1",
            "tridiag"} <= names
    assert {c.name for c in CASES} >= {"diag-zero-128", "identity-128", "hadamard-b-257", "hadamard-r1-257"}
    assert td.SLOTS == S[0] == S[1]
    for c in CASES:
        assert np.array_equal(c.S, c.S.T) and c.lam.shape == (c.n,) and np.all(np.diff(c.lam) <= 0)
        assert td.is_tridiagonal(c) or c.family not in td.TRIDIAGONAL, c.name
        assert not td.is_tridiagonal(c) or c.family in td.TRIDIAGONAL or c.n <= 3, c.name
    b = td.blocks(257)
    assert np.all(np.diag(b.S, -1)[td.block_boundaries(257)] == 0.0) and np.count_nonzero(np.diag(b.S, -1) == 0.0) == 6
    assert np.array_equal(b.S[:37, :37], b.S[37:74, 37:74]) and not b.S[:37, 37:].any() and 257 % 37
    a = td.arrow(130)
    assert np.all(a.S[0, 1:] != 0) and not np.triu(a.S[1:, 1:], 1).any()
    r = td.rank1(130)
    assert np.linalg.matrix_rank(r.S) == 1 and r.lam[0] == np.trace(r.S)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_and_lapack_pass_every_bar_with_a_margin_of_ten(case):
    n = case.n
    for name, reduce in (("model", td.reference_reduction), ("dsytrd", td.lapack_reduction)):
        vh, tau, d, e = reduce(case.S)
        r = td.reduction_ratios(case.S, vh, tau, d, e, n, n, lam=case.lam)
        assert td.failures_of(r, margin=10.0) == [], (name, r)
        assert np.isfinite(r["tau_defect"])       # reported (tests/test_gpu_trd_exact.py), never asserted
        mu = td.eig_tridiagonal(d, e, n)
        w = np.concatenate([mu[:min(n, 128)], np.zeros(n - min(n, 128))])
        assert td.values_failures(w, d, e, n, min(n, 128), case.scale, margin=10.0) == []
        if td.is_tridiagonal(case):
            assert td.exact_failures(case.S, tau, d, e, n) == [], name
        if case.family == "blocks" and name == "model":
            assert np.all(e[td.block_boundaries(n)] == 0.0) and np.all(tau[td.block_boundaries(n)] == 0.0)
    # the two-stage kinds are held to the spectrum alone: the same T under that reading
    assert td.reduction_failures(case.S, vh, tau, d, e, n, n, lam=case.lam, two_stage=True, margin=10.0) == []


# ------------------------------------------------------------------------------------- planted faults
N, LDA, J = 131, 132, 3


def _base(**fault):
    """The model's reduction of graded-131 in the device's layout: lda = 132, rows of lda doubles."""
    case = td.jc.graded(N)
    vh, tau, d, e = td.reference_reduction(case.S, **fault)
    wide = np.zeros((N, LDA))
    wide[:, :N] = vh
    return case, wide, tau, d, e


def _report(case, vh, tau, d, e):
    return set(td.reduction_failures(case.S, vh, tau, d, e, N, LDA, lam=case.lam))


def _poke(array, index, value=None, add=None):
    def plant(vh, tau, d, e):
        target = dict(vh=vh, tau=tau, d=d, e=e)[array]
        target[index] = value if add is None else target[index] + add
    return plant


def _swap_d(vh, tau, d, e):
    d[J], d[J + 1] = d[J + 1], d[J]


def _flip_e(vh, tau, d, e):
    e[J] = -e[J]


def _stale_last_row(vh, tau, d, e):
    vh[N - 1, :] = vh[N - 3, :]


STORED = {   # fault in what is stored -> the items that report it
    "tau off by 1e-9": (_poke("tau", J, add=1e-9), {"orth", "similar"}),
    "reflector entry off by 1e-9": (_poke("vh", (J, J + 9), add=1e-9), {"orth", "similar"}),
    "non-zero at an index <= j": (_poke("vh", (J, J), 1e-300), {"shape"}),
    "non-zero at index 0 of a late row": (_poke("vh", (100, 0), 1e-300), {"shape"}),
    "1 + 2^-52 for the 1.0": (_poke("vh", (J, J + 1), 1.0 + 2.0 ** -52), {"shape"}),
    "stale row n-1": (_stale_last_row, {"shape"}),
    "non-zero in n .. lda-1": (_poke("vh", (J, N), 1e-300), {"shape"}),
    "e_j with the wrong sign": (_flip_e, {"similar"}),
    "d_j and d_j+1 exchanged": (_swap_d, {"similar", "spectrum"}),
    "e[n-1] != 0": (_poke("e", N - 1, 1e-300), {"shape"}),
    "tau[n-1] != 0": (_poke("tau", N - 1, 1.5), {"shape"}),
    "tau below 1": (_poke("tau", N - 2, 2.0 ** -60), {"shape"}),
    "NaN in d": (_poke("d", 7, np.nan), {"shape", "orth", "similar", "spectrum"}),
}
COMPUTED = {   # fault in the reduction itself: the reflectors stay reflectors, T is no longer similar to A
    "a rank-2 update without its w v^T term": (dict(drop_wv_at=5), {"similar", "spectrum"}),
    "an update with the previous column's y": (dict(stale_y_at=5), {"similar", "spectrum"}),
}


def test_nothing_is_reported_without_a_fault():
    assert _report(*_base()) == set()


@pytest.mark.parametrize("name", STORED)
def test_a_fault_in_what_is_stored_is_reported_by_its_items(name):
    plant, want = STORED[name]
    case, vh, tau, d, e = _base()
    plant(vh, tau, d, e)
    assert _report(case, vh, tau, d, e) == want


@pytest.mark.parametrize("name", COMPUTED)
def test_a_fault_in_the_reduction_is_reported_by_its_items(name):
    fault, want = COMPUTED[name]
    assert _report(*_base(**fault)) == want


def test_an_idle_row_may_be_zero_or_a_unit_vector_and_nothing_else():
    case = td.blocks(N)
    vh, tau, d, e = td.reference_reduction(case.S)
    assert tau[5] != 0 and tau[36] == 0 and vh[36, 37] == 1.0
    assert td.reduction_failures(case.S, vh, tau, d, e, N, N, lam=case.lam) == []
    vh[36, :] = 0.0                       # H = I either way
    assert td.reduction_failures(case.S, vh, tau, d, e, N, N, lam=case.lam) == []
    vh[36, 40] = 1e-300
    assert td.reduction_failures(case.S, vh, tau, d, e, N, N, lam=case.lam) == ["shape"]
    vh[36, 40], vh[36, 37] = 0.0, 0.5
    assert td.reduction_failures(case.S, vh, tau, d, e, N, N, lam=case.lam) == ["shape"]


def test_the_two_stage_reading_looks_at_the_spectrum_and_the_last_entry_only():
    case, vh, tau, d, e = _base()
    vh[:] = 7.0
    tau[:] = 0.25
    assert td.reduction_failures(case.S, vh, tau, d, e, N, LDA, lam=case.lam, two_stage=True) == []
    _swap_d(vh, tau, d, e)
    assert td.reduction_failures(case.S, vh, tau, d, e, N, LDA, lam=case.lam, two_stage=True) == ["spectrum"]
    _swap_d(vh, tau, d, e)
    e[N - 1] = 1e-300
    assert td.reduction_failures(case.S, vh, tau, d, e, N, LDA, lam=case.lam, two_stage=True) == ["shape"]


def test_values_failures_reports_bisection_alone():
    case, vh, tau, d, e = _base()
    kv = 128
    mu = td.eig_tridiagonal(d, e, N)
    w = np.concatenate([mu[:kv], np.zeros(N - kv)])
    assert td.values_failures(w, d, e, N, kv) == []
    # a T that is not similar to A changes nothing: the comparison is with the eigenvalues of the T at hand
    d2 = d.copy()
    d2[J], d2[J + 1] = d2[J + 1], d2[J]
    mu2 = td.eig_tridiagonal(d2, e, N)
    assert td.values_failures(np.concatenate([mu2[:kv], np.zeros(N - kv)]), d2, e, N, kv) == []
    bad = w.copy()
    bad[40] += 1e-9 * case.scale
    assert td.values_failures(bad, d, e, N, kv) == ["values"]
    bad = w.copy()
    bad[[10, 11]] = bad[[11, 10]]
    assert set(td.values_failures(bad, d, e, N, kv)) == {"values", "order"}
    bad = w.copy()
    bad[kv] = 1e-300
    assert td.values_failures(bad, d, e, N, kv) == ["tail"]


def test_exact_failures_reports_each_of_its_items():
    case = td.tridiag(N)
    vh, tau, d, e = td.reference_reduction(case.S)
    assert td.exact_failures(case.S, tau, d, e, N) == []
    for array, name in ((d, "d"), (e, "e"), (tau, "tau")):
        keep = array[J]
        array[J] = np.nextafter(keep, 4.0)
        assert td.exact_failures(case.S, tau, d, e, N) == [name]
        array[J] = keep


# ------------------------------------------------------------------------------------- the route table
@pytest.mark.parametrize("row", td.ROUTES, ids=td.route_id)
def test_route_table_is_what_the_solver_plans(lib, monkeypatch, row):
    _setenv(monkeypatch, row["env"])
    orders, k = list(row["orders"]), td.k_max_of(row)
    if row["recover"]:
        first = er.route(lib, orders, k, 1, row["streamed"], S)
        assert first["kernel"] != er.K_NONE, "no resident launch to abort"
        r = er.route(lib, orders, k, 0, row["streamed"], S)
    else:
        r = er.route(lib, orders, k, row["team"], row["streamed"], S)
    assert {f: r[f] for f in row["want"]} == row["want"], td.route_id(row)


def test_route_table_reaches_every_kind_kernel_and_tail():
    assert (td.COLUMNS, td.BAND2, td.BAND4, td.TEAM, td.BIG_TEAM, td.PANEL, td.PANEL_HYBRID) == \
        (er.COLUMNS, er.BAND2, er.BAND4, er.TEAM, er.BIG_TEAM, er.PANEL, er.PANEL_HYBRID)
    assert (td.K_NONE, td.K_TAGGED2, td.K_MEET2, td.K_SYM, td.K_TAGGED4, td.K_TAGGED8, td.K_BAND2, td.K_BAND4) == \
        (er.K_NONE, er.K_TAGGED2, er.K_MEET2, er.K_SYM, er.K_TAGGED4, er.K_TAGGED8, er.K_BAND2, er.K_BAND4)
    assert (td.TAIL_NONE, td.TAIL_REGS, td.TAIL_LDS) == (er.TAIL_NONE, er.TAIL_REGS, er.TAIL_LDS)
    rows = [r for r in td.ROUTES if not r["recover"]]
    assert {r["want"]["reduce"] for r in rows} == set(range(7))
    assert {r["want"]["kernel"] for r in rows} == set(range(8))
    assert {r["want"]["tail"] for r in rows} == set(range(3))
    assert {r["want"]["handover"] for r in rows} == {0, 512, 1024}
    assert {(r["want"]["col_width"], r["want"]["col_rows"]) for r in rows if r["want"]["col_launches"]} == \
        {(8, 2), (32, 2), (8, 4), (8, 8), (8, 16)}
    ids = [td.route_id(r) for r in td.ROUTES]
    assert len(set(ids)) == len(ids)
    for r in td.ROUTES:      # a row that must repeat another row's bits names a row of the same orders
        if r["same_as"]:
            other = next(o for o in td.ROUTES if td.route_id(o) == r["same_as"])
            assert other["orders"] == r["orders"] and not other["same_as"]
    # every resident kernel, the panels, the column launches and both tails have a row that runs every case
    assert {(r["want"]["reduce"], r["want"]["kernel"]) for r in td.ROUTES if r["full"]} >= {
        (td.TEAM, td.K_TAGGED2), (td.TEAM, td.K_MEET2), (td.TEAM, td.K_SYM), (td.BAND2, td.K_BAND2),
        (td.BAND4, td.K_BAND4), (td.BIG_TEAM, td.K_TAGGED4), (td.BIG_TEAM, td.K_TAGGED8), (td.PANEL, td.K_NONE),
        (td.PANEL_HYBRID, td.K_TAGGED2), (td.COLUMNS, td.K_NONE)}
    assert {r["want"]["tail"] for r in td.ROUTES if r["full"] and not r["want"]["col_launches"]
            and r["want"]["reduce"] == td.COLUMNS} == {td.TAIL_REGS, td.TAIL_LDS}


# ------------------------------------------------------------------------------------- the offsets query
SIZES = [(1, 1, 1), (2, 1, 2), (17, 3, 17), (128, 16, 128), (129, 1, 128), (131, 2, 64), (260, 3, 128), (512, 32, 64),
         (513, 1, 128), (1025, 1, 128), (2049, 1, 128), (4096, 2, 128)]


def _offsets(lib, n_max, batch, k_max):
    out = (C.c_int64 * 5)()
    _lib.check(lib.ndmps_syevd_topk_reduction_offsets(n_max, batch, k_max, out))
    return list(out)


@pytest.mark.parametrize("n_max,batch,k_max", SIZES)
def test_reduction_offsets_are_the_layouts(lib, monkeypatch, n_max, batch, k_max):
    vh, tau, d, e, lda = plain = _offsets(lib, n_max, batch, k_max)
    total = lib.ndmps_syevd_topk_workspace_bytes(n_max, batch, k_max)
    assert lda == n_max + n_max % 2
    assert all(off % 256 == 0 for off in (vh, tau, d, e)) and 0 < vh < tau < d < e < total
    assert vh >= batch * n_max * lda * 8                  # the working copy of the matrices lies in front
    assert tau - vh >= batch * n_max * lda * 8
    assert d - tau >= batch * n_max * 8 and e - d >= batch * n_max * 8 and total - e >= batch * n_max * 8
    assert e + batch * n_max * 8 <= lib.ndmps_syevd_topk_stamps_offset(n_max, batch, k_max)
    for env in ("NDMPS_TRD_BAND=2", "NDMPS_TRD_BAND=4", "NDMPS_TRD_SYM=1", "NDMPS_TRD_NO_TEAM=1"):
        with monkeypatch.context() as m:
            _setenv(m, env)
            assert _offsets(lib, n_max, batch, k_max) == plain, env
    assert _offsets(lib, n_max, batch, 1)[:5] == plain       # the vectors' buffers lie behind


def test_reduction_offsets_check_their_arguments(lib):
    out = (C.c_int64 * 5)(*([-7] * 5))
    q = lib.ndmps_syevd_topk_reduction_offsets
    for args in ((0, 1, 1), (4097, 1, 1), (64, 0, 1), (64, 1, 0), (64, 1, 4097)):
        assert q(*args, out) == _lib.EINVAL and lib.ndmps_last_error()
    assert q(64, 1, 1, None) == _lib.EINVAL
    assert list(out) == [-7] * 5
