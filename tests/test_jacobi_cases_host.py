"""The cases and bars of tests/jacobi_cases.py are sound and have teeth (CPU only).

Sound: every family's exactness claim holds on every case, and LAPACK's ``eigh`` (sorted descending, sign-normalised)
stays a factor 10 below every bar on every case, so no bar rests on the luck of one solver.  (The bit-for-bit bar of the
``diag`` family is not LAPACK's to pass -- it orders ties its own way; the expected result is checked to be an exact
eigen-system instead.)  Teeth: each fault a block Jacobi can have is applied to the passing result and must be
rejected on every case where it changes the output, at least once per family it applies to.
"""
import numpy as np
import pytest

import jacobi_cases as jc

CASES = jc.all_cases()
IDS = [c.name for c in CASES]
BY_FAMILY = {}
for _c in CASES:
    BY_FAMILY.setdefault(_c.family, []).append(_c)


@pytest.fixture(scope="module")
def solved():
    return {c.name: jc.lapack(c) for c in CASES + [jc.outside_contract()]}


# ------------------------------------------------------------------------------------- claims
def test_every_family_is_present_at_its_orders():
    assert set(BY_FAMILY) == {"diag", "hadamard", "laplace", "deficient", "graded", "gram", "skew"}
    assert [c.n for c in BY_FAMILY["gram"]] == [5, 32, 40, 96, 512]
    for n in jc.SINGLE_ORDERS:
        fams = {c.family for c in jc.single_cases(n)}
        assert fams >= {"diag", "hadamard", "graded", "skew"} and (("laplace" in fams) == (n <= jc.LAPLACE_MAX))
    assert [(c.n, c.rank) for c in jc.deficient_cases()] == [(l, r) for l in (64, 130, 512) for r in (1, 7, 40)]
    tiny = jc.tiny_batch()
    assert len(tiny) == 130 and {c.n for c in tiny} == set(range(1, 25))
    assert len(tiny) > 64 and jc.np_of(max(c.n for c in tiny)) == 32
    for n_max in jc.BATCH_ORDERS:
        members = jc.batch_cases(n_max)
        assert [c.n for c in members] == jc.batch_sizes(n_max) == [n_max, 5, n_max // 2 + 1]
        assert members[0].family == "hadamard" and not members[0].indefinite
        assert members[1].family == "diag"
        assert members[2].family == "graded" or (members[2].family == "hadamard" and members[2].indefinite)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exactness_claims(case):
    s, g = case.S, case.G
    assert np.array_equal(s, s.T)
    assert np.array_equal(0.5 * (g + g.T), s)
    assert case.lam.shape == (case.n,) and np.all(np.diff(case.lam) <= 0)
    if case.family in ("hadamard", "skew"):
        m = jc.hadamard_m(case.n)
        assert np.array_equal(np.rint(m * s), m * s) and np.abs(m * s).max() < 2.0 ** 52
        assert np.array_equal(np.rint(case.lam), case.lam)                      # planted integers
        assert abs(np.trace(s) - case.lam.sum()) == 0.0                          # both sums are exact
        assert np.sum(s * s) == np.sum(case.lam ** 2)                            # Frobenius norm, exact in these too
    if case.family == "skew":
        k = g - s
        assert np.array_equal(k, -k.T) and np.array_equal(np.rint(4 * k), 4 * k)
        assert case.n == 1 or k.any()
    if case.family == "diag":
        assert np.array_equal(s, np.diag(np.diag(s)))
        w, v = jc.diag_expected(case)
        assert np.array_equal(s @ v, v * w[None, :]) and np.array_equal(v.T @ v, np.eye(case.n))
        assert np.array_equal(w, case.lam) and not jc.failures(case, w, v)
    if case.family == "deficient":
        assert np.array_equal(np.rint(s), s) and np.abs(s).max() < 2.0 ** 52
        assert np.linalg.matrix_rank(s) == case.rank
        assert np.count_nonzero(case.lam) == case.rank and np.all(case.lam[case.rank:] == 0.0)
        assert case.lam[case.rank - 1] > 0
    if case.family == "laplace":
        n = case.n
        assert sorted(np.diag(s)) == [2.0] * n and np.sum(s == -1.0) == 2 * (n - 1) and np.sum(s != 0) == 3 * n - 2
        assert np.all(jc.gaps(case.lam) > 0)
    if case.indefinite:
        assert case.lam[-1] < 0
        assert np.abs(np.diag(s)).max() >= case.scale / 8


def test_the_indefinite_cases_are_there():
    assert sum(c.indefinite for c in BY_FAMILY["hadamard"]) >= len(jc.SINGLE_ORDERS) - 2
    assert any(c.indefinite for c in BY_FAMILY["diag"]) and all(c.indefinite for c in BY_FAMILY["skew"] if c.n > 2)
    out = jc.outside_contract()
    assert not np.diag(out.S).any() and np.array_equal(out.S, np.ones((40, 40)) - np.eye(40))


def test_regime_rules():
    table = {24: (32, True, 4), 33: (64, True, 4), 128: (128, True, 4), 129: (160, True, 8), 672: (672, True, 8),
             673: (704, True, 4), 896: (896, True, 4), 897: (928, False, None)}
    assert tuple(table) == jc.BATCH_ORDERS
    for n_max, (np_, hist, waves) in table.items():
        assert jc.np_of(n_max) == np_ and jc.np_of(n_max) // jc.BS % 2 == 0
        assert jc.history(n_max, 3) is hist
        assert jc.history(n_max, 1) is False and jc.history(n_max, 3, env=0) is False
        assert jc.history(n_max, 1, env=1) is hist
        if hist:
            assert jc.replay_waves(np_) == waves
            lds = (np_ * 17 + waves * 32 * 33) * 8
            assert lds <= (159 if waves == 8 else 160) * 1024
    assert jc.np_of(1) == 32 and jc.np_of(32) == 32 and jc.np_of(513) == 544
    assert (896 * 17 + 4 * 32 * 33) * 8 == 152 * 1024               # the band no other test enters


# ------------------------------------------------------------------------------------- soundness
@pytest.mark.parametrize("case", CASES + [jc.outside_contract()], ids=IDS + ["outside"])
def test_lapack_passes_every_bar_with_a_margin_of_ten(case, solved):
    w, v = solved[case.name]
    assert not jc.failures(case, w, v, margin=10.0, skip=("exact",)), jc.ratios(case, w, v)


# ------------------------------------------------------------------------------------- teeth
def _swap_adjacent(case, w, v):
    j = next((j for j in range(case.n - 1) if w[j] != w[j + 1]), None)
    if j is None:
        return None
    p = np.arange(case.n)
    p[[j, j + 1]] = j + 1, j
    return w[p], v[:, p]


def _negate_column(case, w, v):
    v = v.copy()
    v[:, case.n // 2] *= -1
    return w, v


def _upper_triangle(case, w, v):
    if case.family != "skew":
        return None
    u = np.triu(case.G) + np.triu(case.G, 1).T
    if np.array_equal(u, case.S):
        return None
    w2, v2 = np.linalg.eigh(u)
    return w2[::-1].copy(), jc.sign_normalise(v2[:, ::-1])


def _rows_left_sorted(case, w, v):
    order = np.argsort(-np.diag(case.S), kind="stable")
    if np.array_equal(case.S[np.ix_(order, order)], case.S):
        return None                                   # the sort is a symmetry of the matrix: the same eigen-system
    return w, jc.sign_normalise(v[order])


def _padding_leaks(case, w, v):
    if not case.indefinite:
        return None
    w = w.copy()
    w[-1] = 0.0
    return np.sort(w)[::-1].copy(), v


FAULTS = {"swap": (_swap_adjacent, ("diag", "hadamard", "laplace", "deficient", "graded", "gram", "skew")),
          "negate": (_negate_column, ("diag", "hadamard", "laplace", "deficient", "graded", "gram", "skew")),
          "upper": (_upper_triangle, ("skew",)),
          # laplace has a constant diagonal: its sort is the identity and the fault cannot show
          "rows": (_rows_left_sorted, ("diag", "hadamard", "deficient", "graded", "gram", "skew")),
          "padding": (_padding_leaks, ("diag", "hadamard", "skew"))}


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_rejected_wherever_it_changes_the_output(fault, solved):
    fn, families = FAULTS[fault]
    hit = {}
    for case in CASES:
        w, v = jc.diag_expected(case) if case.family == "diag" else solved[case.name]
        assert not jc.failures(case, w, v)
        bad = fn(case, w, v)
        if bad is None:
            continue
        assert jc.failures(case, *bad), (fault, case.name)
        hit[case.family] = hit.get(case.family, 0) + 1
    assert set(hit) == set(families), (fault, hit)


@pytest.mark.parametrize("case", [jc.graded(40), jc.hadamard(33, "b")], ids=repr)
def test_a_rotation_block_replaced_by_the_identity_is_rejected_by_the_residual(case):
    w, v, _ = jc.numpy_jacobi(case.S)
    assert not jc.failures(case, w, v)
    w2, v2, _ = jc.numpy_jacobi(case.S, skip=(0, 0, 32))
    assert np.array_equal(w2, w)                      # the iteration is the same, only V's product lost a block
    r = jc.ratios(case, w2, v2)
    assert r["orth"] <= 1.0 and r["resid"] > 1.0, r


GRADED_SMALL = [jc.graded(33), jc.graded(40)]


@pytest.fixture(scope="module")
def stopped():
    return {(c.name, tol): jc.numpy_jacobi(c.S, tol) for c in GRADED_SMALL for tol in (1e-6, 1e-10, 1e-15)}


@pytest.mark.parametrize("case", GRADED_SMALL, ids=repr)
def test_an_iteration_stopped_at_1e_6_is_rejected(case, stopped):
    w, v, _ = stopped[case.name, 1e-6]
    assert jc.failures(case, w, v)
    w, v, _ = stopped[case.name, 1e-15]
    assert not jc.failures(case, w, v)


@pytest.mark.parametrize("case", GRADED_SMALL, ids=repr)
def test_the_convergence_bar_holds_for_the_stopping_rule(case, stopped):
    sweeps = []
    for tol in (1e-6, 1e-10, 1e-15):
        w, v, s = stopped[case.name, tol]
        assert jc.offdiag(case, v) <= jc.conv_bar(case, tol)
        assert jc.ratios(case, w, v)["orth"] <= 1.0
        sweeps.append(s)
    assert sweeps == sorted(sweeps) and sweeps[-1] < jc.MAX_SWEEPS
    # the bar is not vacuous: it separates the thresholds
    assert jc.offdiag(case, stopped[case.name, 1e-6][1]) > jc.conv_bar(case, 1e-10)
