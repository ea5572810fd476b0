"""The block Jacobi eigen-solver (csrc/eig_block.hip) on the MI355X, in every regime it has, on the cases of
tests/jacobi_cases.py: matrices whose eigen-system is known without a solver.

Every entry point is called through ctypes with ``stride_G``, ``stride_V`` and ``stride_w`` strictly larger than a
matrix, in buffers pre-filled with a sentinel: after every call the guard in front, the stride gaps, everything of a
member's ``V`` and ``w`` past its own ``n_b^2`` and ``n_b`` and, in history mode, the columns ``>= k_b`` must still hold
it.  The bars are those of tests/jacobi_cases.py (tests/test_jacobi_cases_host.py shows that LAPACK stays a factor 10
below each of them and that each rejects the faults it exists for); no bar is loosened for a family or a regime.  The
regime of a call is asserted from the rules restated in jacobi_cases (``np_of``, ``history``, ``replay_waves``): the
library has no route query for this solver.

Outside the contract (the header: thresholds are relative to ``max |a_ii|``): ``J - I`` of order 40, whose diagonal is
zero.  Observed on the MI355X: NDMPS_ENOCONV, a clean refusal (``test_zero_diagonal_is_solved_or_refused_cleanly``).

``WORST`` keeps, per regime, the largest error / bar seen; ``SWEEPS`` the sweep counts per family.  Both are printed
when the module ends.
"""
import ctypes as C
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import jacobi_cases as jc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402

DEV = "cuda:0"
SENT = jc.SENTINEL
GUARD = 24
WORST = {}    # regime -> {bar: largest error / bar}
SWEEPS = {}   # family or batch -> set of sweep counts


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")
    yield
    for regime in sorted(WORST):
        print(f"\nworst error / bar, {regime}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST[regime].items())))
    for fam in sorted(SWEEPS):
        print(f"sweeps, {fam}: {sorted(SWEEPS[fam])}")


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A launch that faulted leaves the device in an error state: end the session instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


@pytest.fixture(autouse=True)
def _default_mode(monkeypatch):
    monkeypatch.delenv("NDMPS_EIG_HISTORY", raising=False)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def sp():
    return _lib.stream_ptr()


class Bufs:
    """G, V and w of a batch on the device: 24 guard elements, then one stride per member, each stride longer than the
    largest member needs; everything but the matrices themselves holds the sentinel."""

    def __init__(self, mats):
        self.sizes = [int(m.shape[0]) for m in mats]
        self.B, self.n_max = len(mats), max(self.sizes)
        nn = self.n_max * self.n_max
        self.sG, self.sV, self.sw = nn + 40, nn + 24, self.n_max + 7
        host = np.full(GUARD + self.B * self.sG, SENT)
        for b, m in enumerate(mats):
            host[GUARD + b * self.sG:GUARD + b * self.sG + m.size] = np.asarray(m, dtype=np.float64).reshape(-1)
        self.g_gaps = host == SENT
        for b, n in enumerate(self.sizes):
            self.g_gaps[GUARD + b * self.sG:GUARD + b * self.sG + n * n] = False
        self.g = torch.from_numpy(host).to(DEV)
        self.v = torch.full((GUARD + self.B * self.sV,), SENT, dtype=torch.float64, device=DEV)
        self.w = torch.full((GUARD + self.B * self.sw,), SENT, dtype=torch.float64, device=DEV)
        self.h_n = _lib.i64_array(self.sizes)

    def ptr(self, t):
        return t.data_ptr() + 8 * GUARD

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.v == SENT).all()) and bool((self.w == SENT).all())

    def read(self, kcols=None):
        """[(w_b, V_b[:, :k_b])]; asserts that nothing outside them was written."""
        torch.cuda.synchronize()
        g, v, w = self.g.cpu().numpy(), self.v.cpu().numpy(), self.w.cpu().numpy()
        assert np.all(g[self.g_gaps] == SENT), "wrote into the guard or the stride gaps of G"
        assert np.all(v[:GUARD] == SENT) and np.all(w[:GUARD] == SENT), "wrote in front of the first member"
        out = []
        for b, n in enumerate(self.sizes):
            k = n if kcols is None else int(kcols[b])
            vb, wb = v[GUARD + b * self.sV:GUARD + (b + 1) * self.sV], w[GUARD + b * self.sw:GUARD + (b + 1) * self.sw]
            assert np.all(vb[n * n:] == SENT), f"member {b}: wrote past its n^2 entries of V"
            assert np.all(wb[n:] == SENT), f"member {b}: wrote past its n entries of w"
            mat = vb[:n * n].reshape(n, n)
            assert np.all(mat[:, k:] == SENT), f"member {b}: wrote columns >= k = {k} of V"
            out.append((wb[:n].copy(), mat[:, :k].copy()))
        return out


def _workspace(lib, bufs, single=False):
    nbytes = int(lib.ndmps_syevj_workspace_bytes(bufs.n_max) if single
                 else lib.ndmps_syevj_batched_workspace_bytes(bufs.n_max, bufs.B))
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def solve(lib, mats, entry="batched", rel_tol=1e-15, ks=None, want_sweeps=True):
    """One call of an entry point on ``mats``.  Returns (rc, sweeps, bufs).  ``entry``: ``single`` (ndmps_syevj_f64),
    ``batched``, ``tol``, or ``two`` (values, then vectors with ``ks``).  The workspace is sized by the matching query
    after the environment is set: both read NDMPS_EIG_HISTORY."""
    bufs = Bufs(mats)
    ws, nbytes = _workspace(lib, bufs, single=entry == "single")
    sweeps = C.c_int(-1)
    hs = C.byref(sweeps) if want_sweeps else None
    G, V, W = bufs.ptr(bufs.g), bufs.ptr(bufs.v), bufs.ptr(bufs.w)
    if entry == "single":
        assert bufs.B == 1
        rc = lib.ndmps_syevj_f64(G, bufs.n_max, V, W, ws.data_ptr(), nbytes, hs, sp())
    elif entry == "batched":
        rc = lib.ndmps_syevj_batched_f64(bufs.B, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw, ws.data_ptr(), nbytes,
                                         hs, sp())
    elif entry == "tol":
        rc = lib.ndmps_syevj_batched_tol_f64(bufs.B, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw, rel_tol,
                                             ws.data_ptr(), nbytes, hs, sp())
    else:
        rc = lib.ndmps_syevj_batched_values_f64(bufs.B, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw, rel_tol,
                                                ws.data_ptr(), nbytes, hs, sp())
        if rc == _lib.OK:
            assert bool((bufs.v == SENT).all()), "the values phase wrote V"
            rc = lib.ndmps_syevj_batched_vectors_f64(bufs.B, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw,
                                                     _lib.i64_array(ks), ws.data_ptr(), nbytes, sp())
    return rc, sweeps.value, bufs


def _hold(regime, case, w, v):
    """Every bar of ``case`` on (w, V[:, :k]); the ratios go into WORST[regime]."""
    r = jc.ratios(case, w, v)
    worst = WORST.setdefault(regime, {})
    for name, x in r.items():
        worst[name] = max(worst.get(name, 0.0), float(x))
    bad = {name: x for name, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name} ({regime}): error / bar {bad}"


def _sweeps_ok(key, sweeps):
    """The solver's own limit; the bound of 20 sweeps holds where the existing tests state it (the ``gram`` family)."""
    SWEEPS.setdefault(key, set()).add(sweeps)
    assert 1 <= sweeps < jc.MAX_SWEEPS


# ------------------------------------------------------------------------------------- single matrix, every family
@pytest.mark.parametrize("n", jc.SINGLE_ORDERS)
def test_single_matrix_every_family(lib, n):
    assert not jc.history(n, 1)
    for i, case in enumerate(jc.single_cases(n)):
        rc, sweeps, bufs = solve(lib, [case.G], "single", want_sweeps=i != 0)   # once with h_sweeps = NULL (gram_pass)
        _lib.check(rc)
        (w, v), = bufs.read()
        _hold("single, in-loop V", case, w, v)
        if i != 0:
            _sweeps_ok(f"single {case.family}", sweeps)


@pytest.mark.parametrize("case", jc.deficient_cases(), ids=repr)
def test_single_rank_deficient_gram_matrix(lib, case):
    rc, sweeps, bufs = solve(lib, [case.G], "single")
    _lib.check(rc)
    (w, v), = bufs.read()
    _hold("single, in-loop V", case, w, v)
    _sweeps_ok("single deficient", sweeps)


@pytest.mark.parametrize("case", [jc.hadamard(17, "b"), jc.laplace(65), jc.graded(257), jc.deficient(130, 7)], ids=repr)
def test_single_matrix_in_history_mode(lib, case, monkeypatch):
    monkeypatch.setenv("NDMPS_EIG_HISTORY", "1")
    assert jc.history(case.n, 1, env=1)
    rc, sweeps, bufs = solve(lib, [case.G], "single")
    _lib.check(rc)
    (w, v), = bufs.read()
    _hold(f"single, replay with {jc.replay_waves(jc.np_of(case.n))} waves", case, w, v)
    _sweeps_ok(f"single {case.family}", sweeps)


# ------------------------------------------------------------------------------------- batched, every regime
REGIMES = {24: (32, True, 4), 33: (64, True, 4), 128: (128, True, 4), 129: (160, True, 8), 672: (672, True, 8),
           673: (704, True, 4), 896: (896, True, 4), 897: (928, False, None)}


def _regime(n_max, batch, env=None):
    np_ = jc.np_of(n_max)
    if not jc.history(n_max, batch, env):
        return f"np {np_}, in-loop V"
    return f"np {np_}, replay with {jc.replay_waves(np_)} waves"


@pytest.mark.parametrize("n_max", jc.BATCH_ORDERS)
def test_batched_every_regime(lib, n_max):
    cases = jc.batch_cases(n_max)
    np_, hist, waves = REGIMES[n_max]
    assert (jc.np_of(n_max), jc.history(n_max, len(cases))) == (np_, hist)
    assert not hist or jc.replay_waves(np_) == waves
    rc, sweeps, bufs = solve(lib, [c.G for c in cases])
    _lib.check(rc)
    for case, (w, v) in zip(cases, bufs.read()):
        _hold(_regime(n_max, len(cases)), case, w, v)
    _sweeps_ok(f"batch n_max={n_max} ({', '.join(c.family for c in cases)})", sweeps)
    if np_ > 32:               # (one block pair is one "sweep" in LDS)
        assert sweeps > 1      # the diag member converged in sweep 0 beside members that did not


def test_batch_of_130_tiny_matrices(lib):
    cases = jc.tiny_batch()
    assert jc.np_of(max(c.n for c in cases)) == 32 and jc.history(24, len(cases)) and len(cases) > 2 * 64
    rc, sweeps, bufs = solve(lib, [c.G for c in cases])
    _lib.check(rc)
    for case, (w, v) in zip(cases, bufs.read()):
        _hold("np 32, replay with 4 waves", case, w, v)
    assert sweeps == 1         # one block pair, solved in LDS


# ------------------------------------------------------------------------------------- two-phase protocol
@pytest.mark.parametrize("n_max", [128, 129, 673, 897])
def test_two_phase_gives_the_leading_columns_of_the_one_call_form(lib, n_max):
    cases = jc.batch_cases(n_max) + [jc.hadamard(40, "b")]
    mats = [c.G for c in cases]
    sizes = [c.n for c in cases]
    hist = jc.history(n_max, len(cases))
    assert hist == (n_max != 897)
    rc, _, full = solve(lib, mats)
    _lib.check(rc)
    full = full.read()
    for ks in ([17, sizes[1], 16, 1], [n_max, 1, 17, 16]):
        rc, sweeps, bufs = solve(lib, mats, "two", ks=ks)
        _lib.check(rc)
        # without history V is accumulated in the loop and delivered whole
        got = bufs.read(kcols=ks if hist else None)
        for case, k, (w, v), (wf, vf) in zip(cases, ks, got, full):
            assert np.array_equal(w, wf)
            assert np.array_equal(v[:, :k], vf[:, :k]), f"{case.name}: the leading {k} columns differ from the one-call form"
            _hold(_regime(n_max, len(cases)) + ", two-phase", case, w, v[:, :k])


# ------------------------------------------------------------------------------------- history against in-loop
@pytest.mark.parametrize("n_max", [24, 129, 673])
def test_history_and_in_loop_agree(lib, n_max, monkeypatch):
    dense = jc.graded(min(n_max, 40))      # generic eigenvectors: every sign is determined
    cases = jc.batch_cases(n_max) + [dense]
    assert max(c.n for c in cases) == n_max
    res = {}
    for env in (0, 1):
        monkeypatch.setenv("NDMPS_EIG_HISTORY", str(env))
        assert jc.history(n_max, len(cases), env=env) == bool(env)
        rc, sweeps, bufs = solve(lib, [c.G for c in cases])
        _lib.check(rc)
        res[env] = (bufs.read(), sweeps)
        for case, (w, v) in zip(cases, res[env][0]):
            _hold(_regime(n_max, len(cases), env), case, w, v)
    assert res[0][1] == res[1][1]
    determined = 0
    for case, (w0, v0), (w1, v1) in zip(cases, res[0][0], res[1][0]):
        assert np.array_equal(w0, w1), f"{case.name}: the iteration on G depends on how V is formed"
        # The two modes round V differently, so a column whose largest entries tie in magnitude with opposite signs
        # (the Hadamard eigenvectors: every entry +-1 / sqrt(m)) may be normalised either way.  Where the largest entry
        # leads every entry of the other sign by more than 1e-6 -- far above the bar on V -- the sign is determined.
        top = np.argmax(np.abs(v0), axis=0)
        cols = np.arange(case.n)
        lead = v0[top, cols]
        rival = np.where(v0 * np.sign(lead)[None, :] < 0, np.abs(v0), 0.0).max(axis=0)
        sure = np.abs(lead) - rival > 1e-6
        determined += int(sure.sum())
        assert np.array_equal(np.sign(lead[sure]), np.sign(v1[top, cols][sure])), f"{case.name}: signs differ"
        assert np.abs(v0[:, sure] - v1[:, sure]).max(initial=0.0) <= 1e-6, f"{case.name}: V differs between the modes"
    assert determined >= 5 + dense.n      # the diag member and the dense one at the least


# ------------------------------------------------------------------------------------- symmetrisation
@pytest.mark.parametrize("env", [None, 0])
def test_only_the_symmetric_part_is_decomposed_batched(lib, env, monkeypatch):
    if env is not None:
        monkeypatch.setenv("NDMPS_EIG_HISTORY", str(env))
    cases = [jc.skew(129, "b"), jc.diag(5), jc.skew(65, "a")]
    assert all(not np.array_equal(c.G, c.G.T) for c in (cases[0], cases[2]))
    assert jc.history(129, 3, env) == (env is None)
    rc, _, bufs = solve(lib, [c.G for c in cases])
    _lib.check(rc)
    for case, (w, v) in zip(cases, bufs.read()):
        _hold(_regime(129, 3, env), case, w, v)


# ------------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("entry", ["single", "batched"])
def test_nothing_depends_on_the_absolute_scale(lib, entry):
    """Every threshold is relative to max |a_ii| and the rotation normalises by frexp: a power of two in front of the
    matrix changes no bit of V and scales w exactly.  At 1e-15 relative convergence nothing nears the underflow range."""
    groups = [[jc.graded(65)], [jc.hadamard(65, "b")]] if entry == "single" else [[jc.graded(129), jc.hadamard(65, "b")]]
    for cases in groups:
        res = {}
        for p in (0, 100, -100):
            rc, sweeps, bufs = solve(lib, [c.G * 2.0 ** p for c in cases], entry)
            _lib.check(rc)
            res[p] = (bufs.read(), sweeps)
        for case, (w, v) in zip(cases, res[0][0]):
            _hold("scale", case, w, v)
        for p in (100, -100):
            assert res[p][1] == res[0][1], f"2**{p}: {res[p][1]} sweeps, unscaled {res[0][1]}"
            for case, (w0, v0), (w, v) in zip(cases, res[0][0], res[p][0]):
                assert np.array_equal(w, w0 * 2.0 ** p), f"{case.name} * 2**{p}: w is not the scaled w"
                assert np.array_equal(v, v0), f"{case.name} * 2**{p}: V differs"


# ------------------------------------------------------------------------------------- rel_tol
def test_rel_tol_is_what_ends_the_iteration(lib):
    cases = [jc.graded(129), jc.graded(40), jc.graded(65)]
    counts = []
    for tol in (1e-6, 1e-10, 1e-15):
        rc, sweeps, bufs = solve(lib, [c.G for c in cases], "tol", rel_tol=tol)
        _lib.check(rc)
        for case, (w, v) in zip(cases, bufs.read()):
            off, bar = jc.offdiag(case, v), jc.conv_bar(case, tol)
            worst = WORST.setdefault(f"rel_tol {tol:g}", {})
            worst["offdiag"] = max(worst.get("offdiag", 0.0), off / bar)
            worst["orth"] = max(worst.get("orth", 0.0), jc.ratios(case, w, v)["orth"])
            assert off <= bar, f"{case.name} at rel_tol {tol:g}: off-diagonal {off:.3g} above {bar:.3g}"
            assert jc.ratios(case, w, v)["orth"] <= 1.0
            if tol == 1e-15:
                _hold("np 160, replay with 8 waves", case, w, v)
        _sweeps_ok(f"graded batch, rel_tol {tol:g}", sweeps)
        counts.append(sweeps)
    assert counts == sorted(counts), counts


# ------------------------------------------------------------------------------------- sweep counts
@pytest.mark.parametrize("n", jc.GRAM_ORDERS + (jc.GRAM_ORDERS[::-1][1:4],), ids=str)
def test_graded_gram_matrices_converge_in_twenty_sweeps(lib, n):
    """``1 <= sweeps <= 20`` where tests/test_gpu_parity.py asserts it: on its graded Gram matrices ``a^T a`` (the
    ``gram`` family, the same matrices), here in strided, guarded buffers, alone and as one batch in history mode.

    The bound is not claimed on the dense ``graded`` family ``q (a^T a) q^T`` or on any other: it has no derivation
    there, and the row-cyclic NumPy Jacobi of jacobi_cases with the same thresholds, the method itself, needs 17, 20
    and 22 sweeps on ``graded`` at orders 65, 129 and 257.  Measured on the MI355X on ``graded``: at most 18 sweeps up
    to order 65, 25 at order 257, 27 at order 513, 21 for the batch of orders (129, 40, 65).  Those tests assert the
    solver's own limit of 40 and record the counts."""
    batch = isinstance(n, tuple)
    cases = [jc.gram(m) for m in n] if batch else [jc.gram(n)]
    assert not batch or jc.history(max(n), len(n))
    rc, sweeps, bufs = solve(lib, [c.G for c in cases], "batched" if batch else "single")
    _lib.check(rc)
    for case, (w, v) in zip(cases, bufs.read()):
        _hold("gram, batch with replay" if batch else "gram, single", case, w, v)
    print(f"gram {n}: {sweeps} sweeps")
    SWEEPS.setdefault(f"gram {n}", set()).add(sweeps)
    assert 1 <= sweeps <= jc.GRAM_SWEEPS


# ------------------------------------------------------------------------------------- refusals
def _small(lib):
    case = jc.hadamard(17, "a")
    bufs = Bufs([case.G, jc.diag(5).G])
    ws, nbytes = _workspace(lib, bufs)
    return bufs, ws, nbytes


def _refused(lib, bufs, rc, code=_lib.EINVAL):
    assert rc == code and lib.ndmps_last_error()
    assert bufs.untouched(), "a refused call wrote its outputs"


def test_refusals_leave_the_outputs_alone(lib):
    bufs, ws, nbytes = _small(lib)
    G, V, W = bufs.ptr(bufs.g), bufs.ptr(bufs.v), bufs.ptr(bufs.w)
    a = (G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw)
    for tol in (1e-17, 1e-5):
        _refused(lib, bufs, lib.ndmps_syevj_batched_tol_f64(2, *a, tol, ws.data_ptr(), nbytes, None, sp()))
        _refused(lib, bufs, lib.ndmps_syevj_batched_values_f64(2, *a, tol, ws.data_ptr(), nbytes, None, sp()))
    for batch in (0, 4097):
        _refused(lib, bufs, lib.ndmps_syevj_batched_f64(batch, *a, ws.data_ptr(), nbytes, None, sp()))
    _refused(lib, bufs, lib.ndmps_syevj_batched_f64(2, G, bufs.sG, _lib.i64_array([17, 0]), V, bufs.sV, W, bufs.sw,
                                                    ws.data_ptr(), nbytes, None, sp()))
    _refused(lib, bufs, lib.ndmps_syevj_f64(G, 0, V, W, ws.data_ptr(), nbytes, None, sp()))
    for sG, sV, sw in ((17 * 17 - 1, bufs.sV, bufs.sw), (bufs.sG, 17 * 17 - 1, bufs.sw), (bufs.sG, bufs.sV, 16)):
        _refused(lib, bufs, lib.ndmps_syevj_batched_f64(2, G, sG, bufs.h_n, V, sV, W, sw, ws.data_ptr(), nbytes, None,
                                                        sp()))
    for ks in ([0, 1], [18, 1], [1, 6]):
        _refused(lib, bufs, lib.ndmps_syevj_batched_vectors_f64(2, *a, _lib.i64_array(ks), ws.data_ptr(), nbytes, sp()))
    # a workspace one byte short
    short = nbytes - 1
    _refused(lib, bufs, lib.ndmps_syevj_batched_f64(2, *a, ws.data_ptr(), short, None, sp()), _lib.EWORKSPACE)
    _refused(lib, bufs, lib.ndmps_syevj_batched_values_f64(2, *a, 1e-15, ws.data_ptr(), short, None, sp()),
             _lib.EWORKSPACE)
    _refused(lib, bufs, lib.ndmps_syevj_batched_vectors_f64(2, *a, _lib.i64_array([1, 1]), ws.data_ptr(), short, sp()),
             _lib.EWORKSPACE)
    one = Bufs([jc.hadamard(17, "a").G])
    n1 = int(lib.ndmps_syevj_workspace_bytes(17))
    _refused(lib, one, lib.ndmps_syevj_f64(one.ptr(one.g), 17, one.ptr(one.v), one.ptr(one.w), ws.data_ptr(), n1 - 1,
                                           None, sp()), _lib.EWORKSPACE)
    # and the same buffers are solved once the arguments are right
    _lib.check(lib.ndmps_syevj_batched_f64(2, *a, ws.data_ptr(), nbytes, None, sp()))
    for case, (w, v) in zip([jc.hadamard(17, "a"), jc.diag(5)], bufs.read()):
        _hold("np 32, replay with 4 waves", case, w, v)


# ------------------------------------------------------------------------------------- outside the contract
def test_zero_diagonal_is_solved_or_refused_cleanly(lib):
    """``J - I`` of order 40 has a zero diagonal: both thresholds of the solver are 0 for it, which the header puts
    outside the contract.  Either outcome is clean: NDMPS_OK with every bar met, or NDMPS_ENOCONV with a message and no
    state left behind.  Observed on the MI355X: NDMPS_ENOCONV after 40 sweeps; the PSD solve that follows succeeds."""
    case = jc.outside_contract()
    rc, sweeps, bufs = solve(lib, [case.G], "single")
    print(f"J - I of order 40: rc {rc}, {sweeps} sweeps")
    if rc == _lib.OK:
        (w, v), = bufs.read()
        _hold("outside the contract", case, w, v)
        SWEEPS.setdefault("J - I of order 40 (outside the contract)", set()).add(sweeps)
        assert 1 <= sweeps <= jc.MAX_SWEEPS
    else:
        assert rc == _lib.ENOCONV
        assert lib.ndmps_last_error()
        SWEEPS.setdefault("J - I of order 40 (outside the contract): NDMPS_ENOCONV", set()).add(jc.MAX_SWEEPS)
    psd = jc.hadamard(40, "a")
    rc, _, bufs = solve(lib, [psd.G], "single")
    _lib.check(rc)
    (w, v), = bufs.read()
    _hold("single, in-loop V", psd, w, v)


# ------------------------------------------------------------------------------------- two host threads
def test_two_host_threads_solve_at_once(lib):
    """Two threads, each on its own stream, three calls each: the pinned-flag pool and the per-device opt-in are shared;
    the results are those of the same calls made one after the other, bit for bit."""
    batches = [jc.batch_cases(129), [jc.hadamard(512, "a"), jc.diag(5), jc.graded(257)]]
    alone = []
    for cases in batches:
        rc, _, bufs = solve(lib, [c.G for c in cases])
        _lib.check(rc)
        alone.append(bufs.read())
        for case, (w, v) in zip(cases, alone[-1]):
            _hold(_regime(max(c.n for c in cases), 3), case, w, v)
    out, errs = [[], []], []
    start = threading.Barrier(2)

    def run(t):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                start.wait(timeout=60)
                for _ in range(3):
                    rc, _, bufs = solve(lib, [c.G for c in batches[t]])
                    _lib.check(rc)
                    torch.cuda.current_stream().synchronize()
                    out[t].append(bufs.read())
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(2):
        assert len(out[t]) == 3
        for got in out[t]:
            for (w, v), (w0, v0) in zip(got, alone[t]):
                assert np.array_equal(w, w0) and np.array_equal(v, v0)
