"""The direct top-k eigen-solver (csrc/eig_tridiag.hip) on the MI355X: its second phase on every route trd_route
plans, through both of its entries -- ndmps_syevd_topk_vectors_f64 (ranks from the host) and
ndmps_syevd_topk_vectors_auto_f64 (ranks decided on the device) -- on the cases of tests/topk_cases.py, whose
eigen-systems are known without a solver.

One driver (``run``) makes every call.  It places the matrices at ``stride_G``, ``stride_V`` and ``stride_w`` strictly
larger than a matrix, in buffers pre-filled with a sentinel, with guard elements in front; ranks, spectra and status
are pre-filled too.  After the call: G is bit-identical (the matrices and every gap), nothing in front of a buffer or
past a member's ``n^2`` / ``n`` entries was written, no column of V behind ``k_b`` (vectors) or behind
``min(k_cap, n_b)`` (auto) was written, the columns ``[k_b, min(k_cap, n_b))`` of the auto entry are exactly 0.0, its
ranks equal ``rank_from`` of the device's own eigenvalues and, where the guard admits the cutoff, ``rank_exact``; its
spectra are ``sqrt(max(w, 0))`` bit for bit on ``min(k_cap, n_b)`` entries and untouched behind (all of the auto
entry's items are topk_cases.auto_failures, which the host suite shows to report planted faults).  The route of a call
is asked from the device (tests/eig_routes.py) and compared with the row of the table before any number is judged.
The bars are those of topk_cases with the factors tests/test_gpu_parity.py already grants (1 / 4 / 8); WORST keeps the
largest error / bar per route and is printed when the module ends.
"""
import ctypes as C
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import eig_routes as er  # noqa: E402
import topk_cases as tc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402

DEV = "cuda:0"
SENT = tc.SENTINEL
ISENT = -77
GUARD = 24
WORST = {}      # route -> {bar: largest error / bar}
REPEATS = {}    # route -> were two plain runs bit-identical


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")
    yield
    for regime in sorted(WORST):
        print(f"\nworst error / bar, {regime}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST[regime].items())))
    for regime in sorted(REPEATS):
        print(f"two plain runs bit-identical, {regime}: {REPEATS[regime]}")


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A launch that faulted leaves the device in an error state: end the session instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in tc.SWITCHES + ("NDMPS_INVIT_DBG", "NDMPS_TRD_BAND", "NDMPS_TRD_SYM", "NDMPS_TRD_NO_TEAM"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert int(lib.ndmps_syevd_topk_max_k()) == tc.MAX_K
    assert tuple(lib.ndmps_syevd_topk_team_slots(n) for n in (512, 1024, 2048)) == er.MI355X_TEAM_SLOTS
    return lib


def sp():
    return _lib.stream_ptr()


def _setenv(monkeypatch, env):
    for item in env.split():
        monkeypatch.setenv(*item.split("="))


def _route_name(row):
    ortho = ("WideAuto", "Wide", "Small", "Blocks", "Columns")[row["ortho"]]
    back = ("Lanes", "Rows", "Wide")[row["back"]]
    return f"{ortho} / {back}" + (f"({row['seg']},{row['r']})" if row["back"] == tc.LANES else "") + f", cb {row['invit_cb']}"


def assert_route(lib, row):
    """The device plans the row's route for the row's sizes, with the switches as they are now."""
    r = er.route(lib, row["orders"], row["k"])
    assert {f: r[f] for f in tc.route_fields(row)} == tc.route_fields(row), tc.route_id(row)
    return _route_name(row)


class Bufs:
    """G, V, w, ranks, spectra and status of a batch on the device: guard elements, then one stride per member, each
    stride longer than the largest member needs; everything but the matrices holds a sentinel."""

    def __init__(self, mats, k_cap):
        self.sizes = [int(m.shape[0]) for m in mats]
        self.B, self.n_max = len(mats), max(self.sizes)
        nn = self.n_max * self.n_max
        self.sG, self.sV, self.sw, self.ss = nn + 40, nn + 24, self.n_max + 7, k_cap + 5
        host = np.full(GUARD + self.B * self.sG, SENT)
        for b, m in enumerate(mats):
            host[GUARD + b * self.sG:GUARD + b * self.sG + m.size] = np.asarray(m, dtype=np.float64).reshape(-1)
        self.g_host = host
        self.g = torch.from_numpy(host).to(DEV)
        self.v = torch.full((GUARD + self.B * self.sV,), SENT, dtype=torch.float64, device=DEV)
        self.w = torch.full((GUARD + self.B * self.sw,), SENT, dtype=torch.float64, device=DEV)
        self.spectra = torch.full((GUARD + self.B * self.ss,), SENT, dtype=torch.float64, device=DEV)
        self.ranks = torch.full((GUARD + self.B + GUARD,), ISENT, dtype=torch.int32, device=DEV)
        self.status = torch.full((GUARD + self.B + GUARD,), ISENT, dtype=torch.int32, device=DEV)
        self.h_n = _lib.i64_array(self.sizes)

    def ptr(self, t):
        return t.data_ptr() + t.element_size() * GUARD

    def outputs_untouched(self, w_too=True):
        torch.cuda.synchronize()
        return (bool((self.v == SENT).all()) and (not w_too or bool((self.w == SENT).all()))
                and bool((self.spectra == SENT).all()) and bool((self.ranks == ISENT).all())
                and bool((self.status == ISENT).all()) and np.array_equal(self.g.cpu().numpy(), self.g_host))


def _workspace(lib, bufs, k_max, nan=False):
    """``nan``: every double of the workspace starts as a NaN (all bits set) instead of whatever the allocator hands out."""
    nbytes = int(lib.ndmps_syevd_topk_workspace_bytes(bufs.n_max, bufs.B, k_max))
    assert nbytes > 0
    if nan:
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV), nbytes
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def _values(lib, bufs, k_max, ws, nbytes):
    return lib.ndmps_syevd_topk_values_f64(bufs.B, bufs.ptr(bufs.g), bufs.sG, bufs.h_n, bufs.ptr(bufs.v), bufs.sV,
                                           bufs.ptr(bufs.w), bufs.sw, k_max, ws.data_ptr(), nbytes, sp())


def run(lib, mats, k_max, entry, ks=None, cutoff=None, spectra=True, status=True, nan_ws=False, exact=None):
    """Both phases on ``mats``.  ``entry``: ``vectors`` (ranks ``ks`` from the host) or ``auto`` (``k_max`` is the cap;
    every member is held to topk_cases.auto_failures, ``exact``: the exact ranks or None per member).
    Returns [(w_b[:n], V_b as n x n with the sentinel in what was not written, k_b)]; every write extent is asserted."""
    bufs = Bufs(mats, k_max)
    ws, nbytes = _workspace(lib, bufs, k_max, nan=nan_ws)
    _lib.check(_values(lib, bufs, k_max, ws, nbytes))
    torch.cuda.synchronize()
    assert bool((bufs.v == SENT).all()), "the values phase wrote V"
    if entry == "vectors":
        st = (C.c_int * bufs.B)(*([ISENT] * bufs.B))
        _lib.check(lib.ndmps_syevd_topk_vectors_f64(bufs.B, bufs.h_n, _lib.i64_array(ks), k_max, ws.data_ptr(), nbytes,
                                                    st if status else None, sp()))
        assert not status or list(st) == [0] * bufs.B
    else:
        _lib.check(lib.ndmps_syevd_topk_vectors_auto_f64(
            bufs.B, bufs.h_n, k_max, cutoff, bufs.ptr(bufs.ranks), bufs.ptr(bufs.spectra) if spectra else None, bufs.ss,
            bufs.ptr(bufs.status) if status else None, ws.data_ptr(), nbytes, sp()))
    torch.cuda.synchronize()
    g, v, w = bufs.g.cpu().numpy(), bufs.v.cpu().numpy(), bufs.w.cpu().numpy()
    spec, ranks, stat = bufs.spectra.cpu().numpy(), bufs.ranks.cpu().numpy(), bufs.status.cpu().numpy()
    assert np.array_equal(g, bufs.g_host), "G on the device changed (its matrices or the gaps between them)"
    assert np.all(v[:GUARD] == SENT) and np.all(w[:GUARD] == SENT) and np.all(spec[:GUARD] == SENT), "wrote in front"
    assert np.all(ranks[:GUARD] == ISENT) and np.all(ranks[GUARD + bufs.B:] == ISENT), "wrote around the ranks"
    assert np.all(stat[:GUARD] == ISENT) and np.all(stat[GUARD + bufs.B:] == ISENT), "wrote around the status"
    if entry == "vectors":
        assert np.all(ranks == ISENT) and np.all(stat == ISENT) and np.all(spec == SENT)
    else:
        assert np.all(stat[GUARD:GUARD + bufs.B] == (0 if status else ISENT)), stat[GUARD:GUARD + bufs.B]
        assert spectra or np.all(spec == SENT)
    out = []
    for b, n in enumerate(bufs.sizes):
        vb, wb = v[GUARD + b * bufs.sV:GUARD + (b + 1) * bufs.sV], w[GUARD + b * bufs.sw:GUARD + (b + 1) * bufs.sw]
        assert np.all(vb[n * n:] == SENT), f"member {b}: wrote past its n^2 entries of V"
        assert np.all(wb[n:] == SENT), f"member {b}: wrote past its n entries of w"
        mat, wn = vb[:n * n].reshape(n, n), wb[:n].copy()
        if entry == "vectors":
            k = int(ks[b])
            assert np.all(mat[:, k:] == SENT), f"member {b}: wrote columns >= k = {k} of V"
        else:
            k = int(ranks[GUARD + b])
            sb = spec[GUARD + b * bufs.ss:GUARD + (b + 1) * bufs.ss] if spectra else None
            bad = tc.auto_failures(wn, mat, k, sb, cutoff, k_max, exact=exact[b] if exact else None, sentinel=SENT)
            assert not bad, f"member {b} of order {n}, rank {k}, k_cap {k_max}: the contract of the auto entry fails in {bad}"
        out.append((wn, mat.copy(), k))
    return out


def hold(regime, case, w, v, k_max):
    """Every bar of ``case`` on (w, V[:, :k]); the ratios go into WORST[regime]."""
    r = tc.ratios(case, w, v, k_max)
    worst = WORST.setdefault(regime, {})
    for name, x in r.items():
        worst[name] = max(worst.get(name, 0.0), float(x))
    bad = {name: x for name, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name} ({regime}, k = {v.shape[1]}): error / bar {bad}"


def solve_and_hold(lib, regime, cases, k_max, entry, cutoff=None, ks=None, scale=1.0, **kw):
    """``run`` on the cases (times ``scale``), every member held to its bars (w divided by ``scale``).  For the auto
    entry the ranks must also be the exact ones wherever the guard admits the cutoff."""
    if entry == "vectors" and ks is None:
        ks = [min(k_max, c.n) for c in cases]
    exact = None
    if entry == "auto":
        exact = [tc.rank_exact(c.lam, cutoff, k_max) if tc.admitted(c, cutoff) else None for c in cases]
    got = run(lib, [c.G * scale for c in cases], k_max, entry, ks=ks, cutoff=cutoff, exact=exact, **kw)
    for case, (w, v, k) in zip(cases, got):
        hold(regime, case, w / scale, v[:, :k], k_max)
    return got


# ------------------------------------------------------------------------------------- every route, both entries
# every row with both entries; the auto entry takes at most ndmps_syevd_topk_max_k() vectors (beyond: test_refusals_...)
ROW_ENTRIES = [pytest.param(row, entry, id=f"{tc.route_id(row)}-{entry}") for row in tc.ROUTES
               for entry in ("vectors", "auto") if entry == "vectors" or row["k"] <= tc.MAX_K]


@pytest.mark.parametrize("row,entry", ROW_ENTRIES)
def test_every_route_on_a_simple_and_a_multiple_spectrum(lib, monkeypatch, row, entry):
    _setenv(monkeypatch, row["env"])
    regime = assert_route(lib, row)
    for members in tc.row_cases(row):
        cutoff = tc.common_cutoff(members) if entry == "auto" else None
        solve_and_hold(lib, regime, members, row["k"], entry, cutoff=cutoff)


STRADDLE_ROWS = [r for r in tc.ROUTES if r["orders"] in ((1024,), (300,)) and r["k"] in (100, 128)] + \
    [tc._row([1024], 100, tc.NARROW, tc.BLOCKS, tc.LANES, 3, 16), tc._row([1024], 64, "", tc.WIDE_AUTO, tc.ROWS, None, 16)]


@pytest.mark.parametrize("row", STRADDLE_ROWS, ids=tc.route_id)
def test_exact_multiplicities_across_the_column_blocks(lib, monkeypatch, row):
    """Clusters of 20 .. 40 equal eigenvalues across columns 16, 32, 48, ... (the inverse iteration's blocks at order
    1024: the shifts of trd_shift_kernel), 64 (the blocks of the orthonormalisation) and the kept rank itself: kept
    ranks that cut a cluster (the cap) and that end one (the cutoff in a gap)."""
    _setenv(monkeypatch, row["env"])
    regime = assert_route(lib, row)
    case = tc.straddle(row["orders"][0])
    k = row["k"]
    solve_and_hold(lib, regime, [case], k, "vectors")
    for keep in (114, 54):
        cutoff = tc.cutoff_keeping(case, keep)
        assert tc.admitted(case, cutoff)
        (_, _, kb), = solve_and_hold(lib, regime, [case], k, "auto", cutoff=cutoff)
        assert kb == min(keep, k)


# ------------------------------------------------------------------------------------- indefinite input
@pytest.mark.parametrize("n,k", [(17, 17), (17, 5), (129, 64), (129, 129), (513, 128)])
def test_indefinite_input_gives_the_algebraically_largest_pairs(lib, n, k):
    """Negative eigenvalues, ties and zeros, and a matrix that is not symmetric: the leading k pairs are the
    algebraically largest of the symmetric part (the bars compare with the exact spectrum in descending order), and G
    comes back bit for bit (``run`` compares the whole buffer after both phases)."""
    r = er.route(lib, [n], k)
    regime = f"indefinite, ortho {r['ortho']} / back {r['back']}"
    for case in tc.indefinite_cases(n):
        assert case.indefinite and case.lam[-1] < 0
        if case.family == "skew":
            assert not np.array_equal(case.G, case.G.T)
        (w, v, _), = solve_and_hold(lib, regime, [case], k, "vectors")
        assert np.array_equal(w[k:], np.zeros(n - k))
    if k <= tc.MAX_K:       # the rank rule clamps the negative ones: sqrt(max(w, 0))
        case = tc.hadamard(n, "b")
        cutoff = tc.cutoff_keeping(case, int((case.lam >= 1).sum()))
        assert tc.admitted(case, cutoff)
        solve_and_hold(lib, regime, [case], k, "auto", cutoff=cutoff)


# ------------------------------------------------------------------------------------- the auto entry's contract
@pytest.mark.parametrize("case", tc.deficient_cases(), ids=repr)
def test_rank_deficient_gram_matrices_get_their_exact_rank(lib, case):
    k_cap = 64 if case.n == 64 else 128
    cutoff = tc.auto_cutoff(case)
    assert tc.admitted(case, cutoff)
    r = er.route(lib, [case.n], k_cap)
    (w, v, k), = solve_and_hold(lib, f"deficient, ortho {r['ortho']} / back {r['back']}", [case], k_cap, "auto", cutoff=cutoff)
    assert k == case.rank
    # a cap below the rank binds
    if case.rank > 1:
        (_, _, k), = solve_and_hold(lib, "deficient, capped", [case], case.rank - 1, "auto", cutoff=cutoff)
        assert k == case.rank - 1


def test_auto_edges(lib):
    # cutoff 0 on full-rank matrices: the cap, or the order
    for case, k_cap, want in ((tc.laplace(130), 64, 64), (tc.laplace(40), 128, 40), (tc.laplace(300), 128, 128)):
        assert tc.admitted(case, 0.0)
        (_, _, k), = solve_and_hold(lib, "auto edges", [case], k_cap, "auto", cutoff=0.0)
        assert k == want
    # cutoff >= 1: s_0 > cutoff s_0 is false, one pair is kept all the same
    for cutoff in (1.0, 2.5):
        for case in (tc.laplace(130), tc.hadamard_a(1024)):
            (_, v, k), = solve_and_hold(lib, "auto edges", [case], 64, "auto", cutoff=cutoff)
            assert k == 1 and np.all(v[:, 1:min(64, case.n)] == 0.0)
    # the zero matrix: rank 1, a vector of norm 1 (every vector is an eigenvector), residual exactly 0
    for n in (64, 130):
        zero = tc.diag(n, "zero")
        (w, v, k), = run(lib, [zero.G], 16, "auto", cutoff=0.3)
        assert k == 1 and np.all(w == 0.0)
        assert np.all(zero.S @ v[:, :1] == 0.0) and abs(np.linalg.norm(v[:, 0]) - 1.0) <= tc.E(n)   # any unit vector
        hold("auto edges", zero, w, v[:, :1], 16)
    # order 1, positive, zero and negative
    for value in (3.0, 0.0, -2.0):
        (w, v, k), = run(lib, [np.array([[value]])], 8, "auto", cutoff=0.5)
        assert k == 1 and abs(w[0] - value) <= tc.E(1) * abs(value) and abs(v[0, 0] - 1.0) <= tc.E(1)


@pytest.mark.parametrize("row", tc.MIXED, ids=tc.route_id)
def test_mixed_batches_with_orders_below_the_cap(lib, row):
    """Orders below k_cap beside larger ones: the kernels size their grids by min(k_cap, n_max) and every member must
    stop at its own min(k_cap, n_b) -- columns, zero fill and spectra (``run`` pins all of them with the sentinel).
    [1024, 40] takes the chip-wide route, whose first kernel of the back-transformation copies and zero-fills."""
    regime = "mixed, " + assert_route(lib, row)
    cases = tc.mixed_cases(row)
    k_cap = row["k"]
    assert min(c.n for c in cases) < k_cap < max(c.n for c in cases)
    solve_and_hold(lib, regime, cases, k_cap, "vectors")
    cutoff = tc.common_cutoff(cases)
    got = solve_and_hold(lib, regime, cases, k_cap, "auto", cutoff=cutoff)
    assert any(k < min(k_cap, c.n) for c, (_, _, k) in zip(cases, got)), "no member with fill columns"
    got = solve_and_hold(lib, regime, cases, k_cap, "auto", cutoff=0.0 if all(tc.admitted(c, 0.0) for c in cases) else 1e-9)
    solve_and_hold(lib, regime, cases, k_cap, "auto", cutoff=cutoff, spectra=False, status=False)


CHIP_WIDE = [next(r for r in tc.ROUTES if r["orders"] == (1024,) and r["k"] == 128 and not r["env"]),
             next(r for r in tc.MIXED if r["back"] == tc.ROWS)]


@pytest.mark.parametrize("row", CHIP_WIDE, ids=tc.route_id)
def test_chip_wide_route_does_not_read_what_it_never_wrote(lib, row):
    """The workspace is scratch: callers hand over whatever their allocator returns.  On the chip-wide route all
    ``kp`` columns of the eigenvector block are factored, the ones from the rank on masked out of the Gram matrix;
    the triangular solve multiplies them with the exact zeros of L^-1, so they must be zeros themselves
    (trd_invit_kernel clears them), not what the workspace held: 0 * NaN is NaN.  With a workspace of NaNs, kept ranks
    below ``kp`` (the cutoff in a gap, an order below the cap) and the cap itself pass the bars of a clean workspace."""
    assert row["ortho"] == tc.WIDE_AUTO and row["back"] == tc.ROWS
    regime = "NaN workspace, " + assert_route(lib, row)
    cases = tc.mixed_cases(row) if len(row["orders"]) > 1 else [tc.straddle(1024)]
    cutoff = tc.cutoff_keeping(cases[0], 54)
    assert all(tc.admitted(c, cutoff) for c in cases)
    got = solve_and_hold(lib, regime, cases, row["k"], "auto", cutoff=cutoff, nan_ws=True)
    assert got[0][2] == 54 < row["k"]
    solve_and_hold(lib, regime, cases, row["k"], "vectors", nan_ws=True)


def test_null_spectra_and_status_are_accepted(lib):
    case = tc.hadamard_a(130)
    cutoff = tc.auto_cutoff(case)
    for spectra, status in ((False, True), (True, False), (False, False)):
        solve_and_hold(lib, "auto, NULL outputs", [case], 128, "auto", cutoff=cutoff, spectra=spectra, status=status)
    solve_and_hold(lib, "vectors, NULL status", [case], 128, "vectors", status=False)


# ------------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("name,k", [("graded-130", 64), ("graded-130", 128), ("graded-1024", 128), ("hadamard-b-129", 64)])
def test_nothing_depends_on_the_absolute_scale(lib, name, k):
    """A Gram matrix of fp32 data sits anywhere in 2**+-252.  Tridiagonalisation, the Gershgorin scaling of T and the
    floor on e^2 are relative: times 2**+-250, w / 2**+-250 and V pass the unscaled case's bars; where two plain runs of
    the unscaled case are bit-identical, the scaled runs give the same V bit for bit and exactly scaled w."""
    case = {"graded-130": tc.graded(130), "graded-1024": tc.graded(1024), "hadamard-b-129": tc.hadamard(129, "b")}[name]
    r = er.route(lib, [case.n], k)
    regime = f"scale, reduce {r['reduce']} / ortho {r['ortho']} / back {r['back']}"
    plain = [solve_and_hold(lib, regime, [case], k, "vectors")[0] for _ in range(2)]
    same = np.array_equal(plain[0][0], plain[1][0]) and np.array_equal(plain[0][1], plain[1][1])
    REPEATS[f"{regime} ({name}, k {k})"] = same
    for p in (250, -250):
        (w, v, _), = solve_and_hold(lib, regime, [case], k, "vectors", scale=2.0 ** p)
        if same:
            assert np.array_equal(w, plain[0][0] * 2.0 ** p), f"{name} * 2**{p}: w is not the scaled w"
            assert np.array_equal(v, plain[0][1]), f"{name} * 2**{p}: V differs"
    if not case.indefinite:
        cutoff = tc.auto_cutoff(case)
        ranks = {p: solve_and_hold(lib, regime, [case], k, "auto", cutoff=cutoff, scale=2.0 ** p)[0][2] for p in (0, 250, -250)}
        assert len(set(ranks.values())) == 1, ranks


# ------------------------------------------------------------------------------------- two host threads
def test_two_host_threads_on_the_chip_wide_route(lib):
    """Two threads, each with its own stream, buffers and workspace, solve an order-1024, k = 128 case at once: the
    row-dealt back-transformation forms its T factors on the one side stream of the device for both."""
    row = next(r for r in tc.ROUTES if r["orders"] == (1024,) and r["k"] == 128 and not r["env"])
    regime = assert_route(lib, row)
    assert row["back"] == tc.ROWS and row["t_factors"] == 2
    cases = [tc.graded(1024), tc.straddle(1024)]
    out, errs = [[], []], []
    start = threading.Barrier(2)

    def work(t):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                assert er.route(lib, row["orders"], row["k"])["back"] == er.BACK_ROWS
                start.wait(timeout=60)
                for entry in ("vectors", "auto", "vectors"):
                    cutoff = tc.auto_cutoff(cases[t]) if entry == "auto" else None
                    out[t].append(run(lib, [cases[t].G], 128, entry, ks=[128], cutoff=cutoff)[0])
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(2):
        assert len(out[t]) == 3
        for w, v, k in out[t]:
            hold(regime + ", two threads", cases[t], w, v[:, :k], 128)


# ------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_alone(lib):
    cases = [tc.hadamard_a(40), tc.laplace(7)]
    bufs = Bufs([c.G for c in cases], 16)
    ws, nbytes = _workspace(lib, bufs, 16)
    G, V, W = bufs.ptr(bufs.g), bufs.ptr(bufs.v), bufs.ptr(bufs.w)

    def refused(rc, code=_lib.EINVAL, w_too=True):
        assert rc == code and lib.ndmps_last_error()
        assert bufs.outputs_untouched(w_too), "a refused call wrote an output"

    # phase 1: strides smaller than a matrix, sizes, k_max, a short workspace
    for sG, sV, sw in ((40 * 40 - 1, bufs.sV, bufs.sw), (bufs.sG, 40 * 40 - 1, bufs.sw), (bufs.sG, bufs.sV, 39)):
        refused(lib.ndmps_syevd_topk_values_f64(2, G, sG, bufs.h_n, V, sV, W, sw, 16, ws.data_ptr(), nbytes, sp()))
    refused(lib.ndmps_syevd_topk_values_f64(2, G, bufs.sG, _lib.i64_array([40, 0]), V, bufs.sV, W, bufs.sw, 16, ws.data_ptr(),
                                            nbytes, sp()))
    refused(lib.ndmps_syevd_topk_values_f64(2, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw, 0, ws.data_ptr(), nbytes, sp()))
    refused(lib.ndmps_syevd_topk_values_f64(2, G, bufs.sG, bufs.h_n, V, bufs.sV, W, bufs.sw, 16, ws.data_ptr(), nbytes - 1,
                                            sp()), _lib.EWORKSPACE)
    _lib.check(_values(lib, bufs, 16, ws, nbytes))
    torch.cuda.synchronize()
    w_after = bufs.w.clone()
    # phase 2 with the ranks from the host: k[b] > n[b], k[b] > k_max, k[b] = 0, no ranks
    st = (C.c_int * 2)(ISENT, ISENT)
    for ks in ([16, 8], [17, 7], [0, 1]):          # k[1] > n[1], k[0] > k_max, k[0] = 0
        refused(lib.ndmps_syevd_topk_vectors_f64(2, bufs.h_n, _lib.i64_array(ks), 16, ws.data_ptr(), nbytes, st, sp()),
                w_too=False)
    refused(lib.ndmps_syevd_topk_vectors_f64(2, bufs.h_n, None, 16, ws.data_ptr(), nbytes, st, sp()), w_too=False)
    assert list(st) == [ISENT, ISENT]
    # ... and on the device: k_cap above ndmps_syevd_topk_max_k(), a negative cutoff, a NaN, no ranks, a short workspace
    R, S, T = bufs.ptr(bufs.ranks), bufs.ptr(bufs.spectra), bufs.ptr(bufs.status)
    refused(lib.ndmps_syevd_topk_vectors_auto_f64(2, bufs.h_n, 129, 0.1, R, S, bufs.ss, T, ws.data_ptr(), nbytes, sp()), w_too=False)
    for cutoff in (-1e-300, -1.0, float("nan")):
        refused(lib.ndmps_syevd_topk_vectors_auto_f64(2, bufs.h_n, 16, cutoff, R, S, bufs.ss, T, ws.data_ptr(), nbytes, sp()),
                w_too=False)
    refused(lib.ndmps_syevd_topk_vectors_auto_f64(2, bufs.h_n, 16, 0.1, None, S, bufs.ss, T, ws.data_ptr(), nbytes, sp()),
            w_too=False)
    refused(lib.ndmps_syevd_topk_vectors_auto_f64(2, bufs.h_n, 16, 0.1, R, S, bufs.ss, T, ws.data_ptr(), nbytes - 1, sp()),
            _lib.EWORKSPACE, w_too=False)
    assert torch.equal(bufs.w, w_after)
    # more vectors than the auto entry takes, after a first phase that delivered them (the Wide rows of the table)
    wide = Bufs([tc.laplace(130).G], 130)
    wws, wbytes = _workspace(lib, wide, 130)
    _lib.check(_values(lib, wide, 130, wws, wbytes))
    for k_cap in (tc.MAX_K + 1, 130, 200):
        rc = lib.ndmps_syevd_topk_vectors_auto_f64(1, wide.h_n, k_cap, 0.1, wide.ptr(wide.ranks), wide.ptr(wide.spectra),
                                                   wide.ss, wide.ptr(wide.status), wws.data_ptr(), wbytes, sp())
        assert rc == _lib.EINVAL and lib.ndmps_last_error() and wide.outputs_untouched(w_too=False), k_cap
    # the same buffers and workspace are solved once the arguments are right
    cutoff = tc.common_cutoff(cases)
    _lib.check(lib.ndmps_syevd_topk_vectors_auto_f64(2, bufs.h_n, 16, cutoff, R, S, bufs.ss, T, ws.data_ptr(), nbytes, sp()))
    torch.cuda.synchronize()
    v, w, ranks = bufs.v.cpu().numpy(), bufs.w.cpu().numpy(), bufs.ranks.cpu().numpy()
    for b, case in enumerate(cases):
        n, k = case.n, int(ranks[GUARD + b])
        assert k == tc.rank_exact(case.lam, cutoff, 16)
        mat = v[GUARD + b * bufs.sV:GUARD + b * bufs.sV + n * n].reshape(n, n)
        hold("after refusals", case, w[GUARD + b * bufs.sw:GUARD + b * bufs.sw + n].copy(), mat[:, :k].copy(), 16)
