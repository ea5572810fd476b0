"""The first phase of the direct top-k eigen-solver on the MI355X: what ndmps_syevd_topk_values_f64 leaves in the
workspace -- the reflectors Vh, tau and the tridiagonal d, e (ndmps_syevd_topk_reduction_offsets) -- on every route of
tests/trd_cases.py::ROUTES, held to what a tridiagonalisation is (trd_cases.reduction_failures: storage format exactly,
Q orthogonal, Q^T A Q = T, eig(T) = the spectrum, each within E(n) = 2e-15 max(n, 50)), and the delivered eigenvalues
held to the device's own T (trd_cases.values_failures), so that a failure names the reduction or the bisection.

One driver (``run``) makes every call, built like the one of tests/test_gpu_topk_exact.py: matrices at strides longer
than a matrix in buffers pre-filled with a sentinel, guard elements in front; the route is asked from the device and
compared with the row before a number is judged; the workspace is copied back once.  After the call G is bit-identical
(matrices and gaps), V still holds its sentinel, w is written on [0, n_b) only with zeros behind min(k_max, n_b).
Tridiagonal inputs come back bit for bit from every one-stage kernel, and the sub-diagonal of ``blocks`` is exactly 0 at
every block boundary.  WORST keeps the largest error / bar per kernel, LAPACK's dsytrd on the same matrices beside it,
and the largest tau_defect; REPEATS whether two plain runs were bit-identical.  All are printed when the module ends."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import eig_routes as er  # noqa: E402
import trd_cases as td  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402

DEV = "cuda:0"
SENT = td.jc.SENTINEL
GUARD = 24
ITEMS = ("orth", "similar", "spectrum", "values")
WORST = {}      # kernel -> {item: largest error / bar, "tau_defect": largest value}
LAPACK = {}     # kernel -> the same for dsytrd on the matrices the kernel was given
REPEATS = {}    # kernel -> were two plain runs bit-identical
_DSYTRD = {}    # case name -> ratios of dsytrd


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")
    yield
    for kernel in sorted(WORST):
        dev, ref = WORST[kernel], LAPACK.get(kernel, {})
        print(f"\nworst error / bar, {kernel}: " + ", ".join(
            f"{k} {dev[k]:.3g} (dsytrd {ref.get(k, 0.0):.3g})" for k in ITEMS + ("tau_defect",) if k in dev))
    for kernel in sorted(REPEATS):
        print(f"two plain runs bit-identical, {kernel}: {REPEATS[kernel]}")


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
    for name in td.SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert tuple(lib.ndmps_syevd_topk_team_slots(n) for n in (512, 1024, 2048)) == er.MI355X_TEAM_SLOTS
    return lib


def sp():
    return _lib.stream_ptr()


class Bufs:
    """G, V and w of a batch on the device: guard elements, then one stride per member, each stride longer than the
    largest member needs; everything but the matrices holds a sentinel."""

    def __init__(self, mats):
        self.sizes = [int(m.shape[0]) for m in mats]
        self.B, self.n_max = len(mats), max(self.sizes)
        nn = self.n_max * self.n_max
        self.sG, self.sV, self.sw = nn + 40, nn + 24, self.n_max + 7
        host = np.full(GUARD + self.B * self.sG, SENT)
        for b, m in enumerate(mats):
            host[GUARD + b * self.sG:GUARD + b * self.sG + m.size] = np.asarray(m, dtype=np.float64).reshape(-1)
        self.g_host = host
        self.g = torch.from_numpy(host).to(DEV)
        self.v = torch.full((GUARD + self.B * self.sV,), SENT, dtype=torch.float64, device=DEV)
        self.w = torch.full((GUARD + self.B * self.sw,), SENT, dtype=torch.float64, device=DEV)
        self.h_n = _lib.i64_array(self.sizes)

    def ptr(self, t):
        return t.data_ptr() + t.element_size() * GUARD


def _offsets(lib, n_max, batch, k_max):
    out = (C.c_int64 * 5)()
    _lib.check(lib.ndmps_syevd_topk_reduction_offsets(n_max, batch, k_max, out))
    return list(out)


def assert_route(lib, row):
    """The device plans the row's route for the row's sizes, with the switches and the thread's settings as they are
    now (a recovery: the plan with the resident launches off, and a resident launch to abort in the first plan)."""
    orders, k = list(row["orders"]), td.k_max_of(row)
    if row["recover"]:
        assert er.route(lib, orders, k)["kernel"] != er.K_NONE
        r = er.route(lib, orders, k, team=0)
    else:
        r = er.route(lib, orders, k)
    assert {f: r[f] for f in row["want"]} == row["want"], td.route_id(row)
    return td.kernel_name(row) + (" (recovery)" if row["recover"] else "")


def run(lib, row, cases, nan_ws=False, scale=1.0):
    """Phase 1 on ``cases`` (times ``scale``) with the row's k_max, on a fresh workspace (``nan_ws``: every byte set).
    Returns, per member, what the workspace holds for it: dict(vh [n_max, lda], tau, d, e, w [n]); the write extents
    of G, V and w are asserted."""
    mats = [c.G * scale for c in cases]
    bufs = Bufs(mats)
    k_max = td.k_max_of(row)
    assert bufs.n_max == max(row["orders"]) and sorted(bufs.sizes) == sorted(row["orders"])
    nbytes = int(lib.ndmps_syevd_topk_workspace_bytes(bufs.n_max, bufs.B, k_max))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV) if nan_ws else \
        torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if row["recover"]:
        lib.ndmps_debug_inject_team_abort(1)
    _lib.check(lib.ndmps_syevd_topk_values_f64(bufs.B, bufs.ptr(bufs.g), bufs.sG, bufs.h_n, bufs.ptr(bufs.v), bufs.sV,
                                               bufs.ptr(bufs.w), bufs.sw, k_max, ws.data_ptr(), nbytes, sp()))
    if row["recover"]:
        rec = C.c_int(-1)
        _lib.check(lib.ndmps_syevd_topk_recover_f64(bufs.B, bufs.h_n, k_max, ws.data_ptr(), nbytes, C.byref(rec), sp()))
        assert rec.value == 1, "the injected abort was not recovered from"
    torch.cuda.synchronize()
    host = ws.cpu().numpy()
    g, v, w = bufs.g.cpu().numpy(), bufs.v.cpu().numpy(), bufs.w.cpu().numpy()
    assert np.array_equal(g, bufs.g_host), "G on the device changed (its matrices or the gaps between them)"
    assert np.all(v == SENT), "the values phase wrote V"
    assert np.all(w[:GUARD] == SENT), "wrote in front of w"
    o_vh, o_tau, o_d, o_e, lda = _offsets(lib, bufs.n_max, bufs.B, k_max)
    n_max, B = bufs.n_max, bufs.B

    def cut(off, count):
        return host[off:off + 8 * count].view(np.float64)

    vh = cut(o_vh, B * n_max * lda).reshape(B, n_max, lda)
    tau, d, e = (cut(off, B * n_max).reshape(B, n_max) for off in (o_tau, o_d, o_e))
    out = []
    for b, n in enumerate(bufs.sizes):
        wb = w[GUARD + b * bufs.sw:GUARD + (b + 1) * bufs.sw]
        assert np.all(wb[n:] == SENT), f"member {b}: wrote past its n entries of w"
        out.append(dict(vh=vh[b, :n].copy(), tau=tau[b, :n].copy(), d=d[b, :n].copy(), e=e[b, :n].copy(), w=wb[:n].copy(),
                        lda=lda))
    return out


def _note(table, kernel, ratios):
    worst = table.setdefault(kernel, {})
    for name, x in ratios.items():
        if name != "shape":
            worst[name] = max(worst.get(name, 0.0), float(x))


def _dsytrd(case):
    if case.name not in _DSYTRD:
        vh, tau, d, e = td.lapack_reduction(case.S)
        r = td.reduction_ratios(case.S, vh, tau, d, e, case.n, case.n, lam=case.lam)
        w = td.eig_tridiagonal(d, e, case.n)
        r.update(td.values_ratios(w, d, e, case.n, case.n, case.scale))
        _DSYTRD[case.name] = r
    return _DSYTRD[case.name]


def hold(kernel, row, case, got, scale=1.0):
    """One member against every item; ``scale``: the power of two its matrix was multiplied with (d, e, w are scaled
    back exactly).  The ratios go into WORST[kernel], dsytrd's on the same matrix into LAPACK[kernel]."""
    n, two = case.n, td.two_stage(row)
    d, e, w = got["d"] / scale, got["e"] / scale, got["w"] / scale
    r = td.reduction_ratios(case.S, got["vh"], got["tau"], d, e, n, got["lda"], lam=case.lam, two_stage=two)
    kv = min(td.k_max_of(row), n)
    vr = td.values_ratios(w, d, e, n, kv, case.scale)
    print(f"{kernel} | {case.name}: " + ", ".join(f"{k} {x:.3g}" for k, x in {**r, **vr}.items() if k != "shape"))
    _note(WORST, kernel, {**r, "values": vr["values"]})
    _note(LAPACK, kernel, {k: x for k, x in _dsytrd(case).items() if k in r or k == "values"})
    assert not r["shape"], f"{case.name} ({kernel}): the storage format fails in {r['shape']}"
    bad = td.failures_of(r) + [k for k, x in vr.items() if not x <= 1.0]
    assert not bad, f"{case.name} ({kernel}): {bad}: error / bar {r} {vr}"
    if two:
        return
    if td.is_tridiagonal(case):
        exact = td.exact_failures(case.S * scale, got["tau"], got["d"], got["e"], n)
        assert not exact, f"{case.name} ({kernel}): a tridiagonal input did not come back bit for bit in {exact}"
    if case.family == "blocks":
        at = td.block_boundaries(n)
        assert np.all(got["e"][at] == 0.0) and np.all(got["tau"][at] == 0.0), f"{case.name} ({kernel}): block boundaries"


def same_bits(a, b, what=("vh", "tau", "d", "e", "w")):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in what)


@pytest.fixture
def settings(lib):
    """team / streamed of the calling thread as a row wants them; put back, with the abort hook, behind the test."""
    def apply(row):
        lib.ndmps_syevd_topk_set_team(row["team"])
        lib.ndmps_syevd_topk_set_streamed(row["streamed"])
    try:
        yield apply
    finally:
        lib.ndmps_debug_inject_team_abort(0)
        lib.ndmps_syevd_topk_set_team(1)
        lib.ndmps_syevd_topk_set_streamed(0)


def _setenv(monkeypatch, env):
    for item in env.split():
        monkeypatch.setenv(*item.split("="))


# ------------------------------------------------------------------------------------- every route
@pytest.mark.parametrize("row", td.ROUTES, ids=td.route_id)
def test_every_route_leaves_a_tridiagonalisation(lib, monkeypatch, settings, row):
    _setenv(monkeypatch, row["env"])
    settings(row)
    kernel = assert_route(lib, row)
    for members in td.row_cases(row):
        for case, got in zip(members, run(lib, row, members)):
            hold(kernel, row, case, got)


# ------------------------------------------------------------------------------------- repeatability and scale
PER_KERNEL = [r for r in td.ROUTES if (r["full"] or td.route_id(r) in ("260", "1536-team0")) and not r["recover"]]


@pytest.mark.parametrize("row", PER_KERNEL, ids=td.route_id)
def test_repeatability_workspace_placement_and_scale(lib, monkeypatch, settings, row):
    """Per kernel, two plain runs on fresh workspaces.  Where they are bit-identical: a workspace of NaNs changes no bit
    (the workspace is scratch, callers hand over whatever their allocator returns); the rows that differ from this one
    in placement only (``same_as``) give the same bits; G * 2**+-250 (a Gram matrix of fp32 data sits anywhere in
    2**+-252) gives Vh and tau bit for bit and d, e, w exactly scaled.  Where they are not, every run is held to the
    bars all the same (``run`` and ``hold`` judge each)."""
    _setenv(monkeypatch, row["env"])
    settings(row)
    kernel = assert_route(lib, row)
    what = ("d", "e", "w") if td.two_stage(row) else ("vh", "tau", "d", "e", "w")   # two-stage: Vh is a log in another format
    for cases in td.row_cases(row)[:2 if len(row["orders"]) == 1 else 1]:    # simple and hadamard a, or the batch
        plain = [run(lib, row, cases) for _ in range(2)]
        for got in plain:
            for case, g in zip(cases, got):
                hold(kernel, row, case, g)
        same = same_bits(plain[0], plain[1], what)
        REPEATS[kernel] = REPEATS.get(kernel, True) and same
        nan = run(lib, row, cases, nan_ws=True)
        for case, g in zip(cases, nan):
            hold(kernel + ", NaN workspace", row, case, g)
        scaled = {}
        for p in (250, -250):
            scaled[p] = run(lib, row, cases, scale=2.0 ** p)
            for case, g in zip(cases, scaled[p]):
                hold(kernel + ", scaled", row, case, g, scale=2.0 ** p)
        if not same:
            continue
        assert same_bits(plain[0], nan, what), "a workspace of NaNs changed the result"
        for p, got in scaled.items():
            for case, a, b in zip(cases, plain[0], got):
                if td.decays(case):      # reaches the floor of householder(), an absolute number: the bars only
                    continue
                assert same_bits([a], [b], what[:-3]), f"{case.name} * 2**{p}: Vh or tau differ"
                for k in ("d", "e", "w"):
                    assert np.array_equal(a[k] * 2.0 ** p, b[k]), f"{case.name} * 2**{p}: {k} is not the scaled {k}"
        for other in (r for r in td.ROUTES if r["same_as"] == td.route_id(row)):
            with monkeypatch.context() as m:
                _setenv(m, other["env"])
                assert_route(lib, other)
                got = run(lib, other, cases)
            assert same_bits(plain[0], got, what), f"{td.route_id(other)} differs from {td.route_id(row)}"


def test_cached_graph_of_the_panel_launches_gives_the_eager_bits(lib, monkeypatch, settings):
    graph = next(r for r in td.ROUTES if r["want"]["graph"])
    eager = next(r for r in td.ROUTES if td.route_id(r) == graph["same_as"])
    got = {}
    for name, row in (("eager", eager), ("graph", graph), ("graph again", graph)):
        with monkeypatch.context() as m:
            _setenv(m, row["env"])
            settings(row)
            kernel = assert_route(lib, row)
            cases = td.row_cases(row)[0]
            got[name] = run(lib, row, cases)
            for case, g in zip(cases, got[name]):
                hold(kernel + (", graph" if row is graph else ""), row, case, g)
    assert same_bits(got["eager"], got["graph"]) and same_bits(got["eager"], got["graph again"])
