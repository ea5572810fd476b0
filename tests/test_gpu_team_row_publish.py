"""The 32-column counter kernel of the resident tridiagonalisation (trd_team_kernel<2, false, 32>) on the MI355X, where
every live workgroup of a team publishes its 32 entries of row j + 1 instead of the owner of column j + 1 publishing the
column: the row falls on the first and the last lane group of a wave, crosses a tile (32 rows) and a block (32 columns),
and falls in the block whose workgroup leaves on that very column; orders below 512 leave zero rows and columns beyond
the order, and columns beyond lda unwritten.

Buffers, guards and strides are those of tests/test_gpu_trd_exact.py (``Bufs``); the bars are those of
tests/trd_cases.py (``reduction_failures``, ``values_failures``, E(n) = 2e-15 max(n, 50)).  Every call asks the device for
its route first and goes on only if that is the 32-column counter kernel, and reads every status word afterwards: a
status 2 (a bounded wait ran out) fails the test and every test behind it without another launch.

What the batches place (512 resident slots, teams dealt to the XCDs): 9 matrices with a largest order of 512 are the
smallest batch that leaves the 8-column blocks outside a stream (9 x 64 workgroups > 512).  17 of order 512 are 272
workgroups, so 16 CUs hold two, paired in reverse member order; 32 of order 192 are 32 teams of 6 (no pairing: 6 does not
divide 32); 32 of order 512 fill every slot, two workgroups per CU in reverse pairing -- the headline launch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import eig_routes as er  # noqa: E402
import topk_cases as tc  # noqa: E402
import trd_cases as td  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402
from test_gpu_trd_exact import DEV, GUARD, SENT, Bufs, _offsets, same_bits  # noqa: E402

jc = td.jc
DESC_BYTES, DESC_STATUS = 40, 32      # TrdDesc: three pointers, n, k, status, pad
MIXED = (130, 136, 137, 160, 161, 192, 257, 512, 512)      # J = n - 128 = 2, 8, 9, 32, 33, 64, 129, 384
STATE = {"gave_up": False}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


@pytest.fixture(autouse=True)
def _stop_behind_a_status_2_or_a_gpu_error():
    if STATE["gave_up"]:
        pytest.fail("an earlier resident launch gave up waiting (status 2): nothing more is launched")
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
    lib.ndmps_syevd_topk_set_team(1)
    lib.ndmps_syevd_topk_set_streamed(0)
    return lib


@pytest.fixture(scope="module")
def fallbacks(lib):
    return int(lib.ndmps_syevd_topk_team_fallbacks())


def planted(n, m):
    """Two diagonal blocks of orders m and n - m, and a first row that is zero beyond its sub-diagonal entry: column 0
    and column m - 1 are zero below the sub-diagonal when their turn comes (the zeros between the blocks stay exact
    zeros: every update there is a product with one), so tau[0] == tau[m - 1] == 0, e[0] == G[1, 0], e[m - 1] == 0."""
    rng = jc._rng("planted", n, m)
    g = np.zeros((n, n))
    for lo, hi in ((0, m), (m, n)):
        b = rng.standard_normal((hi - lo + 5, hi - lo))
        g[lo:hi, lo:hi] = b.T @ b
    g[0, 2:] = g[2:, 0] = 0.0
    g = 0.5 * (g + g.T)
    return jc.Case(f"planted-{n}-{m}", "planted", g, g, np.linalg.eigvalsh(g)[::-1].copy())


def solve(lib, cases, ws=None):
    """One call of the values phase on ``cases``; asserts the route, the status words and the write extents.  Returns
    (per member: dict(vh, tau, d, e, w, lda), the workspace)."""
    orders = [c.n for c in cases]
    n_max, B, k_max = max(orders), len(orders), min(max(orders), 128)
    r = er.route(lib, orders, k_max)
    assert (r["reduce"], r["kernel"], r["team_size"]) == (er.TEAM, er.K_MEET2, -(-n_max // 32)), \
        f"not the 32-column counter kernel: {r}"
    bufs = Bufs([c.G for c in cases])
    nbytes = int(lib.ndmps_syevd_topk_workspace_bytes(n_max, B, k_max))
    assert nbytes > 0
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert ws.numel() == nbytes
    _lib.check(lib.ndmps_syevd_topk_values_f64(B, bufs.ptr(bufs.g), bufs.sG, bufs.h_n, bufs.ptr(bufs.v), bufs.sV,
                                               bufs.ptr(bufs.w), bufs.sw, k_max, ws.data_ptr(), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    host = ws.cpu().numpy()
    off = int(r["off_desc"])
    status = [int(host[off + DESC_BYTES * b + DESC_STATUS:off + DESC_BYTES * b + DESC_STATUS + 4].view(np.int32)[0])
              for b in range(B)]
    if 2 in status:
        STATE["gave_up"] = True
    assert status == [0] * B, f"status words {status}"
    assert np.array_equal(bufs.g.cpu().numpy(), bufs.g_host), "G on the device changed (its matrices or the gaps between them)"
    assert bool((bufs.v == SENT).all()), "the values phase wrote V"
    w = bufs.w.cpu().numpy()
    assert np.all(w[:GUARD] == SENT), "wrote in front of w"
    o_vh, o_tau, o_d, o_e, lda = _offsets(lib, n_max, B, k_max)

    def cut(o, count):
        return host[o:o + 8 * count].view(np.float64)

    vh = cut(o_vh, B * n_max * lda).reshape(B, n_max, lda)
    tau, d, e = (cut(o, B * n_max).reshape(B, n_max) for o in (o_tau, o_d, o_e))
    out = []
    for b, n in enumerate(orders):
        wb = w[GUARD + b * bufs.sw:GUARD + (b + 1) * bufs.sw]
        assert np.all(wb[n:] == SENT), f"member {b}: wrote past its n entries of w"
        out.append(dict(vh=vh[b, :n].copy(), tau=tau[b, :n].copy(), d=d[b, :n].copy(), e=e[b, :n].copy(), w=wb[:n].copy(),
                        lda=lda))
    return out, ws


def hold(case, got):
    n = case.n
    r = td.reduction_ratios(case.S, got["vh"], got["tau"], got["d"], got["e"], n, got["lda"], lam=case.lam)
    vr = td.values_ratios(got["w"], got["d"], got["e"], n, min(128, n), case.scale)
    print(f"{case.name}: " + ", ".join(f"{k} {x:.3g}" for k, x in {**r, **vr}.items() if k != "shape"))
    assert not r["shape"], f"{case.name}: the storage format fails in {r['shape']}"
    bad = td.failures_of(r) + [k for k, x in vr.items() if not x <= 1.0]
    assert not bad, f"{case.name}: {bad}: error / bar {r} {vr}"
    if td.is_tridiagonal(case):
        exact = td.exact_failures(case.S, got["tau"], got["d"], got["e"], n)
        assert not exact, f"{case.name}: a tridiagonal input did not come back bit for bit in {exact}"


def mixed_cases():
    return [td.simple_case(n) for n in MIXED[:-1]] + [tc.hadamard_a(512)]


def test_small_orders_in_one_mixed_launch(lib, fallbacks):
    cases = mixed_cases()
    assert tuple(c.n for c in cases) == MIXED
    got, _ = solve(lib, cases)
    for case, g in zip(cases, got):
        hold(case, g)


def test_two_runs_on_one_workspace_are_bit_identical(lib, fallbacks):
    cases = mixed_cases()
    first, ws = solve(lib, cases)
    second, _ = solve(lib, cases, ws)
    assert same_bits(first, second), "two runs on one workspace differ"


def test_structured_inputs(lib, fallbacks):
    """Tridiagonal members come back bit for bit; the planted members have tau == 0 exactly where a column is zero below
    its sub-diagonal entry: at column 0 (e[0] the entry itself) and at the last column of the first block, whose row
    j + 1 = m is the first of a tile and of a block (64), sits inside both (40), or is the last one published (383)."""
    plant = {192: 40, 257: 64, 512: 383}
    cases = [td.tridiag(n) for n in MIXED[:5]] + [planted(192, 40), planted(257, 64), td.tridiag(512), planted(512, 383)]
    assert tuple(c.n for c in cases) == MIXED
    got, _ = solve(lib, cases)
    for case, g in zip(cases, got):
        hold(case, g)
        if case.family == "planted":
            m = plant[case.n]
            assert g["tau"][0] == 0.0 and g["e"][0] == case.S[1, 0], f"{case.name}: column 0"
            assert g["tau"][m - 1] == 0.0 and g["e"][m - 1] == 0.0, f"{case.name}: column {m - 1}"
            live = np.ones(case.n - 1, dtype=bool)
            live[[0, m - 2, m - 1, case.n - 2]] = False      # the last reflector of a block is 1 x 1: tau == 0 as well
            assert np.all(g["tau"][:case.n - 1][live] != 0.0), f"{case.name}: a reflector is missing elsewhere"


def test_members_of_order_up_to_128_beside_the_teams(lib, fallbacks):
    """Orders up to 128 have no column for the resident kernel: their workgroups leave at once and the tail kernel reduces
    them from the working copy in memory, beside eight full teams and a member with a single resident column."""
    cases = [jc.graded(512, t) for t in range(8)] + [td.simple_case(n) for n in (40, 128, 129)]
    got, _ = solve(lib, cases)
    for case, g in zip(cases, got):
        hold(case, g)


def _pool(n, count):
    pool = [td.simple_case(n), tc.hadamard_a(n), td.arrow(n), td.rank1(n), td.tridiag(n)]
    return pool + [jc.graded(n, 10 + t) for t in range(count - len(pool))]


@pytest.mark.parametrize("n, count, judged", [(512, 17, range(17)), (192, 32, range(32)), (512, 32, (0, 5, 15, 16, 26, 31))],
                         ids=["17x512", "32x192", "32x512"])
def test_full_teams(lib, fallbacks, n, count, judged):
    """More teams than one per 16 CUs (two workgroups on a CU), and the launch that fills every slot; of the 32
    order-512 members six are judged in full (two of each XCD-dealt kind), every status word of all of them is 0."""
    cases = _pool(n, count)
    assert len(cases) == count and len({c.name for c in cases}) == count
    got, _ = solve(lib, cases)
    for b in judged:
        hold(cases[b], got[b])


def test_no_fallback_was_counted(lib, fallbacks):
    assert int(lib.ndmps_syevd_topk_team_fallbacks()) == fallbacks
