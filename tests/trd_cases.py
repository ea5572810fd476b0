"""The first phase of the direct top-k eigen-solver (csrc/eig_tridiag.hip, eig_panel.inc, eig_sym.inc, eig_band.inc) held
to what a tridiagonalisation is: a model of the reduction, a checker of what the kernels leave in the workspace, the
cases, and the table of phase-1 routes.  Shared by tests/test_trd_cases_host.py (CPU: the model and LAPACK's dsytrd pass
every bar with a margin of 10, every planted fault is reported by the item that exists for it, the route table is what
trd_route plans) and tests/test_gpu_trd_exact.py (the kernels).  NumPy, SciPy and mpmath only: no torch, no device.

Storage (ndmps_syevd_topk_reduction_offsets, include/ndmps_hip.h): with A = (G + G^T) / 2 of order n,

    Q^T A Q = T,   Q = H_0 H_1 ... H_{n-2},   H_j = I - tau[j] v_j v_j^T,   v_j = Vh[j, :]  (lda doubles per row)

``v_j`` is 0.0 at 0 .. j, exactly 1.0 at j + 1 and 0.0 at n .. lda - 1; ``d[j] = T[j, j]``, ``e[j] = T[j + 1, j]``;
``d[n - 1]`` is set, ``e[n - 1] = tau[n - 1] = 0`` and row n - 1 of Vh is zero.  This is LAPACK's dsytrd(lower) with the
reflectors written out in rows.

Items of ``reduction_failures`` (``E(n) = 2e-15 max(n, 50)``, ``scale = max |lambda|``: the solver's contract of
tests/test_gpu_parity.py::_check_topk with factor 1 -- the backward error of a reduction does not depend on
multiplicities):

  shape     exact: the zeros, the 1.0 (where tau[j] == 0 the row is e_{j+1} or zero), row n - 1, e[n - 1], tau[n - 1],
            every tau[j] is 0 or in [1, 2], everything finite
  orth      |Q^T Q - I|_max <= E           Q accumulated in fp64 in compact-WY blocks of 64 reflectors
  similar   |Q^T A Q - T|_max <= E scale
  spectrum  |eig(T) - lambda|_max <= E scale on all n values (lambda: exact where the case knows it, else eigvalsh(A))

``tau_defect = max_j |tau[j] v_j^T v_j - 2|`` over tau[j] != 0 is measured and reported, never asserted: it says how far
the fast reciprocal square root and reciprocal of householder() leave a reflector from an exact reflection.  The
two-stage kinds (NDMPS_TRD_BAND) log the block reflectors of their first stage in Vh, in another format: they are held
to ``spectrum``, finiteness and ``e[n - 1] == 0`` only.  ``values_failures`` isolates bisection from the reduction: it
compares the delivered eigenvalues with those of the device's own T.

Cases: the families of tests/jacobi_cases.py / topk_cases.py, and five that aim at the reduction: ``blocks``
(kron(I, B B^T), integer B of order 37: the sub-diagonal is exactly 0 at every multiple of 37, so sigma == 0 falls in the
middle of the 8- and 32-column blocks, of the panels and of the tail), ``arrow`` (one real reflector; behind it the
trailing matrix is 2 I up to the rounding of a ``w`` that is 0 in exact arithmetic: sigma is 0 or the square of noise to
the end), ``rank1`` (after step 0 the trailing matrix is rounding noise or zero), ``zero`` / ``identity``, and
``tridiag`` (the un-permuted second-difference matrix: ``laplace`` of jacobi_cases is permuted and dense in pattern).
``tridiag``, ``diag``, ``zero`` and ``identity`` are already tridiagonal: every one-stage kernel then takes the
sigma == 0 branch of householder() with tau' = 0 in front of it, all its corrections are products with that zero, and
``exact_failures`` demands d == diag(A), e == subdiag(A), tau == 0 bit for bit.
"""
import functools

import numpy as np
import scipy.linalg

import jacobi_cases as jc
import mpmath
import topk_cases as tc
from jacobi_cases import Case, E

BLOCK = 37
WY = 64
ORDER_SLACK = tc.ORDER_SLACK


# ------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def blocks(n):
    assert n % BLOCK != 0 and n > BLOCK
    rng = jc._rng("blocks", n)
    b = rng.integers(-3, 4, size=(BLOCK, BLOCK)).astype(np.float64)
    p = -(-n // BLOCK)
    g = np.ascontiguousarray(np.kron(np.eye(p), b @ b.T)[:n, :n])     # integers up to 37 * 9: exact
    return Case(f"blocks-{n}", "blocks", g, g, np.linalg.eigvalsh(g)[::-1].copy())


@functools.lru_cache(maxsize=None)
def arrow(n):
    """[[a, b^T], [b, 2 I]] with integers: H_0 b = beta e_1 and H_0 (2 I) H_0 = 2 I, so behind the one real reflector
    the trailing matrix is 2 I and the rounding of ``w = tau y - (tau^2 / 2)(y . v) v``, which is 0 in exact arithmetic.
    Spectrum: 2 (n - 2 times) and the roots of (x - a)(x - 2) = |b|^2."""
    rng = jc._rng("arrow", n)
    g = 2.0 * np.eye(n)
    g[0, 0] = 5.0
    lam = np.array([5.0])
    if n > 1:
        b = rng.integers(1, 4, size=n - 1).astype(np.float64)
        g[0, 1:] = g[1:, 0] = b
        root = float(mpmath.sqrt(mpmath.mpf(9) / 4 + mpmath.mpf(float(b @ b))))
        lam = np.concatenate([[3.5 + root], np.full(n - 2, 2.0), [3.5 - root]])
    return Case(f"arrow-{n}", "arrow", g, g, lam)


@functools.lru_cache(maxsize=None)
def rank1(n):
    rng = jc._rng("rank1", n)
    u = rng.integers(1, 6, size=n).astype(np.float64)
    g = np.outer(u, u)
    lam = np.zeros(n)
    lam[0] = float(u @ u)
    return Case(f"rank1-{n}", "rank1", g, g, lam, rank=1)


def zero(n):
    return jc.diag(n, "zero")


@functools.lru_cache(maxsize=None)
def identity(n):
    g = np.eye(n)
    return Case(f"identity-{n}", "diag", g, g, np.ones(n))


@functools.lru_cache(maxsize=None)
def tridiag(n):
    """2 on the diagonal, -1 beside it, not permuted; lambda_k = 2 - 2 cos(k pi / (n + 1))."""
    g = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    with mpmath.workdps(40):
        lam = np.array([float(2 - 2 * mpmath.cos(mpmath.pi * k / (n + 1))) for k in range(n, 0, -1)])
    return Case(f"tridiag-{n}", "tridiag", g, g, lam)


TRIDIAGONAL = ("tridiag", "diag")          # families whose members are tridiagonal as given (zero, identity: diag)


def is_tridiagonal(case):
    """By the entries, not by the name: a small Hadamard or arrow member may be tridiagonal as well."""
    return bool(np.array_equal(case.S, np.triu(np.tril(case.S, 1), -1)))


def decays(case):
    """``hadamard`` r1 is c h h^T with |h_i| = 1 (and zeros): every entry of a trailing matrix is formed by the same
    operations on the same magnitudes and rounds alike, so what a step leaves is again of rank one and 2^-53 times
    smaller -- column after column, down to the floor of householder() (an absolute number: a column of norm below
    2^-450 is taken for zero).  Where the decay stops depends on the power of two in front of the matrix, and with it
    which reflectors are the identity: such a member is held to the bars at every scale, not to equal bits."""
    return case.name.startswith("hadamard-r1")


def simple_case(n, tag=0):
    return jc.laplace(n) if n <= jc.LAPLACE_MAX else jc.graded(n, tag)


def extras(n):
    """What one row per kernel runs besides ``simple_case`` and hadamard a."""
    out = [arrow(n), rank1(n), zero(n), identity(n), jc.diag(n), tridiag(n)]
    if n > BLOCK and n % BLOCK:
        out.insert(0, blocks(n))
    if 4 <= n < 1024:           # jacobi_cases forms these in int64: seconds from order 1024 on
        out += [jc.hadamard(n, "b"), jc.hadamard(n, "r1"), jc.skew(n, "b")]
    if 16 <= n < 1024:
        out.append(jc.deficient(n, 7))
    return out


# ------------------------------------------------------------------------------------- the model
def reference_reduction(a, drop_wv_at=None, stale_y_at=None):
    """Householder tridiagonalisation of the symmetric ``a`` in the device's convention, plain fp64 NumPy, one column
    at a time: returns (Vh [n, n], tau, d, e).  The two arguments plant what a kernel could get wrong: at that column
    the rank-2 update leaves out its ``w v^T`` term / is applied with the previous column's ``y = A v``."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    vh, tau, d, e = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
    y_prev = None
    for j in range(n - 1):
        d[j] = a[j, j]
        x = a[j + 1:, j].copy()
        alpha, sigma = x[0], float(x[1:] @ x[1:])
        v = np.zeros(n - j - 1)
        v[0] = 1.0
        if sigma == 0.0:
            e[j] = alpha
        else:
            nrm = np.sqrt(alpha * alpha + sigma)
            beta = -nrm if alpha >= 0.0 else nrm
            tau[j] = (beta - alpha) / beta
            v[1:] = x[1:] / (alpha - beta)
            e[j] = beta
        vh[j, j + 1:] = v
        if tau[j] == 0.0:        # H = I: w is zero and the update subtracts zeros
            y_prev = None
            continue
        sub = a[j + 1:, j + 1:]
        y = sub @ v
        use = y_prev[1:] if (stale_y_at == j and y_prev is not None) else y
        w = tau[j] * use - (0.5 * tau[j] * tau[j] * float(use @ v)) * v
        sub -= np.outer(v, w)
        if drop_wv_at != j:
            sub -= np.outer(w, v)
        y_prev = y
    d[n - 1] = a[n - 1, n - 1]
    return vh, tau, d, e


def lapack_reduction(a):
    """scipy.linalg.lapack.dsytrd(lower=1) in the same storage."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    if n == 1:
        return np.zeros((1, 1)), np.zeros(1), np.array([a[0, 0]]), np.zeros(1)
    c, d, e, tau, info = scipy.linalg.lapack.dsytrd(a, lower=1)
    assert info == 0
    vh = np.zeros((n, n))
    for j in range(n - 1):
        vh[j, j + 1] = 1.0
        vh[j, j + 2:] = c[j + 2:, j]
    return vh, np.concatenate([tau, [0.0]]), d.copy(), np.concatenate([e, [0.0]])


def accumulate_q(vh, tau, n):
    """Q = H_0 ... H_{n-2} from the rows of ``vh`` as they are stored (all n entries of a row enter), in blocks of
    WY reflectors: H_a ... H_{b-1} = I - V T V^T with T from LAPACK's dlarft recurrence, applied from the last block."""
    q = np.eye(n)
    starts = list(range(0, max(n - 1, 0), WY))
    for a in reversed(starts):
        b = min(a + WY, n - 1)
        v = np.ascontiguousarray(vh[a:b, :n].T)            # n x m
        m = b - a
        vtv = v.T @ v
        t = np.zeros((m, m))
        for i in range(m):
            t[i, i] = tau[a + i]
            if i:
                t[:i, i] = -tau[a + i] * (t[:i, :i] @ vtv[:i, i])
        q -= v @ (t @ (v.T @ q))
    return q


def tridiagonal_of(d, e, n):
    t = np.diag(d[:n])
    if n > 1:
        t += np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
    return t


def eig_tridiagonal(d, e, n):
    """Eigenvalues of T, descending."""
    if n == 1:
        return np.array([d[0]], dtype=np.float64)
    return scipy.linalg.eigvalsh_tridiagonal(np.asarray(d[:n], dtype=np.float64), np.asarray(e[:n - 1], dtype=np.float64))[::-1].copy()


def _rel(err, bar):
    err = float(err)
    return 0.0 if err == 0.0 else (np.inf if bar == 0.0 or not np.isfinite(err) else err / bar)


def shape_items(vh, tau, d, e, n, lda, two_stage=False):
    """The exact items that fail, by name."""
    vh, tau, d, e = np.asarray(vh), np.asarray(tau), np.asarray(d), np.asarray(e)
    bad = []
    if not (np.all(np.isfinite(d[:n])) and np.all(np.isfinite(e[:n])) and np.all(np.isfinite(tau[:n]))):
        bad.append("finite")
    if not e[n - 1] == 0.0:
        bad.append("e[n-1]")
    if two_stage:
        return bad
    if not np.all(np.isfinite(vh[:n, :lda])):
        bad.append("finite Vh")
    if not tau[n - 1] == 0.0:
        bad.append("tau[n-1]")
    if not np.all((tau[:n] == 0.0) | ((tau[:n] >= 1.0) & (tau[:n] <= 2.0))):
        bad.append("tau range")
    if not np.all(vh[n - 1, :lda] == 0.0):
        bad.append("row n-1")
    body = vh[:n - 1, :lda]
    if np.any(np.tril(body[:, :n]) != 0.0):
        bad.append("zeros up to j")
    if np.any(body[:, n:] != 0.0):
        bad.append("zeros from n")
    j = np.arange(n - 1)
    one = body[j, j + 1]
    live = tau[:n - 1] != 0.0
    if np.any(one[live] != 1.0):
        bad.append("one")
    idle = np.nonzero(~live)[0]         # tau == 0: e_{j+1} or zero
    if np.any((one[idle] != 1.0) & (one[idle] != 0.0)) or any(np.any(body[i, i + 2:n] != 0.0) for i in idle):
        bad.append("idle row")
    return bad


def reduction_ratios(a, vh, tau, d, e, n, lda, lam=None, two_stage=False):
    """{'shape': failing exact items, 'orth' / 'similar' / 'spectrum': error / bar, 'tau_defect': the value}.
    ``a``: the symmetric matrix that was reduced; ``vh``: at least n rows of lda entries; ``lam``: the exact spectrum,
    descending (None: eigvalsh(a))."""
    a = np.asarray(a, dtype=np.float64)
    assert a.shape == (n, n) and vh.shape[0] >= n and vh.shape[1] == lda >= n
    if lam is None:
        lam = np.linalg.eigvalsh(a)[::-1]
    scale = float(np.abs(lam).max())
    out = {"shape": shape_items(vh, tau, d, e, n, lda, two_stage)}
    if any(item.startswith("finite") for item in out["shape"]):
        out.update(spectrum=np.inf) if two_stage else out.update(orth=np.inf, similar=np.inf, spectrum=np.inf)
        return out
    bar = E(n)
    out["spectrum"] = _rel(np.abs(eig_tridiagonal(d, e, n) - lam).max(), bar * scale)
    if two_stage:
        return out
    q = accumulate_q(vh, tau, n)
    out["orth"] = _rel(np.abs(q.T @ q - np.eye(n)).max(), bar)
    out["similar"] = _rel(np.abs(q.T @ a @ q - tridiagonal_of(d, e, n)).max(), bar * scale)
    live = np.nonzero(np.asarray(tau[:n]) != 0.0)[0]
    vv = np.einsum("ij,ij->i", vh[live, :n], vh[live, :n])
    out["tau_defect"] = float(np.abs(np.asarray(tau)[live] * vv - 2.0).max()) if live.size else 0.0
    return out


def failures_of(ratios, margin=1.0):
    return (["shape"] if ratios["shape"] else []) + \
        [k for k in ("orth", "similar", "spectrum") if k in ratios and not ratios[k] * margin <= 1.0]


def reduction_failures(a, vh, tau, d, e, n, lda, lam=None, two_stage=False, margin=1.0):
    """The names of the items that fail: of 'shape', 'orth', 'similar', 'spectrum'."""
    return failures_of(reduction_ratios(a, vh, tau, d, e, n, lda, lam, two_stage), margin)


def values_ratios(w, d, e, n, kv, scale=None):
    """Bisection against the device's own T: ``w`` the n entries of a member's eigenvalue buffer."""
    w = np.asarray(w)
    assert w.shape == (n,) and 1 <= kv <= n
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(d[:n])) and np.all(np.isfinite(e[:n]))):
        return {"values": np.inf, "order": np.inf, "tail": np.inf}
    mu = eig_tridiagonal(d, e, n)
    if scale is None:
        scale = float(np.abs(mu).max())
    return {"values": _rel(np.abs(w[:kv] - mu[:kv]).max(), E(n) * scale),
            "order": 0.0 if np.all(np.diff(w[:kv]) <= ORDER_SLACK * scale) else np.inf,
            "tail": 0.0 if np.all(w[kv:] == 0.0) else np.inf}


def values_failures(w, d, e, n, kv, scale=None, margin=1.0):
    return [k for k, r in values_ratios(w, d, e, n, kv, scale).items() if not r * margin <= 1.0]


def exact_failures(a, tau, d, e, n):
    """A tridiagonal ``a`` must come back as it is: d == diag, e == sub-diagonal, tau == 0, bit for bit."""
    bad = []
    if not np.array_equal(np.asarray(d[:n]), np.diag(a)):
        bad.append("d")
    if not np.array_equal(np.asarray(e[:n - 1]), np.diag(a, -1)):
        bad.append("e")
    if np.any(np.asarray(tau[:n]) != 0.0):
        bad.append("tau")
    return bad


def block_boundaries(n):
    """The columns j of ``blocks(n)`` whose sub-diagonal entry e[j] is exactly 0 (and whose tau[j] is 0)."""
    return np.arange(BLOCK - 1, n - 1, BLOCK)


# ------------------------------------------------------------------------------------- routes
# the kinds by the numbers of tests/eig_routes.py (this module imports no library)
COLUMNS, BAND2, BAND4, TEAM, BIG_TEAM, PANEL, PANEL_HYBRID = range(7)
K_NONE, K_TAGGED2, K_MEET2, K_SYM, K_TAGGED4, K_TAGGED8, K_BAND2, K_BAND4 = range(8)
TAIL_NONE, TAIL_REGS, TAIL_LDS = range(3)
REDUCE_NAMES = ("Columns", "Band2", "Band4", "Team", "BigTeam", "Panel", "PanelHybrid")
KERNEL_NAMES = ("none", "tagged2", "meet2", "sym", "tagged4", "tagged8", "band2", "band4")
TAIL_NAMES = ("no tail", "tail regs", "tail lds")
SWITCHES = ("NDMPS_TRD_BAND", "NDMPS_TRD_SYM", "NDMPS_TRD_NO_TEAM", "NDMPS_TRD_TEAM_MAX", "NDMPS_TRD_NO_HYBRID",
            "NDMPS_TRD_PANEL_MIN", "NDMPS_TRD_NO_PANEL", "NDMPS_TRD_PANEL_GRAPH", "NDMPS_TRD_TEAM_NARROW",
            "NDMPS_TRD_TEAM_WIDE", "NDMPS_TRD_TEAM_HALF", "NDMPS_TRD_XCD", "NDMPS_TRD_PAIR", "NDMPS_TRD_WIDE",
            "NDMPS_TRD_TAIL", "NDMPS_TEAM_FULL_TURN", "NDMPS_INVIT_DBG", "NDMPS_ORTHO_NARROW", "NDMPS_ORTHO_COLUMNS",
            "NDMPS_BACK_NARROW", "NDMPS_NO_SIDE_STREAM")
SYM_ORDERS = [512] * 6 + [500] * 4 + [480, 449, 384, 320, 257, 200, 137, 129, 96, 33]
PANEL_ENV = "NDMPS_TRD_TEAM_MAX=512 NDMPS_TRD_PANEL_MIN=513"
SLOTS = 512       # resident workgroups of the kernels with 2 and 4 rows per thread on the MI355X (eig_routes.MI355X_TEAM_SLOTS)


def _phase1(reduce, handover=0, kernel=0, team_order=0, team_size=0, per_launch=0, lds=0, xcd=0, pair=0, half_turn=0,
            col_width=0, col_rows=0, col_launches=0, tail_cols=0, tail_lower=0, tail=TAIL_REGS, graph=0):
    return dict(reduce=reduce, handover=handover, kernel=kernel, team_order=team_order, team_size=team_size,
                per_launch=per_launch, lds=lds, xcd=xcd, pair=pair, half_turn=half_turn, col_width=col_width,
                col_rows=col_rows, col_launches=col_launches, tail_cols=tail_cols, tail_lower=tail_lower, tail=tail,
                graph=graph)


def _pair(size):
    return int(32 % size == 0 or size % 32 == 0)


def _narrow(n, half_turn=1, **kw):   # 8-column tagged blocks, placed XCD by XCD
    size = -(-n // 8)
    return _phase1(TEAM, kernel=K_TAGGED2, team_order=n, team_size=size, per_launch=SLOTS // size, lds=16384,
                   **{**dict(xcd=1, pair=_pair(size), half_turn=half_turn), **kw})


def _blocks32(n, half_turn=1, **kw):   # 32-column blocks that meet at a counter
    size = -(-n // 32)
    return _phase1(TEAM, kernel=K_MEET2, team_order=n, team_size=size, per_launch=SLOTS // size, lds=16384, xcd=1,
                   pair=_pair(size), half_turn=half_turn, **kw)


def _big(n, per_launch, reduce=BIG_TEAM, **kw):   # 8-column tagged blocks, 4 or 8 rows per thread, 2-D grid, whole turn
    rows8 = n > 1024
    return _phase1(reduce, kernel=K_TAGGED8 if rows8 else K_TAGGED4, team_order=n, team_size=-(-n // 8),
                   per_launch=per_launch, lds=65536 if rows8 else 32768, **kw)


def _columns(n, width, rows, **kw):
    return _phase1(COLUMNS, col_width=width, col_rows=rows, col_launches=max(n - 128, 0), **kw)


_PANEL = _phase1(PANEL, tail_cols=128, tail_lower=1)
_HYBRID512 = _phase1(PANEL_HYBRID, handover=512, kernel=K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
                     xcd=1, pair=1, half_turn=1, tail_cols=512)
_SYM = _phase1(TEAM, kernel=K_SYM, team_order=512, team_size=8, per_launch=64, xcd=1, half_turn=1, tail_lower=1,
               tail=TAIL_LDS)


def _row(orders, want, env="", team=1, streamed=0, full=False, straddle=False, same_as=None, recover=False):
    """``full``: the row that runs every case on its kernel; ``same_as``: the id of the row whose Vh, tau, d, e this
    row must reproduce bit for bit (placement-only switches, the cached graph); ``recover``: the resident launch is
    replaced by an aborted one and the reduction redone by ndmps_syevd_topk_recover_f64 -- ``want`` is the redone plan."""
    return dict(orders=tuple(orders), want=want, env=env, team=team, streamed=streamed, full=full, straddle=straddle,
                same_as=same_as, recover=recover)


ROUTES = [
    # the tail alone (orders up to 128), in registers and in LDS
    _row([1], _columns(1, 8, 2)),
    _row([2], _columns(2, 8, 2)),
    _row([3], _columns(3, 8, 2)),
    _row([128], _columns(128, 8, 2), full=True),
    _row([128] * 16, _columns(128, 8, 2, tail=TAIL_LDS), full=True),
    _row([5, 128, 64], _columns(128, 8, 2, tail=TAIL_LDS), env="NDMPS_TRD_TAIL=lds"),
    # Team: 8-column tagged blocks with 2 rows per thread
    _row([129], _narrow(129)),
    _row([130], _narrow(130)),
    _row([136], _narrow(136)),
    _row([257], _narrow(257), full=True),
    _row([300], _narrow(300), straddle=True),
    _row([512], _narrow(512)),
    _row([512, 40, 300, 129], _narrow(512)),
    _row([130] * 16, _narrow(130, half_turn=0, tail=TAIL_LDS)),
    _row([260], _narrow(260)),
    _row([260], _narrow(260, xcd=0, pair=0), env="NDMPS_TRD_XCD=0", same_as="260"),
    _row([260], _narrow(260, pair=0), env="NDMPS_TRD_PAIR=0", same_as="260"),
    _row([260], _narrow(260, half_turn=0), env="NDMPS_TEAM_FULL_TURN=1", same_as="260"),
    _row([260], _narrow(260), env="NDMPS_TRD_TEAM_HALF=1", same_as="260"),
    # Team: 32-column blocks that meet at a counter
    _row([260], _blocks32(260), env="NDMPS_TRD_TEAM_WIDE=1", full=True),
    _row([512], _blocks32(512), env="NDMPS_TRD_TEAM_WIDE=1"),
    _row([512] * 5, _blocks32(512), streamed=1),
    # Team: half storage
    _row(SYM_ORDERS, _SYM, env="NDMPS_TRD_SYM=1", full=True),
    # two-stage
    _row([260] * 3, _phase1(BAND2, kernel=K_BAND2, team_order=260, team_size=9, per_launch=56, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=2", full=True),
    _row([512], _phase1(BAND2, kernel=K_BAND2, team_order=512, team_size=16, per_launch=32, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=2"),
    _row([512, 384, 200, 137], _phase1(BAND2, kernel=K_BAND2, team_order=512, team_size=16, per_launch=32, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=2"),
    _row([260] * 3, _phase1(BAND4, kernel=K_BAND4, team_order=260, team_size=9, per_launch=56, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=4", full=True),
    _row([512], _phase1(BAND4, kernel=K_BAND4, team_order=512, team_size=16, per_launch=32, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=4"),
    _row([512, 384, 200, 137], _phase1(BAND4, kernel=K_BAND4, team_order=512, team_size=16, per_launch=32, tail=TAIL_NONE),
         env="NDMPS_TRD_BAND=4"),
    # BigTeam: 4 and 8 rows per thread
    _row([513], _big(513, 7), full=True),
    _row([777], _big(777, 5)),
    _row([1024], _big(1024, 4), straddle=True),
    _row([1025], _big(1025, 1), full=True),
    _row([1024, 600, 100, 1000], _big(1024, 4)),
    # panels, and panels with the resident kernel behind them
    _row([576], _HYBRID512, env=PANEL_ENV, full=True),
    _row([640], _HYBRID512, env=PANEL_ENV),
    _row([574], _PANEL, env=PANEL_ENV, full=True),
    _row([641], _PANEL, env=PANEL_ENV),
    _row([640], _PANEL, env=PANEL_ENV + " NDMPS_TRD_NO_HYBRID=1"),
    _row([640], dict(_PANEL, graph=1), env=PANEL_ENV + " NDMPS_TRD_NO_HYBRID=1 NDMPS_TRD_PANEL_GRAPH=1",
         same_as="640-TEAM_MAX=512+PANEL_MIN=513+NO_HYBRID"),
    _row([1100, 777], _PANEL, env=PANEL_ENV),
    _row([1100], _big(1024, 4, reduce=PANEL_HYBRID, handover=1024, tail_cols=1024),
         env="NDMPS_TRD_TEAM_MAX=1024 NDMPS_TRD_PANEL_MIN=513"),
    _row([1536], _PANEL, team=0),
    # one launch per column
    _row([260], _columns(260, 8, 2), env="NDMPS_TRD_NO_TEAM=1", full=True),
    _row([512], _columns(512, 32, 2), env="NDMPS_TRD_WIDE=1", team=0),
    _row([513], _columns(513, 8, 4), team=0),
    _row([1025], _columns(1025, 8, 8), team=0),
    _row([2049], _columns(2049, 8, 16), env="NDMPS_TRD_NO_PANEL=1", team=0),
    # recovery: the redone reduction in the same workspace
    _row([260], _columns(260, 8, 2), recover=True),
    _row([640], _PANEL, env=PANEL_ENV, recover=True),
]


def route_id(row):
    name = "x".join(str(n) for n in row["orders"]) if len(row["orders"]) <= 4 else \
        f"{len(row['orders'])}of{max(row['orders'])}"
    if len(set(row["orders"])) == 1 and len(row["orders"]) > 1:
        name = f"{row['orders'][0]}x{len(row['orders'])}"
    env = row["env"].replace("NDMPS_TRD_", "").replace("NDMPS_", "").replace("=1", "").replace(" ", "+")
    return name + ("-" + env if env else "") + ("-team0" if not row["team"] else "") + \
        ("-streamed" if row["streamed"] else "") + ("-recover" if row["recover"] else "")


def kernel_name(row):
    w = row["want"]
    extra = f" {w['col_width']}x{w['col_rows']}" if w["reduce"] == COLUMNS and w["col_launches"] else ""
    if w["reduce"] == COLUMNS and not w["col_launches"]:
        return TAIL_NAMES[w["tail"]] + " alone"
    return f"{REDUCE_NAMES[w['reduce']]} / {KERNEL_NAMES[w['kernel']]}{extra} / {TAIL_NAMES[w['tail']]}"


def two_stage(row):
    return row["want"]["reduce"] in (BAND2, BAND4)


def k_max_of(row):
    return min(max(row["orders"]), 128)


def row_cases(row):
    """The batches a row is run on, as lists of members.  A single order: one call per case -- ``simple_case`` and
    hadamard a, every case of ``extras`` on a ``full`` row, ``straddle`` where the row says so; order 2049 runs the one
    graded case.  A batch: one call, every member another case (a ``full`` batch walks through ``extras`` as well)."""
    orders = row["orders"]
    if len(orders) == 1:
        n = orders[0]
        if n > 2048:
            return [[simple_case(n)]]
        calls = [[simple_case(n)], [tc.hadamard_a(n)]]
        if row["full"]:
            calls += [[c] for c in extras(n)]
        if row["straddle"]:
            calls.append([tc.straddle(n)])
        return calls
    members, seen = [], {}
    for pos, n in enumerate(orders):
        first, i = seen.setdefault(n, (pos, 0))
        seen[n] = (first, i + 1)
        pool = [simple_case(n, 0), tc.hadamard_a(n)] + (extras(n) if row["full"] else [arrow(n), rank1(n), tridiag(n)])
        pool += [jc.graded(n, 10 + t) for t in range(max(orders.count(n) - len(pool), 0))]
        members.append(pool[(first + i) % len(pool)])    # an order's members walk the pool from where the order starts
    assert len({c.name for c in members}) == len(members)
    return [members]


def all_cases():
    seen = {}
    for row in ROUTES:
        for members in row_cases(row):
            for c in members:
                seen[c.name] = c
    return list(seen.values())
