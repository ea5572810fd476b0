"""The direct top-k eigen-solver (csrc/eig_tridiag.hip) held to exact cases: the families of tests/jacobi_cases.py,
a block-straddling family, the bars for a truncated result, a model of the device-side rank decision and the table of
phase-2 routes.  Shared by tests/test_topk_cases_host.py (CPU: every claim below holds, LAPACK truncated to k passes
every bar with a margin of 10, every bar rejects the fault it exists for, the route table is what trd_route plans) and
tests/test_gpu_topk_exact.py (the kernels).  NumPy, SciPy and mpmath only: no torch, no device.

Families: ``diag``, ``hadamard`` a / b / r1, ``laplace``, ``deficient``, ``graded`` and ``skew`` are those of
jacobi_cases, by import.  ``straddle`` is new: ``H diag(lam) H^T / m`` like ``hadamard``, with the leading spectrum

    12 x 24, 11 x 30, 10 x 20, 9 x 40, 8 x 28          (clusters end at columns 24, 54, 74, 114, 142)

so that an exact multiplicity crosses every multiple of 16 up to 128, in particular columns 16, 32, 64 (the column
blocks of the inverse iteration from order 1024 on, and the 64-column blocks of the one-workgroup
orthonormalisation), the rank boundaries k = 100 and k = 128, and leaves 3, 2, 1, 0 in four large clusters behind.
Exact eigenvectors are known for ``hadamard``, ``straddle``, ``skew`` and ``diag`` (columns of H and unit vectors under
the permutation): ``vectors_of`` returns them and the host suite verifies them against the matrix.

Bars for a truncated result: ``w`` holds the leading ``kv = min(k_max, n)`` eigenvalues and zeros behind, ``V`` the
leading ``k`` columns.  ``E(n) = 2e-15 max(n, 50)``, ``scale = max |lambda|``, ``f`` the factor of the regime:

  order     w[:kv] non-increasing up to 1e-15 scale (what tests/test_gpu_parity.py::_check_topk grants)
  values    |w[:kv] - lambda[:kv]| <= f E scale
  tail      w[kv:] == 0 exactly
  orth      |V^T V - I| <= f E
  resid     |S V - V diag(w[:k])| <= f E scale
  sign      the entry of largest magnitude of every column (first index on ties) is positive
  vectors   laplace only: min over the sign of |v_j -+ v_j^exact|_max <= f E scale / gap_j
  subspace  cases with known vectors: for every exact cluster wholly inside the k kept columns,
            |V_c V_c^T - P_c^exact|_max <= f E scale / gap_c

``f`` is what tests/test_gpu_parity.py already grants: 1 for simple spectra (laplace, graded), 4 for degenerate ones,
8 for 65 .. 128 vectors of a degenerate spectrum (``factor``).  Nothing here uses a larger one.

Rank model: ``rank_exact`` is the rule of ndmps_syevd_topk_vectors_auto_f64 on the exact spectrum, ``rank_from`` the
same on the device's own w (no fast-math in the build: it must reproduce d_ranks exactly).  ``admitted`` is the guard:
a (case, cutoff) pair is used only if ``cutoff^2 lambda_0`` is at least ``100 E scale`` away from every exact
eigenvalue, so the solver's rounding cannot move the rank.  ``auto_failures`` is the whole contract of the auto entry
for one member -- rank, kept and fill columns, write extents of V and of the spectra -- over buffers that held a
sentinel: the GPU driver calls it, the host suite plants the faults it must report.
"""
import functools

import numpy as np
import scipy.linalg

import jacobi_cases as jc
import mpmath
from jacobi_cases import (Case, E, SENTINEL, diag, diag_expected, gaps, graded, hadamard,  # noqa: F401
                          laplace, sign_normalise, skew)

MAX_K = 128                      # ndmps_syevd_topk_max_k(): the most vectors_auto takes
LAPLACE_MAX = jc.LAPLACE_MAX
DEFICIENT_L, DEFICIENT_R = (64, 130, 512, 1024), (1, 7, 40)
STRADDLE_HEAD = ((12, 24), (11, 30), (10, 20), (9, 40), (8, 28))
STRADDLE_ENDS = (24, 54, 74, 114, 142)
ORDER_SLACK = 1e-15


# ------------------------------------------------------------------------------------- deficient
@functools.lru_cache(maxsize=None)
def deficient(l, r):
    """``deficient`` of jacobi_cases; at order 1024 the same construction with the integer products formed in float64
    (every partial sum is an integer below 2**53: exact in any order; the int64 products take most of a minute there)."""
    if l < 1024:
        return jc.deficient(l, r)
    rng = jc._rng("deficient", l, r)
    while True:
        x = rng.integers(-2, 3, size=(2 * l, r)).astype(np.float64)
        y = rng.integers(-2, 3, size=(r, l)).astype(np.float64)
        m, yy = x.T @ x, y @ y.T
        if np.linalg.matrix_rank(m) == r and np.linalg.matrix_rank(yy) == r:
            break
    s = x @ y
    g = s.T @ s
    with mpmath.workdps(40):
        low = mpmath.cholesky(mpmath.matrix(m.astype(np.int64).tolist()))
        small = low.T * mpmath.matrix(yy.astype(np.int64).tolist()) * low
        small = (small + small.T) / 2
        top = sorted((float(v) for v in mpmath.eigsy(small, eigvals_only=True)), reverse=True)
    return Case(f"deficient-{l}-{r}", "deficient", g, g, np.concatenate([np.array(top), np.zeros(l - r)]), rank=r)


# ------------------------------------------------------------------------------------- straddle
@functools.lru_cache(maxsize=None)
def straddle(n):
    """Order 1024 (m = 1024) and order 300 (m = 256 and 44 diagonal entries from 0 .. 3)."""
    rng = jc._rng("straddle", n)
    m = jc.hadamard_m(n)
    head = np.concatenate([np.full(c, v) for v, c in STRADDLE_HEAD])
    assert m > head.size + 16
    rest = m - head.size
    tail = np.concatenate([np.full(rest - 3 * (rest // 4), 0)] + [np.full(rest // 4, v) for v in (1, 2, 3)])
    lam = np.concatenate([head, tail]).astype(np.int64)
    rng.shuffle(lam)
    return _build(f"straddle-{n}", "straddle", n, lam, rng.integers(0, 4, size=n - m), rng)


def _build(name, family, n, lam, extra, rng):
    """``H diag(lam) H^T / m`` summed directly with ``diag(extra)`` and permuted, with its exact eigenvectors.  The
    products run in float64: every partial sum is an integer below 2**53, so they are exact in any order."""
    m = lam.size
    h = scipy.linalg.hadamard(m).astype(np.float64)
    a = np.zeros((n, n))
    a[:m, :m] = ((h * lam[None, :].astype(np.float64)) @ h.T) / m
    a[np.arange(m, n), np.arange(m, n)] = extra
    basis = np.zeros((n, n))
    basis[:m, :m] = h / np.sqrt(m)
    basis[np.arange(m, n), np.arange(m, n)] = 1.0
    full = np.concatenate([lam, extra]).astype(np.float64)
    g, p = jc._perm_sym(a, rng)
    order = np.argsort(-full, kind="stable")
    return Case(name, family, g, g, full[order].copy(), vec=np.ascontiguousarray(basis[p][:, order]),
                indefinite=bool((full < 0).any()))


@functools.lru_cache(maxsize=None)
def hadamard_a(n):
    """``hadamard`` a of jacobi_cases; from order 1024 on a member with the same kind of spectrum built by ``_build``
    (jacobi_cases forms the product in int64, minutes at order 2048)."""
    if n < 1024:
        return hadamard(n, "a")
    rng = jc._rng("hadamard-a-big", n)
    m = jc.hadamard_m(n)
    lam = jc._hadamard_spectrum(m, "a", rng)
    rng.shuffle(lam)
    return _build(f"hadamard-A-{n}", "hadamard", n, lam, rng.integers(0, 6, size=n - m), rng)


def vectors_of(case):
    """An exact orthonormal eigenbasis, column j for lam[j], or None.  Inside a cluster any basis of it."""
    if case.vec is not None:
        return case.vec
    if case.family == "diag":
        return diag_expected(case)[1]
    return None


def clusters(lam):
    """[(first, end, gap)] of the runs of equal exact eigenvalues; gap: distance to the nearest other eigenvalue."""
    out, a = [], 0
    for b in range(1, lam.size + 1):
        if b == lam.size or lam[b] != lam[a]:
            near = [abs(lam[a] - lam[a - 1])] if a > 0 else []
            near += [abs(lam[b] - lam[a])] if b < lam.size else []
            out.append((a, b, min(near) if near else np.inf))
            a = b
    return out


SIMPLE = ("laplace", "graded")


def factor(case, k):
    """The factor over E that tests/test_gpu_parity.py grants the regime of (case, k kept vectors)."""
    if case.family in SIMPLE:
        return 1.0
    return 8.0 if 65 <= k <= 128 else 4.0


# ------------------------------------------------------------------------------------- bars
def ratios(case, w, v, k_max):
    """error / bar for every bar that applies.  ``w``: the n entries of the eigenvalue buffer; ``v``: V[:, :k]."""
    n, scale = case.n, case.scale
    k, kv = v.shape[1], min(k_max, n)
    assert w.shape == (n,) and v.shape[0] == n and 1 <= k <= kv
    f = factor(case, k)
    e = f * E(n)
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(v))):
        return {"finite": np.inf}

    def rel(err, bar):
        return 0.0 if err == 0.0 else (np.inf if bar == 0.0 else float(err / bar))

    out = {"order": 0.0 if np.all(np.diff(w[:kv]) <= ORDER_SLACK * scale) else np.inf,
           "values": rel(np.abs(w[:kv] - case.lam[:kv]).max(), e * scale),
           "tail": 0.0 if np.all(w[kv:] == 0.0) else np.inf,
           "orth": rel(np.abs(v.T @ v - np.eye(k)).max(), e),
           "resid": rel(np.abs(case.S @ v - v * w[None, :k]).max(), e * scale)}
    top = v[np.argmax(np.abs(v), axis=0), np.arange(k)]
    out["sign"] = 0.0 if np.all(top > 0) else np.inf
    exact = vectors_of(case)
    if case.family == "laplace":
        err = np.minimum(np.abs(v - exact[:, :k]).max(axis=0), np.abs(v + exact[:, :k]).max(axis=0))
        gap = gaps(case.lam)[:k]
        gap = np.where(np.isinf(gap), 0.0, gap)
        out["vectors"] = float((err * gap / (e * scale)).max()) if scale > 0 else 0.0
    elif exact is not None:
        worst = 0.0
        for a, b, gap in clusters(case.lam):
            if b > k:
                break
            p = exact[:, a:b] @ exact[:, a:b].T
            err = np.abs(v[:, a:b] @ v[:, a:b].T - p).max()
            worst = max(worst, 0.0 if np.isinf(gap) and err == 0.0 else rel(err, e * scale / gap if not np.isinf(gap) else e))
        out["subspace"] = worst
    return out


def failures(case, w, v, k_max, margin=1.0):
    return {name: r for name, r in ratios(case, w, v, k_max).items() if not r * margin <= 1.0}


def lapack_topk(case, k, k_max, full=None):
    """np.linalg.eigh of the symmetric part (``full``: a jacobi_cases.lapack result at hand), truncated as the solver
    delivers: (w with zeros behind kv, V[:, :k])."""
    w, v = full if full is not None else jc.lapack(case)
    out = np.zeros(case.n)
    kv = min(k_max, case.n)
    out[:kv] = w[:kv]
    return out, v[:, :k].copy()


# ------------------------------------------------------------------------------------- rank model
def rank_exact(lam, cutoff, k_cap):
    """#{i < min(k_cap, n): sqrt(max(lam_i, 0)) > cutoff sqrt(max(lam_0, 0))}, at least 1."""
    kk = min(k_cap, lam.size)
    s = np.sqrt(np.maximum(lam[:kk], 0.0))
    return int(min(max(int((s > cutoff * s[0]).sum()), 1), kk))


def rank_from(w, cutoff, k_cap):
    """The device's decision recomputed from the device's own eigenvalues ``w`` (the n entries of a member)."""
    kk = min(k_cap, w.size)
    s = np.sqrt(np.maximum(w[:kk], 0.0))
    return int(min(max(int((s > cutoff * s[0]).sum()), 1), kk))


def spectra_from(w, k_cap):
    return np.sqrt(np.maximum(w[:min(k_cap, w.size)], 0.0))


def auto_failures(w, block, rank, spectra, cutoff, k_cap, exact=None, sentinel=SENTINEL):
    """What ndmps_syevd_topk_vectors_auto_f64 left for one member, against its contract; returns the failing items.

    ``w``: the member's n eigenvalues from the device; ``block``: its n x n block of V, pre-filled with ``sentinel``;
    ``rank``: its entry of d_ranks; ``spectra``: its whole stride of d_spectra, pre-filled with ``sentinel`` (None: the
    call was given no d_spectra); ``exact``: ``rank_exact`` where the guard admits the cutoff.  With
    ``kk = min(k_cap, n)``:

      range           1 <= rank <= kk
      rank            rank == rank_from(w, cutoff, k_cap)
      rank_exact      rank == exact
      kept            no entry of the columns [0, rank) still holds the sentinel
      fill            the columns [rank, kk) are exactly 0.0
      extent          the columns [kk, n) still hold the sentinel
      spectra         spectra[:kk] == sqrt(max(w[:kk], 0)) bit for bit
      spectra_extent  spectra[kk:] still holds the sentinel
    """
    n = w.size
    assert block.shape == (n, n)
    kk = min(k_cap, n)
    rank = int(rank)
    bad = []
    if not 1 <= rank <= kk:
        bad.append("range")
    if rank != rank_from(w, cutoff, k_cap):
        bad.append("rank")
    if exact is not None and rank != exact:
        bad.append("rank_exact")
    k = min(max(rank, 0), kk)
    if np.any(block[:, :k] == sentinel):
        bad.append("kept")
    if not np.all(block[:, k:kk] == 0.0):
        bad.append("fill")
    if not np.all(block[:, kk:] == sentinel):
        bad.append("extent")
    if spectra is not None:
        if not np.array_equal(spectra[:kk], spectra_from(w, k_cap)):
            bad.append("spectra")
        if not np.all(spectra[kk:] == sentinel):
            bad.append("spectra_extent")
    return bad


def guard_distance(case, cutoff):
    """Distance of cutoff^2 lambda_0 to the nearest exact eigenvalue over its least admissible value."""
    thr = cutoff * cutoff * max(case.lam[0], 0.0)
    return float(np.abs(case.lam - thr).min() / (100 * E(case.n) * case.scale)) if case.scale > 0 else np.inf


def admitted(case, cutoff):
    return guard_distance(case, cutoff) >= 1.0


def cutoff_keeping(case, j):
    """A cutoff in the middle of the gap behind the j-th eigenvalue: the rule keeps exactly j (before the cap)."""
    assert 1 <= j < case.n and case.lam[j - 1] > case.lam[j] and case.lam[j - 1] > 0
    return float(np.sqrt(0.5 * (case.lam[j - 1] + max(case.lam[j], 0.0)) / case.lam[0]))


def auto_cutoff(case):
    """The cutoff the GPU suite pairs with ``case``: in a wide gap of its spectrum, about 1e-3 for ``deficient``."""
    lam = case.lam
    if case.family == "deficient":
        return 1e-3
    if case.family in ("hadamard", "straddle", "skew", "diag"):
        pos = np.unique(lam[lam > 0])
        j = int((lam >= pos[0]).sum()) if pos.size < 3 else int((lam >= pos[pos.size // 2]).sum())
        return cutoff_keeping(case, j) if j < case.n else 0.05
    if case.family == "laplace":
        return cutoff_keeping(case, max(case.n // 3, 1)) if case.n > 1 else 0.5
    # graded: the widest relative gap among the leading quarter
    q = max(case.n // 4, 2)
    j = 1 + int(np.argmax(lam[:q - 1] / lam[1:q]))
    return cutoff_keeping(case, j)


def common_cutoff(cases):
    """One cutoff for a batch: the first of the members' own and of a fixed ladder that every member admits."""
    for cutoff in [auto_cutoff(c) for c in cases if c.family not in SIMPLE] + [auto_cutoff(c) for c in cases] + \
            [0.3, 0.1, 0.03, 0.01]:
        if all(admitted(c, cutoff) for c in cases):
            return cutoff
    raise AssertionError("no common cutoff")


def deficient_cases():
    return [deficient(l, r) for l in DEFICIENT_L for r in DEFICIENT_R]


# ------------------------------------------------------------------------------------- routes
# ortho / back by the numbers of tests/eig_routes.py (this module imports no library)
WIDE_AUTO, WIDE, SMALL, BLOCKS, COLUMNS = range(5)
LANES, ROWS, BACK_WIDE = range(3)
LANE_CLASSES = ((32, 4), (32, 8), (32, 16), (32, 32), (64, 32), (64, 64))
NARROW = "NDMPS_ORTHO_NARROW=1 NDMPS_BACK_NARROW=1"
SWITCHES = ("NDMPS_ORTHO_NARROW", "NDMPS_ORTHO_COLUMNS", "NDMPS_BACK_NARROW", "NDMPS_NO_SIDE_STREAM")


def _row(orders, k, env, ortho, back, lane_class, cb, t_factors=None):
    seg, r = LANE_CLASSES[lane_class] if lane_class is not None else (0, 0)
    if t_factors is None:
        t_factors = 0 if back == LANES else 2
    return dict(orders=tuple(orders), k=k, env=env, ortho=ortho, back=back, seg=seg, r=r, invit_cb=cb,
                t_factors=t_factors, lane_class=lane_class)


# the smallest orders that reach each phase-2 regime
ROUTES = [
    _row([40], 40, "", SMALL, LANES, 0, 128),
    _row([128], 64, "", SMALL, LANES, 0, 128),
    _row([129], 64, "", SMALL, LANES, 1, 128),
    _row([256], 64, "", SMALL, LANES, 1, 128),
    _row([257], 64, "", SMALL, LANES, 2, 128),
    _row([512], 64, "", SMALL, LANES, 2, 128),
    _row([513] * 3, 64, "", SMALL, LANES, 3, 128),
    _row([130], 65, "", BLOCKS, LANES, 1, 128),
    _row([130], 128, "", BLOCKS, LANES, 1, 128),
    _row([130], 65, "NDMPS_ORTHO_COLUMNS=1", COLUMNS, LANES, 1, 128),
    _row([130], 128, "NDMPS_ORTHO_COLUMNS=1", COLUMNS, LANES, 1, 128),
    _row([300], 128, "", BLOCKS, LANES, 2, 128),
    _row([300], 128, "NDMPS_ORTHO_COLUMNS=1", COLUMNS, LANES, 2, 128),
    _row([130], 130, "", WIDE, BACK_WIDE, None, 128),
    _row([260], 200, "", WIDE, BACK_WIDE, None, 128),
    _row([130], 130, "NDMPS_BACK_NARROW=1", WIDE, LANES, 1, 128),
    _row([260], 200, "NDMPS_BACK_NARROW=1", WIDE, LANES, 2, 128),
    _row([1024], 128, "", WIDE_AUTO, ROWS, None, 16),
    _row([1024], 100, "", WIDE_AUTO, ROWS, None, 16),
    _row([1024, 1024], 128, "", WIDE_AUTO, ROWS, None, 16),
    _row([1024, 1024], 100, "", WIDE_AUTO, ROWS, None, 16),
    _row([1024], 128, "NDMPS_NO_SIDE_STREAM=1", WIDE_AUTO, ROWS, None, 16, t_factors=1),
    _row([1024], 100, "NDMPS_NO_SIDE_STREAM=1", WIDE_AUTO, ROWS, None, 16, t_factors=1),
    _row([1024, 1024], 128, "NDMPS_NO_SIDE_STREAM=1", WIDE_AUTO, ROWS, None, 16, t_factors=1),
    _row([1024, 1024], 100, "NDMPS_NO_SIDE_STREAM=1", WIDE_AUTO, ROWS, None, 16, t_factors=1),
    _row([1024], 128, "NDMPS_ORTHO_NARROW=1", BLOCKS, LANES, 3, 16),
    _row([1024], 100, "NDMPS_ORTHO_NARROW=1", BLOCKS, LANES, 3, 16),
    _row([1024, 1024], 128, "NDMPS_ORTHO_NARROW=1", BLOCKS, LANES, 3, 16),
    _row([1024, 1024], 100, "NDMPS_ORTHO_NARROW=1", BLOCKS, LANES, 3, 16),
    _row([1024] * 3, 128, "", BLOCKS, LANES, 3, 16),
    _row([1025], 128, NARROW, BLOCKS, LANES, 4, 16),
    _row([2049], 128, NARROW, BLOCKS, LANES, 5, 16),
]
# the mixed batches of the write-extent tests (orders below k_cap), and the pair that takes the chip-wide route
MIXED = [
    _row([1024, 40, 7], 64, "", SMALL, LANES, 3, 16),
    _row([300, 130, 5], 128, "", BLOCKS, LANES, 2, 128),
    _row([1024, 40], 64, "", WIDE_AUTO, ROWS, None, 16),
]


def route_fields(row):
    return {f: row[f] for f in ("ortho", "back", "seg", "r", "invit_cb", "t_factors")}


def route_id(row):
    return "x".join(str(n) for n in row["orders"]) + f"-k{row['k']}" + ("-" + row["env"].replace("NDMPS_", "").replace("=1", "")
                                                                   .replace(" ", "+") if row["env"] else "")


def simple_case(n, tag=0):
    return laplace(n) if n <= LAPLACE_MAX else graded(n, tag)


def row_cases(row):
    """The members a route-table row is run on: [simple] and [hadamard a] for a single matrix; for a batch one call
    with simple, hadamard a, and a second simple member."""
    orders = row["orders"]
    if len(orders) == 1:
        return [[simple_case(orders[0])], [hadamard_a(orders[0])]]
    members = [simple_case(orders[0]), hadamard_a(orders[1])] + [simple_case(n, 1) for n in orders[2:]]
    return [members]


def mixed_cases(row):
    """The members of a MIXED row: the straddling or a Hadamard member first, small members of other families behind."""
    fams = {1024: straddle, 300: straddle, 130: hadamard_a, 40: laplace, 7: hadamard_a, 5: laplace}
    return [fams[n](n) for n in row["orders"]]


INDEFINITE_ORDERS = (17, 129, 513)


def indefinite_cases(n):
    return [hadamard(n, "b"), diag(n), skew(n, "b")]


def all_cases():
    seen = {}

    def add(c):
        seen[c.name] = c

    for row in ROUTES:
        for members in row_cases(row):
            for c in members:
                add(c)
    for row in MIXED:
        for c in mixed_cases(row):
            add(c)
    for n in INDEFINITE_ORDERS:
        for c in indefinite_cases(n):
            add(c)
    for c in deficient_cases() + [straddle(1024), straddle(300), graded(130), graded(1024), hadamard(129, "b"),
                                  diag(64, "zero"), diag(1), laplace(130), laplace(300)]:
        add(c)
    return list(seen.values())
