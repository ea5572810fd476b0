"""Symmetric matrices whose eigen-system is known without a solver, the regimes of the block Jacobi solver
(csrc/eig_block.hip) and the bars its results are held to.  Shared by tests/test_jacobi_cases_host.py (CPU: the claims
below hold, LAPACK passes every bar with a margin of 10, and every bar rejects the faults it exists for) and
tests/test_gpu_jacobi_exact.py (the kernels).  NumPy, SciPy and mpmath only: no torch, no device.

Families (``Case.family``), and why each is exact:

* ``diag``: a diagonal matrix with ties, negative entries and zeros in arbitrary order.  No rotation is active and
  every product is with an exact identity, so the result is known bit for bit: ``order = argsort(-d, stable)``,
  ``w = d[order]``, ``V[order[j], j] = 1`` and 0 elsewhere.  The zero matrix and ``c I`` are members.
* ``hadamard``: ``A = H diag(lam) H^T / m`` with the Sylvester Hadamard matrix of order ``m = 2**p`` and small integers
  ``lam``: every entry is an exact multiple of ``1 / m`` and the spectrum is exactly ``lam``.  ``A`` is summed directly
  with an integer diagonal block of size ``n - m`` and permuted symmetrically.  Spectra: ``a`` positive semi-definite
  with exact multiplicities and an exact null space, ``b`` the same but indefinite, ``r1`` rank one.
* ``laplace``: ``tridiag(-1, 2, -1)`` under a symmetric permutation; eigenvalues ``2 - 2 cos(k pi / (n + 1))`` and
  eigenvectors ``sqrt(2 / (n + 1)) sin(i k pi / (n + 1))`` from mpmath at 40 digits.  The eigenvalues are simple with
  known gaps, so the vectors themselves are compared.
* ``deficient``: ``G = S^T S`` with ``S = X Y`` of small integers, an exact integer matrix of exact rank ``r``, as the
  Gram pass of the sketches sends it.  ``l - r`` eigenvalues are exactly 0; the other ``r`` are those of the
  ``r x r`` matrix ``L^T (Y Y^T) L`` with ``X^T X = L L^T``, from mpmath at 40 digits.
* ``graded``: ``q (a^T a) q^T`` with ``a`` scaled by ``logspace(0, -5)``: dense and slowly converging; with ``gram`` the only
  family whose reference is LAPACK.
* ``gram``: ``a^T a`` with the columns of ``a`` scaled by ``logspace(0, -5)``, the very matrices (seed and all) on which
  tests/test_gpu_parity.py::test_block_jacobi_graded_spectrum asserts ``1 <= sweeps <= 20``: nearly diagonal where the
  eigenvalues are small.  They carry that bound through the new harness; reference LAPACK.  The bound has no
  derivation for a dense matrix and is not claimed there: the row-cyclic ``numpy_jacobi`` below, the method itself,
  needs 17, 20 and 22 sweeps on ``graded`` at orders 65, 129 and 257.
* ``skew``: ``G = S + K`` with ``S`` a ``hadamard`` member and ``K`` antisymmetric with entries that are multiples of
  1/4: ``0.5 (G + G^T) == S`` exactly, and the expected result is that of ``S``.

Bars.  ``E(n) = 2e-15 max(n, 50)`` is the project's constant for both eigen-solvers (tests/test_gpu_parity.py);
``scale = max |lambda_exact|``:

  order     w is non-increasing, exactly
  values    |w - lambda| <= E scale
  orth      |V^T V - I| <= E
  resid     |S v - v w| <= E scale
  sign      the entry of largest magnitude of every column (first index on ties, as np.argmax) is positive
  vectors   laplace only: min over the sign of |v_j -+ v_j^exact|_max <= E scale / gap_j
  exact     diag only: equality with the expected w and V

``ratios`` returns error / bar for each of them (0 or inf for the exact ones); a result passes when all are <= 1.
"""
import dataclasses
import functools
import zlib

import mpmath
import numpy as np
import scipy.linalg

# ------------------------------------------------------------------------------------- regimes
BS, PS = 16, 32                 # block size, pair size
HIST_MAX_NP = 896               # kHistMaxNp
WAVES8_MIN_NP, WAVES8_MAX_NP = 160, 672
MAX_SWEEPS = 40                 # kMaxSweepsBlock
BATCH_ORDERS = (24, 33, 128, 129, 672, 673, 896, 897)
SINGLE_ORDERS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 513)
LAPLACE_MAX = 300
DEFICIENT_L, DEFICIENT_R = (64, 130, 512), (1, 7, 40)
TINY_BATCH, TINY_MAX = 130, 24
GRAM_ORDERS = (5, 32, 40, 96, 512)      # the orders of test_block_jacobi_graded_spectrum
GRAM_SWEEPS = 20                        # the bound the existing tests state on these matrices
SENTINEL = -7.0


def np_of(n_max):
    """Order of the padded working matrices (block_layout)."""
    return max(-(-n_max // PS) * PS, PS)


def history(n_max, batch, env=None):
    """Whether the rotations are recorded and replayed (use_history); ``env`` is NDMPS_EIG_HISTORY as an int or None."""
    if np_of(n_max) > HIST_MAX_NP:
        return False
    return bool(env) if env is not None else batch >= 2


def replay_waves(np_):
    """Waves of the replay kernel blk_backacc_kernel at padded order ``np_``."""
    return 8 if WAVES8_MIN_NP <= np_ <= WAVES8_MAX_NP else 4


def E(n):
    return 2e-15 * max(n, 50)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    family: str
    G: np.ndarray                 # what the solver is given (not symmetric for ``skew``)
    S: np.ndarray                 # its symmetric part: the matrix that is decomposed
    lam: np.ndarray               # the spectrum, descending
    vec: np.ndarray = None        # laplace, hadamard, skew: exact eigenvectors, column j for lam[j] (any basis of a cluster)
    indefinite: bool = False
    rank: int = None              # deficient: the exact rank

    @property
    def n(self):
        return self.S.shape[0]

    @property
    def scale(self):
        return float(np.abs(self.lam).max())

    def __repr__(self):
        return self.name


def _perm_sym(a, rng):
    p = rng.permutation(a.shape[0])
    return np.ascontiguousarray(a[np.ix_(p, p)]), p


# ------------------------------------------------------------------------------------- diag
@functools.lru_cache(maxsize=None)
def diag(n, kind="mixed"):
    rng = _rng("diag", n, kind)
    if kind == "zero":
        d = np.zeros(n)
    elif kind == "cI":
        d = np.full(n, -2.5)
    else:
        d = rng.integers(-4, 5, size=n).astype(np.float64)    # ties, negatives and zeros
        if n >= 3:
            d[rng.permutation(n)[:3]] = (0.0, -4.0, 3.0)
    g = np.diag(d)
    return Case(f"diag-{kind}-{n}", "diag", g, g, np.sort(d)[::-1].copy(), indefinite=bool((d < 0).any()))


def diag_expected(case):
    d = np.diag(case.S)
    order = np.argsort(-d, kind="stable")
    v = np.zeros((case.n, case.n))
    v[order, np.arange(case.n)] = 1.0
    return d[order], v


# ------------------------------------------------------------------------------------- hadamard
def _hadamard_spectrum(m, spectrum, rng):
    if spectrum == "r1":
        lam = np.zeros(m, dtype=np.int64)
        lam[0] = 3
        return lam
    q = m // 4
    lo = 0 if spectrum == "a" else -3
    hi = 3 if spectrum == "a" else 5
    return np.concatenate([np.full(q, 5), np.full(q, 1), np.full(q, 0), rng.integers(lo, hi + 1, size=m - 3 * q)])


@functools.lru_cache(maxsize=None)
def hadamard(n, spectrum="a"):
    """``m`` is the largest power of two <= n.  An indefinite member is redrawn until ``max |a_ii| >= max |lambda| / 8``
    (the solver's thresholds are relative to the diagonal; only small orders ever need a second draw)."""
    rng = _rng("hadamard", n, spectrum)
    m = 1 << (int(n).bit_length() - 1)
    h = scipy.linalg.hadamard(m).astype(np.int64)
    for _ in range(1000):
        lam = _hadamard_spectrum(m, spectrum, rng)
        rng.shuffle(lam)
        if spectrum == "r1":
            extra = np.zeros(n - m, dtype=np.int64)
        else:
            extra = rng.integers(0 if spectrum == "a" else -3, 6, size=n - m)
        a = np.zeros((n, n))
        a[:m, :m] = ((h * lam[None, :]) @ h.T).astype(np.float64) / m      # integers below 2**53, then a power of two
        a[np.arange(m, n), np.arange(m, n)] = extra
        full = np.concatenate([lam, extra]).astype(np.float64)
        if spectrum != "b" or np.abs(np.diag(a)).max() >= np.abs(full).max() / 8:
            break
    else:
        raise AssertionError("no draw met the diagonal condition")
    g, p = _perm_sym(a, rng)
    basis = np.zeros((n, n))                  # the columns of H / sqrt(m), and unit vectors for the diagonal entries
    basis[:m, :m] = h / np.sqrt(m)
    basis[np.arange(m, n), np.arange(m, n)] = 1.0
    order = np.argsort(-full, kind="stable")
    return Case(f"hadamard-{spectrum}-{n}", "hadamard", g, g, full[order].copy(),
                vec=np.ascontiguousarray(basis[p][:, order]), indefinite=bool((full < 0).any()))


def hadamard_m(n):
    return 1 << (int(n).bit_length() - 1)


# ------------------------------------------------------------------------------------- laplace
@functools.lru_cache(maxsize=None)
def laplace(n):
    rng = _rng("laplace", n)
    t = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    g, p = _perm_sym(t, rng)
    with mpmath.workdps(40):
        # sin(i k pi / (n + 1)) depends on i k mod 2 (n + 1) only
        table = np.array([float(mpmath.sqrt(mpmath.mpf(2) / (n + 1)) * mpmath.sin(mpmath.pi * j / (n + 1)))
                          for j in range(2 * (n + 1))])
        lam = np.array([float(2 - 2 * mpmath.cos(mpmath.pi * k / (n + 1))) for k in range(n, 0, -1)])
    ks = np.arange(n, 0, -1)
    idx = np.arange(1, n + 1)
    vec = table[(idx[:, None] * ks[None, :]) % (2 * (n + 1))]
    return Case(f"laplace-{n}", "laplace", g, g, lam, vec=np.ascontiguousarray(vec[p]))


def gaps(lam):
    """Distance of every eigenvalue to its nearest neighbour."""
    if lam.size == 1:
        return np.array([np.inf])
    d = np.abs(np.diff(lam))
    return np.minimum(np.concatenate([[np.inf], d]), np.concatenate([d, [np.inf]]))


# ------------------------------------------------------------------------------------- deficient
@functools.lru_cache(maxsize=None)
def deficient(l, r):
    rng = _rng("deficient", l, r)
    rows = 2 * l
    while True:
        x = rng.integers(-2, 3, size=(rows, r))
        y = rng.integers(-2, 3, size=(r, l))
        m, yy = x.T @ x, y @ y.T
        if np.linalg.matrix_rank(m.astype(np.float64)) == r and np.linalg.matrix_rank(yy.astype(np.float64)) == r:
            break
    s = x @ y
    g = (s.T @ s).astype(np.float64)          # integers below rows (4 r)^2 < 2**53
    with mpmath.workdps(40):
        low = mpmath.cholesky(mpmath.matrix(m.tolist()))
        small = low.T * mpmath.matrix(yy.tolist()) * low
        small = (small + small.T) / 2
        top = sorted((float(v) for v in mpmath.eigsy(small, eigvals_only=True)), reverse=True)
    lam = np.concatenate([np.array(top), np.zeros(l - r)])
    return Case(f"deficient-{l}-{r}", "deficient", g, g, lam, rank=r)


# ------------------------------------------------------------------------------------- graded
@functools.lru_cache(maxsize=None)
def graded(n, tag=0):
    rng = _rng("graded", n, tag)
    a = rng.standard_normal((n + 9, n)) * np.logspace(0, -5, n)[None, :]
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    g = q @ (a.T @ a) @ q.T
    g = 0.5 * (g + g.T)
    return Case(f"graded-{n}-{tag}", "graded", g, g, np.linalg.eigvalsh(g)[::-1].copy())


@functools.lru_cache(maxsize=None)
def gram(n):
    """The matrix of tests/test_gpu_parity.py::test_block_jacobi_graded_spectrum at order ``n``, its seed included."""
    rng = np.random.default_rng(100 + n)
    a = rng.standard_normal((2 * n, n)) * np.logspace(0, -5, n)[None, :]
    g = a.T @ a
    s = 0.5 * (g + g.T)
    return Case(f"gram-{n}", "gram", g, s, np.linalg.eigvalsh(s)[::-1].copy())


# ------------------------------------------------------------------------------------- skew
@functools.lru_cache(maxsize=None)
def skew(n, spectrum="b"):
    base = hadamard(n, spectrum)
    rng = _rng("skew", n, spectrum)
    r = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    k = (r - r.T) / 4
    if n > 1 and not k.any():
        k[0, 1], k[1, 0] = 0.25, -0.25
    return Case(f"skew-{spectrum}-{n}", "skew", base.S + k, base.S, base.lam, vec=base.vec,
                indefinite=base.indefinite)


def outside_contract():
    """``J - I`` of order 40: ones with a zero diagonal, spectrum 39 once and -1 thirty-nine times.  Its diagonal is
    zero, so both of the solver's thresholds are 0: outside what the header promises."""
    g = np.ones((40, 40)) - np.eye(40)
    return Case("ones-minus-identity-40", "outside", g, g, np.concatenate([[39.0], np.full(39, -1.0)]), indefinite=True)


# ------------------------------------------------------------------------------------- case lists
def single_cases(n):
    """Every family at order ``n`` (laplace up to LAPLACE_MAX)."""
    out = [diag(n), hadamard(n, "a"), hadamard(n, "b"), hadamard(n, "r1"), graded(n), skew(n, "b")]
    if n <= LAPLACE_MAX:
        out.append(laplace(n))
    if n in (1, 17, 64):
        out += [diag(n, "zero"), diag(n, "cI")]
    return out


def deficient_cases():
    return [deficient(l, r) for l in DEFICIENT_L for r in DEFICIENT_R]


def batch_sizes(n_max):
    return [n_max, 5, n_max // 2 + 1]


def batch_cases(n_max):
    """A ``hadamard`` (a) member of order ``n_max``, a ``diag`` of order 5 that converges in sweep 0, and a slowly
    converging third member: ``graded`` for the even entries of BATCH_ORDERS, ``hadamard`` (b) for the odd ones."""
    third = n_max // 2 + 1
    slow = graded(third) if BATCH_ORDERS.index(n_max) % 2 == 0 else hadamard(third, "b")
    return [hadamard(n_max, "a"), diag(5), slow]


def tiny_batch():
    """130 matrices of orders 1..24: more than one trip of the 64 threads of the convergence check."""
    fam = (lambda n: hadamard(n, "a"), lambda n: hadamard(n, "b"), diag, laplace, graded)
    return [fam[b % len(fam)](b % TINY_MAX + 1) for b in range(TINY_BATCH)]


def all_cases():
    seen = {}
    for n in SINGLE_ORDERS:
        for c in single_cases(n):
            seen[c.name] = c
    for c in deficient_cases() + tiny_batch() + [gram(n) for n in GRAM_ORDERS]:
        seen[c.name] = c
    for n_max in BATCH_ORDERS:
        for c in batch_cases(n_max):
            seen[c.name] = c
    return list(seen.values())


# ------------------------------------------------------------------------------------- bars
def sign_normalise(v):
    v = v.copy()
    for j in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, j])), j] < 0:
            v[:, j] = -v[:, j]
    return v


def lapack(case):
    """np.linalg.eigh of the symmetric part, sorted descending and sign-normalised."""
    w, v = np.linalg.eigh(case.S)
    return w[::-1].copy(), sign_normalise(v[:, ::-1])


def ratios(case, w, v):
    """error / bar for every bar that applies; ``v`` may hold only the leading k columns (``w`` is always whole)."""
    n, e, scale = case.n, E(case.n), case.scale
    k = v.shape[1]
    out = {"order": 0.0 if np.all(np.diff(w) <= 0) else np.inf}

    def rel(err, bar):
        return 0.0 if err == 0.0 else (np.inf if bar == 0.0 else err / bar)

    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(v))):
        return dict(out, finite=np.inf)
    out["values"] = rel(np.abs(w - case.lam).max(), e * scale)
    out["orth"] = rel(np.abs(v.T @ v - np.eye(k)).max(), e)
    out["resid"] = rel(np.abs(case.S @ v - v * w[None, :k]).max(), e * scale)
    top = v[np.argmax(np.abs(v), axis=0), np.arange(k)]
    out["sign"] = 0.0 if np.all(top > 0) else np.inf
    if case.family == "laplace":
        err = np.minimum(np.abs(v - case.vec[:, :k]).max(axis=0), np.abs(v + case.vec[:, :k]).max(axis=0))
        gap = gaps(case.lam)[:k]
        gap = np.where(np.isinf(gap), 0.0, gap)       # order 1: no neighbour, no bar
        out["vectors"] = float((err * gap / (e * scale)).max())
    if case.family == "diag":
        we, ve = diag_expected(case)
        out["exact"] = 0.0 if np.array_equal(w, we) and np.array_equal(v, ve[:, :k]) else np.inf
    return out


def failures(case, w, v, margin=1.0, skip=()):
    return {name: r for name, r in ratios(case, w, v).items() if name not in skip and not r * margin <= 1.0}


def conv_bar(case, rel_tol):
    """Largest off-diagonal entry of ``V^T G V`` after a sweep that visited no ``|a_pq| > rel_tol max|a_ii|``: an entry
    at most the threshold when visited can be mixed with one other such entry by the later rotations of the sweep."""
    return 2 * rel_tol * np.abs(np.diag(case.S)).max() + E(case.n) * case.scale


def offdiag(case, v):
    t = v.T @ case.S @ v
    return np.abs(t - np.diag(np.diag(t))).max()


# ------------------------------------------------------------------------------------- NumPy restatement
def numpy_jacobi(s, rel_tol=1e-15, skip=None, max_sweeps=MAX_SWEEPS):
    """Cyclic Jacobi with the kernel's thresholds and stopping rule: rotate every ``|a_pq| > 1e-19 max|a_ii|``; a sweep
    in which no visited ``|a_pq|`` exceeds ``rel_tol max|a_ii|`` ends the iteration.  ``skip = (sweep, lo, hi)`` leaves
    the rotations of that sweep with both indices in ``[lo, hi)`` out of V (but not out of the iteration): the product
    with one rotation block replaced by the identity.  Returns (w, V, sweeps) sorted descending, sign-normalised."""
    a = s.copy()
    n = a.shape[0]
    v = np.eye(n)
    mx = np.abs(np.diag(a)).max()
    tol_conv, tol_rot = rel_tol * mx, 1e-19 * mx
    sweeps = 0
    for sweep in range(max_sweeps):
        sweeps += 1
        above = 0
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q]
                above += abs(apq) > tol_conv
                if not abs(apq) > tol_rot:
                    continue
                tau = (a[q, q] - a[p, p]) / (2 * apq)
                t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.hypot(1.0, tau))
                c = 1 / np.hypot(1.0, t)
                sn = t * c
                rp, rq = a[p].copy(), a[q].copy()
                a[p], a[q] = c * rp - sn * rq, sn * rp + c * rq
                cp, cq = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * cp - sn * cq, sn * cp + c * cq
                a[p, q] = a[q, p] = 0.0
                if skip is None or not (skip[0] == sweep and skip[1] <= p < skip[2] and skip[1] <= q < skip[2]):
                    vp, vq = v[:, p].copy(), v[:, q].copy()
                    v[:, p], v[:, q] = c * vp - sn * vq, sn * vp + c * vq
        if above == 0:
            break
    w = np.diag(a).copy()
    order = np.argsort(-w, kind="stable")
    return w[order], sign_normalise(v[:, order]), sweeps
