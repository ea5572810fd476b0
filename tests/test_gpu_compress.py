"""GPU tests of the truncation step: ``DeviceMPS.compress_bond_`` (``compress_bond_impl``, csrc/tt.hip) at its edges and
``NDMPS.compress(cutoff, max_bond)`` -- SURVEY 7's parity mode -- against the oracle.

The kernel never forms the two-site product P = T1 T2.  It works from G1 = T1^T T1 and G2 = T2 T2^T, takes a square
root Lt of G2 (Cholesky, or W D^(1/2) when the Cholesky fails or NDMPS_COMPRESS_EIG is set), and reads s^2 off the
eigenvalues of H = Lt^T G1 Lt (direct solver, or block Jacobi when the rank is in doubt or NDMPS_SWEEP_JACOBI is set).

Rank contract (the storage floor).  The kernel keeps s_j > max(cutoff, floor) s_0, at least one, at most max_bond, with
floor = 1e-6 for fp32 and bf16 cores (worked in fp32) and 1e-8 for fp64 cores.  The floor applies when cutoff == 0
too: ``compress(0, max_bond=chi)`` keeps min(#{s_j > floor s_0}, chi) values, where the oracle (oracle/mps.py:_truncate)
keeps min(n, chi), zeros included.  Every rank below is therefore compared with ``_truncate(s, max(cutoff, floor),
max_bond)``, the same convention as the sweep tests (tests/test_gpu_parity.py compares with the oracle at 1e-6).

Tolerances.  u_s is the unit roundoff of the storage type (2^-8 bf16, 2^-24 fp32, 2^-53 fp64), u_w that of the type the
kernel works in (fp32 for bf16 and fp32 cores, fp64 for fp64 cores), u = 2^-53 that of the Gram matrices, which are fp64
for every storage type.  kappa is the condition number of the gauge the unit cases split P with.
  * Spectrum.  H is formed from fp64 Gram matrices of the stored values (bf16 and fp32 values are exact in fp64), so all
    three storage types resolve s^2 to dH ~ n u kappa^2 s_0^2 (G1 carries |A|^2, Lt carries |A^-1|), i.e. s to
    sqrt(dH) = sqrt(n u) kappa s_0 at worst.  The bar is 3 sqrt(n u) kappa s_0, and never above the existing 1e-5 s_0.
    The derivation gives one bar for bf16, fp32 and fp64 alike: the storage type enters only through the stored values,
    which the numpy reference uses as well.
  * Product (Eckart-Young).  |T1'T2' - P|_F - sqrt(sum_{j>=k} s_j^2) is bounded by the sum of
      - 4 u_s sum_{j<k} s_j: rounding of the new cores to storage (absorb "both": |T1'|_F^2 = |T2'|_F^2 = sum s_j);
      - 8 u_w kappa sqrt(n k) s_0: the two products T1 (Lt V_k s^-1/2) and (s^-3/2 G1 Lt V_k)^T T2 in the work type,
        whose operands cancel by kappa;
      - 8 u kappa^2 s_0^2 sum_{j<k} 1 / s_j: a kept s_j is scaled by s_j^-3/2 after G1 Lt V_k, which carries the
        absolute Gram error u kappa^2 s_0^2; this is the digit loss of the squaring.
    Where s_{k-1} >= 1e-3 s_0 and s_k <= 0.9 s_{k-1}, |T1'T2' - P_k|_F obeys the same bar plus the Davis-Kahan rotation
    of the kept subspace, 8 u kappa^2 s_0^2 s_{k-1} sqrt(k) / (s_{k-1}^2 - s_k^2).
  * Class level (NDMPS vs OracleNDMPS): the existing bars of tests/test_gpu_parity.py and tests/test_gpu_f64_storage.py --
    reconstruction 5e-5 (fp32) / 1e-9 (fp64) relative Frobenius, |dSSIM| <= 1e-5, norm_value 1e-5 / 1e-10 relative,
    compression_ratio 1e-12 relative, boundary_list magnitudes 2e-4 / 1e-7 relative, bf16 storage BF16_TOL.
"""
import copy
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from oracle import mps as omps  # noqa: E402
from oracle.metrics import compute_ssim_by_dim, synthetic_mri  # noqa: E402
from oracle.ndmps_oracle import OracleNDMPS  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
STORAGE = {"f32": F32, "f64": F64, "bf16": BF16}
FLOOR = {F32: 1e-6, BF16: 1e-6, F64: 1e-8}       # kCutoffFloor / kCutoffFloorF64 (csrc/tt.hip)
U_STORE = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F64: 2.0 ** -53}
U_WORK = {F32: 2.0 ** -24, BF16: 2.0 ** -24, F64: 2.0 ** -53}
U64 = 2.0 ** -53
BF16_TOL = 1e-2  # tests/test_gpu_parity.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device; the product has no CPU path")
    _lib.load()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


# ------------------------------------------------------------------------------------------ unit level
def _orth(rng, m, n):
    q, r = np.linalg.qr(rng.standard_normal((m, n)))
    return q * np.sign(np.diag(r))


def _gauge(rng, n, kappa):
    """A non-orthogonal n x n gauge with condition number kappa."""
    if n == 1:
        return np.array([[1.0 + 0.5 * rng.random()]])
    return _orth(rng, n, n) @ np.diag(np.logspace(0, -np.log10(kappa), n)) @ _orth(rng, n, n)


def _pair(s, chi, chi_l, d1, d2, chi_r, kappa, seed, t2_tail="zero", left_orth=False):
    """Cores T1 (chi_l, d1, chi) and T2 (chi, d2, chi_r) with T1 T2 = U diag(s) V^T, s of length r <= chi.

    The r design values are split with the gauge A: T1 = U diag(s) A, T2 = A^-1 V^T on r of the chi bond indices
    (a random permutation of them).  The other chi - r columns of T1 are exactly zero, so a zero tail survives rounding
    to any storage type; the matching rows of T2 are zero (G1 and G2 singular: the Cholesky fails) or random
    (``t2_tail="random"``: G2 regular, or singular by shape when chi > d2 chi_r).  ``left_orth``: T1 has orthonormal
    columns instead (absorb-"both" check)."""
    rng = np.random.default_rng(seed)
    m1, n2 = chi_l * d1, d2 * chi_r
    s = np.asarray(s, dtype=np.float64)
    r = len(s)
    assert r <= min(m1, n2, chi)
    U, V = _orth(rng, m1, r), _orth(rng, n2, r)
    if left_orth:
        Q = _orth(rng, m1, chi)
        W = _orth(rng, chi, r)
        return Q, (W * s) @ V.T
    A = _gauge(rng, r, kappa)
    T1 = np.zeros((m1, chi))
    T2 = np.zeros((chi, n2))
    T1[:, :r] = (U * s) @ A
    T2[:r] = np.linalg.solve(A, V.T)
    if t2_tail == "random" and chi > r:
        T2[r:] = rng.standard_normal((chi - r, n2)) / np.sqrt(n2)
    perm = rng.permutation(chi)
    return T1[:, perm], T2[perm]


def _store(a, dtype, shape):
    return dev(a.reshape(shape), F64).to(dtype)


def _spectrum(kind, chi, n_nonzero=None):
    """Design spectra, s_0 = 1.  Values that would land near a threshold (0.3, 1e-3 and the two floors) are moved to
    about half of it: the rank is then decided by construction, outside the band where the fp64 Gram squaring (and
    direct_rank_is_safe's doubt band around c^2 w_0) leaves it open.  _check_margins verifies that on the stored values."""
    r = chi if n_nonzero is None else n_nonzero
    if kind == "geometric":
        s = np.logspace(0, -4, r) if r > 1 else np.ones(1)
    elif kind == "cluster":  # eight exactly equal values, the caps below fall inside them
        s = np.logspace(0, -2, r)
        s[8:16] = s[8]
    else:
        raise ValueError(kind)
    for thr in (0.3, 1e-3, 1e-6, 1e-8):
        band = (s > 0.6 * thr) & (s < 1.7 * thr)
        s[band] = thr * 0.5 * s[band] / (1.7 * thr)
    return np.sort(s)[::-1]


def _straddle(thr, chi=16):
    """Geometric values from 1 down to 8 thr, then 2 thr, 0.5 thr and 0.25 thr: the threshold sits between two values
    a factor four apart."""
    head = np.logspace(0, np.log10(min(8 * thr, 0.7)), chi - 3)
    return np.concatenate([head, [2 * thr, 0.5 * thr, 0.25 * thr]])


def _ref_svd(c1, c2):
    """fp64 SVD of the STORED product (bf16 / fp32 values cast to fp64)."""
    chi = c1.shape[2]
    a = c1.double().cpu().numpy().reshape(-1, chi)
    b = c2.double().cpu().numpy().reshape(chi, -1)
    P = a @ b
    u, s, vh = np.linalg.svd(P, full_matrices=False)
    return P, u, s, vh


def _check_margins(s, thresholds):
    """The construction keeps every stored singular value out of [0.7, 1.4] x threshold: a test precondition."""
    if s[0] == 0:
        return
    for thr in thresholds:
        r = s / s[0] / thr
        assert not np.any((r > 0.7) & (r < 1.4)), (thr, r[(r > 0.7) & (r < 1.4)])


def _cutoffs(dtype):
    """0, 1e-3 and 0.3; bf16 cores carry rounding noise of ~u_s kappa s_0 (4e-2 s_0 at kappa = 10) in the stored
    product, which fills the band around 1e-3 with noise values whose rank no construction can decide: 0 and 0.3."""
    return (0.0, 0.3) if dtype == BF16 else (0.0, 1e-3, 0.3)


def _mid(dtype):
    return _cutoffs(dtype)[-2] if dtype != BF16 else 0.3


def _tol_spectrum(n, kappa):
    return min(3.0 * math.sqrt(n * U64) * kappa, 1e-5)


def _tol_product(s, k, n, kappa, dtype):
    s0 = s[0]
    if s0 == 0:
        return 0.0
    kept = s[:k][s[:k] > 0]
    return (4 * U_STORE[dtype] * kept.sum() + 8 * U_WORK[dtype] * kappa * math.sqrt(n * k) * s0
            + 8 * U64 * kappa ** 2 * s0 ** 2 * np.sum(1.0 / kept))


def _run_bond(T1, T2, shape1, shape2, dtype, cutoff, max_bond, edges=True):
    """compress_bond_ on the bond between T1 and T2, inside a four-site chain (edges) or as the whole chain."""
    c1, c2 = _store(T1, dtype, shape1), _store(T2, dtype, shape2)
    before1, before2 = c1.clone(), c2.clone()
    cores = [c1, c2]
    if edges:
        rng = np.random.default_rng(7)
        cores = [dev(rng.standard_normal((1, 2, shape1[0])), F64).to(dtype), c1, c2,
                 dev(rng.standard_normal((shape2[2], 2, 1)), F64).to(dtype)]
    mps = DeviceMPS(cores)
    i = 2 if edges else 1
    spec = mps.compress_bond_(i, cutoff, max_bond)
    assert torch.equal(c1, before1) and torch.equal(c2, before2)  # the inputs are not written
    return mps.cores[i - 1], mps.cores[i], spec, c1, c2


def _check_bond(T1, T2, shape1, shape2, dtype, cutoff, max_bond, kappa, edges=True, check_pk=True):
    """compress_bond_ once; every assertion of the unit level.  Returns (k, product) for cross-route comparisons."""
    chi = shape1[2]
    n1, n2_, spec, c1, c2 = _run_bond(T1, T2, shape1, shape2, dtype, cutoff, max_bond, edges)
    P, u, s, vh = _ref_svd(c1, c2)
    s_full = np.zeros(chi)
    s_full[: len(s)] = s[:chi]
    floor = FLOOR[dtype]
    _check_margins(s, {max(cutoff, floor)})
    k_ref = omps._truncate(s_full, max(cutoff, floor), max_bond)
    k = int(n1.shape[2])
    assert k == k_ref, (k, k_ref, cutoff, max_bond)
    # shapes and storage type
    assert tuple(n1.shape) == (shape1[0], shape1[1], k) and tuple(n2_.shape) == (k, shape2[1], shape2[2])
    assert n1.dtype == dtype and n2_.dtype == dtype
    a = n1.double().cpu().numpy().reshape(-1, k)
    b = n2_.double().cpu().numpy().reshape(k, -1)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(spec))
    s0 = s_full[0]
    if s0 == 0:  # all-zero cores: one zero column / row
        assert k == 1 and not a.any() and not b.any() and not spec.any()
        return k, a @ b
    # spectrum
    assert spec.shape == (chi,)
    assert np.abs(spec - s_full).max() <= _tol_spectrum(chi, kappa) * s0, np.abs(spec - s_full).max() / s0
    # Eckart-Young: the truncation error is the discarded tail, whatever basis a degenerate cluster yields
    got = a @ b
    tail = math.sqrt(float(np.sum(s_full[k:] ** 2)))
    tol = _tol_product(s_full, k, chi, kappa, dtype)
    err = float(np.linalg.norm(got - P))
    assert abs(err - tail) <= tol + 1e-12 * tail, (err, tail, tol)
    if check_pk and k < len(s) and s[k - 1] >= 1e-3 * s0 and s[k] <= 0.9 * s[k - 1]:
        pk = (u[:, :k] * s[:k]) @ vh[:k]
        rot = 8 * U64 * kappa ** 2 * s0 ** 2 * s[k - 1] * math.sqrt(k) / (s[k - 1] ** 2 - s[k] ** 2)
        assert float(np.linalg.norm(got - pk)) <= tol + rot, (float(np.linalg.norm(got - pk)), tol + rot)
    return k, got


def _caps(s_stored, cutoff, floor, chi):
    """None, 1, below the cutoff rank, equal to it, above chi."""
    kc = omps._truncate(s_stored, max(cutoff, floor), None)
    return sorted({None, 1, max(1, kc // 2), kc, chi + 3}, key=lambda v: -1 if v is None else v)


def _dims(chi):
    """(chi_l, d1, d2, chi_r) of an interior bond whose unfoldings have at least chi + 4 rows and columns."""
    side = -(-(chi + 4) // 4)
    return side, 4, 4, side


BOND_CHIS = [1, 7, 64, 128, 129, 512, 1024]


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("chi", BOND_CHIS)
def test_compress_bond_geometric_spectrum(storage, chi):
    """Geometric spectrum 1 .. 1e-4 over chi values, non-canonical cores (kappa = 10), every cutoff x cap."""
    dtype = STORAGE[storage]
    kappa = 10.0
    chi_l, d1, d2, chi_r = _dims(chi)
    T1, T2 = _pair(_spectrum("geometric", chi), chi, chi_l, d1, d2, chi_r, kappa, seed=chi)
    shape1, shape2 = (chi_l, d1, chi), (chi, d2, chi_r)
    _, _, s, _ = _ref_svd(_store(T1, dtype, shape1), _store(T2, dtype, shape2))
    for cutoff in _cutoffs(dtype):
        for max_bond in _caps(s, cutoff, FLOOR[dtype], chi):
            _check_bond(T1, T2, shape1, shape2, dtype, cutoff, max_bond, kappa)


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("end", ["first", "last"])
def test_compress_bond_at_the_ends_of_the_chain(storage, end):
    """chi_l = 1 (first bond) and chi_r = 1 (last bond), the two-site chain itself."""
    dtype = STORAGE[storage]
    chi, kappa = 64, 10.0
    chi_l, d1, d2, chi_r = (1, 70, 4, 17) if end == "first" else (17, 4, 70, 1)
    T1, T2 = _pair(_spectrum("geometric", chi), chi, chi_l, d1, d2, chi_r, kappa, seed=3)
    for cutoff, max_bond in ((0.0, None), (_mid(dtype), 20), (0.3, None), (0.0, 1)):
        _check_bond(T1, T2, (chi_l, d1, chi), (chi, d2, chi_r), dtype, cutoff, max_bond, kappa, edges=False)


@pytest.mark.parametrize("storage", list(STORAGE))
def test_compress_bond_cap_inside_a_cluster_of_equal_values(storage):
    """s_8 = ... = s_15 exactly: the caps 9, 12 and 15 cut the cluster, where the top-k vectors can lose rank and the
    kernel routes to the block Jacobi.  Eckart-Young holds for any basis of the cluster."""
    dtype = STORAGE[storage]
    chi, kappa = 64, 10.0
    chi_l, d1, d2, chi_r = _dims(chi)
    T1, T2 = _pair(_spectrum("cluster", chi), chi, chi_l, d1, d2, chi_r, kappa, seed=11)
    for cutoff in (0.0, _mid(dtype)):
        for max_bond in (9, 12, 15, 16):
            _check_bond(T1, T2, (chi_l, d1, chi), (chi, d2, chi_r), dtype, cutoff, max_bond, kappa)


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("t2_tail", ["zero", "random"])
@pytest.mark.parametrize("chi,d2,chi_r,r", [(64, 4, 18, 40), (129, 4, 34, 100), (64, 4, 8, 32)],
                         ids=["zero-tail-64", "zero-tail-129", "chi-above-d2-chi_r"])
def test_compress_bond_rank_deficient_product(storage, t2_tail, chi, d2, chi_r, r):
    """P has rank r < chi with exact zeros (T1's other columns are zero in any storage type).  t2_tail="zero": G1 and G2
    singular, the Cholesky fails and the eigen square root with its zero columns runs; "random": G2 regular (or, for
    chi > d2 chi_r, singular by shape) and only H sees the zero eigenvalues.  The s^-1/2 and s^-3/2 scalings must not
    meet the zeros: every kept value is above the floor."""
    dtype = STORAGE[storage]
    kappa = 10.0
    chi_l, d1 = -(-(chi + 4) // 4), 4
    T1, T2 = _pair(_spectrum("geometric", r), chi, chi_l, d1, d2, chi_r, kappa, seed=r, t2_tail=t2_tail)
    for cutoff, max_bond in ((0.0, None), (0.0, chi + 3), (_mid(dtype), None), (0.0, r - 5), (0.3, 1)):
        _check_bond(T1, T2, (chi_l, d1, chi), (chi, d2, chi_r), dtype, cutoff, max_bond, kappa)


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("thr", [0.3, 1e-3, 1e-6, 1e-8])
def test_compress_bond_values_straddling_the_threshold(storage, thr):
    """Values at 2x and 0.5x the threshold max(cutoff, floor), for the cutoffs and for each storage floor (cutoff 0).
    kappa = 1.5 here: at 1e-8 the fp64 Gram squaring resolves s only to ~u kappa^2 s_0^2 / s, and the construction must
    keep the rank decidable (a numpy replay of the route recovers 2e-8 s_0 to ~1% at such a gauge).  A floor below the storage
    type's own is not a threshold the kernel applies, and bf16 cores carry rounding noise of ~u_s kappa s_0 = 6e-3 s_0,
    which buries the values below it: those combinations are not cases."""
    dtype = STORAGE[storage]
    floor = FLOOR[dtype]
    if thr < floor or (dtype == BF16 and thr < 0.3):
        pytest.skip("threshold below what this storage type decides")
    kappa = 1.5
    chi = 16
    chi_l, d1, d2, chi_r = _dims(chi)
    T1, T2 = _pair(_straddle(thr, chi), chi, chi_l, d1, d2, chi_r, kappa, seed=int(-math.log10(thr)) + 20)
    cutoff = 0.0 if thr == floor else thr
    for max_bond in (None, chi - 2, chi - 3):
        _check_bond(T1, T2, (chi_l, d1, chi), (chi, d2, chi_r), dtype, cutoff, max_bond, kappa)


@pytest.mark.parametrize("storage", list(STORAGE))
def test_compress_bond_all_zero_cores(storage):
    dtype = STORAGE[storage]
    for chi in (1, 7, 64):
        T1, T2 = np.zeros((3 * 5, chi)), np.zeros((chi, 4 * 6))
        for cutoff, max_bond in ((0.0, None), (0.3, 4), (0.0, 1)):
            _check_bond(T1, T2, (3, 5, chi), (chi, 4, 6), dtype, cutoff, max_bond, 1.0)


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("chi", [7, 64, 129])
def test_compress_bond_absorbs_sqrt_s_on_both_sides(storage, chi):
    """absorb="both": with T1 left-orthonormal, the columns of T1' have norms sqrt(s_j).  Each column is rounded to
    storage (relative u_s on the norm) and computed in the work type (a few u_w kappa relative, kappa = 1 here), with the
    spectrum error of _tol_spectrum on s_j >= 1e-2 s_0: relative 1e-3 at most, halved by the square root."""
    dtype = STORAGE[storage]
    chi_l, d1, d2, chi_r = _dims(chi)
    s = np.logspace(0, -2, chi) if chi > 1 else np.ones(1)
    T1, T2 = _pair(s, chi, chi_l, d1, d2, chi_r, 1.0, seed=chi + 100, left_orth=True)
    for max_bond in (None, max(1, chi // 3)):
        n1, _, spec, c1, c2 = _run_bond(T1, T2, (chi_l, d1, chi), (chi, d2, chi_r), dtype, 0.0, max_bond)
        _, _, s_ref, _ = _ref_svd(c1, c2)
        k = int(n1.shape[2])
        norms = np.linalg.norm(n1.double().cpu().numpy().reshape(-1, k), axis=0)
        rtol = 2 * U_STORE[dtype] + 8 * U_WORK[dtype] * math.sqrt(chi) + 0.5 * _tol_spectrum(chi, 1.0) / 1e-2
        assert np.allclose(norms, np.sqrt(s_ref[:k]), rtol=rtol, atol=0), np.abs(norms / np.sqrt(s_ref[:k]) - 1).max()


ROUTE_CASES = [("geometric", 64, None, "zero"), ("geometric", 129, None, "zero"), ("geometric", 1024, None, "zero"),
               ("geometric", 64, 40, "zero"), ("geometric", 64, 40, "random"), ("cluster", 64, None, "zero")]


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("kind,chi,r,t2_tail", ROUTE_CASES, ids=lambda v: str(v))
def test_compress_bond_routes_agree(storage, kind, chi, r, t2_tail, monkeypatch):
    """Cholesky vs eigen square root of G2 (NDMPS_COMPRESS_EIG) and direct solver vs block Jacobi (NDMPS_SWEEP_JACOBI):
    each route meets every unit-level bar on its own, and the routes agree with each other -- same k, products within
    the sum of their two bars."""
    dtype = STORAGE[storage]
    kappa = 10.0
    chi_l, d1, d2, chi_r = _dims(chi)
    s = _spectrum(kind, chi if r is None else r)
    T1, T2 = _pair(s, chi, chi_l, d1, d2, chi_r, kappa, seed=chi + 7, t2_tail=t2_tail)
    shape1, shape2 = (chi_l, d1, chi), (chi, d2, chi_r)
    _, _, s_ref, _ = _ref_svd(_store(T1, dtype, shape1), _store(T2, dtype, shape2))
    for cutoff, max_bond in ((0.0, None), (_mid(dtype), 12), (0.0, 9)):
        results = []
        for env in (None, "NDMPS_COMPRESS_EIG", "NDMPS_SWEEP_JACOBI"):
            monkeypatch.delenv("NDMPS_COMPRESS_EIG", raising=False)
            monkeypatch.delenv("NDMPS_SWEEP_JACOBI", raising=False)
            if env:
                monkeypatch.setenv(env, "1")
            results.append(_check_bond(T1, T2, shape1, shape2, dtype, cutoff, max_bond, kappa))
        monkeypatch.delenv("NDMPS_COMPRESS_EIG", raising=False)
        monkeypatch.delenv("NDMPS_SWEEP_JACOBI", raising=False)
        k0, p0 = results[0]
        s_full = np.zeros(chi)
        s_full[: len(s_ref)] = s_ref[:chi]
        tol = _tol_product(s_full, k0, chi, kappa, dtype)
        for k, p in results[1:]:
            assert k == k0
            if kind != "cluster" or max_bond is None:  # a cut cluster leaves the basis of its kept part open
                assert float(np.linalg.norm(p - p0)) <= 2 * tol + 2e-12 * float(np.linalg.norm(p0))


# ------------------------------------------------------------------------------------------ class level
def _ssim_gap(x, rec_gpu, rec_ref):
    x64 = x.astype(np.float64)
    return abs(compute_ssim_by_dim(x64, rec_gpu.astype(np.float64)) - compute_ssim_by_dim(x64, rec_ref))


REC_TOL = {F32: 5e-5, F64: 1e-9}
NORM_TOL = {F32: 1e-5, F64: 1e-10}
BOUNDARY_TOL = {F32: 2e-4, F64: 1e-7}


def _assert_parity(gpu, ref, x, dtype):
    assert gpu.bond_sizes() == ref.bond_sizes()
    rg, rr = gpu.to_tensor(), ref.to_tensor()
    assert np.all(np.isfinite(rg))
    rel = np.linalg.norm(rg - rr) / np.linalg.norm(rr)
    assert rel <= REC_TOL[dtype], rel
    assert _ssim_gap(x, rg, rr) <= 1e-5
    assert math.isclose(gpu.norm_value, ref.norm_value, rel_tol=NORM_TOL[dtype])
    assert math.isclose(gpu.compression_ratio(), ref.compression_ratio(), rel_tol=1e-12)
    for (lo, hi), (rlo, rhi) in zip(np.abs(np.asarray(gpu.boundary_list)), np.abs(np.asarray(ref.boundary_list))):
        assert math.isclose(max(lo, hi), max(rlo, rhi), rel_tol=BOUNDARY_TOL[dtype])  # cores agree up to sign


def _gpu_from(x, mode, dtype, **kw):
    return NDMPS.from_tensor(x.astype(np.float64) if dtype == F64 else x, mode=mode, dtype=dtype, **kw)


PARITY_CASES = [((64, 64, 64), 16, "Std"), ((128, 128, 128), 32, "Std"), ((16, 16, 8, 12), 10, "Std"),
                ((48, 40, 36), 12, "DCT")]


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("shape,chi,mode", PARITY_CASES, ids=str)
def test_parity_mode_matches_the_oracle(storage, shape, chi, mode):
    """from_tensor (exact), then compress(0, chi), compress(0.01, chi), compress(0.05), cumulatively, against the oracle
    run at max(cutoff, floor) (the floor contract).  On these volumes no singular value lies between the floor and the
    raw cutoff 0 within the first chi, so the oracle run at the raw cutoffs keeps the same bonds and the same cores: the
    GPU is held to the same bars against it."""
    dtype = STORAGE[storage]
    floor = FLOOR[dtype]
    x = synthetic_mri(shape, seed=2025)
    gpu = _gpu_from(x, mode, dtype)
    ref = OracleNDMPS.from_tensor(x, mode=mode, cutoff=floor)
    raw = OracleNDMPS.from_tensor(x, mode=mode)
    assert gpu.bond_sizes() == ref.bond_sizes()
    for cutoff, max_bond in ((0.0, chi), (0.01, chi), (0.05, None)):
        gpu.compress(cutoff, max_bond=max_bond)
        ref.compress(max(cutoff, floor), max_bond=max_bond)
        raw.compress(cutoff, max_bond=max_bond)
        assert all(b <= chi for b in gpu.bond_sizes())
        _assert_parity(gpu, ref, x, dtype)
        _assert_parity(gpu, raw, x, dtype)


def test_parity_mode_bf16_storage_against_the_oracle_on_rounded_values():
    xb = torch.from_numpy(synthetic_mri((64, 64, 64), seed=5)).to(DEV).to(BF16)
    # from a capped sweep, as tests/test_gpu_parity.py's bf16 parity test: an exact bf16 state rounds 512-wide cores
    # (the sweep carried in fp32, cores rounded once: what is measured is compress's own bf16 rounding)
    obj = NDMPS.from_tensor(xb, max_bond=32, dtype=BF16, carry_dtype=F32)
    ref = OracleNDMPS.from_tensor(xb.float().cpu().numpy(), max_bond=32, cutoff=FLOOR[BF16])
    # parity mode only: the cap binds on every interior bond.  Without a cap a relative cutoff is decided on singular
    # values that carry bf16 noise of ~u_s s_0 = 4e-3 s_0, so a value near the threshold may go either way and move the
    # reconstruction by far more than rounding.
    # Each step starts from the capped state: a bf16 compress rounds every core twice (once per bond it touches), ~0.5%
    # of product error per call over six cores, so a chain of calls compounds past BF16_TOL, which bounds one encode.
    start, start_ref = obj, ref
    for cutoff, max_bond in ((0.0, 16), (0.01, 16), (0.0, 8)):
        obj, ref = copy.deepcopy(start), copy.deepcopy(start_ref)
        obj.compress(cutoff, max_bond=max_bond)
        ref.compress(max(cutoff, FLOOR[BF16]), max_bond=max_bond)
        assert all(c.dtype == BF16 for c in obj.mps.cores)
        assert obj.bond_sizes() == ref.bond_sizes()
        rr = ref.to_tensor()
        rec = obj.to_tensor(as_torch=True).double().cpu().numpy()
        assert np.all(np.isfinite(rec))
        rel = np.linalg.norm(rec - rr) / np.linalg.norm(rr)
        assert rel <= BF16_TOL, (cutoff, max_bond, rel)
        assert math.isclose(obj.norm_value, ref.norm_value, rel_tol=BF16_TOL)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_compress_with_a_cap_above_every_bond_is_idempotent(storage):
    """compress(0, max_bond >= every bond) re-gauges the cores and drops nothing: the bonds stay, the reconstruction
    moves by rounding only -- the exact round-trip bars, 2e-5 (fp32) and 1e-10 (fp64) relative."""
    dtype = STORAGE[storage]
    x = synthetic_mri((64, 64, 64), seed=31)
    obj = _gpu_from(x, "Std", dtype)
    obj.compress(0.0, max_bond=16)
    bonds, before = obj.bond_sizes(), obj.to_tensor()
    obj.compress(0.0, max_bond=10 ** 6)
    assert obj.bond_sizes() == bonds
    after = obj.to_tensor()
    assert np.linalg.norm(after - before) <= (2e-5 if dtype == F32 else 1e-10) * np.linalg.norm(before)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_parity_mode_on_low_rank_and_degenerate_volumes(storage):
    dtype = STORAGE[storage]
    shape = (32, 32, 32)
    # exact sweeps of these volumes put every eigenvalue of a site in doubt and measure the tail norms directly, on the
    # last site with 4096 rows against an order-8 eigenproblem (fewer, longer row blocks): their bonds against the oracle
    def exact(x):
        obj = _gpu_from(x, "Std", dtype)
        assert obj.bond_sizes() == OracleNDMPS.from_tensor(x, cutoff=FLOOR[dtype]).bond_sizes()
        return obj

    zero = exact(np.zeros(shape, dtype=np.float32))
    assert zero.bond_sizes() == [1] * len(zero.bond_sizes())
    zero.compress(0.0, max_bond=16)
    rec = zero.to_tensor()
    assert np.all(np.isfinite(rec)) and not rec.any()
    assert all(torch.isfinite(c).all() for c in zero.mps.cores)
    assert zero.norm_value == 0 and not math.isnan(zero.norm_value)

    const = exact(np.full(shape, 0.7, dtype=np.float32))
    const.compress(0.0, max_bond=16)
    assert const.bond_sizes() == [1] * len(const.bond_sizes())
    assert np.abs(const.to_tensor() - np.float32(0.7)).max() <= (2e-6 if dtype == F32 else 1e-12)

    # three terms separable over every digit of every coordinate (the sites are digits, not axes: a sum of three
    # axis-separable terms is of full rank across them); the oracle's fourth singular value is below 1e-8 s_0 (fp32
    # values) and 1e-15 s_0 (fp64) on every bond
    i = np.arange(32, dtype=np.float64)
    low = sum(np.exp(a * i[:, None, None] + b * i[None, :, None] + c * i[None, None, :])
              for a, b, c in ((0.05, -0.03, 0.02), (-0.04, 0.06, 0.01), (0.02, 0.02, -0.05)))
    if dtype == F32:
        low = low.astype(np.float32)
    obj = exact(low)
    assert obj.bond_sizes() == [3] * len(obj.bond_sizes())
    obj.compress(0.0, max_bond=16)
    assert all(b <= 3 for b in obj.bond_sizes())
    # exact reconstruction: the round-trip bars (tests/test_gpu_parity.py, tests/test_gpu_f64_storage.py)
    assert np.abs(obj.to_tensor() - low).max() <= (2e-5 if dtype == F32 else 1e-10) * np.abs(low).max()


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_lockstep_group_compress_equals_one_by_one(storage):
    """Objects of one from_tensors call share a _GroupState; compress with a cap must treat each like a lone object."""
    dtype = STORAGE[storage]
    vols = [synthetic_mri((32, 32, 32), seed=s) for s in (1, 2, 3)]
    vols[1] = vols[1] * 0.25
    cast = [v.astype(np.float64) if dtype == F64 else v for v in vols]
    group = NDMPS.from_tensors(cast, max_bond=24, dtype=dtype)
    for v, g in zip(cast, group):
        one = NDMPS.from_tensor(v, max_bond=24, dtype=dtype)
        assert g.bond_sizes() == one.bond_sizes()
        g.compress(0.0, max_bond=10)
        one.compress(0.0, max_bond=10)
        assert g.bond_sizes() == one.bond_sizes()
        assert np.array_equal(g.to_tensor(), one.to_tensor())
        assert g.norm_value == one.norm_value
        assert np.array_equal(np.asarray(g.boundary_list), np.asarray(one.boundary_list))


def test_compress_list_with_a_cap_on_three_lanes_equals_the_loop_and_the_oracle(monkeypatch):
    from imgcompressionmps_amd.core import batch

    vols = [synthetic_mri((64, 64, 64), seed=500 + i) for i in range(4)]
    a = batch.conv_to_mps(vols, mode="Std")
    b = copy.deepcopy(a)
    batch.compress_list(a, 0.0, max_bond=12)
    monkeypatch.setenv("NDMPS_COMPRESS_LIST_SERIAL", "1")
    batch.compress_list(b, 0.0, max_bond=12)
    for v, x, y in zip(vols, a, b):
        assert x.bond_sizes() == y.bond_sizes()
        assert all(torch.equal(p, q) for p, q in zip(x.mps.cores, y.mps.cores))
        assert x.norm_value == y.norm_value and np.array_equal(np.asarray(x.boundary_list), np.asarray(y.boundary_list))
        ref = OracleNDMPS.from_tensor(v, cutoff=FLOOR[F32])
        ref.compress(FLOOR[F32], max_bond=12)
        assert x.bond_sizes() == ref.bond_sizes()


# ------------------------------------------------------------------------------------------ the reference flow at 256^3
def test_reference_flow_256_cubed_against_the_oracle():
    """bench.py's volume: exact state (middle bond of order 4084 in fp32, 4096 in fp64 and in the oracle), compress(0.01)
    and, from a fresh exact state, compress(0, max_bond=64), each in fp32 and fp64 storage against one oracle run."""
    x = synthetic_mri((256, 256, 256), seed=2025)
    ora = OracleNDMPS.from_tensor(x)
    spectra = ora.sweep_spectra
    ora_a = copy.deepcopy(ora)
    ora_a.compress(0.01)
    ora_b = ora
    ora_b.compress(0.0, max_bond=64)
    gpu = fresh = None
    try:
        for dtype in (F32, F64):
            floor = FLOOR[dtype]
            # the exact-state bonds of the oracle run at the storage floor: its spectra counted at that floor.  At 1e-8 every
            # value is clear of the threshold; at 1e-6 the middle bond holds one value 0.9% above it (4084 of 4096 kept),
            # which the fp32 sweep resolves (its s carry ~1e-8 s_0).
            if dtype == F64:
                for s in spectra[1:]:
                    _check_margins(s, [floor])
            want = [int(np.count_nonzero(s > floor * s[0])) for s in spectra[1:]]
            gpu = _gpu_from(x, "Std", dtype)
            assert gpu.bond_sizes() == want
            fresh = copy.deepcopy(gpu)
            gpu.compress(0.01)
            assert gpu.bond_sizes() == ora_a.bond_sizes()
            rr = ora_a.to_tensor()
            assert np.linalg.norm(gpu.to_tensor() - rr) / np.linalg.norm(rr) <= REC_TOL[dtype]
            gpu = None
            fresh.compress(0.0, max_bond=64)
            assert fresh.bond_sizes() == ora_b.bond_sizes()
            rr = ora_b.to_tensor()
            assert np.linalg.norm(fresh.to_tensor() - rr) / np.linalg.norm(rr) <= REC_TOL[dtype]
            fresh = None
    finally:  # the exact states hold a bond of order 4096: freed whether or not an assertion failed
        gpu = fresh = None
        torch.cuda.empty_cache()
