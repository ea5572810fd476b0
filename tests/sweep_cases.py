"""Planted-rank volumes for testing the TT-SVD sweep per bond and per core.  tests/test_sweep_cases_host.py shows on the
CPU that every case is well posed: the planted bonds are what the fp64 reference finds, every rank decision sits in a
gap of at least 1e-2 s_0 and survives the rounding of the storage type, and the case reaches the route it names.

tests/test_gpu_sweep_cases.py runs the library's sweep on every case, on every route the case names, and hands cores,
spectra and reconstruction of every member to ``check_sweep``: bonds, shapes, padding, ``boundary_list`` and
``norm_value`` exactly; per bond the kept subspace (``max_sin_theta``) and the kept singular values, per inner core the
``isometry_defect``, the carrying end's ``site0_defect`` against the sweep's own basis and the reconstruction, each
against ``MARGIN * yardstick + solver_terms``.  The host tests call the same ``check_sweep`` on the models' output and on
mutations of it, so what the GPU suite asserts is itself tested without a GPU.

NumPy fp64 only; nothing of the product is imported.  The reference is ``oracle.mps.mps_from_dense`` on the site-order
tensor (``oracle.index_map``).  ``emulated_sweep`` is the same sweep with the input, the cores and every carried matrix
rounded to the storage type: a family of models of WHERE a sweep in that type rounds and of nothing else -- the SVD or
the Gram route of csrc/tt.hip, the carry product rounded once or accumulated in the device's accumulator type, forwards
or backwards.  ``yardstick`` is the elementwise maximum over that family (a sweep that rounds where it must cannot do
better; one that is more than ``MARGIN`` -- twice the spread between two summation orders of one model -- worse has a
wrong vector somewhere); what the device's eigen-solver may add by its own contract is ``solver_terms``.

A volume is planted by drawing Gaussian cores of given bond ranks over the site dimensions of its shape, contracting
them in fp64 and scattering the site-order tensor back to the C-order volume; ``tail=(ranks_hi, eps)`` adds ``eps``
times a second planted volume of higher ranks, so that a cap cuts inside a spectrum with a known gap.  Seeds are chosen
(by tests/test_sweep_cases_host.py failing otherwise, never on the GPU) so that Gaussian cores are well enough
conditioned for the gap condition.

Interface bases.  After a right-to-left sweep, ``W_i`` (bond i, between sites i-1 and i) is the product of cores
i..L-1 as a ``k_i x N_i`` matrix with orthonormal rows; after a left-to-right sweep it is the product of cores 0..i-1,
transposed to ``k_i x M_i``.  Two sweeps agree at a bond when the row spaces agree (``max_sin_theta``): signs and
rotations inside the kept subspace are gauge.
"""
import numpy as np

from oracle import index_map as oim
from oracle import mps as omps

# unit roundoff of the storage types (bf16: 8 significant bits, round to nearest)
U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f64": 2.0 ** -53}
# the relative cutoff below which a sweep in that storage type does not resolve singular values (documented on
# NDMPS.from_tensor / from_tensors: fp32 and bf16 clamp at 1e-6, fp64 at 1e-8)
CUTOFF_FLOOR = {"f32": 1e-6, "bf16": 1e-6, "f64": 1e-8}
DEFAULT_CUTOFF = 1e-10


# ------------------------------------------------------------------------------------------------ index map
def site_dims(shape):
    """Site dimensions of ``shape``: the oracle's ``qubit_size``."""
    factor_arr, _ = oim.get_factorlist(tuple(int(s) for s in shape))
    return [int(q) for q in np.prod(factor_arr, axis=1)]


def to_site_order(x):
    """The C-order volume as the flat site-order tensor."""
    x = np.asarray(x, dtype=np.float64)
    dense = np.empty(x.size)
    dense[oim.flat_destination(tuple(x.shape)).reshape(-1)] = x.reshape(-1)
    return dense


def from_site_order(dense, shape):
    return np.asarray(dense, dtype=np.float64).reshape(-1)[oim.flat_destination(tuple(shape)).reshape(-1)].reshape(shape)


# ------------------------------------------------------------------------------------------------ planted volumes
def _planted_dense(dims, ranks, rng):
    bonds = [1] + [int(r) for r in ranks] + [1]
    assert len(bonds) == len(dims) + 1, (dims, ranks)
    cores = [rng.standard_normal((bonds[j], d, bonds[j + 1])) for j, d in enumerate(dims)]
    dense = omps.mps_to_dense(cores).reshape(-1)
    return dense / np.sqrt(np.mean(dense * dense))


def planted_volume(shape, ranks, seed, tail=None):
    """C-order fp64 volume of unit RMS whose site-order tensor has the bond ranks ``ranks`` (L - 1 of them); with
    ``tail=(ranks_hi, eps)`` plus ``eps`` times a second planted volume (unit RMS as well) of ranks ``ranks_hi``."""
    shape = tuple(int(s) for s in shape)
    dims = site_dims(shape)
    rng = np.random.default_rng(seed)
    dense = _planted_dense(dims, ranks, rng)
    if tail is not None:
        ranks_hi, eps = tail
        dense = dense + float(eps) * _planted_dense(dims, ranks_hi, rng)
    dense = dense / np.sqrt(np.mean(dense * dense))
    return from_site_order(dense, shape)


# ------------------------------------------------------------------------------------------------ sweeps
def interface_bases(cores, sweep_from="right"):
    """[None, W_1, .., W_{L-1}]: the accumulated basis of every bond, ``k_i x N_i`` (see the module docstring)."""
    L = len(cores)
    bases = [None] * L
    if sweep_from == "right":
        w = np.ones((1, 1))
        for i in range(L - 1, 0, -1):
            k, d, kr = cores[i].shape
            w = (np.asarray(cores[i], dtype=np.float64).reshape(k * d, kr) @ w).reshape(k, -1)
            bases[i] = w
        return bases
    w = np.ones((1, 1))
    for i in range(L - 1):
        kl, d, k = cores[i].shape
        w = (w @ np.asarray(cores[i], dtype=np.float64).reshape(kl, d * k)).reshape(-1, k)
        bases[i + 1] = w.T
    return bases


def reference_sweep(x, cutoff=DEFAULT_CUTOFF, max_bond=None, sweep_from="right"):
    """``oracle.mps.mps_from_dense`` in fp64 on the site-order tensor of ``x``: dict(cores, spectra, bases, bonds)."""
    dims = site_dims(x.shape)
    cores, spectra = omps.mps_from_dense(to_site_order(x), dims, cutoff=cutoff, max_bond=max_bond, sweep_from=sweep_from)
    return dict(cores=cores, spectra=spectra, bases=interface_bases(cores, sweep_from),
                bonds=[int(c.shape[2]) for c in cores[:-1]], recon=reconstruction(cores, x.shape))


def reconstruction(cores, shape):
    """The C-order fp64 volume a chain stands for."""
    return from_site_order(omps.mps_to_dense([np.asarray(c, dtype=np.float64) for c in cores]).reshape(-1), shape)


def round_to(a, storage):
    """fp64 array holding ``a`` rounded to the storage type: fp32 through ``astype``, bf16 by truncating the mantissa
    of the fp32 value (an error of up to 2 u: the yardstick errs on the generous side of round-to-nearest)."""
    a = np.asarray(a, dtype=np.float64)
    if storage == "f64":
        return a.copy()
    f = np.ascontiguousarray(a, dtype=np.float32)
    if storage == "bf16":
        f = (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return f.astype(np.float64)


# the carry product A V_k as the device forms it: (accumulator, k per matrix instruction) of the storage type -- fp32 data
# on the 32x32x2 MFMA, bf16 data on the 32x32x16 MFMA with an fp32 accumulator, fp64 data on the 16x16x4 MFMA
KSTEP = {"f32": 2, "bf16": 16, "f64": 4}
_ACC = {"f32": np.float32, "bf16": np.float32, "f64": np.float64}
MODELS = tuple((route, acc, rev) for route in ("svd", "gram")
               for acc, rev in (("exact", False), ("steps", False), ("steps", True)))


def carry_product(mat, core, storage, accumulate="exact", reverse=False):
    """``mat @ core.T`` (the next carried matrix, m x k) stored in ``storage``.  ``"exact"``: the fp64 product rounded
    once.  ``"steps"``: a running sum in the accumulator type over the products of ``KSTEP`` consecutive k (each chunk in
    fp64: exact for fp32 and bf16 data up to 2**-53, itself rounded for fp64 data), in ascending order of k or, with
    ``reverse``, descending; rounded to storage at the end (a no-op unless the storage is bf16)."""
    if accumulate == "exact":
        return round_to(mat @ core.T, storage)
    assert accumulate == "steps", accumulate
    step, acc_t = KSTEP[storage], _ACC[storage]
    starts = range(0, mat.shape[1], step)
    acc = np.zeros((mat.shape[0], core.shape[0]), dtype=acc_t)
    for c in (reversed(starts) if reverse else starts):
        acc = (acc.astype(np.float64) + mat[:, c: c + step] @ core[:, c: c + step].T).astype(acc_t)
    return round_to(acc, storage)


def _site_svd(mat):
    """(s, rows): singular values and ALL right vectors as rows, descending."""
    _, s, vh = np.linalg.svd(mat, full_matrices=False)
    return s, vh


def _site_gram(mat):
    """The Gram route of csrc/tt.hip on the stored carry, its eigenproblem solved by LAPACK in fp64: for n <= m the
    eigenvectors of A^T A are the right vectors; for n > m those of A A^T are the left ones and the right vectors are
    ``diag(1/s) U^T A`` (rows whose s is zero stay zero).  Returns (s, rows, u) with u = None for n <= m."""
    m, n = mat.shape
    g = mat.T @ mat if n <= m else mat @ mat.T
    w, v = np.linalg.eigh(g)
    w, v = w[::-1], v[:, ::-1]
    s = np.sqrt(np.maximum(w, 0.0))
    if n <= m:
        return s, v.T.copy(), None
    inv = np.where(s > 0.0, 1.0 / np.where(s > 0.0, s, 1.0), 0.0)
    return s, inv[:, None] * (v.T @ mat), v


def emulated_sweep(x, cutoff=DEFAULT_CUTOFF, max_bond=None, sweep_from="right", storage="f32", accumulate="exact",
                   route="svd", reverse=False, tamper=None, polish=False):
    """The sweep of ``reference_sweep`` with the input, every core and every carried matrix rounded to ``storage``: a
    family of models of WHERE a sweep in that type rounds.

    ``route="svd"``: per site an fp64 SVD of the stored carry, the kept vectors rounded once (the core), the next carry
    = the stored carry times the stored core.  ``route="gram"``: what csrc/tt.hip does -- ``eigh`` of the fp64 Gram matrix
    of the stored carry; for n <= m the core is ``V_k^T`` and the carry the same product; for n > m the core is
    ``diag(1/s_k) U_k^T A`` evaluated in fp64 and rounded, the carry ``U_k diag(s_k)`` rounded.

    ``accumulate`` says how the carry product is summed (``carry_product``): ``"exact"`` rounds an fp64 product once,
    ``"steps"`` keeps a running sum in the device's accumulator type, ``reverse=True`` in descending order of k.

    ``polish=True`` (what ``yardstick`` uses for fp64 storage; off by default) takes one Newton-Schulz step on the kept
    vectors within their span before they are stored: LAPACK's vectors are orthonormal to some 10 u only and nothing is
    rounded behind them in fp64 storage, so the step leaves what the STORAGE does (nothing) -- the isometry yardstick of
    such a site is then a few u and the solver's orthogonality enters the bar once, through ``solver_terms``.

    The relative cutoff is clamped at the storage type's floor.  ``tamper`` (tests of the comparator only) maps
    ``"core"`` to ``f(site, rows, k, core) -> core`` (rows: every right vector) and / or ``"carry"`` to
    ``f(site, mat, core, carry) -> carry``; sites are those of the swept (for ``sweep_from="left"``: mirrored) chain.  Same dict as ``reference_sweep``."""
    assert route in ("svd", "gram"), route
    tamper = tamper or {}
    dims = site_dims(x.shape)
    L = len(dims)
    cut = max(float(cutoff), CUTOFF_FLOOR[storage])
    dense = round_to(to_site_order(x), storage)
    nd = dense.reshape(dims)
    if sweep_from == "left":  # the same sweep on the chain read backwards
        nd = nd.transpose(range(L - 1, -1, -1))
        dims = dims[::-1]
    cores, spectra = [None] * L, [None] * L
    work, chi_r = nd.reshape(-1, 1), 1
    for i in range(L - 1, 0, -1):
        mat = work.reshape(-1, dims[i] * chi_r)
        if route == "svd":
            (s, rows), u = _site_svd(mat), None
        else:
            s, rows, u = _site_gram(mat)
        k = omps._truncate(s, cut, max_bond)
        kept = rows[:k]
        if polish and u is None:
            kept = 1.5 * kept - 0.5 * (kept @ kept.T) @ kept
        core = round_to(kept, storage)
        if "core" in tamper:
            core = tamper["core"](i, rows, k, core)
        if u is None:
            carry = carry_product(mat, core, storage, accumulate, reverse)
        else:
            carry = round_to(u[:, :k] * s[:k], storage)
        if "carry" in tamper:
            carry = tamper["carry"](i, mat, core, carry)
        cores[i], spectra[i] = core.reshape(k, dims[i], chi_r), s.copy()
        work, chi_r = carry, k
    cores[0] = work.reshape(1, dims[0], chi_r)
    if sweep_from == "left":
        cores = [c.transpose(2, 1, 0) for c in reversed(cores)]
        spectra = [None] + [spectra[L - j] for j in range(1, L)]
    return dict(cores=cores, spectra=spectra, bases=interface_bases(cores, sweep_from),
                bonds=[int(c.shape[2]) for c in cores[:-1]])


# ------------------------------------------------------------------------------------------------ gauge-free comparisons
def max_sin_theta(wa, wb):
    """Sine of the largest principal angle between the row spaces of ``wa`` and ``wb`` (orthonormal rows, the same
    number of them): ``sqrt(1 - sigma_min(wa wb^T)^2)``, evaluated as ``||wa (I - wb^T wb)||_2`` -- the same quantity
    for orthonormal rows, without the cancellation that stops the first form at sqrt(eps)."""
    wa, wb = np.asarray(wa, dtype=np.float64), np.asarray(wb, dtype=np.float64)
    if wa.shape != wb.shape:
        return 1.0
    resid = wa - (wa @ wb.T) @ wb
    return float(min(1.0, np.linalg.norm(resid, 2)))


def isometry_defect(core, sweep_from="right"):
    """max |C C^T - I| on the ``k x (d chi_r)`` unfolding (right sweep); ``C^T C`` on ``(chi_l d) x k`` for the left."""
    c = np.asarray(core, dtype=np.float64)
    if sweep_from == "right":
        m = c.reshape(c.shape[0], -1)
        g = m @ m.T
    else:
        m = c.reshape(-1, c.shape[2])
        g = m.T @ m
    return float(np.abs(g - np.eye(g.shape[0])).max())


def site0_defect(core_end, w, x, sweep_from="right"):
    """``||C_0 - X_(0) W_1^T||_F / ||X||_F``: the carrying end of the chain against the volume projected on the sweep's
    OWN basis of the neighbouring bond (``w`` = W_1, ``k_1 x N_1``).  Left sweep: C_{L-1} against ``W_{L-1} X``."""
    dense = to_site_order(x)
    c = np.asarray(core_end, dtype=np.float64)
    if sweep_from == "right":
        d0 = c.shape[1]
        diff = c.reshape(d0, -1) - dense.reshape(d0, -1) @ w.T
    else:
        d = c.shape[1]
        diff = c.reshape(-1, d) - w @ dense.reshape(-1, d)
    return float(np.linalg.norm(diff) / np.linalg.norm(dense))


def relative_gap(s, k):
    """(s_k - s_{k+1}) / s_0 behind the k-th kept value (s_{k+1} = 0 past the end)."""
    nxt = s[k] if k < len(s) else 0.0
    return float((s[k - 1] - nxt) / s[0])


# ------------------------------------------------------------------------------------------------ route model
# What the cases are meant to reach, restated from the sweep's documented rules (include/ndmps_hip.h) so that
# the CPU tests can say which route a case takes; where the library has a host query the CPU tests assert it instead.
MERGE_MAX = 512   # largest raw Gram order of the merged trailing run
TOPK_MAX_K = 128  # largest bond cap whose ranks are decided on the device


def merge_start(dims, max_bond):
    """First site of the merged trailing run, ``len(dims)`` when nothing is merged."""
    L, numel = len(dims), int(np.prod(dims, dtype=np.int64))
    if not max_bond:
        return L
    best, right = L, 1
    for i in range(L - 1, 0, -1):
        n_i = right * dims[i]
        if right > max_bond or n_i > MERGE_MAX or numel // n_i < n_i:
            break
        best, right = i, n_i
    return L if best >= L - 1 else best


# ------------------------------------------------------------------------------------------------ the cases
def _member(ranks, seed, tail=None):
    return dict(ranks=list(ranks), seed=int(seed), tail=tail)


def _case(shape, members, cap, route, storage="f32", cutoff=DEFAULT_CUTOFF, sweep_from="right", routes=()):
    """``members``: the volumes of the case's lockstep group (at most 4), each with its own planted ranks; ``cap``: the
    bond cap (None: exact sweep); ``route``: what the case is meant to reach; ``routes``: the environment switches the
    case is also meant to be run under, in addition to the default route."""
    assert 1 <= len(members) <= 4 and int(np.prod(shape)) <= 64 ** 3
    return dict(shape=tuple(shape), members=members, cap=cap, cutoff=cutoff, storage=storage, sweep_from=sweep_from,
                route=route, routes=tuple(routes))


SWITCHES = ("NDMPS_SWEEP_NO_MERGE", "NDMPS_SWEEP_HOST_RANK", "NDMPS_SWEEP_JACOBI")

_M16 = [_member([8, 8, 8], 16010), _member([8, 9, 8], 1602, tail=([8, 16, 8], 1e-2))]
_M64 = [_member([8, 32, 32, 32, 8], 64010, tail=([8, 48, 48, 48, 8], 1e-2)),
        _member([8, 33, 32, 33, 8], 64063, tail=([8, 48, 48, 48, 8], 1e-2))]
# bf16 members of their own: with the seeds above the subspace yardstick of bond 1 (which gathers the rounding of every
# site) reaches 0.013 .. 0.022, and MARGIN times that is no bar (VACUOUS); only the seeds differ (planted ranks and tails
# are those of _M16 and _M64), and they keep every bf16 bar below 0.1
_M16_BF16 = [_member([8, 8, 8], 16110), _member([8, 9, 8], 16234, tail=([8, 16, 8], 1e-2))]
_M64_BF16 = [_M64[0], _member([8, 33, 32, 33, 8], 64306, tail=([8, 48, 48, 48, 8], 1e-2))]

CASES = {
    # merged run of two sites (2 and 3) on the site-order tensor; orders 8 and 64
    "merged16_f32": _case((16, 16, 16), _M16, 8, "merged run, unfused", routes=SWITCHES),
    "merged16_f64": _case((16, 16, 16), _M16, 8, "merged run, unfused", storage="f64"),
    "merged16_bf16": _case((16, 16, 16), _M16_BF16, 8, "merged run, unfused", storage="bf16"),
    # merge width 64, k = 32: resident solver, gathered streamed projection, site 3 of order 256
    "cap32_f32": _case((64, 64, 64), _M64, 32, "fused encode, gathered projection", routes=SWITCHES),
    "cap32_f64": _case((64, 64, 64), _M64, 32, "merged run, unfused", storage="f64"),
    "cap32_bf16": _case((64, 64, 64), _M64_BF16, 32, "merged run, unfused", storage="bf16"),
    # rank against the cap on the fused route with the tile projection (k = 8): equal, one above, one below
    "rank_eq_cap": _case((32, 32, 32), [_member([8, 8, 8, 8], 32013), _member([8, 8, 8, 8], 3202)], 8, "fused encode"),
    "rank_above_cap": _case((32, 32, 32), [_member([8, 9, 9, 8], 3203, tail=([8, 16, 16, 8], 1e-2)),
                                           _member([8, 9, 9, 8], 32041, tail=([8, 16, 16, 8], 1e-2))], 8, "fused encode"),
    "rank_below_cap": _case((32, 32, 32), [_member([7, 7, 7, 7], 3205), _member([6, 7, 7, 5], 3206)], 8,
                            "fused encode, padded cores"),
    # one lockstep group whose members differ at the same bond: below the cap, at the cap, cut by it
    "nonuniform_group": _case((32, 32, 32), [_member([7, 7, 6, 7], 3207), _member([8, 8, 8, 8], 3208),
                                             _member([8, 9, 9, 8], 3209, tail=([8, 16, 16, 8], 1e-2))], 8,
                              "fused encode, padded cores; per-volume stages under HOST_RANK", routes=SWITCHES),
    # exact sweep: no cap, default cutoff; direct-full solver, zero eigenvalues in doubt measured as |A v|
    "exact": _case((16, 16, 16), [_member([5, 11, 6], 1603), _member([8, 20, 3], 1604)], None, "exact sweep",
                   routes=("NDMPS_SWEEP_JACOBI", "NDMPS_EXACT_JACOBI")),
    # a cap beyond the device rank decision
    "cap160": _case((16, 16, 16, 16), [_member([12, 130, 12], 44035), _member([10, 100, 14], 4402)], 160,
                    "host rank decision, merged run"),
    # three merged sites (3, 4 and 5; raw Gram of order 512, merge width 64) with ranks below the cap in padded cores: the
    # only start of a merged run other than L-2 that a shape of at most 64^3 reaches
    "merged3_f32": _case((64, 64, 64), [_member([8, 40, 40, 40, 8], 6506), _member([8, 30, 50, 30, 8], 6525)], 64,
                         "fused encode, three-site merged run, padded cores"),
    # mixed radix: a search over 3-D and 4-D mixed-radix shapes of at most 64^3 found none whose merged run is longer than
    # two sites (site dimensions are products of one factor per axis: 8 at the least, and the last site is wider); what
    # such shapes do reach is NO merged run -- the last site is wider than the cap and every site takes the ordinary path
    # (power-of-two shapes always merge sites L-2 and L-1); the 3-D plan is below the tile size of the permutation
    "mixed3d": _case((12, 44, 18), [_member([9, 9], 1201, tail=([16, 16], 1e-2)), _member([7, 6], 1202)], 8,
                     "no merged run, generic permutation"),
    "mixed4d": _case((16, 16, 8, 12), [_member([11, 11], 1611, tail=([20, 20], 1e-2)), _member([9, 7], 1612)], 10,
                     "no merged run"),
    "left": _case((32, 32, 32), [_member([8, 8, 7, 6], 3210), _member([8, 9, 9, 8], 32112, tail=([8, 16, 16, 8], 1e-2))], 8,
                  "mirrored sweep", sweep_from="left"),
}


def volumes(name):
    """The fp64 volumes of a case's members."""
    case = CASES[name]
    return [planted_volume(case["shape"], m["ranks"], m["seed"], m["tail"]) for m in case["members"]]


def expected_bonds(name, member):
    """min(planted (plus the tail's rank), cap, what the shape allows) at every bond."""
    case = CASES[name]
    dims = site_dims(case["shape"])
    out = []
    for i in range(1, len(dims)):
        full = min(int(np.prod(dims[:i])), int(np.prod(dims[i:])))
        planted = case["members"][member]["ranks"][i - 1]
        if case["members"][member]["tail"] is not None:  # the ranks of a sum add
            planted += case["members"][member]["tail"][0][i - 1]
        k = min(planted, full)
        out.append(min(k, case["cap"]) if case["cap"] else k)
    return out


_SWEEPS = {}


def sweeps(name):
    """Per member (x, reference_sweep, emulated_sweep at the case's storage type); computed once per process and
    shared (callers must not modify them)."""
    if name not in _SWEEPS:
        case = CASES[name]
        out = []
        for x in volumes(name):
            ref = reference_sweep(x, case["cutoff"], case["cap"], case["sweep_from"])
            emu = emulated_sweep(x, case["cutoff"], case["cap"], case["sweep_from"], case["storage"])
            out.append((x, ref, emu))
        _SWEEPS[name] = out
    return _SWEEPS[name]


# ------------------------------------------------------------------------------------------------ yardstick and bars
# bar of a quantity = MARGIN * yardstick + solver term.  MARGIN = max(4, 2 R rounded up to a power of two), R the largest
# ratio of one quantity between the "steps" model summed forwards and backwards (measured on the CPU by
# tests/test_sweep_cases_host.py::test_summation_order_spread_sets_the_margin, which fails when R reaches MARGIN / 2).
MARGIN = 8.0  # R = 3.0 (isometry defect of cap32_f64, member 1: 2 u against 6 u), theta 2.1, the others below 2
VACUOUS = 0.1  # a subspace bar of this size or more says nothing


def solver_eps(n):
    """The eigen-solver's contract (tests/test_gpu_parity.py::_check_topk): residual and orthogonality relative to the
    largest eigenvalue of an eigenproblem of order n."""
    return 2e-15 * max(int(n), 50)


def _swept_sites(name, member):
    """Per bond b = 1..L-1: (site that was decomposed for it, rows m, columns n of its unfolding) at the reference's
    bonds -- right sweep: site b, left sweep: site b - 1 (unfolded the other way round)."""
    case = CASES[name]
    dims = site_dims(case["shape"])
    L = len(dims)
    k = [1] + list(sweeps(name)[member][1]["bonds"]) + [1]
    out = {}
    for b in range(1, L):
        if case["sweep_from"] == "right":
            out[b] = (b, int(np.prod(dims[:b])), dims[b] * k[b + 1])
        else:
            out[b] = (b - 1, int(np.prod(dims[b:])), dims[b - 1] * k[b - 1])
    return out


def solver_terms(name, member):
    """What the device's eigen-solver may add to each quantity, from its own contract ``eps = solver_eps(order)`` with
    order = min(m, n) of the site's unfolding: the subspace of bond b by ``eps / gap2_b`` (gap2 = the relative gap of the
    SQUARED values behind the rank, Davis-Kahan on the Gram matrix); the isometry of the site's core by ``eps`` where the
    core is a set of eigenvectors (n <= m) and by ``eps (s_0 / s_k)^2`` where it is ``diag(1/s) U^T A`` (n > m); a kept
    value s_j by ``eps s_0^2 / s_j`` (d s = d(s^2) / 2 s, headroom 2).  Nothing for the site-0 defect and the
    reconstruction.  Far below u for f32 and bf16."""
    ref = sweeps(name)[member][1]
    theta, iso, spec = {}, {}, {}
    for b, (site, m, n) in _swept_sites(name, member).items():
        s, k = ref["spectra"][b], ref["bonds"][b - 1]
        eps = solver_eps(min(m, n))
        nxt = s[k] if k < len(s) else 0.0
        theta[b] = eps / ((s[k - 1] ** 2 - nxt ** 2) / s[0] ** 2)
        iso[site] = eps if n <= m else eps * (s[0] / s[k - 1]) ** 2
        spec[b] = eps * s[0] ** 2 / s[:k]
    return dict(theta=theta, iso=iso, site0=0.0, spec=spec, recon=0.0)


def sweep_quantities(cores, spectra, recon, x, ref, sweep_from):
    """The five gauge-free quantities of a sweep's output against the reference: dict(theta={bond: sin}, iso={site:
    defect}, site0=defect against the sweep's OWN basis, spec={bond: |s - s_ref| of the kept values}, recon=relative
    Frobenius distance to the reference's reconstruction)."""
    L = len(cores)
    bases = interface_bases(cores, sweep_from)
    inner = range(1, L) if sweep_from == "right" else range(L - 1)
    end, w_end = (0, 1) if sweep_from == "right" else (L - 1, L - 1)
    spec = {}
    for b in range(1, L):
        k = ref["bonds"][b - 1]
        got = np.asarray(spectra[b], dtype=np.float64)[:k]
        spec[b] = np.abs(got - ref["spectra"][b][:k]) if len(got) == k else np.full(k, np.inf)
    return dict(theta={b: max_sin_theta(bases[b], ref["bases"][b]) for b in range(1, L)},
                iso={i: isometry_defect(cores[i], sweep_from) for i in inner},
                site0=site0_defect(cores[end], bases[w_end], x, sweep_from), spec=spec,
                recon=float(np.linalg.norm(np.asarray(recon, dtype=np.float64) - ref["recon"]) / np.linalg.norm(ref["recon"])))


def _flat(q):
    """(quantity, key, value) of every scalar in a quantities dict (a spectrum counts by its worst value)."""
    for b, v in q["theta"].items():
        yield "theta", b, v
    for i, v in q["iso"].items():
        yield "iso", i, v
    yield "site0", None, q["site0"]
    for b, v in q["spec"].items():
        yield "spec", b, float(np.max(v))
    yield "recon", None, q["recon"]


def _floored(q, u, s0):
    return dict(theta={b: max(v, u) for b, v in q["theta"].items()}, iso={i: max(v, u) for i, v in q["iso"].items()},
                site0=max(q["site0"], u), spec={b: np.maximum(v, u * s0[b]) for b, v in q["spec"].items()},
                recon=max(q["recon"], u))


def _pointwise_max(a, b):
    return dict(theta={k: max(a["theta"][k], b["theta"][k]) for k in a["theta"]},
                iso={k: max(a["iso"][k], b["iso"][k]) for k in a["iso"]}, site0=max(a["site0"], b["site0"]),
                spec={k: np.maximum(a["spec"][k], b["spec"][k]) for k in a["spec"]}, recon=max(a["recon"], b["recon"]))


_YARD = {}


def yardstick(name):
    """Per member the elementwise maximum of ``sweep_quantities`` over the model family ``MODELS`` ({svd, gram} x {exact,
    steps, steps reversed}), every value floored at u of the storage type (theta, the defects, the reconstruction) or at
    u s_0 (spectra): what a correct sweep in that storage type may show, up to the order of its sums.  Besides the five
    quantities each member's dict holds ``models`` (the floored quantities of every model, keyed as in ``MODELS``),
    ``spread`` (per quantity the largest ratio between "steps" forwards and backwards, either way round, over both
    routes) and ``vacuous`` (the number of bonds whose subspace bar ``MARGIN * theta + solver`` reaches ``VACUOUS``).
    Computed once per process; callers must not modify it."""
    if name not in _YARD:
        case = CASES[name]
        u, sf = U[case["storage"]], case["sweep_from"]
        out = []
        for member, (x, ref, _) in enumerate(sweeps(name)):
            s0 = {b: ref["spectra"][b][0] for b in range(1, len(ref["cores"]))}
            models = {}
            for route, acc, rev in MODELS:
                emu = emulated_sweep(x, case["cutoff"], case["cap"], sf, case["storage"], acc, route, rev,
                                     polish=case["storage"] == "f64")
                if emu["bonds"] != ref["bonds"]:
                    raise AssertionError(f"{name}[{member}]: model {route}/{acc}/{rev} decides the bonds {emu['bonds']}, "
                                         f"the reference {ref['bonds']}")
                rec = reconstruction(emu["cores"], x.shape)
                models[(route, acc, rev)] = _floored(sweep_quantities(emu["cores"], emu["spectra"], rec, x, ref, sf), u, s0)
            yard = None
            for q in models.values():
                yard = q if yard is None else _pointwise_max(yard, q)
            yard = dict(yard)
            spread = {}
            for route in ("svd", "gram"):
                fwd, bwd = dict(), dict()
                for qn, key, v in _flat(models[(route, "steps", False)]):
                    fwd[(qn, key)] = v
                for qn, key, v in _flat(models[(route, "steps", True)]):
                    bwd[(qn, key)] = v
                for (qn, key), v in fwd.items():
                    spread[qn] = max(spread.get(qn, 1.0), v / bwd[(qn, key)], bwd[(qn, key)] / v)
            solver = solver_terms(name, member)
            yard.update(models=models, spread=spread,
                        vacuous=sum(MARGIN * yard["theta"][b] + solver["theta"][b] >= VACUOUS for b in yard["theta"]))
            out.append(yard)
        _YARD[name] = out
    return _YARD[name]


class SweepCheckError(AssertionError):
    """A failed comparison of ``check_sweep``; ``check`` names it: "shape", "bonds", "padding", "state", "isometry",
    "theta", "site0", "spectra" or "recon"."""

    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


def check_sweep(cores, spectra, recon, x, ref, yard, case, margin, solver, padded=None, boundary=None, norm_value=None):
    """Every comparison of a sweep's output with the reference, on plain NumPy arrays, for ``case = (name, member)``:
    ``cores`` (chi_l, d, chi_r) in the reference's site order, ``spectra`` per bond (index 0 unused), ``recon`` the
    volume the sweep's own decoder returns, ``x`` the fp64 volume, ``ref`` its ``reference_sweep``, ``yard`` its entry of
    ``yardstick(name)``, ``solver`` its ``solver_terms`` (None: no solver terms).  Bar of a quantity: ``margin * yard +
    solver``.  Exact: shapes and finiteness, the bonds (``expected_bonds``), and where given ``padded`` (cap-shaped cores:
    exactly zero outside the cut core, exactly the core inside), ``boundary`` (row i == (min, max) of core i) and
    ``norm_value`` (the Frobenius norm of the norm-carrying core to 4 u).  Raises ``SweepCheckError`` naming case,
    member, site or bond, value and bar; returns the measured quantities."""
    name, member = case
    cs = CASES[name]
    u, sf = U[cs["storage"]], cs["sweep_from"]
    tag = f"{name}[{member}]"
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    L = len(ref["cores"])
    if len(cores) != L or any(c.ndim != 3 for c in cores):
        raise SweepCheckError("shape", f"{tag}: {len(cores)} cores of dims {[c.ndim for c in cores]}, expected {L} of 3")
    bonds = [int(c.shape[2]) for c in cores[:-1]]
    if bonds != expected_bonds(name, member):
        raise SweepCheckError("bonds", f"{tag}: bonds {bonds}, expected {expected_bonds(name, member)}")
    for i, c in enumerate(cores):
        if c.shape != ref["cores"][i].shape:
            raise SweepCheckError("shape", f"{tag} site {i}: core of shape {c.shape}, expected {ref['cores'][i].shape}")
        if not np.isfinite(c).all():
            raise SweepCheckError("shape", f"{tag} site {i}: core is not finite")
    if np.shape(recon) != x.shape or not np.isfinite(recon).all():
        raise SweepCheckError("shape", f"{tag}: reconstruction of shape {np.shape(recon)} or not finite")
    if padded is not None:
        dirty = {}
        for i, (p, c) in enumerate(zip(padded, cores)):
            p = np.array(p, dtype=np.float64)
            if p.ndim != 3 or any(ps < cs for ps, cs in zip(p.shape, c.shape)):
                raise SweepCheckError("padding", f"{tag} site {i}: padded core of shape {p.shape} around {c.shape}")
            if not np.array_equal(p[: c.shape[0], :, : c.shape[2]], c):
                raise SweepCheckError("padding", f"{tag} site {i}: the cut core differs from the padded core's leading block")
            p[: c.shape[0], :, : c.shape[2]] = 0.0
            if np.count_nonzero(p):  # NaN and inf count as non-zero
                dirty[i] = (int(np.count_nonzero(p)), float(np.abs(p).max()))
        if dirty:
            raise SweepCheckError("padding", f"{tag}: non-zeros behind the rank, bar 0 -- site: (count, largest) = {dirty}")
    if boundary is not None:
        b = np.asarray(boundary, dtype=np.float64)
        want = np.array([[c.min(), c.max()] for c in cores])
        if b.shape != want.shape or not np.array_equal(b, want):
            raise SweepCheckError("state", f"{tag}: boundary_list {b.tolist()} is not (min, max) of the cores {want.tolist()}")
    end, w_end = (0, 1) if sf == "right" else (L - 1, L - 1)
    if norm_value is not None:
        want = float(np.linalg.norm(cores[end]))
        if not abs(float(norm_value) - want) <= 4 * u * want:
            raise SweepCheckError("state", f"{tag}: norm_value {float(norm_value)!r}, the norm of core {end} is {want!r}: "
                                           f"off by {abs(float(norm_value) - want) / want:.3e}, bar {4 * u:.3e}")
    for b in range(1, L):
        k = bonds[b - 1]
        if spectra[b] is None or len(spectra[b]) < k or not np.isfinite(np.asarray(spectra[b], dtype=np.float64)[:k]).all():
            raise SweepCheckError("spectra", f"{tag} bond {b}: fewer than {k} finite singular values")
    got = sweep_quantities(cores, spectra, recon, x, ref, sf)
    zero = dict(theta={}, iso={}, site0=0.0, spec={}, recon=0.0)
    sol = solver or zero

    def bar(qn, key):
        if key is None:
            return margin * yard[qn] + sol[qn]
        return margin * yard[qn][key] + sol[qn].get(key, 0.0)

    for i, v in got["iso"].items():
        if not v <= bar("iso", i):
            raise SweepCheckError("isometry", f"{tag} site {i}: isometry defect {v:.3e}, bar {bar('iso', i):.3e}")
    for b, v in got["theta"].items():
        if not v <= bar("theta", b):
            raise SweepCheckError("theta", f"{tag} bond {b}: subspace error {v:.3e}, bar {bar('theta', b):.3e}")
    if not got["site0"] <= bar("site0", None):
        raise SweepCheckError("site0", f"{tag} site {end}: defect {got['site0']:.3e} against its own basis, "
                                       f"bar {bar('site0', None):.3e}")
    for b, v in got["spec"].items():
        over = v - bar("spec", b)
        if not (over <= 0).all():
            j = int(np.argmax(over))
            raise SweepCheckError("spectra", f"{tag} bond {b}: |s_{j} - s_ref| = {v[j]:.3e}, bar "
                                             f"{np.broadcast_to(bar('spec', b), v.shape)[j]:.3e}")
    if not got["recon"] <= bar("recon", None):
        raise SweepCheckError("recon", f"{tag}: reconstruction off the reference's by {got['recon']:.3e}, "
                                       f"bar {bar('recon', None):.3e}")
    return got


def worst_ratios(got, yard, margin, solver):
    """Per quantity the largest value / bar of ``check_sweep``'s return value (for reports)."""
    out = {}
    for qn in ("theta", "iso", "spec"):
        out[qn] = max(float(np.max(np.asarray(got[qn][k]) / (margin * np.asarray(yard[qn][k]) + np.asarray(solver[qn][k]))))
                      for k in got[qn])
    for qn in ("site0", "recon"):
        out[qn] = got[qn] / (margin * yard[qn] + solver[qn])
    return out
