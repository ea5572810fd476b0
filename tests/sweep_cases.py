"""Planted-rank volumes for testing the TT-SVD sweep per bond and per core.  tests/test_sweep_cases_host.py shows on the
CPU that every case is well posed: the planted bonds are what the fp64 reference finds, every rank decision sits in a
gap of at least 1e-2 s_0 and survives the rounding of the storage type, and the case reaches the route it names.

Preparatory: the GPU suite that runs the library's sweep on these cases and compares its cores with
``reference_sweep``, with ``emulated_sweep`` as the yardstick, is not written yet; until it is, nothing here touches
the product's arithmetic, and the ``routes`` of a case are only checked against the library's host queries.

NumPy fp64 only; nothing of the product is imported.  The reference is ``oracle.mps.mps_from_dense`` on the site-order
tensor (``oracle.index_map``).  ``emulated_sweep`` is the same sweep with the input, the cores and every carried matrix
rounded to the storage type: a model of WHERE a sweep in that type rounds and of nothing else, used only as the
yardstick of the subspace and site-0 checks (a sweep that rounds where it must cannot do better than it; one that is
more than a small factor worse has a wrong vector somewhere).

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
                bonds=[int(c.shape[2]) for c in cores[:-1]])


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


def emulated_sweep(x, cutoff=DEFAULT_CUTOFF, max_bond=None, sweep_from="right", storage="f32"):
    """The sweep of ``reference_sweep`` with the input, every core and every carried matrix rounded to ``storage``: per
    site an fp64 SVD of the stored carry, the kept vectors rounded once (the core), the next carry = the stored carry
    times the stored core, rounded.  The relative cutoff is clamped at the storage type's floor.  Same dict."""
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
        _, s, vh = np.linalg.svd(mat, full_matrices=False)
        k = omps._truncate(s, cut, max_bond)
        core = round_to(vh[:k], storage)
        cores[i], spectra[i] = core.reshape(k, dims[i], chi_r), s.copy()
        work, chi_r = round_to(mat @ core.T, storage), k
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

CASES = {
    # merged run of two sites (2 and 3) on the site-order tensor; orders 8 and 64
    "merged16_f32": _case((16, 16, 16), _M16, 8, "merged run, unfused", routes=SWITCHES),
    "merged16_f64": _case((16, 16, 16), _M16, 8, "merged run, unfused", storage="f64"),
    "merged16_bf16": _case((16, 16, 16), _M16, 8, "merged run, unfused", storage="bf16"),
    # merge width 64, k = 32: resident solver, gathered streamed projection, site 3 of order 256
    "cap32_f32": _case((64, 64, 64), _M64, 32, "fused encode, gathered projection", routes=SWITCHES),
    "cap32_f64": _case((64, 64, 64), _M64, 32, "merged run, unfused", storage="f64"),
    "cap32_bf16": _case((64, 64, 64), _M64, 32, "merged run, unfused", storage="bf16"),
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
