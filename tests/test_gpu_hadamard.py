"""NDMPS.multiply / square on the MI355X (csrc/hadamard.hip, core/hadamard.py).

Bars, and where they come from:

* Sandwich kernel (``ndmps_hadamard_sandwich``, both forms, every site of a chain) against the fp64 NumPy product on the
  same cores and ``E``: per element ``(t + 1) u sum |A| |E| |B|`` with ``u = 2**-53`` and ``t`` the number of terms
  that are chained into one result (forward ``chi_a + chi_b``; environment ``d (chi_a' + chi_b')``), the standard bound
  of a sum of ``t`` products (the bound form of tests/test_gpu_axisop.py).  Cores are multiples of 1/8 in [-8, 8],
  exact in every storage type, so all storages share one reference; ``E`` is Gaussian on a grid of 2**-10, which keeps
  every partial sum of the NumPy reference exact in fp64 (40 bits at most), so the bound is held against the device's
  error alone.  The output buffer is pre-filled with a sentinel and everything past the results keeps it.
* Sketch (``oncore.hadamard_sketch``) against ``core.hadamard.emulate`` with the same random cores: identical ranks, and
  the decoded chains agree within ``1e-9 |product|`` (the projector is gauge-free and both sides work in fp64).
* End to end: ``|a.multiply(b).to_tensor() - a.to_tensor() * b.to_tensor()| <= tol |product|`` (Frobenius), tol from
  tests/test_gpu_lincomb.py (1e-5 for fp32 / bf16 work, 1e-7 for fp64).
* Truncation: the bar of tests/test_hadamard_host.py (``hadamard_cases.hmt_bar``) with ``best`` the error of
  ``from_tensor(dense product, max_bond)``, plus ``tol |product|``.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import hadamard as hd  # noqa: E402
from imgcompressionmps_amd.core import oncore  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.utils import core as _core  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

import hadamard_cases as hc  # noqa: E402  (tests/ is on the path: rootdir conftest)

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CODE = {F32: 0, BF16: 1, F64: 2}
SENTINEL = -12345.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _tol(*storages):
    return 1e-7 if any(s == F64 for s in storages) else 1e-5


def _bonds(dims, chi):
    return [1] + [int(min(chi, np.prod(dims[:i]), np.prod(dims[i:]))) for i in range(1, len(dims))] + [1]


def _object(cores, shape, storage, mode="Std"):
    """An NDMPS around host cores (nothing encoded), with its boundary_list and norm_value."""
    dev = [torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(storage).contiguous() for c in cores]
    dims = _core.site_dims(shape)
    obj = NDMPS._from_mps(DeviceMPS(dev), dims, tuple(shape), False, mode, len(shape))
    obj.update_boundary_list()
    obj.update_norm()
    return obj


def _dense(obj):
    """fp64 to_tensor (bf16 cores widened exactly first)."""
    o = obj.astype(F32) if obj.mps.dtype == BF16 else obj
    return np.asarray(o.to_tensor(), dtype=np.float64)


def _host(mps):
    return [c.to(F64).cpu().numpy() for c in mps.cores]


def _eighths(rng, shape):
    return rng.integers(-64, 65, size=shape).astype(np.float64) / 8


# ------------------------------------------------------------------------------------------------ the sandwich kernel
KERNEL_CASES = {
    "12x8x18": ((12, 8, 18), 5, 7),
    "6x20x9x4": ((6, 20, 9, 4), 5, 5),
    "64c-64x64": ((64, 64, 64), 64, 64),   # full 64 x 64 tiles, m = 4096
    "64c-64x3": ((64, 64, 64), 64, 3),
    "64c-80x4": ((64, 64, 64), 80, 4),     # a bond above 64: the general route at the sites that touch it
}
N_RHO = 3


@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    """Cores, E and the fp64 references with their bounds for every site and both forms (shared by the storages)."""
    shape, chi_a, chi_b = KERNEL_CASES[name]
    dims = [int(d) for d in _core.site_dims(shape)]
    ba, bb = _bonds(dims, chi_a), _bonds(dims, chi_b)
    rng = np.random.default_rng(sum(shape) + chi_a + chi_b)
    A = [_eighths(rng, (ba[k], dims[k], ba[k + 1])) for k in range(len(dims))]
    B = [_eighths(rng, (bb[k], dims[k], bb[k + 1])) for k in range(len(dims))]
    u = 2.0 ** -53
    sites = []
    for k, d in enumerate(dims):
        ca, ca2, cb, cb2 = ba[k], ba[k + 1], bb[k], bb[k + 1]
        Ef = np.round(rng.standard_normal((N_RHO, ca, cb)) * 1024) / 1024
        Ee = np.round(rng.standard_normal((N_RHO, d, ca2, cb2)) * 1024) / 1024
        fwd = np.einsum("aib,rac,cid->ribd", A[k], Ef, B[k], optimize=True)
        fwd_abs = np.einsum("aib,rac,cid->ribd", np.abs(A[k]), np.abs(Ef), np.abs(B[k]), optimize=True)
        env = np.einsum("aib,ribc,eic->rae", A[k], Ee, B[k], optimize=True)
        env_abs = np.einsum("aib,ribc,eic->rae", np.abs(A[k]), np.abs(Ee), np.abs(B[k]), optimize=True)
        sites.append(dict(ca=ca, ca2=ca2, cb=cb, cb2=cb2, d=d, E=(Ef, Ee), want=(fwd, env),
                          bound=((ca + cb + 1) * u * fwd_abs, (d * (ca2 + cb2) + 1) * u * env_abs)))
    return A, B, sites


@pytest.mark.parametrize("sa,sb", [(F32, F32), (BF16, BF16), (F64, F64), (BF16, F64), (F32, BF16)],
                         ids=["f32", "bf16", "f64", "bf16*f64", "f32*bf16"])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_sandwich_against_its_bound(name, sa, sb):
    lib = _lib.load()
    A, B, sites = _kernel_case(name)
    worst = 0.0
    for k, s in enumerate(sites):
        a = torch.from_numpy(A[k]).to(DEV).to(sa).contiguous()
        b = torch.from_numpy(B[k]).to(DEV).to(sb).contiguous()
        ws = torch.empty(8 * (a.numel() + b.numel() + N_RHO * s["ca"] * s["d"] * s["cb2"]) + 768, dtype=torch.uint8, device=DEV)
        for form in (0, 1):
            E = torch.from_numpy(np.ascontiguousarray(s["E"][form])).to(DEV)
            want, bound = s["want"][form], s["bound"][form]
            out = torch.full((want.size + 64,), SENTINEL, dtype=F64, device=DEV)
            rc = lib.ndmps_hadamard_sandwich(form, s["ca"], s["d"], s["ca2"], s["cb"], s["cb2"], CODE[sa], a.data_ptr(),
                                             CODE[sb], b.data_ptr(), N_RHO, E.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _lib.stream_ptr())
            assert rc == _lib.OK, lib.ndmps_last_error()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got[want.size:] == SENTINEL), (name, k, form)
            err = np.abs(got[: want.size].reshape(want.shape) - want)
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (name, k, form, float(np.max(err / np.maximum(bound, 1e-300))))
    print(f"sandwich {name}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ sketch against emulate
def _graded_cores(shape, chi, seed):
    """Gaussian cores whose right bond index b carries the weight 2**-b: the spectrum of a compressed image."""
    dims = [int(d) for d in _core.site_dims(shape)]
    bonds = _bonds(dims, chi)
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((bonds[k], dims[k], bonds[k + 1])) * 2.0 ** -np.arange(bonds[k + 1])[None, None, :]
            for k in range(len(dims))]


def _sketch_and_emulate(a_cores, b_cores, shape, storage, max_bond, oversample, seed):
    a, b = _object(a_cores, shape, storage), _object(b_cores, shape, storage)
    ah, bh = _host(a.mps), _host(b.mps)  # what the storage type holds
    dims = a.mps.dims
    ell = hd.sketch_bonds(dims, a.mps.bonds, b.mps.bonds, max_bond, oversample)
    R = hd.sketch_cores(dims, ell, seed)
    got = oncore.hadamard_sketch(a.mps, b.mps, ell, R)
    want, ranks = hd.emulate(ah, bh, dims, ell, R)
    return got, want, ranks, hc.dense_product(ah, bh)


@pytest.mark.parametrize("oversample", [4, 8])
def test_sketch_of_planted_ranks_matches_emulate(oversample):
    a_cores, b_cores = hc.planted(0)
    got, want, ranks, product = _sketch_and_emulate(a_cores, b_cores, (32, 32, 32), F64, 12, oversample, 0)
    assert got.bonds == ranks == hc.PLANTED_RANKS
    assert all(c.dtype == F64 for c in got.cores)
    dist = np.linalg.norm(mps_to_dense(_host(got)) - mps_to_dense(want)) / np.linalg.norm(product)
    print(f"planted p {oversample}: sketch vs emulate {dist:.2e}")
    assert dist <= 1e-9
    assert hc.rel_err(_host(got), product) <= 1e-10
    for c in _host(got)[:-1]:
        q = c.reshape(-1, c.shape[2])
        assert np.max(np.abs(q.T @ q - np.eye(q.shape[1]))) <= 1e-12


@pytest.mark.parametrize("storage", [F32, F64], ids=["f32", "f64"])
def test_sketch_at_bond_64_matches_emulate(storage):
    shape = (64, 64, 64)
    got, want, ranks, product = _sketch_and_emulate(_graded_cores(shape, 64, 1), _graded_cores(shape, 64, 2), shape, storage,
                                                    16, 16, 3)
    assert got.bonds == ranks
    dist = np.linalg.norm(mps_to_dense(_host(got)) - mps_to_dense(want)) / np.linalg.norm(product)
    print(f"chi 64 {storage}: ranks {ranks} sketch vs emulate {dist:.2e}")
    assert dist <= 1e-9


# ------------------------------------------------------------------------------------------------ end to end
def _planted_exact(seed):
    """a of true bond 3 and b of true bond 4 in bond 10, exact in every storage type: cores in multiples of 1/8,
    zero-padded and gauged by signed permutations with power-of-two scales."""
    rng = np.random.default_rng(seed)
    dims = hc.PLANTED_DIMS
    L = len(dims)
    chi = _bonds(dims, 10)  # [1, 8, 10, 10, 8, 1]: no bond above what an unfolding can have (the decoders insist)
    out = []
    for true in (3, 4):
        cores = [_eighths(rng, ((1 if k == 0 else true), dims[k], (1 if k == L - 1 else true))) for k in range(L)]
        perm = [None] + [rng.permutation(chi[k]) for k in range(1, L)] + [None]
        scale = [None] + [2.0 ** rng.integers(-1, 2, size=chi[k]) * rng.choice([-1.0, 1.0], size=chi[k])
                          for k in range(1, L)] + [None]
        emb = []
        for k, c in enumerate(cores):
            p = np.zeros((chi[k], dims[k], chi[k + 1]))
            p[: c.shape[0], :, : c.shape[2]] = c
            if k > 0:  # G_k^{-1} on the left
                p = (p / scale[k][:, None, None])[np.argsort(perm[k])]
            if k < L - 1:  # G_{k+1} on the right
                p = (p * scale[k + 1][None, None, :])[:, :, np.argsort(perm[k + 1])]
            emb.append(p)
        out.append(emb)
    return out


def _check_gauge_and_spectra(obj, bonds):
    assert obj.mps.bonds == bonds
    for c in _host(obj.mps)[1:]:
        q = c.reshape(c.shape[0], -1)
        assert np.max(np.abs(q @ q.T - np.eye(q.shape[0]))) <= (1e-10 if obj.mps.dtype == F64 else 1e-4)
    spec = obj.sweep_spectra
    assert spec[0] is None and [len(s) for s in spec[1:]] == bonds[1:-1]
    assert obj.norm is False


@pytest.mark.parametrize("kw", [dict(), dict(max_bond=16, oversample=4)], ids=["exact", "sketched"])
@pytest.mark.parametrize("sa,sb", [(F32, F32), (BF16, F32), (F64, F64), (F32, F64)], ids=["f32", "bf16*f32", "f64", "f32*f64"])
def test_multiply_reveals_planted_ranks(sa, sb, kw):
    ac, bc = _planted_exact(5)
    shape = (32, 32, 32)
    a, b = _object(ac, shape, sa), _object(bc, shape, sb)
    # the storage-exact gauges keep the planted structure, so the dense references agree with the fp64 product
    want = _dense(a) * _dense(b)
    out = a.multiply(b, **kw)
    assert out.mps.dtype == (F64 if F64 in (sa, sb) else F32)
    err = np.linalg.norm(_dense(out) - want) / np.linalg.norm(want)
    print(f"multiply planted {sa} {sb} {kw}: rel err {err:.2e} bonds {out.mps.bonds}")
    assert err <= _tol(sa, sb)
    _check_gauge_and_spectra(out, hc.PLANTED_RANKS)


def test_dtype_argument_sets_the_storage():
    ac, bc = _planted_exact(6)
    a, b = _object(ac, (32, 32, 32), F32), _object(bc, (32, 32, 32), F32)
    assert a.multiply(b, dtype=F64).mps.dtype == F64
    assert a.multiply(b, dtype=BF16).mps.dtype == BF16
    assert _object(ac, (32, 32, 32), F64).multiply(b, dtype=F32).mps.dtype == F32


def test_box_mask_times_bond_64_object():
    shape = (64, 64, 64)
    box = np.zeros(shape, dtype=np.float32)
    box[:41, 17:, :33] = 1.0  # one edge per axis: two states per axis, bond <= 8
    mask = NDMPS.from_tensor(box, device=DEV)
    assert max(mask.mps.bonds) <= 8
    obj = _object(_graded_cores(shape, 64, 4), shape, F32)
    want = _dense(mask) * _dense(obj)
    out = mask.multiply(obj)  # sketch bonds chi_mask * 64 <= 512: the exact product
    err = np.linalg.norm(_dense(out) - want) / np.linalg.norm(want)
    print(f"mask x chi 64: rel err {err:.2e} bonds {out.mps.bonds}")
    assert err <= _tol(F32)
    outside = np.asarray(out.to_tensor(), dtype=np.float64)[box == 0]
    assert np.linalg.norm(outside) <= _tol(F32) * np.linalg.norm(want)


def test_square_and_seed_reproducibility():
    shape = (32, 32, 32)
    a = NDMPS.from_tensor(synthetic_mri(shape, seed=11), max_bond=12, device=DEV)
    sq, mu = a.square(max_bond=16, seed=4), a.multiply(a, max_bond=16, seed=4)
    again = a.multiply(a, max_bond=16, seed=4)
    other = a.multiply(a, max_bond=16, seed=5)
    for x, y, z in zip(sq.mps.cores, mu.mps.cores, again.mps.cores):
        assert torch.equal(x, y) and torch.equal(y, z)
    assert any(not torch.equal(x, y) for x, y in zip(mu.mps.cores, other.mps.cores))
    want = _dense(a) ** 2
    best = np.linalg.norm(_dense(NDMPS.from_tensor(want.astype(np.float32), max_bond=16, device=DEV)) - want)
    err = np.linalg.norm(_dense(sq) - want)
    assert err <= hc.hmt_bar(a.mps.L, 16, 16, best, np.linalg.norm(want)) + _tol(F32) * np.linalg.norm(want)


# ------------------------------------------------------------------------------------------------ truncation
def test_truncated_product_of_two_images():
    shape = (64, 64, 64)
    a = NDMPS.from_tensor(synthetic_mri(shape, seed=2025), max_bond=16, device=DEV)
    b = NDMPS.from_tensor(synthetic_mri(shape, seed=7), max_bond=16, device=DEV)
    want = _dense(a) * _dense(b)
    norm = np.linalg.norm(want)
    best = np.linalg.norm(_dense(NDMPS.from_tensor(want.astype(np.float32), max_bond=32, device=DEV)) - want)
    out = a.multiply(b, max_bond=32)
    err = np.linalg.norm(_dense(out) - want)
    bar = hc.hmt_bar(a.mps.L, 32, 32, best, norm) + _tol(F32) * norm
    print(f"truncated: error {err:.4e} best {best:.4e} ratio {err / best:.3f} bar {bar:.4e} bonds {out.mps.bonds}")
    assert max(out.mps.bonds) <= 32
    assert err <= bar


# ------------------------------------------------------------------------------------------------ zero and errors
def _digit_mask(shape, site, digit, storage=F32):
    """The indicator of ``digit`` of axis 0 at ``site``: a bond-1 chain, exact."""
    fa = _core.get_factorlist(tuple(shape))[0]
    cores = []
    for k, row in enumerate(fa):
        c = np.ones([int(v) for v in row])
        if k == site:
            c[np.arange(int(row[0])) != digit] = 0.0
        cores.append(c.reshape(1, -1, 1))
    return _object(cores, shape, storage)


def test_disjoint_masks_give_the_zero_mps():
    shape = (32, 32, 32)
    a, b = _digit_mask(shape, 2, 0), _digit_mask(shape, 2, 1)
    assert np.linalg.norm(_dense(a) * _dense(b)) == 0.0 and np.linalg.norm(_dense(a)) > 0
    for kw in (dict(), dict(max_bond=4)):
        out = a.multiply(b, **kw)
        assert out.mps.bonds == [1] * (out.mps.L + 1)
        assert all(float(c.abs().max()) == 0.0 for c in out.mps.cores)
        assert all(np.array_equal(s, [0.0]) for s in out.sweep_spectra[1:])
        assert float(out.norm_value) == 0.0
    same = a.multiply(a)
    assert np.linalg.norm(_dense(same) - _dense(a)) <= _tol(F32) * np.linalg.norm(_dense(a))


def test_rejected_arguments():
    shape = (32, 32, 32)
    a = NDMPS.from_tensor(synthetic_mri(shape, seed=1), max_bond=8, device=DEV)
    with pytest.raises(TypeError):
        a.multiply(2.0)
    with pytest.raises(TypeError):
        a * a
    with pytest.raises(ValueError, match="shape"):
        a.multiply(NDMPS.from_tensor(synthetic_mri((16, 32, 32), seed=1), max_bond=8, device=DEV))
    dct = NDMPS.from_tensor(synthetic_mri(shape, seed=1), max_bond=8, mode="DCT", device=DEV)
    with pytest.raises(ValueError, match="DCT"):
        dct.multiply(dct, max_bond=8)
    with pytest.raises(ValueError, match="mode"):
        a.multiply(dct, max_bond=8)
    big = _object(_graded_cores((64, 64, 64), 64, 0), (64, 64, 64), F32)
    with pytest.raises(ValueError, match="pass max_bond"):
        big.multiply(big)
    assert big.multiply(big, max_bond=8, oversample=600).mps.bonds[3] <= 8  # sketch bonds capped by prod d = 512 here
    huge = _object(_graded_cores((256, 256, 256), 64, 0), (256, 256, 256), F32)  # prod d reaches 4096
    with pytest.raises(ValueError, match=r"must be <= 512"):
        huge.multiply(huge, max_bond=300, oversample=300)
    for kw in (dict(oversample=-1), dict(seed=0.5), dict(cutoff=-1.0), dict(max_bond=0), dict(dtype=torch.float16)):
        with pytest.raises(ValueError):
            a.multiply(a, **{**dict(max_bond=8), **kw})


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.load()
    ac, bc = hc.planted(1)
    a, b = _object(ac, (32, 32, 32), F64), _object(bc, (32, 32, 32), F64)
    L, dims = a.mps.L, a.mps.dims
    ell = hd.sketch_bonds(dims, a.mps.bonds, b.mps.bonds, 12, 4)
    R = np.concatenate([r.ravel() for r in hd.sketch_cores(dims, ell, 0)])
    c_dims = _lib.i64_array(dims)
    off, ws_bytes = (C.c_int64 * (L + 1))(), C.c_int64(0)

    def layout(ba, bb, el):
        return lib.ndmps_hadamard_layout(L, c_dims, _lib.i64_array(ba), _lib.i64_array(bb), _lib.i64_array(el), off,
                                         C.byref(ws_bytes))

    total = layout(a.mps.bonds, b.mps.bonds, ell)
    assert total == sum(ell[k] * dims[k] * ell[k + 1] for k in range(L)) == R.size
    assert [off[k + 1] - off[k] for k in range(L)] == [ell[k] * dims[k] * ell[k + 1] for k in range(L)]
    arena = torch.full((total,), SENTINEL, dtype=F64, device=DEV)
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=DEV)
    ranks = (C.c_int64 * (L + 1))()

    def call(ba=a.mps.bonds, bb=b.mps.bonds, el=ell, code_a=2, code_b=2, pa=a.mps._core_ptrs(), r=R, out=arena.data_ptr(),
             nbytes=ws.numel(), rk=ranks):
        return lib.ndmps_hadamard_sketch(L, c_dims, _lib.i64_array(ba), code_a, pa, _lib.i64_array(bb), code_b,
                                         b.mps._core_ptrs(), _lib.i64_array(el), None if r is None else r.ctypes.data_as(_lib.p_f64),
                                         0 if r is None else r.size, out, total, rk, ws.data_ptr(), nbytes, _lib.stream_ptr())

    bad_outer = list(a.mps.bonds)
    bad_outer[-1] = 2
    wide = list(ell)
    wide[2] = 513
    null_core = (C.c_void_p * L)(*[c.data_ptr() for c in a.mps.cores])
    null_core[1] = None
    for kw, msg in [(dict(code_a=3), b"dtype code"), (dict(code_b=-1), b"dtype code"), (dict(ba=bad_outer), b"outer bonds"),
                    (dict(el=wide), b"sketch bond"), (dict(el=[2] + list(ell[1:])), b"outer sketch"),
                    (dict(nbytes=64), b"workspace too small"), (dict(r=None), b"NULL"), (dict(out=None), b"NULL"),
                    (dict(rk=None), b"NULL"), (dict(pa=null_core), b"NULL core"), (dict(pa=None), b"NULL")]:
        assert call(**kw) == _lib.EINVAL, kw
        assert msg in lib.ndmps_last_error(), (kw, lib.ndmps_last_error())
    assert layout(bad_outer, b.mps.bonds, ell) == _lib.EINVAL
    assert layout(a.mps.bonds, b.mps.bonds, wide) == _lib.EINVAL
    core = a.mps.cores[1]
    sw = lambda **kw: lib.ndmps_hadamard_sandwich(*[kw.get(n, v) for n, v in [  # noqa: E731
        ("form", 0), ("ca", 10), ("d", 8), ("ca2", 10), ("cb", 10), ("cb2", 10), ("code_a", 2), ("A", core.data_ptr()),
        ("code_b", 2), ("B", core.data_ptr()), ("n", 1), ("E", ws.data_ptr()), ("out", arena.data_ptr()), ("ws", None),
        ("ws_bytes", 0), ("stream", _lib.stream_ptr())]])
    for kw in (dict(form=2), dict(code_a=5), dict(A=None), dict(E=None), dict(out=None), dict(n=0), dict(n=513), dict(ca=0),
               dict(ca=80, ca2=80)):  # the last one: the general route without a workspace
        assert sw(**kw) == _lib.EINVAL, kw
    torch.cuda.synchronize()
    assert bool((arena == SENTINEL).all())  # nothing was launched
    assert call() == _lib.OK
    assert [int(v) for v in ranks] == hc.PLANTED_RANKS
