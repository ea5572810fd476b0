"""GPU parity tests: the HIP path through the C ABI against the CPU oracle.

Tolerances (fp32 data in HBM, fp64 Gram / eigen / overlap accumulation):
  * permutation, quantised cores: bit-exact;
  * exact round trip: |x - to_tensor(from_tensor(x))| <= 2e-5 * max|x| (reference: 1e-10 in fp64);
  * truncated reconstruction vs oracle: relative Frobenius <= 2e-5, |dSSIM| <= 1e-5;
  * singular values vs oracle: 1e-5 relative to s_0;
  * norm_value^2 == mps@mps: 1e-6 relative (reference: 1e-12 in fp64).
Truncated results are "parity unpinned" at the quimb boundary (no known-answer vector in the
reference): they are compared with the oracle restatement and with
size-independent properties.
"""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from imgcompressionmps_amd.utils import core as hc  # noqa: E402
from imgcompressionmps_amd.utils import filetools as hft  # noqa: E402
from oracle import filetools as oft  # noqa: E402
from oracle import index_map as oim  # noqa: E402
from oracle import mps as omps  # noqa: E402
from oracle.metrics import compute_ssim_by_dim, synthetic_mri  # noqa: E402
from oracle.ndmps_oracle import OracleNDMPS  # noqa: E402

import eig_routes as er  # noqa: E402  (tests/ is on the path: rootdir conftest)

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device; the product has no CPU path")
    _lib.load()


def sp():
    return _lib.stream_ptr()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


# ----------------------------------------------------------------------------- permutation
PERM_SHAPES = [(32, 32), (8, 9), (4, 6), (30, 40, 50), (16, 16, 16), (12, 8, 20, 6), (7, 12), (1, 4),
               (64,), (64, 64, 64), (512, 680), (8, 512, 680), (96, 80, 112), (128, 128, 128), (5,)]


@pytest.mark.parametrize("shape", PERM_SHAPES, ids=str)
def test_permute_bit_exact(shape):
    lib = _lib.load()
    n = int(np.prod(shape))
    plan = _plan_for(shape, 0)
    flat_dest = oim.flat_destination(shape).reshape(-1)
    rng = np.random.default_rng(n)
    for dtype, nbytes in ((np.uint16, 2), (np.float32, 4), (np.float64, 8)):
        if dtype == np.uint16:
            src = rng.integers(0, 65535, size=n).astype(np.uint16)
            tsrc = torch.from_numpy(src.view(np.int16)).to(DEV)
        else:
            src = rng.standard_normal(n).astype(dtype)
            tsrc = torch.from_numpy(src).to(DEV)
        expect = np.empty_like(src)
        expect[flat_dest] = src  # the reference scatter, core/ndmps.py:66-71
        for enc, dec in ((lib.ndmps_encode_permute, lib.ndmps_decode_permute),
                         (lib.ndmps_encode_permute_generic, lib.ndmps_decode_permute_generic)):
            dense = torch.zeros_like(tsrc)
            _lib.check(enc(plan.handle, tsrc.data_ptr(), dense.data_ptr(), nbytes, sp()))
            got = dense.cpu().numpy().view(src.dtype)
            assert np.array_equal(got, expect), (shape, dtype)
            back = torch.zeros_like(tsrc)
            _lib.check(dec(plan.handle, dense.data_ptr(), back.data_ptr(), nbytes, sp()))
            assert np.array_equal(back.cpu().numpy().view(src.dtype), src), (shape, dtype)


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


@pytest.mark.parametrize("shape,count", [((128, 128, 128), 5), ((16, 16, 16), 40), ((30, 40, 50), 3), ((7, 12), 33),
                                         ((12, 8, 20, 6), 2)], ids=str)
def test_permute_of_a_group_in_one_launch_is_bit_exact(shape, count):
    """ndmps_encode_permute_many / ndmps_decode_permute_many (one launch per thirty-two volumes, tiled and generic plans,
    2 / 4 / 8-byte elements) against the single-volume calls, bit for bit, on separately allocated volumes."""
    lib = _lib.load()
    n = int(np.prod(shape))
    plan = _plan_for(shape, 0)
    gen = torch.Generator(device=DEV).manual_seed(n + count)
    for dt, nbytes in ((torch.int16, 2), (torch.float32, 4), (torch.float64, 8)):
        if dt == torch.int16:
            srcs = [torch.randint(-32768, 32767, (n,), dtype=dt, device=DEV, generator=gen) for _ in range(count)]
        else:
            srcs = [torch.randn(n, dtype=dt, device=DEV, generator=gen) for _ in range(count)]
        one = [torch.zeros_like(x) for x in srcs]
        for x, d in zip(srcs, one):
            _lib.check(lib.ndmps_encode_permute(plan.handle, x.data_ptr(), d.data_ptr(), nbytes, sp()))
        many = list(torch.zeros((count, n), dtype=dt, device=DEV).unbind(0))
        _lib.check(lib.ndmps_encode_permute_many(plan.handle, count, _ptrs(srcs), _ptrs(many), nbytes, sp()))
        assert all(torch.equal(a, b) for a, b in zip(one, many)), (shape, dt)
        back = [torch.zeros_like(x) for x in srcs]
        _lib.check(lib.ndmps_decode_permute_many(plan.handle, count, _ptrs(many), _ptrs(back), nbytes, sp()))
        assert all(torch.equal(a, b) for a, b in zip(srcs, back)), (shape, dt)
    with pytest.raises(ValueError):  # a volume permuted onto itself
        _lib.check(lib.ndmps_encode_permute_many(plan.handle, 2, _ptrs(srcs[:2]), _ptrs([many[0], srcs[1]]), 8, sp()))


@pytest.mark.parametrize("rows,n,count", [(64, 128, 3), (37, 512, 35), (9, 96, 4), (1001, 256, 2)])
def test_dct_and_scaling_of_a_group_in_one_launch(rows, n, count):
    """ndmps_dct_last_many_f32 / ndmps_idct_last_many_f32 / ndmps_scale_many_f32 against the single-volume calls, bit for
    bit (FFT route in chunks of thirty-two volumes, basis product for other row lengths)."""
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(rows * n + count)
    xs = [torch.rand((rows, n), dtype=torch.float32, device=DEV, generator=gen) for _ in range(count)]
    basis = torch.empty((n, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_dct_basis_f32(basis.data_ptr(), n, sp()))
    one = [torch.empty_like(x) for x in xs]
    for x, y in zip(xs, one):
        _lib.check(lib.ndmps_dct_last_f32(x.data_ptr(), y.data_ptr(), rows, n, basis.data_ptr(), sp()))
    many = list(torch.empty((count, rows, n), dtype=torch.float32, device=DEV).unbind(0))
    _lib.check(lib.ndmps_dct_last_many_f32(count, _ptrs(xs), _ptrs(many), rows, n, basis.data_ptr(), sp()))
    assert all(torch.equal(a, b) for a, b in zip(one, many))
    back_one = [torch.empty_like(x) for x in xs]
    for y, x in zip(one, back_one):
        _lib.check(lib.ndmps_idct_last_f32(y.data_ptr(), x.data_ptr(), rows, n, basis.data_ptr(), sp()))
    back_many = [torch.empty_like(x) for x in xs]
    _lib.check(lib.ndmps_idct_last_many_f32(count, _ptrs(many), _ptrs(back_many), rows, n, basis.data_ptr(), sp()))
    assert all(torch.equal(a, b) for a, b in zip(back_one, back_many))
    assert max(float((a - b).abs().max()) for a, b in zip(xs, back_many)) <= 3e-6
    # a stacked group is one tall matrix for the single call: the same bits again
    tall = torch.empty((count, rows, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_idct_last_f32(torch.stack(one).data_ptr(), tall.data_ptr(), count * rows, n, basis.data_ptr(), sp()))
    assert all(torch.equal(a, b) for a, b in zip(back_one, tall.unbind(0)))
    factors = [1.0 / (1.5 + i) for i in range(count)]
    want = [x.clone() for x in xs]
    for x, f in zip(want, factors):
        _lib.check(lib.ndmps_scale_f32(x.data_ptr(), rows * n, f, sp()))
    got = [x.clone() for x in xs]
    _lib.check(lib.ndmps_scale_many_f32(count, _ptrs(got), rows * n, _lib.f64_array(factors), sp()))
    assert all(torch.equal(a, b) for a, b in zip(want, got))


def test_permute_rejects_bad_arguments():
    lib = _lib.load()
    plan = _plan_for((8, 8), 0)
    t = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError):
        _lib.check(lib.ndmps_encode_permute(plan.handle, t.data_ptr(), t.data_ptr(), 4, sp()))
    with pytest.raises(ValueError):
        _lib.check(lib.ndmps_encode_permute(plan.handle, t.data_ptr(), torch.zeros(64, device=DEV).data_ptr(), 3, sp()))


def test_permute_256_cubed_is_a_bijection_and_morton():
    """Full BASELINE size through size-independent properties: decode(encode(x)) == x bit for
    bit, checksum preserved, and spot checks of the Z-order closed form."""
    lib = _lib.load()
    shape = (256, 256, 256)
    n = 256 ** 3
    plan = _plan_for(shape, 0)
    assert lib.ndmps_plan_is_tiled(plan.handle) == 1
    x = torch.arange(n, dtype=torch.int32, device=DEV)
    dense = torch.empty_like(x)
    _lib.check(lib.ndmps_encode_permute(plan.handle, x.data_ptr(), dense.data_ptr(), 4, sp()))
    back = torch.empty_like(x)
    _lib.check(lib.ndmps_decode_permute(plan.handle, dense.data_ptr(), back.data_ptr(), 4, sp()))
    assert torch.equal(back, x)
    assert int(dense.to(torch.int64).sum()) == n * (n - 1) // 2
    d = dense.cpu().numpy()
    rng = np.random.default_rng(0)
    for _ in range(200):
        xx, yy, zz = (int(v) for v in rng.integers(0, 256, 3))
        code = 0
        for b in range(8):
            code |= ((xx >> b) & 1) << (3 * b + 2) | ((yy >> b) & 1) << (3 * b + 1) | ((zz >> b) & 1) << (3 * b)
        assert d[code] == (xx * 256 + yy) * 256 + zz
    gen = torch.empty_like(x)
    _lib.check(lib.ndmps_encode_permute_generic(plan.handle, x.data_ptr(), gen.data_ptr(), 4, sp()))
    assert torch.equal(gen, dense)


# ------------------------------------------------------------------------------ dense blocks
GEMM_CASES = [(5, 7, 3), (33, 17, 65), (128, 128, 16), (200, 40, 136), (64, 512, 64), (1000, 8, 8),
              (8, 512, 8), (130, 129, 131), (1, 1, 1), (300, 64, 512)]


@pytest.mark.parametrize("m,n,k", GEMM_CASES)
def test_sgemm_and_dgemm(m, n, k):
    lib = _lib.load()
    rng = np.random.default_rng(m * 1000 + n * 10 + k)
    for ta in (0, 1):
        for tb in (0, 1):
            a = rng.standard_normal((k, m) if ta else (m, k))
            b = rng.standard_normal((n, k) if tb else (k, n))
            ref = (a.T if ta else a) @ (b.T if tb else b)
            scale = np.abs(a).sum(axis=0 if ta else 1).max() * np.abs(b).max() + 1e-30
            a32, b32 = dev(a, torch.float32), dev(b, torch.float32)
            c32 = torch.full((m, n), float("nan"), dtype=torch.float32, device=DEV)
            _lib.check(lib.ndmps_sgemm(ta, tb, m, n, k, a32.data_ptr(), a32.shape[1], b32.data_ptr(),
                                       b32.shape[1], c32.data_ptr(), n, sp()))
            ref32 = (a32.cpu().numpy().astype(np.float64).T if ta else a32.cpu().numpy().astype(np.float64)) @ (
                b32.cpu().numpy().astype(np.float64).T if tb else b32.cpu().numpy().astype(np.float64))
            assert np.abs(c32.cpu().numpy() - ref32).max() <= 4e-7 * scale * max(1, k ** 0.5)
            a64, b64 = dev(a), dev(b)
            c64 = torch.full((m, n), float("nan"), dtype=torch.float64, device=DEV)
            _lib.check(lib.ndmps_dgemm(ta, tb, m, n, k, a64.data_ptr(), a64.shape[1], b64.data_ptr(),
                                       b64.shape[1], c64.data_ptr(), n, sp()))
            assert np.abs(c64.cpu().numpy() - ref).max() <= 1e-14 * scale * max(1, k ** 0.5)


def test_sgemm_matches_fma_chain_on_integers_asymmetric():
    """A = I with an asymmetric B catches a transposed accumulator map (guide 3)."""
    lib = _lib.load()
    n = 96
    b = np.arange(n * n, dtype=np.float32).reshape(n, n) % 251
    a = np.eye(n, dtype=np.float32)
    ta, tb_ = dev(a), dev(b)
    c = torch.zeros((n, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_sgemm(0, 0, n, n, n, ta.data_ptr(), n, tb_.data_ptr(), n, c.data_ptr(), n, sp()))
    assert np.array_equal(c.cpu().numpy(), b)


@pytest.mark.parametrize("m,n", [(64, 8), (1000, 8), (4096, 64), (777, 33), (5000, 130), (16, 16), (3, 20),
                                 (20000, 512), (100, 257), (4096, 512), (300, 128), (1001, 136), (200001, 8),
                                 (1000, 5), (333, 680), (257, 131), (70000, 2)])
def test_gram_fp64(m, n):
    lib = _lib.load()
    a = np.random.default_rng(m + n).standard_normal((m, n)).astype(np.float32)
    ta = dev(a)
    g = torch.full((n, n), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_gram_workspace_bytes(m, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ndmps_gram_f32(ta.data_ptr(), m, n, n, g.data_ptr(), ws.data_ptr(), nbytes, sp()))
    ref = a.astype(np.float64).T @ a.astype(np.float64)
    got = g.cpu().numpy()
    assert np.array_equal(got, got.T)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("batch,m,n,k,ta,tb", [(3, 33, 17, 65, 0, 0), (5, 200, 64, 136, 0, 1), (2, 64, 512, 64, 1, 0),
                                               (7, 1000, 8, 8, 0, 0), (4, 130, 129, 131, 1, 1), (64, 16, 16, 16, 0, 1)])
def test_gemm_batched_equals_gemm_per_triple(batch, m, n, k, ta, tb):
    """ndmps_sgemm_batched / ndmps_dgemm_batched run the same tiles on operand triples taken from the kernel
    arguments: bit-identical to one ndmps_sgemm / ndmps_dgemm call per triple, and correct against NumPy."""
    lib = _lib.load()
    assert lib.ndmps_gemm_batched_max() >= 64
    rng = np.random.default_rng(batch * 7 + m)
    for dt, one, many, tol in ((torch.float32, lib.ndmps_sgemm, lib.ndmps_sgemm_batched, 4e-7),
                               (torch.float64, lib.ndmps_dgemm, lib.ndmps_dgemm_batched, 1e-14)):
        a = [dev(rng.standard_normal((k, m) if ta else (m, k)), dt) for _ in range(batch)]
        b = [dev(rng.standard_normal((n, k) if tb else (k, n)), dt) for _ in range(batch)]
        c1 = [torch.full((m, n), float("nan"), dtype=dt, device=DEV) for _ in range(batch)]
        c2 = [torch.full((m, n), float("nan"), dtype=dt, device=DEV) for _ in range(batch)]
        for x, y, z in zip(a, b, c1):
            _lib.check(one(ta, tb, m, n, k, x.data_ptr(), x.shape[1], y.data_ptr(), y.shape[1], z.data_ptr(), n, sp()))
        pa = (C.c_void_p * batch)(*[x.data_ptr() for x in a])
        pb = (C.c_void_p * batch)(*[x.data_ptr() for x in b])
        pc = (C.c_void_p * batch)(*[x.data_ptr() for x in c2])
        _lib.check(many(batch, ta, tb, m, n, k, pa, a[0].shape[1], pb, b[0].shape[1], pc, n, sp()))
        for x, y, z1, z2 in zip(a, b, c1, c2):
            assert torch.equal(z1, z2)
            x64, y64 = x.double().cpu().numpy(), y.double().cpu().numpy()
            ref = (x64.T if ta else x64) @ (y64.T if tb else y64)
            scale = np.abs(x64).sum(axis=0 if ta else 1).max() * np.abs(y64).max() + 1e-30
            assert np.abs(z2.double().cpu().numpy() - ref).max() <= tol * scale * max(1, k ** 0.5)
    with pytest.raises(ValueError):
        _lib.check(lib.ndmps_sgemm_batched(65, 0, 0, 1, 1, 1, pa, 1, pb, 1, pc, 1, sp()))


@pytest.mark.parametrize("batch,m,n", [(1, 4096, 512), (3, 1000, 200), (5, 300, 128), (32, 512, 512), (2, 20000, 384),
                                       (4, 257, 131), (32, 32768, 64), (3, 5000, 64), (2, 300, 100), (70, 700, 96), (2, 4099, 64), (66, 260, 64)])
def test_gram_batched_fp64(batch, m, n):
    """One launch for the Gram matrices of a group (n >= 128: 128 x 128 tiles; 64 < n < 128 and at least two
    matrices: 64 x 64 tiles; n == 64, the raw Gram of a bond cap of 32: the streaming kernel, with row counts that
    are and are not multiples of its 16-row steps and 128-row blocks, more than 64 matrices): exactly symmetric,
    fp64-accurate, and reproducible (a second call gives the same bits)."""
    lib = _lib.load()
    rng = np.random.default_rng(batch + m + n)
    mats = [dev(rng.standard_normal((m, n)).astype(np.float32), torch.float32) for _ in range(batch)]
    g = torch.full((batch, n, n), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_gram_batched_workspace_bytes(batch, m, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ptrs = (C.c_void_p * batch)(*[x.data_ptr() for x in mats])
    _lib.check(lib.ndmps_gram_batched_f32(batch, ptrs, m, n, n, g.data_ptr(), n * n, ws.data_ptr(), nbytes, sp()))
    first = g.clone()
    _lib.check(lib.ndmps_gram_batched_f32(batch, ptrs, m, n, n, g.data_ptr(), n * n, ws.data_ptr(), nbytes, sp()))
    assert torch.equal(first, g)
    for b in range(batch):
        a64 = mats[b].double().cpu().numpy()
        ref = a64.T @ a64
        got = g[b].cpu().numpy()
        assert np.array_equal(got, got.T)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    assert lib.ndmps_gram_batched_workspace_bytes(batch, m, 48) == 0  # narrower matrices: ndmps_gram_f32 per matrix
    assert lib.ndmps_gram_batched_workspace_bytes(1, m, 64) == 0      # a lone 64-column matrix as well


def _syevj(lib, g):
    n = g.shape[0]
    tg = dev(g)
    v = torch.empty((n, n), dtype=torch.float64, device=DEV)
    w = torch.empty(n, dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_syevj_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sweeps = C.c_int()
    _lib.check(lib.ndmps_syevj_f64(tg.data_ptr(), n, v.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes,
                                   C.byref(sweeps), sp()))
    return w.cpu().numpy(), v.cpu().numpy(), sweeps.value


@pytest.mark.parametrize("n", [5, 32, 40, 96, 512])
def test_block_jacobi_graded_spectrum(n):
    lib = _lib.load()
    rng = np.random.default_rng(100 + n)
    a = rng.standard_normal((2 * n, n)) * np.logspace(0, -5, n)[None, :]
    g = a.T @ a
    w, v, sweeps = _syevj(lib, g)
    ref = np.linalg.eigvalsh(g)[::-1]
    assert np.abs(w - ref).max() <= 2e-15 * max(n, 50) * ref[0]
    assert np.abs(v.T @ v - np.eye(n)).max() <= 2e-15 * max(n, 50)
    assert np.abs(g @ v - v * w[None, :]).max() <= 2e-15 * max(n, 50) * ref[0]
    assert sweeps <= 20


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 33, 64, 130, 256])
def test_syevj_against_lapack(n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n + 5, n))
    a[:, : n // 2] *= 1e-3  # graded spectrum
    g = a.T @ a
    tg = dev(g)
    v = torch.empty((n, n), dtype=torch.float64, device=DEV)
    w = torch.empty(n, dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_syevj_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sweeps = C.c_int()
    _lib.check(lib.ndmps_syevj_f64(tg.data_ptr(), n, v.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes,
                                   C.byref(sweeps), sp()))
    wv, vv = w.cpu().numpy(), v.cpu().numpy()
    ref = np.linalg.eigvalsh(g)[::-1]
    assert np.all(np.diff(wv) <= 0)
    assert np.abs(wv - ref).max() <= 1e-13 * ref[0]
    assert np.abs(vv.T @ vv - np.eye(n)).max() <= 2e-15 * max(n, 50)
    assert np.abs(vv @ np.diag(wv) @ vv.T - g).max() <= 2e-15 * max(n, 50) * ref[0]
    for j in range(n):  # sign convention: largest component positive
        assert vv[np.argmax(np.abs(vv[:, j])), j] > 0
    assert 1 <= sweeps.value <= 20


def test_syevj_rank_deficient_and_zero():
    lib = _lib.load()
    for g in (np.zeros((6, 6)), np.outer(np.arange(1.0, 9.0), np.arange(1.0, 9.0))):
        n = g.shape[0]
        tg = dev(g)
        v = torch.empty((n, n), dtype=torch.float64, device=DEV)
        w = torch.empty(n, dtype=torch.float64, device=DEV)
        nbytes = lib.ndmps_syevj_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ndmps_syevj_f64(tg.data_ptr(), n, v.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes, None, sp()))
        wv, vv = w.cpu().numpy(), v.cpu().numpy()
        assert np.allclose(np.sort(wv), np.linalg.eigvalsh(g), atol=1e-12 * max(1.0, np.abs(g).max()))
        assert np.abs(vv.T @ vv - np.eye(n)).max() <= 1e-13


# ------------------------------------------------------------------------------ reductions
def test_reductions_and_scale():
    lib = _lib.load()
    x = np.random.default_rng(1).standard_normal(100003).astype(np.float32)
    t = dev(x)
    ws = torch.empty(lib.ndmps_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    ss = C.c_double()
    _lib.check(lib.ndmps_sumsq_f32(t.data_ptr(), t.numel(), C.byref(ss), ws.data_ptr(), ws.numel(), sp()))
    assert math.isclose(ss.value, float(np.sum(x.astype(np.float64) ** 2)), rel_tol=1e-13)
    assert hft.minmax(t) == (float(x.min()), float(x.max()))
    _lib.check(lib.ndmps_scale_f32(t.data_ptr(), t.numel(), 0.25, sp()))
    assert np.array_equal(t.cpu().numpy(), x * np.float32(0.25))


def test_quantise_bit_exact_against_reference_semantics():  # larger random input vs the oracle; fixture: next test
    x = np.random.default_rng(2).standard_normal((9, 7, 5)).astype(np.float32)
    t = dev(x)
    for dt in (np.uint8, np.uint16):
        q = hft.to_numpy_uint(hft.scale_to_dtype(t, dt), dt)
        ref = oft.scale_to_dtype(x.astype(np.float64), dt)
        assert q.dtype == dt and np.array_equal(q, ref)
        back = hft.scale_back(hft.scale_to_dtype(t, dt), float(x.min()), float(x.max()), dt).cpu().numpy()
        refb = oft.scale_back(ref, float(x.min()), float(x.max()), dt)
        assert np.abs(back - refb).max() <= 1e-6 * np.abs(refb).max()
    with pytest.raises(ValueError):
        hft.scale_to_dtype(t, np.int32)


def test_quantiser_against_the_reference_generated_fixture(golden_dir):
    """The HIP quantiser / dequantiser on the INPUTS of tests/golden/filetools.npz against the outputs the reference's
    own utils/filetools.py:20-39 produced for them (tests/golden/make_golden_filetools.py): fp64 kernels on the fp64
    inputs and fp32 kernels on the fp32-representable inputs, quantised values bit for bit; scale_back bit for bit in
    fp64, and the fp32 kernel's result = the fp32 rounding of the reference's float64 result."""
    g = np.load(os.path.join(golden_dir, "filetools.npz"))
    for name in ("a", "b", "c"):
        for key, tdtype in ((name + "/x", torch.float64), (name + "/x32", torch.float32)):
            x = g[key]
            t = dev(x)
            assert t.dtype == tdtype
            prefix = name if key.endswith("/x") else name + "/x32"
            for dt in (np.uint8, np.uint16):
                n = np.dtype(dt).name
                dq = hft.scale_to_dtype(t, dt)
                q = hft.to_numpy_uint(dq, dt)
                assert q.dtype == dt and np.array_equal(q, g[f"{prefix}/{n}/q"]), (key, n)
                want = g[f"{prefix}/{n}/back"]
                back64 = hft.scale_back(dq, float(x.min()), float(x.max()), dt, out_dtype=torch.float64).cpu().numpy()
                assert np.array_equal(back64, want), (key, n)
                if tdtype == torch.float32:  # the fp32 kernel takes fp32 bounds: exact for fp32-representable input only
                    back32 = hft.scale_back(dq, float(x.min()), float(x.max()), dt).cpu().numpy()
                    assert back32.dtype == np.float32 and np.array_equal(back32, want.astype(np.float32)), (key, n)


# ------------------------------------------------------------------------------------ DCT
@pytest.mark.parametrize("rows,n", [(4, 8), (37, 680), (100, 50), (64, 512), (3, 1), (5, 64), (1001, 128), (262, 256),
                                    (1, 512), (4099, 512), (7, 1024), (9, 96)])
def test_dct_last_axis(rows, n):
    """Rows whose length is a power of two from 64 to 1024 take the O(N log N) kernel (FFT in LDS), every other
    length the basis product on the MFMA; both against SciPy's pocketfft, as the reference calls it
    (core/ndmps.py:63, :153), and against each other where both exist."""
    from scipy.fft import dct, idct

    lib = _lib.load()
    x = np.random.default_rng(n).random((rows, n)).astype(np.float32)
    t = dev(x)
    basis = torch.empty((n, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_dct_basis_f32(basis.data_ptr(), n, sp()))
    y = torch.empty_like(t)
    _lib.check(lib.ndmps_dct_last_f32(t.data_ptr(), y.data_ptr(), rows, n, basis.data_ptr(), sp()))
    ref = dct(x.astype(np.float64), type=2, norm="ortho", axis=-1)
    assert np.abs(y.cpu().numpy() - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max())
    back = torch.empty_like(t)
    _lib.check(lib.ndmps_idct_last_f32(y.data_ptr(), back.data_ptr(), rows, n, basis.data_ptr(), sp()))
    assert np.abs(back.cpu().numpy() - x).max() <= 3e-6
    assert np.abs(idct(ref, type=2, norm="ortho", axis=-1) - x).max() <= 1e-6
    if 64 <= n <= 1024 and n & (n - 1) == 0:  # the basis product on the same input, and the inverse of SciPy's output
        os.environ["NDMPS_DCT_GEMM"] = "1"
        try:
            y2 = torch.empty_like(t)
            _lib.check(lib.ndmps_dct_last_f32(t.data_ptr(), y2.data_ptr(), rows, n, basis.data_ptr(), sp()))
        finally:
            del os.environ["NDMPS_DCT_GEMM"]
        assert float((y - y2).abs().max()) <= 3e-6 * max(1.0, np.abs(ref).max())
        yref = dev(ref.astype(np.float32))
        _lib.check(lib.ndmps_idct_last_f32(yref.data_ptr(), back.data_ptr(), rows, n, basis.data_ptr(), sp()))
        assert np.abs(back.cpu().numpy() - x).max() <= 3e-6


# ------------------------------------------------------------- the reference's own properties
REF_SHAPES = [(512, 680), (8, 512, 680)]


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(2025)


@pytest.fixture(scope="module", params=REF_SHAPES, ids=lambda s: f"shape={s}")
def tensor(request, rng):
    return rng.random(request.param)


@pytest.fixture(params=["Std", "DCT"])
def mode(request):
    return request.param


_BUILT = {}


@pytest.fixture
def ndmps_obj(tensor, mode):
    key = (tensor.shape, mode)
    if key not in _BUILT:
        _BUILT[key] = NDMPS.from_tensor(tensor, norm=False, mode=mode)
    return copy.deepcopy(_BUILT[key])


def test_roundtrip_exact(ndmps_obj, tensor):
    """tests/core/test_ndmps.py:35-38 with the fp32 tolerance stated at the top."""
    out = ndmps_obj.to_tensor()
    assert out.shape == tensor.shape
    assert np.abs(out - tensor).max() <= 2e-5, np.abs(out - tensor).max()


def test_norm_option(tensor):
    obj = NDMPS.from_tensor(tensor, norm=True)
    assert math.isclose(obj.norm_value, 1.0, rel_tol=1e-6)
    fast = obj.norm_value          # ||site 0|| of the right-canonical sweep output
    obj.update_norm()              # full overlap contraction, as the reference
    assert math.isclose(obj.norm_value, fast, rel_tol=2e-6)
    assert math.isclose(obj.norm_value ** 2, obj.mps @ obj.mps, rel_tol=1e-12)


def test_compression_reduces_elements(ndmps_obj):
    before = ndmps_obj.number_elements_in_MPS()
    ndmps_obj.compress(cutoff=0.1)
    assert ndmps_obj.number_elements_in_MPS() < before


def test_boundary_and_norm_refresh(ndmps_obj):
    ndmps_obj.mps.arrays[0][:] *= 10
    ndmps_obj.update_boundary_list()
    ndmps_obj.update_norm()
    new_min, new_max = ndmps_obj.boundary_list[0]
    assert new_min <= np.min(ndmps_obj.mps.arrays[0]) and new_max >= np.max(ndmps_obj.mps.arrays[0])
    assert math.isclose(ndmps_obj.norm_value ** 2, ndmps_obj.mps @ ndmps_obj.mps, rel_tol=1e-12)
    dense = ndmps_obj.mps.to_dense().cpu().numpy().astype(np.float64)
    assert math.isclose(ndmps_obj.norm_value ** 2, float(np.sum(dense * dense)), rel_tol=1e-5)


def test_disk_compression_ratio(ndmps_obj):
    ndmps_obj.compress(cutoff=0.4)
    r = ndmps_obj.compression_ratio_on_disk(dtype=np.uint16, replace=False)
    assert 0 < r < 1


def test_continuous_compress_prints(ndmps_obj, capsys):
    ndmps_obj.continuous_compress(cutoff=0.05, print_ratio=True)
    assert capsys.readouterr().out.count("Compression ratio at") == 20


# ------------------------------------------------------------------ parity with the oracle
def _ssim_gap(x, rec_gpu, rec_ref):
    x64 = x.astype(np.float64)
    return abs(compute_ssim_by_dim(x64, rec_gpu.astype(np.float64)) - compute_ssim_by_dim(x64, rec_ref))


@pytest.mark.parametrize("shape,chi,mode", [((32, 32), 8, "Std"), ((64, 64, 64), 16, "Std"),
                                            ((64, 64, 64), 32, "DCT"), ((48, 40, 36), 12, "Std"),
                                            ((16, 16, 8, 12), 10, "Std"), ((128, 128, 128), 32, "Std")],
                         ids=str)
def test_truncated_sweep_matches_oracle(shape, chi, mode):
    x = synthetic_mri(shape, seed=2025)
    gpu = NDMPS.from_tensor(x, mode=mode, max_bond=chi)
    ref = OracleNDMPS.from_tensor(x, mode=mode, max_bond=chi)
    assert gpu.bond_sizes() == ref.bond_sizes()
    assert list(gpu.qubit_size) == list(ref.qubit_size)
    rg, rr = gpu.to_tensor(), ref.to_tensor()
    rel = np.linalg.norm(rg - rr) / np.linalg.norm(rr)
    assert rel <= 2e-5, rel
    if x.ndim in (2, 3, 4):
        assert _ssim_gap(x, rg, rr) <= 1e-5
    assert math.isclose(gpu.norm_value, ref.norm_value, rel_tol=1e-5)
    assert math.isclose(gpu.compression_ratio(), ref.compression_ratio(), rel_tol=1e-12)
    # orthogonal projection: truncation error adds in quadrature to the kept norm
    x64 = x.astype(np.float64)
    if mode == "Std":
        assert math.isclose(np.linalg.norm(x64 - rg) ** 2 + gpu.norm_value ** 2, np.linalg.norm(x64) ** 2,
                            rel_tol=1e-4)


def test_sweep_spectra_match_oracle():
    x = synthetic_mri((64, 64, 64), seed=7)
    gpu = NDMPS.from_tensor(x, max_bond=24)
    dense = np.empty(8 ** 6)
    dense[oim.flat_destination((64, 64, 64)).reshape(-1)] = x.astype(np.float64).reshape(-1)
    _, spectra = omps.mps_from_dense(dense, [8] * 6, max_bond=24)
    for i in range(1, 6):
        s_ref, s_gpu = spectra[i], gpu.sweep_spectra[i]
        m = min(len(s_ref), len(s_gpu), 24)  # a bond-capped sweep computes the max_bond leading values only
        assert np.abs(s_gpu[:m] - s_ref[:m]).max() <= 1e-5 * s_ref[0], i


def test_exact_sweep_finds_low_rank_bonds_like_the_reference():
    """exp(a.x) factorises over every digit of every coordinate, so all bonds are 1: the rel
    cutoff must collapse them on both paths.  A smooth but not digit-separable tensor has a
    numerically low rank: the fp32 path (cutoff floor 1e-6) may keep fewer singular values
    than the fp64 reference (1e-10) but must reconstruct to fp32 accuracy."""
    i = np.arange(16)
    x = np.exp(0.05 * i[:, None, None] - 0.03 * i[None, :, None] + 0.02 * i[None, None, :]).astype(np.float32)
    gpu = NDMPS.from_tensor(x)
    ref = OracleNDMPS.from_tensor(x.astype(np.float64), cutoff=1e-6)
    assert gpu.bond_sizes() == ref.bond_sizes() == [1, 1, 1]
    assert np.abs(gpu.to_tensor() - x).max() <= 2e-6 * np.abs(x).max()
    a = np.linspace(1, 2, 16)
    y = np.einsum("i,j,k->ijk", a, a[::-1], np.cos(a)).astype(np.float32)
    gpu, ref = NDMPS.from_tensor(y), OracleNDMPS.from_tensor(y)
    assert all(g <= r for g, r in zip(gpu.bond_sizes(), ref.bond_sizes()))
    assert gpu.bond_sizes() == OracleNDMPS.from_tensor(y.astype(np.float64), cutoff=1e-6).bond_sizes()
    assert np.abs(gpu.to_tensor() - y).max() <= 5e-6 * np.abs(y).max()


@pytest.mark.parametrize("cutoff", [0.02, 0.1, 0.3])
def test_compress_matches_oracle(cutoff):
    x = synthetic_mri((32, 48, 40), seed=11)
    gpu = NDMPS.from_tensor(x)
    ref = OracleNDMPS.from_tensor(x)
    assert gpu.bond_sizes() == ref.bond_sizes()
    gpu.compress(cutoff)
    ref.compress(cutoff)
    assert gpu.bond_sizes() == ref.bond_sizes()
    rg, rr = gpu.to_tensor(), ref.to_tensor()
    assert np.linalg.norm(rg - rr) / np.linalg.norm(rr) <= 3e-5
    assert _ssim_gap(x, rg, rr) <= 1e-5
    assert math.isclose(gpu.norm_value, ref.norm_value, rel_tol=1e-5)
    gpu.compress(cutoff * 2)  # cumulative, like run_benchmark (evaluation/benchmark.py:176-178)
    ref.compress(cutoff * 2)
    assert gpu.bond_sizes() == ref.bond_sizes()
    assert np.linalg.norm(gpu.to_tensor() - ref.to_tensor()) / np.linalg.norm(rr) <= 5e-5


def test_compress_bond_is_truncated_two_site_svd():
    rng = np.random.default_rng(5)
    t1 = rng.standard_normal((6, 5, 12)).astype(np.float32)
    t2 = rng.standard_normal((12, 4, 7)).astype(np.float32)
    from imgcompressionmps_amd.core.mps import DeviceMPS

    edge_l = rng.standard_normal((1, 3, 6)).astype(np.float32)
    edge_r = rng.standard_normal((7, 2, 1)).astype(np.float32)
    mps = DeviceMPS([dev(edge_l), dev(t1), dev(t2), dev(edge_r)])
    two = t1.reshape(30, 12).astype(np.float64) @ t2.reshape(12, 28).astype(np.float64)
    u, s, vh = np.linalg.svd(two, full_matrices=False)
    spec = mps.compress_bond_(2, cutoff=0.35)
    k = int(np.sum(s > 0.35 * s[0]))
    assert mps.cores[1].shape == (6, 5, k) and mps.cores[2].shape == (k, 4, 7)
    assert spec.shape == (12,) and np.abs(spec - s[:12]).max() <= 1e-5 * s[0]
    got = mps.cores[1].cpu().numpy().reshape(30, k).astype(np.float64) @ mps.cores[2].cpu().numpy().reshape(k, 28)
    assert np.abs(got - (u[:, :k] * s[:k]) @ vh[:k]).max() <= 2e-5 * s[0]
    # absorb="both": both sides carry sqrt(s)
    g1 = mps.cores[1].cpu().numpy().reshape(30, k)
    assert np.allclose(np.sqrt(np.sum(g1.astype(np.float64) ** 2, axis=0)), np.sqrt(s[:k]), rtol=1e-4)


def test_single_site_unknown_mode_and_errors():
    x = np.random.default_rng(5).random((7, 12))
    o = NDMPS.from_tensor(x)
    assert o.bond_sizes() == [] and np.abs(o.to_tensor() - x).max() <= 1e-6
    o.compress(0.3)
    assert np.abs(o.to_tensor() - x).max() <= 1e-6
    assert NDMPS.from_tensor(x, mode="weird").to_tensor() is None
    with pytest.raises(AssertionError):
        o.replace_tensordata([np.zeros((3, 3))])
    with pytest.raises(ValueError):
        NDMPS.from_tensor(np.float32(3.0))
    keep = x.copy()
    NDMPS.from_tensor(x, norm=True)
    assert np.array_equal(x, keep)  # input never mutated (ndmps.py:56)


def test_accessors_and_replace():
    x = synthetic_mri((16, 16, 16), seed=3)
    o = NDMPS.from_tensor(x, max_bond=6)
    assert o.number_elements_in_MPS() == sum(t.size for t in o.mps)
    assert o.compression_ratio() == o.number_elements_in_MPS() / 4096
    assert o.get_storage_space(np.uint16) == o.number_elements_in_MPS() * 2
    assert o.encoding_map.shape == (16, 16, 16, 4)
    assert np.array_equal(np.moveaxis(o.encoding_map, -1, 0), oim.gen_encoding_map((16, 16, 16))[1])
    data = [np.asarray(t) * 2 for t in o.return_tensors_data()]
    before = o.norm_value
    o.replace_tensordata(data)
    assert math.isclose(o.norm_value, before * 2 ** len(data), rel_tol=1e-5)
    ints = o.compress_to_dtype(np.uint8, replace=True)
    assert all(a.dtype == np.uint8 for a in ints)
    ob = copy.deepcopy(o)
    ob.mps.arrays[0][:] *= 0
    assert o.norm_value > 0 and np.asarray(o.mps.arrays[0]).any()


def test_torch_input_and_device_output_stay_on_gpu():
    x = torch.rand((32, 32, 32), device=DEV)
    keep = x.clone()
    o = NDMPS.from_tensor(x, max_bond=8)
    out = o.to_tensor(as_torch=True)
    assert out.is_cuda and out.shape == x.shape and torch.equal(x, keep)


# ------------------------------------------------------------------------- batched (lockstep) path
def test_batched_eigensolver_mixed_sizes():
    lib = _lib.load()
    sizes = [40, 7, 96, 33, 1]
    nmax = max(sizes)
    rng = np.random.default_rng(42)
    mats = []
    g_all = np.zeros((len(sizes), nmax * nmax))
    for b, n in enumerate(sizes):
        a = rng.standard_normal((n + 3, n)) * np.logspace(0, -4, n)[None, :]
        g = a.T @ a
        mats.append(g)
        g_all[b, : n * n] = g.reshape(-1)
    tg = dev(g_all)
    tv = torch.zeros_like(tg)
    tw = torch.zeros((len(sizes), nmax), dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_syevj_batched_workspace_bytes(nmax, len(sizes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sweeps = C.c_int()
    _lib.check(lib.ndmps_syevj_batched_f64(len(sizes), tg.data_ptr(), nmax * nmax, _lib.i64_array(sizes),
                                           tv.data_ptr(), nmax * nmax, tw.data_ptr(), nmax, ws.data_ptr(), nbytes,
                                           C.byref(sweeps), sp()))
    for b, n in enumerate(sizes):
        w = tw[b, :n].cpu().numpy()
        v = tv[b, : n * n].cpu().numpy().reshape(n, n)
        ref = np.linalg.eigvalsh(mats[b])[::-1]
        assert np.abs(w - ref).max() <= 1e-13 * ref[0]
        assert np.abs(v.T @ v - np.eye(n)).max() <= 1e-13
        assert np.abs(mats[b] @ v - v * w[None, :]).max() <= 1e-13 * ref[0]


@pytest.mark.parametrize("sizes", [[300, 512, 257], [900, 1000]])
def test_batched_eigensolver_large_and_two_phase(sizes):
    """Orders 257..512 in a batch run in history mode (rotation blocks recorded, eigenvectors replayed on
    the wanted columns); orders above 896 keep the in-loop V update.  Both against LAPACK, full
    vectors and the two-phase form with only k leading columns."""
    lib = _lib.load()
    nmax = max(sizes)
    rng = np.random.default_rng(sum(sizes))
    mats = []
    g_all = np.zeros((len(sizes), nmax * nmax))
    for b, n in enumerate(sizes):
        a = rng.standard_normal((n + 9, n)) * np.logspace(0, -5, n)[None, :]
        q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        g = q @ (a.T @ a) @ q.T  # graded spectrum, dense eigenvectors
        g = 0.5 * (g + g.T)
        mats.append(g)
        g_all[b, : n * n] = g.reshape(-1)
    nbytes = lib.ndmps_syevj_batched_workspace_bytes(nmax, len(sizes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    tw = torch.zeros((len(sizes), nmax), dtype=torch.float64, device=DEV)
    sweeps = C.c_int()
    tg = dev(g_all)
    tv = torch.zeros_like(tg)
    _lib.check(lib.ndmps_syevj_batched_f64(len(sizes), tg.data_ptr(), nmax * nmax, _lib.i64_array(sizes),
                                           tv.data_ptr(), nmax * nmax, tw.data_ptr(), nmax, ws.data_ptr(), nbytes,
                                           C.byref(sweeps), sp()))
    full = []
    for b, n in enumerate(sizes):
        w = tw[b, :n].cpu().numpy()
        v = tv[b, : n * n].cpu().numpy().reshape(n, n)
        ref = np.linalg.eigvalsh(mats[b])[::-1]
        assert np.all(np.diff(w) <= 0)
        assert np.abs(w - ref).max() <= 2e-15 * n * ref[0]  # LAPACK's own backward error is n eps |G|
        assert np.abs(v.T @ v - np.eye(n)).max() <= 2e-15 * n
        assert np.abs(mats[b] @ v - v * w[None, :]).max() <= 2e-15 * n * ref[0]
        full.append(v)
    # two-phase: values, then k leading vectors only (identical to the leading columns of the full solve)
    ks = [max(1, n // 8) for n in sizes]
    tg = dev(g_all)
    tv2 = torch.zeros_like(tg)
    _lib.check(lib.ndmps_syevj_batched_values_f64(len(sizes), tg.data_ptr(), nmax * nmax, _lib.i64_array(sizes),
                                                  tv2.data_ptr(), nmax * nmax, tw.data_ptr(), nmax, 1e-15,
                                                  ws.data_ptr(), nbytes, C.byref(sweeps), sp()))
    _lib.check(lib.ndmps_syevj_batched_vectors_f64(len(sizes), tg.data_ptr(), nmax * nmax, _lib.i64_array(sizes),
                                                   tv2.data_ptr(), nmax * nmax, tw.data_ptr(), nmax,
                                                   _lib.i64_array(ks), ws.data_ptr(), nbytes, sp()))
    for b, (n, k) in enumerate(zip(sizes, ks)):
        v = tv2[b, : n * n].cpu().numpy().reshape(n, n)[:, :k]
        assert np.array_equal(v, full[b][:, :k])


# ---------------------------------------------------------------- direct top-k solver (eig_tridiag.hip)
def _topk(lib, mats, ks, k_max=None):
    """ndmps_syevd_topk_* on a batch of symmetric matrices: (eigenvalues, leading k eigenvectors) per matrix."""
    sizes = [m.shape[0] for m in mats]
    nmax, B = max(sizes), len(mats)
    k_max = k_max or max(ks)
    g_all = np.zeros((B, nmax * nmax))
    for b, m in enumerate(mats):
        g_all[b, : m.size] = m.reshape(-1)
    tg = dev(g_all)
    tv = torch.zeros_like(tg)
    tw = torch.zeros((B, nmax), dtype=torch.float64, device=DEV)
    nbytes = lib.ndmps_syevd_topk_workspace_bytes(nmax, B, k_max)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    n_arr = _lib.i64_array(sizes)
    _lib.check(lib.ndmps_syevd_topk_values_f64(B, tg.data_ptr(), nmax * nmax, n_arr, tv.data_ptr(), nmax * nmax,
                                               tw.data_ptr(), nmax, k_max, ws.data_ptr(), nbytes, sp()))
    status = (C.c_int * B)()
    _lib.check(lib.ndmps_syevd_topk_vectors_f64(B, n_arr, _lib.i64_array(ks), k_max, ws.data_ptr(), nbytes, status, sp()))
    assert list(status) == [0] * B
    out = []
    for b, (n, k) in enumerate(zip(sizes, ks)):
        out.append((tw[b, :n].cpu().numpy(), tv[b, : n * n].cpu().numpy().reshape(n, n)[:, :k]))
    return out


def _check_topk(g, w, v, k, tol_scale=1.0, k_max=None):
    """w: the min(k_max, n) largest eigenvalues, zeros behind them; v: the k leading eigenvectors."""
    n = g.shape[0]
    kv = min(k_max or k, n)
    ref = np.linalg.eigvalsh(g)[::-1]
    scale = max(abs(ref[0]), abs(ref[-1]), 1e-300)
    eps = 2e-15 * max(n, 50) * tol_scale
    assert np.all(np.diff(w[:kv]) <= 1e-15 * scale)
    assert np.abs(w[:kv] - ref[:kv]).max() <= eps * scale
    assert np.all(w[kv:] == 0.0)
    assert np.abs(v.T @ v - np.eye(k)).max() <= eps
    assert np.abs(g @ v - v * w[None, :k]).max() <= eps * scale
    for j in range(k):  # sign convention: largest component positive
        assert v[np.argmax(np.abs(v[:, j])), j] > 0


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 33, 64, 100, 128, 129, 130, 200, 257, 512, 513, 777, 1024, 1100, 2048,
                               2100])
def test_topk_solver_against_lapack(n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n + 5, n)) * np.logspace(0, -4, n)[None, :]
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    g = q @ (a.T @ a) @ q.T
    g = 0.5 * (g + g.T)
    k = min(n, 64)
    (w, v), = _topk(lib, [g], [k])
    _check_topk(g, w, v, k)


def test_topk_solver_batch_of_mixed_sizes_and_ranks():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    sizes, ks = [512, 40, 300, 512, 7, 131], [64, 40, 17, 128, 1, 100]
    mats = []
    for n in sizes:
        a = rng.standard_normal((2 * n, n)) * np.logspace(0, -5, n)[None, :]
        mats.append(a.T @ a)
    for g, k, (w, v) in zip(mats, ks, _topk(lib, mats, ks, k_max=128)):
        _check_topk(g, w, v, k, k_max=128)


def test_topk_solver_batches_beyond_the_narrow_teams():
    """More matrices than 8-column teams fit the chip at once (batch * n / 8 workgroups > the resident slots) take
    32-column blocks that meet at a counter: 20 matrices of order 260, and 9 of order 512."""
    lib = _lib.load()
    rng = np.random.default_rng(21)
    for n, count, k in ((260, 20, 16), (512, 9, 32)):
        assert count * -(-n // 8) > lib.ndmps_syevd_topk_team_slots(n) > 0
        plan = er.route(lib, [n] * count, k)
        assert (plan["reduce"], plan["kernel"], plan["team_size"]) == (er.TEAM, er.K_MEET2, -(-n // 32))
        mats = []
        for _ in range(count):
            a = rng.standard_normal((n + 16, n)) * np.logspace(0, -4, n)[None, :]
            mats.append(a.T @ a)
        for g, (w, v) in zip(mats, _topk(lib, mats, [k] * count)):
            _check_topk(g, w, v, k)


def test_topk_solver_orders_above_512_in_mixed_batches():
    """Orders above 512 (BASELINE config 5: 2048; chi = 128 on a 256^3 volume: 1024) in batches that mix big and small
    members: four of order <= 1024 take the resident kernel whole (4 x 128 workgroups fit the slots), 2048 with 1300
    does not (2 x 256 workgroups) and, being mixed, has no resident end either: panel launches to the last 128 columns."""
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for sizes, ks, kind in (([1024, 600, 100, 1000], [128, 64, 10, 128], er.BIG_TEAM), ([2048, 1300], [128, 100], er.PANEL)):
        plan = er.route(lib, sizes, 128)
        assert (plan["reduce"], plan["handover"]) == (kind, 0)
        mats = []
        for n in sizes:
            a = rng.standard_normal((n + 64, n)) * np.logspace(0, -5, n)[None, :]
            mats.append(a.T @ a)
        for g, k, (w, v) in zip(mats, ks, _topk(lib, mats, ks, k_max=128)):
            _check_topk(g, w, v, k, k_max=128)


@pytest.mark.parametrize("n,team_max", [(640, 512), (1537, 512), (3000, 512), (4096, 512), (2500, 1024), (3000, None),
                                        (4096, None)])
def test_topk_solver_panel_blocked_reduction(n, team_max, monkeypatch):
    """Orders the resident kernel does not take whole (above 2048; here, with NDMPS_TRD_TEAM_MAX=512, above 512) are
    reduced panel by panel (csrc/eig_panel.inc: two launches per column on the lower tiles, one MFMA update per 32
    columns) and, when the order is even, handed to the resident kernel for the last 2048 / 1024 / 512 columns: orders
    that are no multiple of the 64-wide tiles or of the panel width, odd ones (panel launches to the end), the largest
    order the solver takes, 128 vectors."""
    lib = _lib.load()
    monkeypatch.setenv("NDMPS_TRD_PANEL_MIN", "513")
    if team_max:
        monkeypatch.setenv("NDMPS_TRD_TEAM_MAX", str(team_max))
    handover = {(640, 512): 512, (1537, 512): 0, (3000, 512): 512, (4096, 512): 512, (2500, 1024): 1024, (3000, None): 2048,
                (4096, None): 2048}[(n, team_max)]
    plan = er.route(lib, [n], 128)
    assert (plan["reduce"], plan["handover"], plan["tail_cols"]) == (er.PANEL_HYBRID if handover else er.PANEL, handover,
                                                                     handover or 128)
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n + 5, n)) * np.logspace(0, -5, n)[None, :]
    g = a.T @ a
    (w, v), = _topk(lib, [g], [128])
    _check_topk(g, w, v, 128)


@pytest.mark.parametrize("route", ["panel", "resident"])
def test_topk_solver_panel_blocked_reduction_degenerate_spectra(route, monkeypatch):
    """The panel path, and the resident kernel at orders above 512, on matrices whose reflectors vanish or whose
    spectra are multiple: zero, identity, rank one, exact multiplicities, diagonal, decoupled identical blocks, orders
    600 .. 700 in ONE batch (mixed orders: the kernels read the order from the descriptors)."""
    lib = _lib.load()
    monkeypatch.setenv("NDMPS_TRD_PANEL_MIN", "513")
    if route == "panel":
        monkeypatch.setenv("NDMPS_TRD_TEAM_MAX", "512")
    rng = np.random.default_rng(2)
    n = 600
    u = rng.standard_normal(n)
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = np.r_[np.full(10, 5.0), np.full(20, 1.0), np.zeros(n - 30)]
    blk = rng.standard_normal((70, 70))
    cases = [(np.zeros((n, n)), 8), (np.eye(n), 8), (np.outer(u, u), 8), ((q * lam) @ q.T, 30),
             (np.diag(np.arange(n, 0, -1.0)), 10), (np.kron(np.eye(10), blk @ blk.T), 40), (np.eye(650) * 3.0, 50)]
    mats = [0.5 * (g + g.T) for g, _ in cases]
    ks = [k for _, k in cases]
    # the resident route needs every team of a batch resident at once: 82 workgroups per matrix here, three at a time
    step = len(mats) if route == "panel" else 3
    for at in range(0, len(mats), step):
        part, kpart = mats[at:at + step], ks[at:at + step]
        assert er.route(lib, [g.shape[0] for g in part], 50)["reduce"] == (er.PANEL if route == "panel" else er.BIG_TEAM)
        for g, k, (w, v) in zip(part, kpart, _topk(lib, part, kpart, k_max=50)):
            _check_topk(g, w, v, k, tol_scale=4.0, k_max=50)


def test_topk_solver_panel_path_against_the_column_launches(monkeypatch):
    """The same matrices through the panel-blocked reduction, its launches issued one by one and replayed from a cached
    graph (NDMPS_TRD_PANEL_GRAPH; bit-identical: same kernels in the same order), and through the one-launch-per-column
    reduction it replaces from order 1536 on (same eigenvalues, same kept subspace)."""
    lib = _lib.load()
    monkeypatch.setenv("NDMPS_TRD_PANEL_MIN", "513")
    monkeypatch.setenv("NDMPS_TRD_TEAM_MAX", "512")
    rng = np.random.default_rng(3)
    mats = []
    for n in (1100, 777):
        a = rng.standard_normal((n + 64, n)) * np.logspace(0, -5, n)[None, :]
        mats.append(a.T @ a)
    ks = [96, 64]
    assert er.route(lib, [1100, 777], 128)["reduce"] == er.PANEL
    first = _topk(lib, mats, ks, k_max=128)
    again = _topk(lib, mats, ks, k_max=128)
    monkeypatch.setenv("NDMPS_TRD_PANEL_GRAPH", "1")  # the same launches replayed from a graph
    assert er.route(lib, [1100, 777], 128)["graph"] == 1
    _topk(lib, mats, ks, k_max=128)
    eager = _topk(lib, mats, ks, k_max=128)  # replayed from the cached graph if the workspace came back at the same address
    monkeypatch.delenv("NDMPS_TRD_PANEL_GRAPH")
    monkeypatch.setenv("NDMPS_TRD_NO_PANEL", "1")
    assert er.route(lib, [1100, 777], 128)["reduce"] == er.COLUMNS
    columns = _topk(lib, mats, ks, k_max=128)
    for g, k, (w, v), (w1, v1), (w2, v2), (w3, v3) in zip(mats, ks, first, again, eager, columns):
        assert np.array_equal(w, w1) and np.array_equal(v, v1)
        assert np.array_equal(w, w2) and np.array_equal(v, v2)
        _check_topk(g, w3, v3, k, k_max=128)
        assert np.abs(w - w3).max() <= 1e-13 * w[0]
        gap = (w[k - 1] - w[k]) / w[0] if k < 128 else 1.0
        assert np.abs(v @ v.T - v3 @ v3.T).max() <= 50 * 2.2e-16 / max(gap, 1e-300) + 1e-11


@pytest.mark.parametrize("n,k", [(200, 200), (512, 512), (777, 300), (1024, 1024), (1600, 129)])
def test_direct_solver_more_than_128_vectors(n, k):
    """Every eigenpair (or any number beyond 128) of a graded Gram matrix: what exact sweeps and compress() ask for
    (core/ndmps.py:74,104-106 of the reference: dgesdd).  Inverse iteration in column blocks of 128, Cholesky-QR of the
    whole n x k block across the chip (csrc/eig_wide.inc), against LAPACK at the tolerances of the narrow solver."""
    lib = _lib.load()
    assert int(lib.ndmps_syevd_topk_max_k_wide()) >= 4096
    rng = np.random.default_rng(n + k)
    a = rng.standard_normal((n + 5, n)) * np.logspace(0, -4, n)[None, :]
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    g = q @ (a.T @ a) @ q.T
    g = 0.5 * (g + g.T)
    (w, v), = _topk(lib, [g], [k], k_max=max(k, min(n, 400)))
    _check_topk(g, w, v, k, k_max=max(k, min(n, 400)))
    if k == n:  # a full decomposition: V diag(w) V^T gives the matrix back
        assert np.abs((v * w[None, :]) @ v.T - g).max() <= 2e-15 * max(n, 50) * np.abs(g).max()


def test_direct_solver_all_vectors_of_degenerate_spectra():
    """All eigenvectors where they are not unique: the identity (an n-fold eigenvalue: every start vector is an
    eigenvector and the block is a random matrix until it is orthonormalised), the zero matrix, rank one, exact
    multiplicities, a volume's Gram matrix with its noise floor, mixed orders in one batch."""
    lib = _lib.load()
    rng = np.random.default_rng(4)
    n = 300
    u = rng.standard_normal(n)
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = np.r_[np.full(10, 5.0), np.full(120, 1.0), np.linspace(0.5, 0.1, n - 130)]
    x = synthetic_mri((32, 32, 32), seed=3).astype(np.float64).reshape(-1, 256)
    cases = [np.eye(n), np.zeros((200, 200)), np.outer(u, u), (q * lam) @ q.T, x.T @ x]
    mats = [0.5 * (g + g.T) for g in cases]
    ks = [m.shape[0] for m in mats]
    for g, k, (w, v) in zip(mats, ks, _topk(lib, mats, ks)):
        _check_topk(g, w, v, k, tol_scale=4.0)


@pytest.mark.parametrize("n", [1, 40, 64, 130, 512, 1000])
def test_blocked_cholesky_against_numpy(n):
    """ndmps_potrf_lower_f64 (the square root compress() takes of G2 = T2 T2^T): the factor against numpy's, zeros above
    the diagonal, the breakdown flag on a matrix that is not positive definite."""
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n + 3, n)) * np.logspace(0, -3, n)[None, :]
    g = a.T @ a + 1e-9 * np.eye(n)
    s = dev(g.copy())
    scratch = torch.empty(int(lib.ndmps_potrf_scratch_elems(n)), dtype=torch.float64, device=DEV)
    status = C.c_int(-1)
    _lib.check(lib.ndmps_potrf_lower_f64(s.data_ptr(), n, scratch.data_ptr(), C.byref(status), sp()))
    assert status.value == 0
    got, want = s.cpu().numpy(), np.linalg.cholesky(g)
    assert np.all(np.triu(got, 1) == 0.0)
    assert np.abs(got @ got.T - g).max() <= 4e-15 * max(n, 16) * np.abs(g).max()
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    if n >= 40:
        bad = g.copy()
        bad[n // 2, n // 2] = -1.0
        s = dev(bad)
        _lib.check(lib.ndmps_potrf_lower_f64(s.data_ptr(), n, scratch.data_ptr(), C.byref(status), sp()))
        assert status.value == 1


def test_topk_solver_volume_gram_matrices_with_noise_floor_clusters():
    """The matrices the sweep meets: Gram matrices of the chi-capped unfoldings of a noisy volume, a few large
    eigenvalues over a floor of ~n near-equal ones (gaps ~1e-9 of the largest).  The kept subspace must agree
    with LAPACK's to the accuracy its conditioning allows: |P - P_ref| <= 50 eps |G| / gap."""
    lib = _lib.load()
    x = synthetic_mri((64, 64, 64), seed=3).astype(np.float64)
    dense = np.empty(x.size)
    dense[oim.flat_destination(x.shape).reshape(-1)] = x.reshape(-1)
    mats, work, chi_r = [], dense.reshape(-1, 1), 1
    for i in range(5, 0, -1):
        mat = work.reshape(-1, 8 * chi_r)
        if mat.shape[1] > mat.shape[0]:
            break
        g = mat.T @ mat
        wv, vv = np.linalg.eigh(g)
        kk = min(32, g.shape[0])
        if g.shape[0] > 32:
            mats.append(g)
        work, chi_r = mat @ vv[:, ::-1][:, :kk], kk
    assert len(mats) >= 2
    for g, (w, v) in zip(mats, _topk(lib, mats, [32] * len(mats))):
        _check_topk(g, w, v, 32)
        wr, vr = np.linalg.eigh(g)
        wr, vr = wr[::-1], vr[:, ::-1]
        gap = (wr[31] - wr[32]) / wr[0]
        assert np.abs(v @ v.T - vr[:, :32] @ vr[:, :32].T).max() <= 50 * 2.2e-16 / gap + 1e-12


def test_topk_solver_degenerate_spectra():
    """Zero matrix, identity (n-fold eigenvalue), rank one, exact multiplicities, a diagonal matrix (every
    reflector is the identity) and decoupled identical blocks: orthonormal vectors with small residuals even
    where the eigenvectors themselves are not unique."""
    lib = _lib.load()
    rng = np.random.default_rng(1)
    n = 96
    u = rng.standard_normal(n)
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = np.r_[np.full(10, 5.0), np.full(20, 1.0), np.zeros(n - 30)]
    blk = rng.standard_normal((8, 8))
    cases = [(np.zeros((n, n)), 8), (np.eye(n), 8), (np.outer(u, u), 8), ((q * lam) @ q.T, 30), ((q * lam) @ q.T, 12),
             (np.diag(np.arange(n, 0, -1.0)), 10), (np.kron(np.eye(12), blk @ blk.T), 24), (np.eye(200) * 3.0, 50)]
    mats = [0.5 * (g + g.T) for g, _ in cases]
    for g, k, (w, v) in zip(mats, [k for _, k in cases], _topk(lib, mats, [k for _, k in cases])):
        _check_topk(g, w, v, k, tol_scale=4.0, k_max=50)


def test_topk_solver_more_than_64_vectors_by_column_blocks():
    """k > 64 (BASELINE config 5 wants 128): the eigenvector block is orthonormalised in column blocks of 64 (block
    Gram-Schmidt with re-orthogonalisation + blocked Cholesky-QR on the MFMA).  Ranks 65 .. 128 incl. ragged last
    blocks, clusters that straddle the block boundary, exact multiplicities; the column-by-column path on the same
    input as a cross-check."""
    lib = _lib.load()
    rng = np.random.default_rng(21)
    n = 300
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam_cluster = np.r_[np.linspace(2.0, 1.0, 60), np.full(10, 0.5), np.linspace(0.4, 0.1, 230)]  # a 10-fold one over 64
    lam_flat = np.r_[np.full(30, 1.0), np.linspace(0.9, 0.3, 60), np.zeros(210)]  # exact multiplicity, then an exact null space
    a = rng.standard_normal((700, 512)) * np.logspace(0, -6, 512)[None, :]
    mats = [(q * lam_cluster) @ q.T, (q * lam_flat) @ q.T, a.T @ a, np.eye(200) * 2.0]
    mats = [0.5 * (g + g.T) for g in mats]
    ks = [70, 88, 128, 65]
    for g, k, (w, v) in zip(mats, ks, _topk(lib, mats, ks, k_max=128)):
        _check_topk(g, w, v, k, tol_scale=8.0, k_max=128)
    os.environ["NDMPS_ORTHO_COLUMNS"] = "1"
    try:
        old = _topk(lib, mats[2:3], [128], k_max=128)
    finally:
        del os.environ["NDMPS_ORTHO_COLUMNS"]
    new = _topk(lib, mats[2:3], [128], k_max=128)
    assert np.abs(old[0][1] @ old[0][1].T - new[0][1] @ new[0][1].T).max() <= 1e-9  # same subspace (gaps ~1e-12 |G|)


def test_from_tensors_equals_from_tensor_one_by_one():
    vols = [synthetic_mri((32, 32, 32), seed=s) for s in (1, 2, 3)]
    vols[1] = vols[1] * 0.25  # different scales and spectra inside one batch
    batched = NDMPS.from_tensors(vols, max_bond=12)
    for v, ob in zip(vols, batched):
        single = NDMPS.from_tensor(v, max_bond=12)
        assert ob.bond_sizes() == single.bond_sizes()
        assert np.array_equal(ob.to_tensor(), single.to_tensor())
        assert ob.norm_value == single.norm_value
        assert np.array_equal(ob.boundary_list, single.boundary_list)
    exact = NDMPS.from_tensors(vols)  # cutoff-limited bonds may differ per volume
    for v, ob in zip(vols, exact):
        assert np.abs(ob.to_tensor() - v).max() <= 2e-5 * np.abs(v).max()
    with pytest.raises(ValueError):
        NDMPS.from_tensors([vols[0], np.zeros((4, 4), dtype=np.float32)])
    assert NDMPS.from_tensors([]) == []


@pytest.mark.parametrize("shape,chi,mode,norm,enqueued", [((64, 64, 64), 16, "Std", False, True),
                                                           ((128, 128, 128), 32, "DCT", True, True),
                                                           ((32, 32, 16, 24), 12, "Std", False, False),  # no merged run
                                                           ((48, 40, 36), None, "Std", False, False)], ids=str)
def test_from_tensors_in_two_halves_equals_the_one_call_form(shape, chi, mode, norm, enqueued):
    """from_tensors_begin enqueues sweep and decode (the fp32 bond-capped sweep decides its ranks on the device: nothing on
    the host waits), result() reads the ranks behind an event and builds the objects: the same kernels in the same order
    as from_tensors -- cores, bonds, spectra, state and reconstructions are bit-identical, also when a second batch is
    begun before the first one's result is asked for; exact sweeps (host-side ranks) take the synchronous route."""
    from imgcompressionmps_amd.core import batch as hbatch

    vols = [dev(synthetic_mri(shape, seed=90 + i)) for i in range(5)]
    want_objs, want_recs = NDMPS.from_tensors(vols, mode=mode, norm=norm, max_bond=chi, reconstruct=True)
    first = NDMPS.from_tensors_begin(vols, mode=mode, norm=norm, max_bond=chi, reconstruct=True)
    second = NDMPS.from_tensors_begin(vols[::-1], mode=mode, norm=norm, max_bond=chi, reconstruct=True)
    assert first.asynchronous == enqueued
    objs, recs = first.result()
    assert first.result()[0] is objs  # a second call returns the same objects
    objs2, recs2 = second.result()
    for got_o, got_r in ((objs, recs), (objs2[::-1], recs2[::-1])):
        for a, b, ra, rb in zip(want_objs, got_o, want_recs, got_r):
            assert a.bond_sizes() == b.bond_sizes()
            assert all(torch.equal(x, y) for x, y in zip(a.mps.cores, b.mps.cores))
            assert torch.equal(ra, rb)
            assert np.array_equal(np.asarray(a.boundary_list), np.asarray(b.boundary_list))
            assert a.norm_value == b.norm_value
            sa, sb = a.sweep_spectra, b.sweep_spectra
            assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(sa, sb))
    assert NDMPS.from_tensors_begin([]).result() == [] and NDMPS.from_tensors_begin([], reconstruct=True).result() == ([], [])
    dropped = NDMPS.from_tensors_begin(vols, mode=mode, norm=norm, max_bond=chi, reconstruct=True)
    del dropped  # never read: waits for its copies into pinned memory, nothing else
    only = NDMPS.from_tensors_begin(vols[:2], mode=mode, norm=norm, max_bond=chi).result()
    assert all(torch.equal(x, y) for a, b in zip(want_objs[:2], only) for x, y in zip(a.mps.cores, b.mps.cores))
    # the batch layer: two groups on their own streams, a second batch begun before the first is read
    one = hbatch.encode_decode_concurrent(vols[:4], groups=2, mode=mode, norm=norm, max_bond=chi)
    p1 = hbatch.encode_decode_begin(vols[:4], groups=2, mode=mode, norm=norm, max_bond=chi)
    p2 = hbatch.encode_decode_begin(vols[:4], groups=2, mode=mode, norm=norm, max_bond=chi)
    for pend in (p1, p2):
        o, r = pend.result()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(one[1], r))
        assert all(torch.equal(x, y) for a, b in zip(one[0], o) for x, y in zip(a.mps.cores, b.mps.cores))
    # the generator form: batches in, (objects, reconstructions) out, in input order
    chunks = [vols[:4], vols[1:5], vols[:2]]
    seen = 0
    for (o, r), chunk in zip(hbatch.encode_decode_stream(iter(chunks), mode=mode, norm=norm, max_bond=chi), chunks):
        torch.cuda.synchronize()
        want = NDMPS.from_tensors(chunk, mode=mode, norm=norm, max_bond=chi, reconstruct=True)
        assert len(o) == len(chunk) and all(torch.equal(a, b) for a, b in zip(want[1], r))
        assert all(torch.equal(x, y) for a, b in zip(want[0], o) for x, y in zip(a.mps.cores, b.mps.cores))
        seen += 1
    assert seen == 3 and list(hbatch.encode_decode_stream([], max_bond=chi)) == []
    # three lanes, eight volumes per batch: the resident reductions of such batches take 32-column blocks (the solver is
    # told that batches overlap) -- the same MPS up to the rounding of the fp64 eigen-solver, not bit for bit
    eight = [dev(synthetic_mri(shape, seed=120 + i)) for i in range(8)]
    ref8 = hbatch.encode_decode_concurrent(eight, groups=1, mode=mode, norm=norm, max_bond=chi)
    flight = [hbatch.encode_decode_begin(eight, groups=1, mode=mode, norm=norm, max_bond=chi, lane=k, lanes=3) for k in range(3)]
    for pend in flight:
        o, r = pend.result()
        torch.cuda.synchronize()
        assert [x.bond_sizes() for x in o] == [x.bond_sizes() for x in ref8[0]]
        for a, b in zip(ref8[1], r):
            assert float((a - b).norm() / a.norm()) <= 2e-5


def test_streams_create_returns_usable_distinct_streams():
    lib = _lib.load()
    raw = (C.c_void_p * 4)()
    found = C.c_int(-1)
    _lib.check(lib.ndmps_streams_create(4, raw, C.byref(found)))
    assert 1 <= found.value <= 4
    assert len({int(raw[i]) for i in range(4)}) == 4
    x = torch.arange(1000, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    for i in range(4):  # the handles are ordinary HIP streams
        with torch.cuda.stream(torch.cuda.ExternalStream(int(raw[i]))):
            y = x * 2
        torch.cuda.synchronize()
        assert float(y.sum()) == float(x.sum()) * 2
    _lib.check(lib.ndmps_streams_destroy(4, raw))
    with pytest.raises(ValueError):
        _lib.check(lib.ndmps_streams_create(0, raw, None))


def test_concurrent_groups_equal_one_by_one():
    """encode_decode_concurrent (groups on their own host threads and streams) returns, in input
    order, exactly what from_tensor / to_tensor give volume by volume; second call reuses the streams."""
    from imgcompressionmps_amd.core import batch as batch_mod

    vols = [torch.from_numpy(synthetic_mri((32, 32, 32), seed=20 + s)).to(DEV) for s in range(7)]
    for groups in (3, 1):
        objs, recs = batch_mod.encode_decode_concurrent(vols, groups=groups, max_bond=10)
        torch.cuda.synchronize()
        assert len(objs) == len(recs) == 7
        for v, ob, rec in zip(vols, objs, recs):
            single = NDMPS.from_tensor(v, max_bond=10)
            assert ob.bond_sizes() == single.bond_sizes()
            assert torch.equal(rec, single.to_tensor(as_torch=True))
    assert batch_mod.group_streams(3) is batch_mod.group_streams(3)
    objs, recs = batch_mod.encode_decode_concurrent(vols, groups=4, mode="DCT", max_bond=10)
    torch.cuda.synchronize()
    for v, rec in zip(vols, recs):
        assert torch.equal(rec, NDMPS.from_tensor(v, mode="DCT", max_bond=10).to_tensor(as_torch=True))
    objs, recs = batch_mod.encode_decode_concurrent(vols[:2], groups=4, max_bond=10, reconstruct=False)
    assert recs is None and len(objs) == 2


@pytest.mark.parametrize("shape,chi", [((64, 64, 64), 16), ((128, 128, 128), 32), ((32, 32, 16, 24), 12),
                                       ((48, 40, 36), 12), ((512, 680), 24), ((8, 512, 680), None), ((7, 11, 13), None)],
                         ids=str)
def test_fused_decode_is_bit_identical_to_chain_plus_permute(shape, chi):
    """to_tensor writes the volume from the accumulators of the last chain product (inverse permutation in the
    epilogue); the site-order tensor is never formed.  Same products in the same order as the unfused route
    (chain -> site-order tensor -> decode_permute), so the results are bit-identical."""
    lib = _lib.load()
    x = synthetic_mri(shape, seed=9) if len(shape) <= 4 and min(shape) > 8 else np.random.default_rng(9).random(shape).astype(np.float32)
    obj = NDMPS.from_tensor(x, max_bond=chi)
    fused = obj.to_tensor(as_torch=True)
    dense = obj.mps.to_dense()
    plan = _plan_for(shape, 0)
    unfused = torch.empty(shape, dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_decode_permute(plan.handle, dense.data_ptr(), unfused.data_ptr(), 4, sp()))
    assert torch.equal(fused, unfused)
    n_tail = lib.ndmps_chain_tail_columns(len(obj.mps.dims), _lib.i64_array(obj.mps.dims))
    assert (n_tail > 0) == (len(obj.mps.dims) >= 2 and obj.mps.dims[-1] <= 4096)


@pytest.mark.parametrize("dtype", ["bfloat16", "float64", "float32-unfused"])
@pytest.mark.parametrize("mode,norm", [("Std", False), ("DCT", True)])
def test_group_paths_of_the_other_storage_types_equal_one_by_one(dtype, mode, norm, monkeypatch):
    """bf16 / fp64 storage (and fp32 with the fused reshape stage switched off) run the stand-alone reshape stage, the
    norm and the DCT / IDCT of a lockstep group in one launch each: cores and reconstructions equal the volume-by-volume
    calls bit for bit."""
    shape, chi, count = (32, 32, 16, 24), 12, 4
    if dtype == "float32-unfused":
        monkeypatch.setenv("NDMPS_NO_FUSED_ENCODE", "1")
        monkeypatch.setenv("NDMPS_NO_FUSED_DECODE", "1")
        store = torch.float32
    else:
        store = getattr(torch, dtype)
    vols = [synthetic_mri(shape, seed=70 + i) for i in range(count)]
    group = NDMPS.from_tensors(vols, mode=mode, norm=norm, max_bond=chi, dtype=store)
    single = [NDMPS.from_tensor(v, mode=mode, norm=norm, max_bond=chi, dtype=store) for v in vols]
    for g, s1 in zip(group, single):
        assert g.bond_sizes() == s1.bond_sizes()
        assert all(torch.equal(a, b) for a, b in zip(g.mps.cores, s1.mps.cores))
    together = NDMPS.to_tensors(group, as_torch=True)
    for g, r in zip(group, together):
        assert torch.equal(r, g.to_tensor(as_torch=True))
    as_numpy = NDMPS.to_tensors(group)
    for g, r in zip(group, as_numpy):
        assert np.array_equal(r, g.to_tensor())


@pytest.mark.parametrize("shape,chi,mode,count", [((64, 64, 64), 16, "Std", 5), ((32, 32, 16, 24), 12, "DCT", 3),
                                                  ((48, 40, 36), None, "Std", 2), ((7, 11, 13), 4, "Std", 3)], ids=str)
def test_to_tensors_equals_to_tensor_per_object(shape, chi, mode, count):
    """NDMPS.to_tensors issues the chain products of a whole list from one library call; same kernels on the same
    operands as to_tensor per object, so bit-identical -- also for objects with different bonds (one of them is
    truncated further) and through the NumPy return path."""
    vols = [synthetic_mri(shape, seed=40 + i) if min(shape) > 8 else
            np.random.default_rng(40 + i).random(shape).astype(np.float32) for i in range(count)]
    objs = NDMPS.from_tensors(vols, mode=mode, max_bond=chi)
    # equal bonds (the caps bind): the whole list goes through the chain together, one batched launch per stage
    for a, b in zip([o.to_tensor(as_torch=True) for o in objs], NDMPS.to_tensors(objs, as_torch=True)):
        assert torch.equal(a, b)
    objs[-1].compress(0.05)
    assert objs[-1].bond_sizes() != objs[0].bond_sizes() or chi is None or not objs[0].bond_sizes()  # (7, 11, 13): one site
    one_by_one = [o.to_tensor(as_torch=True) for o in objs]
    together = NDMPS.to_tensors(objs, as_torch=True)
    assert len(together) == count
    for a, b in zip(one_by_one, together):
        assert a.shape == tuple(shape) and torch.equal(a, b)
    as_numpy = NDMPS.to_tensors(objs)
    assert all(isinstance(r, np.ndarray) and np.array_equal(r, a.cpu().numpy()) for r, a in zip(as_numpy, one_by_one))
    assert NDMPS.to_tensors([]) == []
    # reconstruct=True: the decode is issued before the objects exist; same result
    objs2, recs2 = NDMPS.from_tensors(vols, mode=mode, max_bond=chi, reconstruct=True)
    for o, r in zip(objs2, recs2):
        assert torch.equal(r, o.to_tensor(as_torch=True))
    assert NDMPS.from_tensors([], reconstruct=True) == ([], [])
    assert torch.equal(NDMPS.to_tensors(objs[:1], as_torch=True)[0], one_by_one[0])


def test_group_state_arrives_on_first_access_and_matches_the_eager_reductions():
    """After from_tensors the min / max / norm reductions of the whole group are in flight on the device; the numbers
    arrive when boundary_list / norm_value are first read (core/ndmps.py:75-76 computes them inside from_tensor).
    They equal the eager per-object reductions, survive deepcopy, and values set explicitly in between win."""
    import copy

    vols = [synthetic_mri((64, 64, 64), seed=70 + i) for i in range(4)]
    objs = NDMPS.from_tensors(vols, max_bond=16)
    assert all(o.__dict__.get("_state_group") is not None for o in objs)  # nothing collected yet
    objs[3].norm_value = 123.0                      # explicit value before the collection
    clone = copy.deepcopy(objs[1])                  # collects
    assert all(o.__dict__.get("_state_group") is None for o in objs)
    assert objs[3].norm_value == 123.0
    for o in objs[:3] + [clone]:
        eager = np.array([list(v) for v in hft.minmax_many(o.mps.cores)])
        assert np.array_equal(np.asarray(o.boundary_list), eager)
        assert math.isclose(o.norm_value ** 2, o.mps @ o.mps, rel_tol=1e-5)
    single = NDMPS.from_tensor(vols[0], max_bond=16)  # a single volume takes the eager path
    assert np.array_equal(np.asarray(single.boundary_list), np.asarray(objs[0].boundary_list))
    assert math.isclose(single.norm_value, objs[0].norm_value, rel_tol=1e-6)
    objs[0].mps.arrays[0][:] *= 10
    objs[0].update_boundary_list()
    assert objs[0].boundary_list[0][1] > 5 * clone.boundary_list[0][1] or objs[0].boundary_list[0][1] > 0


@pytest.mark.parametrize("shape,chi,mode", [((64, 64, 64), 16, "Std"), ((128, 128, 128), 64, "Std"),
                                            ((128, 128, 128), 32, "DCT"), ((64, 64, 64), 32, "DCT")], ids=str)
def test_fused_encode_matches_permute_then_sweep(shape, chi, mode):
    """The bond-capped fp32 sweep reads the volume through the permutation tables (raw Gram pass + projection of
    the merged run); no site-order tensor is formed and the input is left untouched.  The Gram matrices agree with
    the unfused route to fp64 rounding; the carried matrix sums its products over the columns in memory order
    instead of site order, so everything downstream agrees to fp32 rounding."""
    lib = _lib.load()
    x = torch.from_numpy(synthetic_mri(shape, seed=13)).to(DEV)
    keep = x.clone()
    plan = _plan_for(shape, 0)
    dims = [int(q) for q in plan.qubit_size]
    L = len(dims)
    n_merge = lib.ndmps_tt_merge_columns(L, _lib.i64_array(dims), chi)
    assert n_merge > 0 and plan.gather_tables(n_merge, torch.device(DEV)) is not None
    fused = NDMPS.from_tensor(x, max_bond=chi, mode=mode)
    assert torch.equal(x, keep)
    # the unfused route through the C ABI: permute, then the plain sweep
    xin = x
    if mode == "DCT":
        from imgcompressionmps_amd.core.ndmps import _dct_basis
        xin = torch.empty_like(x)
        _lib.check(lib.ndmps_dct_last_f32(x.data_ptr(), xin.data_ptr(), x.numel() // shape[-1], shape[-1],
                                          _dct_basis(shape[-1], torch.device(DEV)).data_ptr(), sp()))
    dense = torch.empty(x.numel(), dtype=torch.float32, device=DEV)
    _lib.check(lib.ndmps_encode_permute(plan.handle, xin.data_ptr(), dense.data_ptr(), 4, sp()))
    cdims = _lib.i64_array(dims)
    core_off = (C.c_int64 * (L + 1))()
    spec_off = (C.c_int64 * (L + 1))()
    max_bonds = (C.c_int64 * (L + 1))()
    _lib.check(lib.ndmps_tt_layout(L, cdims, chi, max_bonds, core_off, spec_off, None))
    nbytes = lib.ndmps_tt_sweep_batched_workspace_bytes(1, L, cdims, chi)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    arena = torch.zeros(int(core_off[L]), dtype=torch.float32, device=DEV)
    bonds = (C.c_int64 * (L + 1))()
    _lib.check(lib.ndmps_tt_sweep_batched_f32(1, (C.c_void_p * 1)(dense.data_ptr()), L, cdims, 1e-10, chi,
                                              (C.c_void_p * 1)(arena.data_ptr()), core_off, bonds, None, spec_off,
                                              ws.data_ptr(), nbytes, sp()))
    assert [int(b) for b in bonds][1:-1] == fused.bond_sizes()
    merged_from = next(i for i in range(1, L) if int(np.prod(dims[i:])) == n_merge)
    from imgcompressionmps_amd.core.mps import DeviceMPS

    ref_cores = []
    for i, core in enumerate(fused.mps.cores):
        k0, k1 = int(bonds[i]), int(bonds[i + 1])
        ref = arena[int(core_off[i]): int(core_off[i]) + k0 * dims[i] * k1].view(k0, dims[i], k1)
        ref_cores.append(ref)
    assert merged_from >= 1
    # the two routes sum the same exact products, but a pair of columns that shares a diagonal tile in memory order
    # may sit in an off-diagonal one in site order, and those have different slab lengths (gram128_kernel): the
    # Gram matrices agree to fp64 rounding, not bit for bit.  Cores are eigenvectors (inside noise-floor clusters
    # individually ill-conditioned): compare what they represent
    a, b = fused.mps.to_dense(), DeviceMPS(ref_cores).to_dense()
    assert float((a - b).norm() / b.norm()) <= 2e-6


def test_minmax_many_matches_single():
    ts = [torch.randn(n, device=DEV) for n in (1, 17, 4096, 100003)]
    got = hft.minmax_many(ts)
    assert got == [hft.minmax(t) for t in ts]


# ------------------------------------------------------ BASELINE configs at full size (properties)
def _projection_checks(x, obj, rec, tol=2e-4):
    """Size-independent properties of a truncated sweep: the reconstruction is an orthogonal
    projection of the (possibly DCT-transformed) data, so ||x||^2 = ||rec||^2 + ||x - rec||^2 and
    <x - rec, rec> = 0; the stored norm is ||rec||."""
    x64 = x.double()
    r64 = rec.double()
    nx, nr, ne = float((x64 * x64).sum()), float((r64 * r64).sum()), float(((x64 - r64) ** 2).sum())
    assert abs(nx - nr - ne) <= tol * nx
    assert abs(float(((x64 - r64) * r64).sum())) <= tol * nx
    assert math.isclose(obj.norm_value ** 2, nr, rel_tol=max(1e-4, tol))
    return ne / nx


def test_config2_256_cubed_chi32_properties_and_idempotence():
    """BASELINE configs[1]: 256^3 fp32, chi = 32 (oracle-sized cases are covered at 128^3)."""
    x = torch.from_numpy(synthetic_mri((256, 256, 256), seed=2025)).to(DEV)
    obj = NDMPS.from_tensor(x, max_bond=32)
    assert obj.bond_sizes() == [8, 32, 32, 32, 32, 32, 8]
    assert obj.number_elements_in_MPS() == 36992
    rec = obj.to_tensor(as_torch=True)
    err = _projection_checks(x, obj, rec)
    assert err < 1e-2
    # re-encoding the rank-32 reconstruction changes nothing (idempotence of the truncation)
    again = NDMPS.from_tensor(rec, max_bond=32).to_tensor(as_torch=True)
    assert float((again - rec).norm() / rec.norm()) <= 1e-5
    # a larger bond cap can only reduce the error
    err64 = _projection_checks(x, *(lambda o: (o, o.to_tensor(as_torch=True)))(NDMPS.from_tensor(x, max_bond=64)))
    assert err64 <= err


def test_metric_config_256_cubed_chi64_matches_oracle():
    """The configuration BASELINE.json's metric is quoted on (256^3 fp32, chi = 64, Std), against the
    oracle on the same volume (closed-form permutation: the materialised map needs ~10 GiB): equal bonds,
    relative Frobenius <= 2e-5, |dSSIM| <= 1e-5 -- the figures bench.py prints in `parity`.
    Parity unpinned at the quimb boundary: the oracle is this repo's restatement."""
    x = synthetic_mri((256, 256, 256), seed=2025)
    gpu = NDMPS.from_tensor(x, max_bond=64)
    ref = OracleNDMPS.from_tensor(x, max_bond=64, materialise_map=False)
    assert gpu.bond_sizes() == ref.bond_sizes() == [8, 64, 64, 64, 64, 64, 8]
    assert gpu.number_elements_in_MPS() == 139392
    rg, rr = gpu.to_tensor(), ref.to_tensor()
    assert np.linalg.norm(rg - rr) / np.linalg.norm(rr) <= 2e-5
    assert _ssim_gap(x, rg, rr) <= 1e-5
    assert math.isclose(gpu.norm_value, ref.norm_value, rel_tol=1e-5)
    for i in range(1, 8):
        s_ref, s_gpu = ref.sweep_spectra[i], gpu.sweep_spectra[i]
        m = min(len(s_ref), len(s_gpu), 64)
        assert np.abs(s_gpu[:m] - s_ref[:m]).max() <= 1e-5 * s_ref[0], i


def test_config3_512_cubed_dct_chi64_properties():
    """BASELINE configs[2]: 512^3 fp32, DCT mode, chi = 64 (HBM-bound reshape path)."""
    g = torch.Generator(device=DEV).manual_seed(2025)
    z = torch.linspace(0, 1, 512, device=DEV)
    x = (torch.sin(6.0 * z)[:, None, None] * torch.cos(4.0 * z)[None, :, None] * (1.0 + z)[None, None, :]
         + 0.3 * torch.exp(-((z[:, None, None] - 0.4) ** 2 + (z[None, :, None] - 0.6) ** 2 + (z[None, None, :] - 0.5) ** 2) / 0.02)
         + 0.01 * torch.randn((512, 512, 512), device=DEV, generator=g)).float()
    x -= x.min()
    x /= x.max()
    obj = NDMPS.from_tensor(x, mode="DCT", max_bond=64)
    assert obj.bond_sizes() == [8, 64, 64, 64, 64, 64, 64, 8]
    assert obj.number_elements_in_MPS() == 172160
    rec = obj.to_tensor(as_torch=True)
    assert rec.shape == x.shape
    err = _projection_checks(x, obj, rec)  # the orthonormal DCT keeps the projection identities
    assert err < 2e-3
    del rec, obj
    torch.cuda.empty_cache()


def test_config4_batch_of_128_cubed_chi32_matches_oracle_on_samples():
    """BASELINE configs[3] (one rank's shard): 8 independent 128^3 volumes, chi = 32, encoded in
    lockstep; two of them are checked against the oracle, all of them through properties."""
    vols = [synthetic_mri((128, 128, 128), seed=2025 + i) for i in range(8)]
    objs = NDMPS.from_tensors(vols, max_bond=32)
    for i, (v, o) in enumerate(zip(vols, objs)):
        assert o.bond_sizes() == [8, 32, 32, 32, 32, 8] and o.number_elements_in_MPS() == 28800
        rec = o.to_tensor(as_torch=True)
        _projection_checks(torch.from_numpy(v).to(DEV), o, rec)
        if i in (0, 5):
            ref = OracleNDMPS.from_tensor(v, max_bond=32)
            rr = ref.to_tensor()
            assert np.linalg.norm(rec.cpu().numpy() - rr) / np.linalg.norm(rr) <= 2e-5
            assert _ssim_gap(v, rec.cpu().numpy(), rr) <= 1e-5


def test_config5_shape_4d_fmri_chi128_fp32_properties():
    """BASELINE configs[4] geometry (128x128x64x256, site dims 64,32,16,16,16,32, chi = 128) in fp32
    storage (the bf16 storage the config names: test_config5_full_size_bf16_storage_chi128_properties):
    eigenproblems up to 2048 x 2048."""
    g = torch.Generator(device=DEV).manual_seed(7)
    ax = [torch.linspace(-1, 1, n, device=DEV) for n in (128, 128, 64)]
    vol = torch.zeros((128, 128, 64), device=DEV)
    for c, w_, a in ((0.2, 0.3, 1.0), (-0.4, 0.15, 0.7), (0.5, 0.5, 0.4)):
        vol += a * (torch.exp(-0.5 * ((ax[0] - c) / w_) ** 2)[:, None, None]
                    * torch.exp(-0.5 * ((ax[1] + c) / w_) ** 2)[None, :, None]
                    * torch.exp(-0.5 * (ax[2] / (2 * w_)) ** 2)[None, None, :])
    tt = torch.linspace(0, 1, 256, device=DEV)
    x = vol[..., None] * (1.0 + 0.25 * torch.sin(2 * math.pi * 2.0 * tt))
    x = (x + 0.01 * torch.randn(x.shape, device=DEV, generator=g)).float()
    x -= x.min()
    x /= x.max()
    assert list(hc.site_dims((128, 128, 64, 256))) == [64, 32, 16, 16, 16, 32]
    obj = NDMPS.from_tensor(x, max_bond=128)
    assert obj.bond_sizes() == [64, 128, 128, 128, 32]
    assert obj.number_elements_in_MPS() == 857088
    rec = obj.to_tensor(as_torch=True)
    err = _projection_checks(x, obj, rec)
    assert err < 5e-3
    del rec, obj, x
    torch.cuda.empty_cache()


def test_bf16_volume_in_and_out():
    """bf16 storage at the boundary (BASELINE configs[4] names bf16): the volume is read as bf16,
    arithmetic is fp32, the reconstruction can be returned as bf16.  Checked against the oracle on
    the bf16-rounded values; tolerance = bf16 rounding of the output (2^-8 relative)."""
    x32 = torch.from_numpy(synthetic_mri((32, 32, 16, 24), seed=5)).to(DEV)
    xb = x32.to(torch.bfloat16)
    obj = NDMPS.from_tensor(xb, max_bond=20)
    ref = OracleNDMPS.from_tensor(xb.float().cpu().numpy(), max_bond=20)
    assert obj.bond_sizes() == ref.bond_sizes()
    rr = ref.to_tensor()
    r32 = obj.to_tensor(as_torch=True)
    assert float((r32.double().cpu() - torch.from_numpy(rr)).norm() / np.linalg.norm(rr)) <= 2e-5
    rb = obj.to_tensor(as_torch=True, dtype=torch.bfloat16)
    assert rb.dtype == torch.bfloat16 and rb.shape == xb.shape
    assert float((rb.float() - r32).abs().max()) <= 2.0 ** -8 * float(r32.abs().max())


# ------------------------------------------------------------------ bf16 storage path (BASELINE configs[4])
# Tolerance of everything below: bf16 keeps 8 significant bits, every stored value (volume, carried matrix,
# core, chain intermediate, reconstruction) is rounded to 2^-9 relative; a reconstruction goes through ~2 L of
# them, so results are compared at 2e-2 relative (fp32 accumulation errors are four orders smaller).
BF16_TOL = 1e-2  # twice what the 64 x 64 x 32 x 64 sample of BASELINE config 5 measures (4.8e-3 relative, bench.py bf16_price)


@pytest.mark.parametrize("m,n,k,transB", [(128, 128, 64, 1), (1000, 130, 70, 0), (4097, 256, 128, 0), (300, 8, 8, 1),
                                           (64, 512, 32, 0), (5, 3, 2, 1)])
def test_gemm_bf16_against_fp32_products(m, n, k, transB):
    """v_mfma_f32_32x32x16_bf16 GEMM: bf16 operands, fp32 accumulation, bf16 result; both layouts of the right
    operand, ragged extents, against the fp32 product of the same bf16 values rounded once."""
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = torch.randn((m, k), device=DEV, generator=g).to(torch.bfloat16)
    b = torch.randn((n, k) if transB else (k, n), device=DEV, generator=g).to(torch.bfloat16)
    c = torch.full((m, n), float("nan"), device=DEV, dtype=torch.bfloat16)
    nbytes = lib.ndmps_gemm_bf16_workspace_bytes(transB, n, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    _lib.check(lib.ndmps_gemm_bf16(transB, m, n, k, a.data_ptr(), k, b.data_ptr(), k if transB else n, c.data_ptr(), n,
                                   ws.data_ptr(), nbytes, sp()))
    ref = a.float() @ (b.float().T if transB else b.float())
    assert torch.isfinite(c.float()).all()
    err = (c.float() - ref).abs()
    assert float((err / (ref.abs() + math.sqrt(k))).max()) <= 2.0 ** -8  # one bf16 rounding of the fp32 sum


def test_gram_bf16_is_exact_in_fp64():
    """Integers up to 255 are bf16 numbers; their products and every partial sum of 5000 of them are integers below
    2**53, so the fp64 accumulation is exact in any order: G is the integer matrix, bit for bit."""
    lib = _lib.load()
    for m, n in ((5000, 8), (4096, 40), (3000, 512), (700, 130)):
        a = torch.randint(-255, 256, (m, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(m + n))
        ab = a.to(torch.bfloat16)
        assert torch.equal(ab.to(torch.int64), a)
        g = torch.full((n, n), float("nan"), dtype=torch.float64, device=DEV)
        nbytes = lib.ndmps_gram_workspace_bytes(m, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ndmps_gram_bf16(ab.data_ptr(), m, n, n, g.data_ptr(), ws.data_ptr(), nbytes, sp()))
        a64 = a.cpu().numpy().astype(np.float64)
        assert np.array_equal(g.cpu().numpy(), a64.T @ a64)   # exact in NumPy's order of summation as well


def test_bf16_and_fp32_sweep_on_a_4d_sample_with_three_capped_bonds_match_the_oracle():
    """64 x 64 x 64 x 64 (16.8 Mvoxels: site dims 16 x 6, exact bonds [16, 256, 4096, 256, 16]) at chi = 128: the cap
    binds on THREE bonds and three eigenproblems of order 16 x 128 = 2048 (BASELINE config 5's; the panel-blocked
    reduction) are on the path.  bf16 storage end to end and bf16 cores behind an fp32 sweep (carry_dtype) against the
    oracle on the bf16-rounded tensor at BF16_TOL; fp32 storage at the fp32 bar."""
    shape, chi = (64, 64, 64, 64), 128
    xb = torch.from_numpy(synthetic_mri(shape, seed=5)).to(DEV).to(torch.bfloat16)
    x32 = xb.float()
    ref = OracleNDMPS.from_tensor(x32.cpu().numpy(), max_bond=chi)
    assert ref.bond_sizes() == [16, 128, 128, 128, 16]
    rr = ref.to_tensor()
    for carry in (None, torch.float32):
        obj = NDMPS.from_tensor(xb, max_bond=chi, dtype=torch.bfloat16, carry_dtype=carry)
        assert all(c.dtype == torch.bfloat16 for c in obj.mps.cores) and obj.bond_sizes() == ref.bond_sizes()
        rec = obj.to_tensor(as_torch=True).double().cpu().numpy()
        assert np.linalg.norm(rec - rr) <= BF16_TOL * np.linalg.norm(rr)
        assert math.isclose(obj.norm_value, ref.norm_value, rel_tol=BF16_TOL)
        if carry is None:
            x64 = x32.double().cpu().numpy()
            assert abs(compute_ssim_by_dim(x64, rec) - compute_ssim_by_dim(x64, rr)) <= BF16_TOL
    obj = NDMPS.from_tensor(x32, max_bond=chi)
    assert obj.bond_sizes() == ref.bond_sizes()
    rec = obj.to_tensor(as_torch=True).double().cpu().numpy()
    assert np.linalg.norm(rec - rr) <= 3e-5 * np.linalg.norm(rr)


@pytest.mark.parametrize("shape,chi,mode", [((32, 32, 16, 24), 20, "Std"), ((64, 64, 64), 32, "Std"),
                                            ((32, 32, 16, 24), 16, "DCT"), ((48, 40, 36), 12, "Std"),
                                            ((64, 64, 32, 64), 128, "Std")], ids=str)
def test_bf16_storage_matches_oracle_on_bf16_rounded_input(shape, chi, mode):
    """dtype=torch.bfloat16: bf16 volume, bf16 carried matrices and cores, bf16 chain; against the fp64 oracle on
    the same bf16-rounded values.  Bonds are equal (the cap binds), everything else within BF16_TOL.
    (64, 64, 32, 64) at chi = 128 is BASELINE config 5 at an eighth of its extent per axis pair: site dims
    [64, 16, 16, 16, 32], exact bonds [64, 1024, 512, 32], so chi = 128 BINDS on two bonds and the order-2048
    eigenproblem of config 5's middle sites (k = 128 of n = 16 x 128) is on the path."""
    xb = torch.from_numpy(synthetic_mri(shape, seed=5)).to(DEV).to(torch.bfloat16)
    obj = NDMPS.from_tensor(xb, max_bond=chi, mode=mode, dtype=torch.bfloat16)
    ref = OracleNDMPS.from_tensor(xb.float().cpu().numpy(), max_bond=chi, mode=mode)
    assert all(c.dtype == torch.bfloat16 for c in obj.mps.cores)
    assert obj.bond_sizes() == ref.bond_sizes()
    rr = ref.to_tensor()
    rec = obj.to_tensor(as_torch=True)
    assert rec.dtype == (torch.bfloat16 if mode == "Std" else torch.float32) and tuple(rec.shape) == shape
    rel = float((rec.double().cpu() - torch.from_numpy(rr)).norm() / np.linalg.norm(rr))
    assert rel <= BF16_TOL, rel
    x64 = xb.double().cpu().numpy()
    assert abs(compute_ssim_by_dim(x64, rec.double().cpu().numpy()) - compute_ssim_by_dim(x64, rr)) <= BF16_TOL
    assert math.isclose(obj.norm_value, ref.norm_value, rel_tol=BF16_TOL)
    # the rest of the class surface works on bf16 cores (fp32 copies of the small cores where a kernel is fp32)
    assert math.isclose(obj.mps @ obj.mps, obj.norm_value ** 2, rel_tol=BF16_TOL)
    assert 0 < obj.compression_ratio_on_disk(np.uint16) < 1
    obj.compress(0.05)
    assert all(c.dtype == torch.bfloat16 for c in obj.mps.cores)
    assert obj.to_tensor().shape == shape


@pytest.mark.parametrize("shape,chi,mode,dtype,tol", [
    ((32, 32), 8, "Std", None, 2e-5), ((64, 64, 64), 16, "Std", None, 2e-5), ((48, 40, 36), 12, "DCT", None, 3e-5),
    ((16, 16, 8, 12), 10, "Std", None, 2e-5), ((128, 128, 128), 32, "Std", None, 2e-5),
    ((64, 64, 64), 16, "Std", torch.float64, 1e-9), ((48, 40, 36), 12, "Std", torch.float64, 1e-9)], ids=str)
def test_sweep_from_left_matches_the_oracles_left_sweep(shape, chi, mode, dtype, tol):
    """quimb's OTHER possible from_dense convention (SURVEY a4's caveat): sites 0 .. L-2, U is the site, S V^T carried
    right.  The GPU path runs it as the ordinary sweep on the mirrored chain (reversed-axes reshape stage, cores
    transposed back); the oracle writes the left sweep out directly.  Same bar as the default convention."""
    x = synthetic_mri(shape, seed=11)
    obj = NDMPS.from_tensor(x, max_bond=chi, mode=mode, dtype=dtype, sweep_from="left")
    ref = OracleNDMPS.from_tensor(x, max_bond=chi, mode=mode, sweep_from="left")
    assert obj.bond_sizes() == ref.bond_sizes()
    assert [tuple(c.shape) for c in obj.mps.cores] == [tuple(c.shape) for c in ref.mps.cores]
    rec, rr = obj.to_tensor(), ref.to_tensor()
    assert np.linalg.norm(rec - rr) <= tol * np.linalg.norm(rr)
    x64 = x.astype(np.float64)
    assert abs(compute_ssim_by_dim(x64, rec.astype(np.float64)) - compute_ssim_by_dim(x64, rr)) <= 1e-5
    # the gauge: sites 0 .. L-2 are left-isometric, the norm sits on the last site
    rtol = 1e-5 if dtype is None else 1e-10
    assert math.isclose(obj.norm_value, ref.norm_value, rel_tol=rtol)
    last = obj.mps.cores[-1].double()
    assert math.isclose(float(last.norm()), ref.norm_value, rel_tol=rtol)
    for c in obj.mps.cores[:-1]:
        m = c.double().reshape(-1, c.shape[2])
        assert float((m.T @ m - torch.eye(c.shape[2], dtype=torch.float64, device=DEV)).abs().max()) <= (2e-5 if dtype is None else 1e-10)
    # singular vectors are fixed up to a sign per bond (the library makes the largest component positive, LAPACK does
    # not): min and max of a core may trade places, the larger magnitude of the two does not
    assert np.allclose(np.abs(np.asarray(obj.boundary_list)).max(axis=1), np.abs(np.asarray(ref.boundary_list)).max(axis=1),
                       rtol=2e-4 if dtype is None else 1e-8)
    for i in range(1, len(ref.sweep_spectra)):
        k = min(len(obj.sweep_spectra[i]), chi)  # the direct solver computes the kept singular values only
        assert np.allclose(obj.sweep_spectra[i][:k], ref.sweep_spectra[i][:k], rtol=0, atol=1e-5 * ref.sweep_spectra[i][0])
    # the two conventions are different truncations of the same tensor, and compress starts from a different gauge
    other = NDMPS.from_tensor(x, max_bond=chi, mode=mode, dtype=dtype)
    assert other.bond_sizes() == obj.bond_sizes()
    assert np.linalg.norm(other.to_tensor() - rec) > 10 * tol * np.linalg.norm(rr) or chi >= min(shape)
    obj.compress(0.02)
    ref.compress(0.02)
    assert obj.bond_sizes() == ref.bond_sizes()
    assert np.linalg.norm(obj.to_tensor() - ref.to_tensor()) <= 2 * tol * np.linalg.norm(rr)


def test_sweep_from_left_exact_round_trip_and_lists():
    x = np.random.default_rng(2025).random((96, 80)).astype(np.float32)
    obj = NDMPS.from_tensor(x, sweep_from="left")
    assert np.allclose(obj.to_tensor(), x, atol=2e-5)
    xs = [synthetic_mri((32, 32, 32), seed=s) for s in (1, 2, 3)]
    objs, recs = NDMPS.from_tensors(xs, max_bond=8, sweep_from="left", reconstruct=True)
    for o, r, v in zip(objs, recs, xs):
        single = NDMPS.from_tensor(v, max_bond=8, sweep_from="left")
        assert o.bond_sizes() == single.bond_sizes()
        assert np.allclose(r.cpu().numpy(), single.to_tensor(), atol=2e-6)
    with pytest.raises(ValueError):
        NDMPS.from_tensor(x, sweep_from="middle")


def test_config5_full_size_bf16_storage_chi128_properties():
    """BASELINE configs[4] as stated: 128x128x64x256 bf16, chi = 128, one GPU.  Size-independent properties
    of the truncation (orthogonal projection: ||x||^2 = ||rec||^2 + ||x - rec||^2, <x - rec, rec> = 0) within
    BF16_TOL, bonds and element count of SURVEY's table, bf16 cores and bf16 reconstruction."""
    g = torch.Generator(device=DEV).manual_seed(7)
    ax = [torch.linspace(-1, 1, n, device=DEV) for n in (128, 128, 64)]
    vol = torch.zeros((128, 128, 64), device=DEV)
    for c, w_, a in ((0.2, 0.3, 1.0), (-0.4, 0.15, 0.7), (0.5, 0.5, 0.4)):
        vol += a * (torch.exp(-0.5 * ((ax[0] - c) / w_) ** 2)[:, None, None]
                    * torch.exp(-0.5 * ((ax[1] + c) / w_) ** 2)[None, :, None]
                    * torch.exp(-0.5 * (ax[2] / (2 * w_)) ** 2)[None, None, :])
    tt = torch.linspace(0, 1, 256, device=DEV)
    x = vol[..., None] * (1.0 + 0.25 * torch.sin(2 * math.pi * 2.0 * tt))
    x = (x + 0.01 * torch.randn(x.shape, device=DEV, generator=g)).float()
    x -= x.min()
    x /= x.max()
    xb = x.to(torch.bfloat16)
    del x, vol
    obj = NDMPS.from_tensor(xb, max_bond=128, dtype=torch.bfloat16)
    assert obj.bond_sizes() == [64, 128, 128, 128, 32]
    assert obj.number_elements_in_MPS() == 857088
    assert all(c.dtype == torch.bfloat16 for c in obj.mps.cores)
    rec = obj.to_tensor(as_torch=True)
    assert rec.dtype == torch.bfloat16
    err = _projection_checks(xb.float(), obj, rec.float(), tol=BF16_TOL)
    assert err < 1e-2
    del rec, obj, xb
    torch.cuda.empty_cache()


def test_reference_flow_exact_then_compress_64_and_128_cubed():
    """The reference's own flow (from_tensor without a bond cap, then cumulative compress(cutoff),
    evaluation/benchmark.py:176-178) at 64^3 against the oracle, and its exact step at 128^3
    (bonds 8, 64, 512, 512, 64, 8: 512 x 512 and wide 512 x 4096 unfoldings)."""
    x = synthetic_mri((64, 64, 64), seed=21)
    gpu, ref = NDMPS.from_tensor(x), OracleNDMPS.from_tensor(x)
    assert gpu.bond_sizes() == ref.bond_sizes() == [8, 64, 512, 64, 8]
    assert np.abs(gpu.to_tensor() - x).max() <= 2e-5
    for cutoff in (0.01, 0.03, 0.1):
        gpu.compress(cutoff)
        ref.compress(cutoff)
        assert gpu.bond_sizes() == ref.bond_sizes(), cutoff
        rg, rr = gpu.to_tensor(), ref.to_tensor()
        assert np.linalg.norm(rg - rr) / np.linalg.norm(rr) <= 5e-5
        assert _ssim_gap(x, rg, rr) <= 1e-5
        assert math.isclose(gpu.compression_ratio(), ref.compression_ratio(), rel_tol=1e-12)
    y = torch.from_numpy(synthetic_mri((128, 128, 128), seed=22)).to(DEV)
    big = NDMPS.from_tensor(y)
    assert big.bond_sizes() == [8, 64, 512, 512, 64, 8]
    assert float((big.to_tensor(as_torch=True) - y).abs().max()) <= 2e-5


# ----------------------------------------------------------------- device-side quality metrics
def test_device_ssim_psnr_match_oracle_and_reference_fixtures(golden_dir):
    from imgcompressionmps_amd.utils import metrics as dm
    from oracle import metrics as om

    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    for name in ("2d", "3d", "4d", "2d_small"):
        a32, b32 = g[name + "/a"].astype(np.float32), g[name + "/b"].astype(np.float32)
        # same fp32 values on both sides: agreement to fp64 rounding
        want = om.compute_ssim_by_dim(a32.astype(np.float64), b32.astype(np.float64))
        got = dm.compute_ssim_by_dim(a32, b32)
        assert abs(got - want) <= 1e-12, (name, got, want)
        # against the value the reference's own metrics.py produced on the fp64 arrays
        assert abs(got - float(g[name + "/ssim"])) <= 5e-6
        wantp = om.compute_psnr(a32.astype(np.float64), b32.astype(np.float64))
        assert abs(dm.compute_psnr(a32, b32) - wantp) <= 1e-9 * abs(wantp)
        assert abs(dm.compute_psnr(a32, b32) - float(g[name + "/psnr"])) <= 1e-4
    x = synthetic_mri((48, 40, 56), seed=9)
    y = x + 0.03 * np.random.default_rng(1).standard_normal(x.shape).astype(np.float32)  # negative values: clip
    assert abs(dm.compute_ssim_by_dim(x, y) - om.compute_ssim_by_dim(x.astype(np.float64), y.astype(np.float64))) <= 1e-12
    assert dm.compute_psnr(x, x) == np.inf
    with pytest.raises(ValueError):
        dm.compute_ssim_by_dim(np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError):
        dm.compute_ssim_by_dim(np.zeros((2, 9), dtype=np.float32), np.zeros((2, 9), dtype=np.float32))


def test_device_ssim_3d_axis_lists_match_the_reference_fixture(golden_dir):
    """ssim_3d_axis (utils/metrics.py:35-65): the per-slice lists along each axis against the lists the reference's own
    function produced (tests/golden/make_golden_metrics.py, skimage 0.18.3) and against the oracle on the same fp32
    values; a volume with negative values (the clip), the axis checks, negative axis numbers."""
    from imgcompressionmps_amd.utils import metrics as dm
    from oracle import metrics as om

    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    a32, b32 = g["3d/a"].astype(np.float32), g["3d/b"].astype(np.float32)
    means = []
    for axis in range(3):
        got = dm.ssim_3d_axis(a32, b32, axis)
        assert isinstance(got, list) and len(got) == a32.shape[axis]
        want = om.ssim_3d_axis(a32.astype(np.float64), b32.astype(np.float64), axis)
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12
        assert np.abs(np.array(got) - g[f"3d/ssim_axis{axis}"]).max() <= 5e-6  # the reference ran on the fp64 arrays
        means.append(np.mean(got))
    assert abs(np.mean(means) - dm.compute_ssim_by_dim(a32, b32)) <= 1e-12
    assert dm.ssim_3d_axis(a32, b32, -1) == dm.ssim_3d_axis(a32, b32, 2)
    x = synthetic_mri((48, 40, 56), seed=9)
    y = x + 0.03 * np.random.default_rng(1).standard_normal(x.shape).astype(np.float32)  # negative values: clip
    for axis in range(3):
        want = om.ssim_3d_axis(x.astype(np.float64), y.astype(np.float64), axis)
        assert np.abs(np.array(dm.ssim_3d_axis(torch.from_numpy(x).to(DEV), y, axis)) - np.array(want)).max() <= 1e-12
    with pytest.raises(ValueError):
        dm.ssim_3d_axis(x, y, 3)
    with pytest.raises(ValueError):
        dm.ssim_3d_axis(x, y[:-1], 0)
    with pytest.raises(ValueError):
        dm.ssim_3d_axis(x[0], y[0], 0)


def test_device_ssim_256_cubed_against_oracle_sample():
    """Full-size SSIM on the device; the oracle checks one axis' worth of slices (host SSIM of a
    whole 256^3 pair takes ~10 s) plus the full value on a 96^3 crop."""
    from imgcompressionmps_amd.utils import metrics as dm
    from oracle import metrics as om

    x = synthetic_mri((256, 256, 256), seed=2025)
    obj = NDMPS.from_tensor(x, max_bond=16)
    rec = obj.to_tensor(as_torch=True)
    full = dm.compute_ssim_by_dim(torch.from_numpy(x).to(DEV), rec)
    assert 0.3 < full < 1.0
    xc, rc = x[80:176, 80:176, 80:176], rec[80:176, 80:176, 80:176].cpu().numpy()
    assert abs(dm.compute_ssim_by_dim(xc, rc) - om.compute_ssim_by_dim(xc.astype(np.float64), rc.astype(np.float64))) <= 1e-12


def test_conv_to_mps_streams_a_list_in_chunks_and_keeps_its_order(monkeypatch):
    """core/batch.conv_to_mps (evaluation/benchmark.py:58-77): same-shape lists go through the lockstep path chunk after chunk
    (chunks of 3 here: 64 volumes or 8 GiB otherwise), mixed shapes through the reference's loop; either way element i of the
    result is the MPS of tensor i -- bonds equal from_tensor's, reconstructions within the solver's rounding."""
    from imgcompressionmps_amd.core import batch

    vols = [synthetic_mri((32, 32, 32), seed=200 + i) for i in range(8)]
    monkeypatch.setattr(batch, "default_stream_shape", lambda n, o=512: (1, 2))
    real_min = min
    monkeypatch.setattr(batch, "min", lambda *a: real_min(3, *a) if len(a) == 2 and a[0] == 64 else real_min(*a), raising=False)
    for kw in ({"mode": "Std", "max_bond": 8}, {"mode": "DCT"}):
        got = batch.conv_to_mps(vols, **kw)
        assert len(got) == len(vols)
        for v, g in zip(vols, got):
            one = NDMPS.from_tensor(v, **kw)
            assert g.bond_sizes() == one.bond_sizes()
            a, b = g.to_tensor(as_torch=True), one.to_tensor(as_torch=True)
            assert float((a - b).norm() / b.norm()) <= 2e-5
    mixed = batch.conv_to_mps([vols[0], synthetic_mri((16, 16), seed=1)], mode="Std")
    assert [m.dim for m in mixed] == [3, 2]
    assert batch.conv_to_mps([]) == [] and len(batch.conv_to_mps(vols[:1])) == 1


def test_compress_list_on_three_lanes_equals_the_loop(monkeypatch):
    """core/batch.compress_list (evaluation/benchmark.py:103-118) deals the objects of a list to three host threads with a
    stream each; every object gets the same calls on the same operands as in the reference's loop: cores bit for bit."""
    from imgcompressionmps_amd.core import batch

    vols = [synthetic_mri((64, 64, 64), seed=400 + i) for i in range(7)]
    a = batch.conv_to_mps(vols, mode="Std")
    b = copy.deepcopy(a)
    batch.compress_list(a, 0.05)
    monkeypatch.setenv("NDMPS_COMPRESS_LIST_SERIAL", "1")
    batch.compress_list(b, 0.05)
    for x, y in zip(a, b):
        assert x.bond_sizes() == y.bond_sizes() and x.bond_sizes() != [1] * len(x.bond_sizes())
        assert all(torch.equal(p, q) for p, q in zip(x.mps.cores, y.mps.cores))
        assert x.norm_value == y.norm_value and np.array_equal(np.asarray(x.boundary_list), np.asarray(y.boundary_list))
    with pytest.raises(ValueError):
        batch.compress_list(a, None)


def test_run_benchmark_matches_an_oracle_driven_loop():
    """the reference's quality-vs-ratio loop (evaluation/benchmark.py:121-194) over a
    small list of volumes, device path vs the same loop driven with the oracle classes."""
    from imgcompressionmps_amd.core import batch
    from oracle import metrics as om

    vols = [synthetic_mri((32, 32, 32), seed=s) for s in (4, 5)]
    cutoffs = [0.02, 0.05]
    gpu_list = batch.conv_to_mps(vols, mode="Std")
    res = batch.run_benchmark(gpu_list, [torch.from_numpy(v).to(DEV) for v in vols], cutoffs, verbose=False)

    ora = [OracleNDMPS.from_tensor(v) for v in vols]
    ora0 = copy.deepcopy(ora)
    want = {k: [] for k in ("ssim", "compression_ratio", "bond_dims", "psnr", "fidelity", "gzip_ratio")}

    def snapshot():
        want["ssim"].append([om.compute_ssim_by_dim(o.to_tensor(), v.astype(np.float64)) for o, v in zip(ora, vols)])
        want["compression_ratio"].append([o.compression_ratio() for o in ora])
        want["bond_dims"].append([o.bond_sizes() for o in ora])
        want["psnr"].append([om.compute_psnr(o.to_tensor(), v.astype(np.float64)) for o, v in zip(ora, vols)])
        want["fidelity"].append([om.compute_overlap(o, r) for o, r in zip(ora, ora0)])
        want["gzip_ratio"].append([o.compression_ratio_on_disk(dtype=np.uint16, replace=True) for o in ora])

    snapshot()
    for c in cutoffs:
        for o in ora:
            o.compress(c)
        snapshot()
    assert set(res) == {"ssim", "compression_ratio", "bond_dims", "psnr", "fidelity", "storage", "gzip_bytes", "gzip_ratio"}
    assert res["ssim"].shape == (2, 3) and res["gzip_ratio"].shape == (2, 3)
    assert res["bond_dims"] == want["bond_dims"]
    assert np.allclose(res["compression_ratio"], np.array(want["compression_ratio"]).T, rtol=1e-12)
    assert np.abs(res["ssim"] - np.array(want["ssim"]).T).max() <= 2e-5
    # before any truncation the PSNR measures rounding noise: ~140 dB in fp32, ~296 dB in fp64
    assert np.all(res["psnr"][:, 0] > 120.0)
    assert np.abs(res["psnr"][:, 1:] - np.array(want["psnr"]).T[:, 1:]).max() <= 5e-3
    assert np.abs(res["fidelity"] - np.array(want["fidelity"]).T).max() <= 1e-5
    assert np.abs(res["gzip_ratio"] - np.array(want["gzip_ratio"]).T).max() <= 0.05  # gzip of fp32- vs fp64-derived uint16
    with pytest.raises(ValueError):
        batch.benchmark_metric(gpu_list, None, metric="nope")
    with pytest.raises(IndexError):
        batch.benchmark_metric(gpu_list, [1], metric="ssim")


# ------------------------------------------------------------------- 8f#4: container and driver
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.float32])
def test_container_round_trip(dtype, tmp_path):
    """dumps / loads: the payload is the reference's per-core gzip members (ndmps.py:209-234), the
    reloaded object reconstructs exactly what compress_to_dtype(replace=True) leaves."""
    from imgcompressionmps_amd.core import codec

    x = synthetic_mri((32, 32, 32), seed=31)
    for mode in ("Std", "DCT"):
        obj = NDMPS.from_tensor(x, mode=mode, max_bond=12)
        blob = codec.dumps(obj, dtype)
        again = codec.loads(blob)
        assert again.bond_sizes() == obj.bond_sizes() and again.mode == mode and again.dim == 3
        assert again.norm_value == obj.norm_value and tuple(again.qubit_size) == tuple(obj.qubit_size)
        if dtype is np.float32:
            assert np.array_equal(again.to_tensor(), obj.to_tensor())
        else:
            assert codec.payload_bytes(blob) == obj.get_bytesize_on_disk(dtype)
            twin = copy.deepcopy(obj)
            twin.compress_to_dtype(dtype, replace=True)
            assert np.array_equal(again.to_tensor(), twin.to_tensor())
            for a, b in zip(again.mps.cores, twin.mps.cores):
                assert torch.equal(a, b)
        assert np.array_equal(again.boundary_list, np.array([list(v) for v in hft.minmax_many(again.mps.cores)]))
    path = tmp_path / "vol.ndmps"
    size = codec.save(obj, path, np.uint16)
    assert path.stat().st_size == size
    assert np.array_equal(codec.load(path).to_tensor(), codec.loads(codec.dumps(obj, np.uint16)).to_tensor())
    # a uint16 container of a chi = 12 volume is far smaller than the volume
    assert size < x.nbytes / 8
    with pytest.raises(ValueError):
        codec.dumps(obj, np.int32)
    with pytest.raises(ValueError):
        codec.loads(blob[:-5])


def test_rccl_gathers_of_real_cores_single_rank():
    """the optional gathers with device tensors over the nccl (= RCCL) backend.  One GPU box:
    world size 1 (the multi-rank exchange pattern is covered with gloo in tests/test_batch_sharding.py)."""
    import socket

    import torch.distributed as dist

    from imgcompressionmps_amd.core import batch

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(DEV))
    try:
        vols = [torch.from_numpy(synthetic_mri((16, 16, 16), seed=40 + s)).to(DEV) for s in range(3)]
        objs = NDMPS.from_tensors(vols, max_bond=6)
        gathered = batch.all_gather_cores([o.mps.cores for o in objs])
        assert len(gathered) == 3
        for o, cores in zip(objs, gathered):
            assert all(c.is_cuda and torch.equal(a, c) for a, c in zip(o.mps.cores, cores))
        recs = [o.to_tensor(as_torch=True) for o in objs]
        allv = batch.all_gather_volumes(recs, 3)
        assert all(torch.equal(a, b) for a, b in zip(recs, allv))
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------- degenerate inputs
def _edge_cases():
    rng = np.random.default_rng(0)
    delta = np.zeros((16, 16, 16), np.float32)
    delta[3, 4, 5] = 2.0
    return {
        "zeros": np.zeros((16, 16, 16), np.float32),
        "const": np.full((16, 16, 16), 3.5, np.float32),
        "delta": delta,
        "tiny": (rng.random((16, 16, 16)) * 1e-30).astype(np.float32),
        "huge": (rng.random((16, 16, 16)) * 1e18).astype(np.float32),
        "2d": rng.random((12, 20)).astype(np.float32),
        "1d": rng.random((64,)).astype(np.float32),
        "prime": rng.random((7, 11, 13)).astype(np.float32),  # a single site: no bond at all
    }


@pytest.mark.parametrize("name", list(_edge_cases()))
@pytest.mark.parametrize("kw", [{}, {"max_bond": 4}, {"mode": "DCT"}], ids=["exact", "chi4", "dct"])
def test_degenerate_inputs_match_the_oracle(name, kw):
    """All-zero, constant, one-voxel, 1e-30 / 1e18 scaled, 1-D, 2-D and single-site inputs: same bonds,
    same norm and the same reconstruction as the oracle, nothing non-finite."""
    x = _edge_cases()[name]
    g = NDMPS.from_tensor(x, **kw)
    o = OracleNDMPS.from_tensor(x, **kw)
    rg, ro = g.to_tensor(), o.to_tensor()
    assert g.bond_sizes() == o.bond_sizes()
    assert np.isfinite(rg).all()
    scale = float(np.abs(x).max())
    assert np.abs(rg - ro).max() <= 2e-6 * scale
    assert abs(g.norm_value - o.norm_value) <= 2e-6 * o.norm_value
    if not kw.get("max_bond"):
        assert np.abs(rg - x).max() <= 2e-6 * scale


@pytest.mark.parametrize("m,n,batch", [(4096, 512, 1), (2048, 256, 3), (1024, 96, 1), (600, 64, 1), (8192, 64, 5), (900, 96, 2), (8203, 64, 3),
                                           (300, 64, 2)])
def test_gathered_gram_stores_its_result_through_the_column_permutation(m, n, batch):
    """The raw Gram of the fused sweep visits the columns in memory order (d_col_off ascending) and its slab
    reduction stores entry (a, b) at G[perm[a]][perm[b]]: the result equals the Gram of the gathered matrix with
    its columns in the caller's order."""
    lib = _lib.load()
    rng = np.random.default_rng(m + n)
    quads = rng.permutation(n // 4)
    perm = (4 * quads[:, None] + np.arange(4)[None, :]).reshape(-1).astype(np.int32)   # site-order column of position a
    col_off = np.arange(n, dtype=np.int64)                                             # position a reads offset a
    row_off = rng.permutation(m).astype(np.int64) * n
    bases = [rng.standard_normal(m * n).astype(np.float32) for _ in range(batch)]
    d_b = [dev(b) for b in bases]
    t_r, t_c, t_p = dev(row_off), dev(col_off), dev(perm)
    out = torch.zeros((batch, n, n), dtype=torch.float64, device=DEV)
    if batch == 1:
        nbytes = lib.ndmps_gram_workspace_bytes(m, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ndmps_gram_indexed_f32(d_b[0].data_ptr(), m, n, t_r.data_ptr(), t_c.data_ptr(), t_p.data_ptr(),
                                              out.data_ptr(), ws.data_ptr(), nbytes, sp()))
    else:
        nbytes = lib.ndmps_gram_batched_workspace_bytes(batch, m, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        ptrs = (C.c_void_p * batch)(*[t.data_ptr() for t in d_b])
        _lib.check(lib.ndmps_gram_batched_indexed_f32(batch, ptrs, m, n, t_r.data_ptr(), t_c.data_ptr(), t_p.data_ptr(),
                                                      out.data_ptr(), n * n, ws.data_ptr(), nbytes, sp()))
    got = out.cpu().numpy()
    for z in range(batch):
        a = bases[z][row_off[:, None] + col_off[None, :]].astype(np.float64)   # columns in visiting order
        ref = np.empty((n, n))
        ref[np.ix_(perm, perm)] = a.T @ a
        assert np.abs(got[z] - ref).max() <= 1e-13 * np.abs(ref).max() * math.sqrt(m)
        assert np.array_equal(got[z], got[z].T)


@pytest.mark.parametrize("m,n,batch", [(4096, 32, 3), (1000, 32, 2), (8200, 64, 2), (33, 32, 1)])
def test_streamed_projection_of_64_gathered_columns(m, n, batch):
    """ndmps_sgemm_gathered64_stream_batched (the first projection of a bond cap of 32 in the fused sweep): rows
    visited in ascending order of their offsets, every result row stored at its own place; against the fp64
    product of the gathered matrix, and bit for bit against the tile kernel on the same tables' site order."""
    lib = _lib.load()
    rng = np.random.default_rng(m + n + batch)
    quads = rng.permutation(16)
    col_off = (8 * quads[:, None] + np.arange(4)[None, :]).reshape(-1).astype(np.int64)   # aligned runs of four
    row_off = rng.permutation(m).astype(np.int64) * 128                                    # rows 128 floats apart
    order = np.argsort(row_off, kind="stable")
    bases = [rng.standard_normal(m * 128).astype(np.float32) for _ in range(batch)]
    ws_ = [rng.standard_normal((64, n)).astype(np.float32) for _ in range(batch)]
    d_a, d_w = [dev(b) for b in bases], [dev(w) for w in ws_]
    out = [torch.full((m, n), float("nan"), dtype=torch.float32, device=DEV) for _ in range(batch)]
    ref_out = [torch.empty((m, n), dtype=torch.float32, device=DEV) for _ in range(batch)]
    t_sorted, t_order, t_col, t_row = dev(row_off[order]), dev(order.astype(np.int32)), dev(col_off), dev(row_off)
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    _lib.check(lib.ndmps_sgemm_gathered64_stream_batched(batch, m, n, ptrs(d_a), t_sorted.data_ptr(), t_order.data_ptr(),
                                                         t_col.data_ptr(), ptrs(d_w), n, ptrs(out), n, sp()))
    _lib.check(lib.ndmps_sgemm_indexed_batched(batch, m, n, 64, ptrs(d_a), 0, t_row.data_ptr(), t_col.data_ptr(), 1, ptrs(d_w), n,
                                               ptrs(ref_out), n, None, None, sp()))
    for z in range(batch):
        a = bases[z][row_off[:, None] + col_off[None, :]].astype(np.float64)
        ref = a @ ws_[z].astype(np.float64)
        got = out[z].cpu().numpy()
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max() * 8
        assert np.abs(got - ref_out[z].cpu().numpy()).max() <= 2e-6 * np.abs(ref).max() * 8
