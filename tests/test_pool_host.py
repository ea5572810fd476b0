"""Host planner of the block-averaged decode (core/pool.py), without a GPU.

The block structure the planner relies on is checked on the materialised encoding map.  The planner's reduced
cores, suffix collapse and absorb are run through a NumPy fp64 emulation of what csrc/pool.hip computes, on random
cores, and compared with the dense contraction permuted to C order, reshaped and reduced.
"""
import itertools

import numpy as np
import pytest
from scipy.fft import idct

from imgcompressionmps_amd.core import pool
from imgcompressionmps_amd.utils import core as _core

SHAPES = [(64, 64, 64), (30, 45, 20), (512, 680), (16, 16, 8, 32)]  # tests/test_gpu_region.py
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
BLOCKS = {  # block sizes per k = 1, 2, ... (the issue's table)
    (30, 45, 20): [(5, 3, 5), (15, 9, 10), (30, 45, 20)],
    (512, 680): [(4, 2), (16, 4), (64, 8), (256, 40), (512, 680)],
    (16, 16, 8, 32): [(4, 2, 2, 2), (8, 4, 4, 8), (16, 16, 8, 32)],
    (64, 64, 64): [(2, 2, 2), (4, 4, 4), (8, 8, 8), (16, 16, 16), (32, 32, 32), (64, 64, 64)],
}


def _random_cores(shape, chi=6, seed=0):
    dims = _core.site_dims(shape)
    rng = np.random.default_rng(seed)
    bonds = [1]
    for i in range(1, len(dims)):
        bonds.append(int(min(chi, np.prod(dims[:i]), np.prod(dims[i:]))))
    bonds.append(1)
    return [rng.standard_normal((bonds[i], int(d), bonds[i + 1])) for i, d in enumerate(dims)]


def _site_tensor(cores):
    t = np.ones((1, 1))
    for c in cores:
        t = (t @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return t.reshape([c.shape[1] for c in cores])


def _dense_volume(shape, cores):
    _, enc = _core.gen_encoding_map(shape)
    return _site_tensor(cores)[tuple(enc)]


def _block_reduce(vol, blocks, op):
    shape = vol.shape
    inter = [v for n, b in zip(shape, blocks) for v in (n // b, b)]
    r = vol.reshape(inter)
    odd = tuple(range(1, 2 * len(shape), 2))
    return r.mean(axis=odd) if op == "mean" else r.sum(axis=odd)


def _coarse_from_plan(plan, cores, shape):
    """The emulated reduced chain decoded through the coarse factor array (site order -> C order)."""
    red = pool.emulate(cores, plan)
    if plan.L_keep == 0:
        return red[0].reshape(plan.coarse_shape)
    site = _site_tensor(red).ravel()
    pos = pool.site_order_positions(plan.coarse_shape, plan.out_factor)
    return site[pos].reshape(plan.coarse_shape)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_last_k_sites_enumerate_blocks(shape):
    fa, _ = _core.get_factorlist(shape)
    L = fa.shape[0]
    _, enc = _core.gen_encoding_map(shape)
    idx = np.indices(shape)
    for k in range(L + 1):
        B = pool.block_shape(fa, [k] * len(shape))
        if k:
            assert B == BLOCKS[shape][k - 1]
        # voxels sharing the digits of sites 0 .. L-k-1 are exactly the blocks i_a // B_a
        prefix = np.zeros(shape, dtype=np.int64)
        for l in range(L - k):
            prefix = prefix * int(np.prod(fa[l])) + enc[l]
        block = np.zeros(shape, dtype=np.int64)
        for a in range(len(shape)):
            block = block * (shape[a] // B[a]) + idx[a] // B[a]
        pairs = np.unique(np.stack([prefix.ravel(), block.ravel()]), axis=1)
        n_blocks = int(np.prod([n // b for n, b in zip(shape, B)]))
        assert pairs.shape[1] == n_blocks  # a bijection between prefixes and blocks
        assert np.unique(pairs[0]).size == n_blocks and np.unique(pairs[1]).size == n_blocks


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_block_shape_per_axis_levels(shape):
    fa, _ = _core.get_factorlist(shape)
    L = fa.shape[0]
    rng = np.random.default_rng(1)
    for _ in range(5):
        lev = rng.integers(0, L + 1, size=len(shape))
        want = tuple(int(np.prod(fa[L - k:, a])) for a, k in enumerate(lev))
        assert pool.block_shape(fa, lev) == want
        assert all(n % b == 0 for n, b in zip(shape, want))


def _level_cases(shape, L):
    nd = len(shape)
    cases = [[k] * nd for k in range(L + 1)]
    rng = np.random.default_rng(2)
    cases += [list(rng.integers(0, L + 1, size=nd)) for _ in range(3)]
    cases.append([L] + [0] * (nd - 1))
    cases.append([0] * (nd - 1) + [1])
    return cases


@pytest.mark.parametrize("op", ["mean", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulated_reduction_matches_dense(shape, op):
    cores = _random_cores(shape)
    vol = _dense_volume(shape, cores)
    fa, _ = _core.get_factorlist(shape)
    L = fa.shape[0]
    for lev in _level_cases(shape, L):
        plan = pool.PoolPlan(fa, lev, op)
        want = _block_reduce(vol, pool.block_shape(fa, lev), op)
        got = _coarse_from_plan(plan, cores, shape)
        assert got.shape == want.shape == plan.out_shape
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(vol).max() * vol.size, err_msg=str(lev))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulated_axis_sums_match_numpy(shape):
    cores = _random_cores(shape, seed=3)
    vol = _dense_volume(shape, cores)
    fa, _ = _core.get_factorlist(shape)
    L, nd = fa.shape
    for r in range(nd + 1):
        for axes in itertools.combinations(range(nd), r):
            lev = [L if a in axes else 0 for a in range(nd)]
            for op in ("mean", "sum"):
                plan = pool.PoolPlan(fa, lev, op)
                want = getattr(vol, op)(axis=axes, keepdims=True)
                got = _coarse_from_plan(plan, cores, shape)
                np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(vol).sum(), err_msg=str(axes))


def test_planner_tables():
    fa, _ = _core.get_factorlist((30, 45, 20))
    plan = pool.PoolPlan(fa, [1, 2, 0], "mean")
    assert plan.L_keep == 3
    assert plan.passthrough.tolist() == [True, False, False]
    # site 2 reduces axes 0 and 1, site 1 axis 1; output factors carry 1 in each reduced entry
    assert plan.out_factor.tolist() == [list(fa[0]), [fa[1, 0], 1, fa[1, 2]], [1, 1, fa[2, 2]]]
    assert plan.coarse_shape == (6, 5, 20) == plan.out_shape
    assert plan.weight[2] == pytest.approx(1.0 / (fa[2, 0] * fa[2, 1]))
    assert plan.offsets.dtype == np.int32
    for l in range(plan.L):
        dq, nr, q0, r0 = plan.sites[l]
        assert dq * nr == np.prod(fa[l])
        p = (plan.offsets[q0:q0 + dq][:, None] + plan.offsets[r0:r0 + nr][None, :]).ravel()
        assert np.array_equal(np.sort(p), np.arange(np.prod(fa[l])))  # every physical index exactly once
    full = pool.PoolPlan(fa, 3, "sum")
    assert full.L_keep == 0 and full.coarse_shape == (1, 1, 1) and np.all(full.weight == 1.0)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_plan_emulate_on_coarse_factor_array(shape):
    from imgcompressionmps_amd import _lib

    lib = _lib.load()
    fa, _ = _core.get_factorlist(shape)
    L = fa.shape[0]
    for lev in _level_cases(shape, L):
        plan = pool.PoolPlan(fa, lev, "mean")
        if plan.L_keep == 0:
            continue
        cshape, cfa = plan.coarse_shape, np.ascontiguousarray(plan.out_factor)
        numel = int(np.prod(cshape))
        out = np.empty(numel, dtype=np.int64)
        rc = lib.ndmps_plan_emulate(len(cshape), _lib.i64_array(cshape), cfa.shape[0], cfa.ctypes.data_as(_lib.p_i64),
                                    1, out.ctypes.data_as(_lib.p_i64))
        assert rc >= 0
        # mode 1: the site-order offset each C-order voxel reads
        assert np.array_equal(out, pool.site_order_positions(cshape, cfa)), lev
    # the explicit array of levels 0 is get_factorlist's: the map is gen_encoding_map's
    _, enc = _core.gen_encoding_map(shape)
    dims = np.prod(fa, axis=1)
    want = np.zeros(shape, dtype=np.int64)
    for l in range(L):
        want = want * int(dims[l]) + enc[l]
    assert np.array_equal(pool.site_order_positions(shape, fa), want.ravel())


@pytest.mark.parametrize("n", [8, 20, 64, 256])
def test_dct_dc_selection_and_pooled_basis(n):
    rng = np.random.default_rng(4)
    y = rng.standard_normal((5, n))
    x = idct(y, axis=-1, norm="ortho")
    np.testing.assert_allclose(x.sum(axis=-1), np.sqrt(n) * y[:, 0], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(x.mean(axis=-1), y[:, 0] / np.sqrt(n), rtol=1e-12, atol=1e-12)
    # the per-site weights of a picked last axis multiply to sqrt(n) / 1 / sqrt(n)
    fa, _ = _core.get_factorlist((3, n))
    for op, want in (("sum", np.sqrt(n)), ("mean", 1 / np.sqrt(n))):
        plan = pool.PoolPlan(fa, [0, fa.shape[0]], op, dct=True)
        assert np.prod(plan.weight) == pytest.approx(want)
        assert (plan.modes[:, -1] == pool.PICK).all()
    # pooled basis W[j, k] = w sum_{m in block j} B[m][k] (host model of ndmps_pool_dct_basis_*)
    j, k = np.arange(n)[:, None], np.arange(n)[None, :]
    basis = np.where(k == 0, np.sqrt(1 / n), np.sqrt(2 / n)) * np.cos(np.pi * (2 * j + 1) * k / (2 * n))
    for blk in (b for b in (2, 4, n) if n % b == 0):
        W = basis.reshape(n // blk, blk, n).sum(axis=1) / blk
        np.testing.assert_allclose(y @ W.T, x.reshape(5, n // blk, blk).mean(axis=-1), rtol=1e-10, atol=1e-12)


def test_dct_partial_last_axis_stays_on_the_sites():
    fa, _ = _core.get_factorlist((16, 16, 8, 32))
    plan = pool.PoolPlan(fa, [1, 1, 1, 2], "mean", dct=True)
    assert plan.chain_levels.tolist() == [1, 1, 1, 0]
    assert plan.dct_pool == 8 and plan.coarse_shape == (4, 8, 4, 32) and plan.out_shape == (4, 8, 4, 4)


def test_argument_errors():
    fa, _ = _core.get_factorlist((64, 64, 64))
    L = fa.shape[0]
    for bad in (1.0, "1", None, True, [1, 2.0, 0], [True, 0, 0], np.float64(1)):
        with pytest.raises(TypeError):
            pool.normalize_levels(bad, 3, L)
    for bad in (-1, L + 1, [0, 0], [0, 0, 0, 0], [0, -1, 0], [0, 0, L + 1]):
        with pytest.raises(ValueError):
            pool.normalize_levels(bad, 3, L)
    assert pool.normalize_levels(np.int32(2), 3, L).tolist() == [2, 2, 2]
    assert pool.normalize_levels((1, 0, L), 3, L).tolist() == [1, 0, L]
    for bad in (1.0, "0", True, (0, 1.5), [0, 1]):
        with pytest.raises(TypeError):
            pool.normalize_axes(bad, 3)
    for bad in (3, -4, (0, 3)):
        with pytest.raises(np.exceptions.AxisError):
            pool.normalize_axes(bad, 3)
    with pytest.raises(ValueError):
        pool.normalize_axes((0, -3), 3)
    assert pool.normalize_axes((-1, 0), 3) == (0, 2) and pool.normalize_axes(None, 3) == (0, 1, 2)
    with pytest.raises(ValueError):
        pool.PoolPlan(fa, [1, 1, 1], "max")


def test_ndmps_errors_need_no_gpu():
    from imgcompressionmps_amd import NDMPS

    obj = NDMPS()
    for call in (lambda: obj.block_shape(1), lambda: obj.downsample(1), lambda: obj.sum(), lambda: obj.mean(0)):
        with pytest.raises(ValueError, match="shape is unknown"):
            call()
    obj._shape = (30, 45, 20)
    assert obj.block_shape(1) == (5, 3, 5) and obj.block_shape([0, 3, 1]) == (1, 45, 5)
    with pytest.raises(TypeError):
        obj.block_shape(1.5)
    with pytest.raises(ValueError):
        obj.downsample(4)
    with pytest.raises(ValueError):
        obj.downsample(1, op="max")
    with pytest.raises(np.exceptions.AxisError):
        obj.sum(axis=3)
    with pytest.raises(ValueError):
        obj.mean(axis=(1, 1))
    with pytest.raises(TypeError):
        obj.mean(axis=False)
    obj.mode = "Other"
    assert obj.downsample(1) is None and obj.sum(axis=0) is None and obj.mean() is None


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulated_dct_reduction_matches_idct(shape):
    """DCT mode: the cores hold coefficients along the last axis.  A full last-axis reduction picks digit 0 on the
    sites; a partial one is decoded in the coefficient domain and pooled with the block-summed basis."""
    cores = _random_cores(shape, seed=5)
    y = _dense_volume(shape, cores)
    x = idct(y, axis=-1, norm="ortho")
    fa, _ = _core.get_factorlist(shape)
    L, n = fa.shape[0], shape[-1]
    j, k = np.arange(n)[:, None], np.arange(n)[None, :]
    basis = np.where(k == 0, np.sqrt(1 / n), np.sqrt(2 / n)) * np.cos(np.pi * (2 * j + 1) * k / (2 * n))
    for lev in _level_cases(shape, L):
        for op in ("mean", "sum"):
            plan = pool.PoolPlan(fa, lev, op, dct=True)
            coarse = _coarse_from_plan(plan, cores, shape)
            if plan.dct_pool > 1:
                W = basis.reshape(n // plan.dct_pool, plan.dct_pool, n).sum(axis=1)
                coarse = coarse @ (W / plan.dct_pool if op == "mean" else W).T
            elif lev[-1] == 0:
                coarse = idct(coarse, axis=-1, norm="ortho")
            want = _block_reduce(x, pool.block_shape(fa, lev), op)
            assert coarse.shape == want.shape == plan.out_shape
            np.testing.assert_allclose(coarse, want, rtol=1e-9, atol=1e-10 * np.abs(x).sum(), err_msg=str((lev, op)))
