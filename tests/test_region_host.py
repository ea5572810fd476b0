"""Host planner of the region decode (core/region.py), without a GPU.

The planner's tables are run through a NumPy emulation of the level-by-level contraction that
csrc/region.hip performs, on random small fp64 cores, and compared with the full dense contraction
permuted to C order (through the materialised encoding map) and then indexed like NumPy's np.ix_.
"""
import numpy as np
import pytest

from imgcompressionmps_amd.core import region
from imgcompressionmps_amd.utils import core as _core


def _random_cores(shape, chi=6, seed=0):
    dims = _core.site_dims(shape)
    rng = np.random.default_rng(seed)
    bonds = [1]
    for i in range(1, len(dims)):
        bonds.append(int(min(chi, np.prod(dims[:i]), np.prod(dims[i:]))))
    bonds.append(1)
    return [rng.standard_normal((bonds[i], int(d), bonds[i + 1])) for i, d in enumerate(dims)]


def _dense_volume(shape, cores):
    """Full chain product in site order, then into the C-order volume through the encoding map."""
    t = np.ones((1, 1))
    for c in cores:
        t = (t @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    site = t.reshape([c.shape[1] for c in cores])
    _, enc = _core.gen_encoding_map(shape)
    return site[tuple(enc)]


def _emulate(plan, cores):
    """What the kernels compute, level by level, from the tables only (the packed int32 buffer included)."""
    tab = plan.tables()
    pos = 0
    E = np.ones((1, 1))
    for s, n in enumerate(plan.nodes):
        parent = tab[pos: pos + n]
        tiles = tab[pos + n: pos + n + 3 * plan.n_tiles[s]].reshape(-1, 3)
        pos += n + 3 * plan.n_tiles[s]
        nxt = np.full((n, cores[s].shape[2]), np.nan)
        for p, row0, cnt in tiles:
            rows = np.arange(row0, row0 + cnt)
            nxt[rows] = E[parent[rows]] @ cores[s][:, p, :]
        assert not np.isnan(nxt).any(), "a node no tile covers"
        E = nxt
    leaf_parent = tab[pos: pos + plan.n_out]
    leaf_phys = tab[pos + plan.n_out: pos + 2 * plan.n_out]
    assert pos + 2 * plan.n_out == tab.size
    return np.einsum("ek,ke->e", E[leaf_parent], cores[-1][:, leaf_phys, 0])


def _ix(shape, key):
    idx, keep = region.normalize_key(key, shape)
    return idx, keep, [n for n, k in zip((i.size for i in idx), keep) if k]


def _check_bound(plan, shape, n_region):
    dims = _core.site_dims(shape)
    for s, n in enumerate(plan.nodes):
        assert n <= min(n_region, int(np.prod(dims[: s + 1]))), (s, n, n_region)


SHAPES = [(64, 64, 64), (30, 45, 20), (512, 680), (16, 16, 8, 32)]


def _keys(shape):
    rng = np.random.default_rng(len(shape))
    D = len(shape)
    arr = [list(rng.integers(0, n, 7)) + [0, 0] for n in shape]  # unsorted, with repeats
    keys = [
        (),                                                   # the full region
        (Ellipsis,),
        (slice(5, min(37, shape[0])),),                       # unaligned slice
        (slice(None, None, 3),) * D,
        (slice(None, None, -2),) + (1,) * (D - 1),
        tuple(arr),
        tuple(-1 - i for i in range(D)),                      # all ints: 0-d
        (Ellipsis, np.array(arr[-1])),
        (arr[0], Ellipsis, -3),
        (3, slice(2, None, 5)) + (slice(None, 4),) * (D - 2),
    ]
    return keys


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_region_matches_dense_indexing(shape):
    cores = _random_cores(shape, seed=sum(shape))
    vol = _dense_volume(shape, cores)
    for key in _keys(shape):
        idx, keep, out_shape = _ix(shape, key)
        ref = vol[np.ix_(*idx)].reshape(out_shape)
        plan = region.plan_outer(shape, idx)
        got = _emulate(plan, cores).reshape(out_shape)
        assert got.shape == ref.shape
        assert np.max(np.abs(got - ref), initial=0.0) <= 1e-12 * max(1.0, np.abs(vol).max()), key
        _check_bound(plan, shape, int(np.prod([i.size for i in idx])))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_points_match_dense_indexing(shape):
    cores = _random_cores(shape, seed=7 + sum(shape))
    vol = _dense_volume(shape, cores)
    rng = np.random.default_rng(3)
    coords = np.stack([rng.integers(-n, n, 300) for n in shape], axis=1)
    coords[5] = coords[9]  # a repeated point
    pts = region.normalize_points(coords, shape)
    plan = region.plan_points(shape, pts)
    got = _emulate(plan, cores)
    assert np.max(np.abs(got - vol[tuple(coords.T)])) <= 1e-12 * max(1.0, np.abs(vol).max())
    _check_bound(plan, shape, coords.shape[0])


def test_slice_level_sizes_scale_with_the_region():
    """One axial slice of 256^3: 4^(s+1) live prefixes after site s, 65536 output elements."""
    shape = (256, 256, 256)
    idx, _ = region.normalize_key((100,), shape)
    plan = region.plan_outer(shape, idx)
    assert plan.nodes == [4 ** (s + 1) for s in range(7)]
    assert plan.n_out == 256 * 256
    assert all(t[:, 2].max() <= region.TILE_ROWS for t in plan.tiles)


def test_single_site_chain():
    """A 1-D prime length has one site: no levels, the leaves read the only core."""
    shape = (7,)
    cores = _random_cores(shape)
    assert len(cores) == 1
    vol = _dense_volume(shape, cores)
    idx, _ = region.normalize_key(([3, -1, 3],), shape)
    plan = region.plan_outer(shape, idx)
    assert plan.nodes == []
    assert np.allclose(_emulate(plan, cores), vol[[3, 6, 3]], rtol=0, atol=1e-14)


def test_key_errors():
    shape = (8, 6, 4)
    with pytest.raises(IndexError):
        region.normalize_key((8,), shape)
    with pytest.raises(IndexError):
        region.normalize_key((0, 0, -5), shape)
    with pytest.raises(IndexError):
        region.normalize_key((0, 0, 0, 0), shape)
    with pytest.raises(IndexError):
        region.normalize_key((Ellipsis, 0, Ellipsis), shape)
    with pytest.raises(IndexError):
        region.normalize_key(([0, 9],), shape)
    for bad in (True, 1.0, None, "a", np.array([True, False]), [0.5, 1.0], slice(0.0, 2), np.zeros((2, 2), int)):
        with pytest.raises(TypeError):
            region.normalize_key((bad,), shape)
    with pytest.raises(IndexError):
        region.normalize_points(np.zeros((3, 2), int), shape)
    with pytest.raises(IndexError):
        region.normalize_points([[0, 0, 4]], shape)
    with pytest.raises(TypeError):
        region.normalize_points(np.zeros((3, 3)), shape)


def test_key_normalisation_follows_numpy():
    shape = (9, 5, 7)
    vol = np.arange(np.prod(shape)).reshape(shape)
    for key in [(slice(None, None, -2),), (Ellipsis, -1), (2, Ellipsis), (slice(-3, None), [4, 0, 4]),
                (np.int64(3), slice(1, 4, 2)), (slice(1, 4, 2), slice(None), np.array([6, 1], dtype=np.uint8)),
                (-9, -5, -7)]:
        idx, keep = region.normalize_key(key, shape)
        out_shape = [i.size for i, k in zip(idx, keep) if k]
        assert np.array_equal(vol[np.ix_(*idx)].reshape(out_shape), vol[key]), key
