"""NDMPS.decode_regions / NDMPS.values_at_many on the MI355X (series kernels of csrc/region.hip, core/region.py
plan_series): one region of every frame of a series in one call.

The yardstick in Std mode is the loop over ``decode_region`` / ``values_at`` on the same objects, bit for bit: both
kernel families run one tile body.  Ragged random-core frames are also held, element by element, to
``oracle.chain_bound`` around the fp64 contraction of their stored cores, with the round-off pair of
tests/test_gpu_decode_reference.py for region decode (bf16 cores are widened and contracted in fp32).  DCT mode uses
the relative-Frobenius bars of tests/test_gpu_region.py, 1e-5 (fp32) and 1e-12 (fp64).

The ragged frames live on (64, 64, 64) (L = 6, d = 8, caps 8-64-70-64-8): 3-3-3-3-3 leaves whole 32-column blocks
idle, 8-33-33-33-8 and 8-40-40-40-8 have a partial second block and k tails off the 32-wide (fp32) load batch,
8-64-70-64-8 a partial third block.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import readout, region  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import chain_cases as cc  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAME_OF = {F32: "f32", BF16: "bf16", F64: "f64"}
STORAGES = [F32, F64, BF16]
STORAGE_IDS = ["f32", "f64", "bf16"]
CUBE = (64, 64, 64)
PROFILES = [[3, 3, 3, 3, 3], [8, 33, 33, 33, 8], [8, 40, 40, 40, 8], [8, 64, 70, 64, 8]]
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


# ------------------------------------------------------------------------------------------------ helpers
def _keys(shape):
    """The key list of tests/test_gpu_region.py: unsorted arrays with repeats, negative ints, steps, Ellipsis, levels
    with more than 32 rows on one physical index (the full slices) and with fewer (the int and 9-entry keys)."""
    rng = np.random.default_rng(len(shape))
    D = len(shape)
    arr = [[int(v) for v in rng.integers(0, n, 7)] + [0, 0] for n in shape]  # unsorted, with repeats
    return [
        (),
        (Ellipsis,),
        (slice(5, min(37, shape[0])),),
        (slice(None, None, 3),) * D,
        (slice(None, None, -2),) + (1,) * (D - 1),
        tuple(arr),
        tuple(-1 - i for i in range(D)),
        (Ellipsis, np.array(arr[-1])),
        (arr[0], Ellipsis, -3),
        (3, slice(2, None, 5)) + (slice(None, 4),) * (D - 2),
    ]


def _points(shape, n=500):
    rng = np.random.default_rng(5)
    coords = np.stack([rng.integers(-m, m, n) for m in shape], axis=1)  # negative indices included
    coords[7] = coords[3]
    return coords


def _ix(a, key, shape):
    """a[np.ix_(per-axis indices)] with int axes dropped: the outer-indexing meaning of `key`."""
    key = key if isinstance(key, tuple) else (key,)
    if any(k is Ellipsis for k in key):
        i = next(j for j, k in enumerate(key) if k is Ellipsis)
        key = key[:i] + (slice(None),) * (len(shape) - len(key) + 1) + key[i + 1:]
    key = key + (slice(None),) * (len(shape) - len(key))
    idx, out_shape = [], []
    for k, n in zip(key, shape):
        if isinstance(k, (int, np.integer)):
            idx.append(np.array([k % n]))
        elif isinstance(k, slice):
            idx.append(np.arange(*k.indices(n)))
            out_shape.append(idx[-1].size)
        else:
            idx.append(np.asarray(k) % n)
            out_shape.append(idx[-1].size)
    return a[np.ix_(*idx)].reshape(out_shape)


def _encoded(shape, storage, bonds, mode="Std", sweep_from="right"):
    """One encoded frame per entry of `bonds` (max_bond), from different volumes."""
    out = []
    for t, mb in enumerate(bonds):
        obj = NDMPS.from_tensor(synthetic_mri(shape, seed=50 + t), mode=mode, max_bond=mb, device=DEV,
                                dtype=F64 if storage == F64 else None, sweep_from=sweep_from)
        out.append(obj.astype(BF16) if storage == BF16 else obj)
    return out


_BASE = {}


def _ragged(storage, profiles=PROFILES, tag="series"):
    """Frames over CUBE with random cores (oracle.chain_cases.draw_cores, exact in `storage`) of the given inner-bond
    profiles; returns (objects, their fp64 host cores)."""
    if "cube" not in _BASE:
        _BASE["cube"] = NDMPS.from_tensor(synthetic_mri(CUBE, seed=50), max_bond=4, device=DEV)
    base = _BASE["cube"]
    dims = base.mps.dims
    assert dims == [8] * 6
    objs, hosts = [], []
    for t, prof in enumerate(profiles):
        cores = cc.draw_cores(tag, dims, [1] + prof + [1], "uniform", NAME_OF[storage], salt=t)
        obj = base._like([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(storage).contiguous() for c in cores])
        assert obj.bond_sizes() == prof  # the case is not hollowed out by a lower rank
        for got, want in zip(obj.mps.cores, cores):
            assert np.array_equal(got.to(F64).cpu().numpy(), want)
        objs.append(obj)
        hosts.append(cores)
    return objs, hosts


def _series(kind, storage):
    if kind == "ragged":
        return CUBE, _ragged(storage)[0]
    if kind == "left":
        return (30, 45, 20), _encoded((30, 45, 20), storage, [12, 5, 9], sweep_from="left")
    shape = (30, 45, 20)
    return shape, _encoded(shape, storage, [12] if kind == "T1" else [12, 5, 9])


def _rel(got, ref, vol):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    rms = np.linalg.norm(np.asarray(vol, dtype=np.float64)) / np.sqrt(np.asarray(vol).size)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), rms * np.sqrt(max(ref.size, 1)))


# ------------------------------------------------------------------------------------------------ 1. the loop
@pytest.mark.parametrize("storage", STORAGES, ids=STORAGE_IDS)
@pytest.mark.parametrize("kind", ["T1", "T3", "ragged", "left"])
def test_series_equals_the_loop_bit_for_bit(kind, storage):
    shape, objs = _series(kind, storage)
    T = len(objs)
    for key in _keys(shape):
        got = NDMPS.decode_regions(objs, key, as_torch=True)
        for t, o in enumerate(objs):
            want = o.decode_region(key, as_torch=True)
            assert got.dtype == want.dtype and tuple(got.shape) == (T,) + tuple(want.shape), (key, got.shape)
            assert torch.equal(got[t], want), (key, t)
        host = NDMPS.decode_regions(objs, key)
        want = np.asarray(objs[-1].decode_region(key))
        assert host.dtype == want.dtype and host.shape == (T,) + want.shape and np.array_equal(host[-1], want), key
    coords = _points(shape)
    got = NDMPS.values_at_many(objs, coords, as_torch=True)
    assert tuple(got.shape) == (T, 500) and got.is_cuda
    for t, o in enumerate(objs):
        want = o.values_at(coords, as_torch=True)
        assert got.dtype == want.dtype and torch.equal(got[t], want), t
    host = NDMPS.values_at_many(objs, coords)
    assert host.dtype == objs[0].values_at(coords).dtype and np.array_equal(host[0], objs[0].values_at(coords))
    half = NDMPS.decode_regions(objs, (3,), as_torch=True, dtype=torch.float16)
    assert half.dtype == torch.float16 and tuple(half.shape) == (T,) + shape[1:]


# ------------------------------------------------------------------------------------------------ 2. fp64 contraction
@pytest.mark.parametrize("storage", STORAGES, ids=STORAGE_IDS)
def test_ragged_series_within_the_chain_bound_of_the_fp64_contraction(storage):
    objs, hosts = _ragged(storage)
    dest = im.flat_destination(CUBE).reshape(-1)
    wide = cb.CHAIN_ROUNDOFF["f64" if storage == F64 else "f32"]  # bf16 cores are widened and contracted in fp32
    refs = [cb.to_volume(mps_to_dense(c), dest).reshape(CUBE) for c in hosts]
    bounds = [cb.to_volume(cb.chain_bound(c, *wide), dest).reshape(CUBE) for c in hosts]
    coords = _points(CUBE)
    cases = [(repr(key)[:40], NDMPS.decode_regions(objs, key), lambda v, key=key: _ix(v, key, CUBE))
             for key in _keys(CUBE)]
    cases.append(("values_at_many", NDMPS.values_at_many(objs, coords), lambda v: v[tuple(coords.T)]))
    worst = 0.0
    for label, got, pick in cases:
        for t in range(len(objs)):
            want, bound = pick(refs[t]), pick(bounds[t])
            g = np.asarray(got[t], dtype=np.float64)
            assert g.shape == want.shape, (label, t, g.shape, want.shape)
            assert not np.isnan(g).any(), (label, t)
            err = np.abs(g - want)
            pos = bound > 0
            ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
            worst = max(worst, ratio)
            bad = err > bound
            assert not bad.any(), f"{label} frame {t}: {int(bad.sum())} of {bad.size} elements outside the bound, " \
                                  f"worst ratio {ratio:.3e}"
    print(f"[region-series] {NAME_OF[storage]}: largest error / bound = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 3. mixed storage
def test_fp32_and_bf16_frames_are_contracted_in_fp32():
    shape = (30, 45, 20)
    a, b = _encoded(shape, F32, [12, 7])
    objs = [a, b.astype(BF16), a.astype(BF16)]
    coords = _points(shape)
    for key in _keys(shape):
        got = NDMPS.decode_regions(objs, key, as_torch=True)
        assert got.dtype == F32
        for t, o in enumerate(objs):
            assert torch.equal(got[t], o.decode_region(key, as_torch=True, dtype=F32)), (key, t)
    got = NDMPS.values_at_many(objs, coords)
    assert got.dtype == np.float32
    for t, o in enumerate(objs):
        assert np.array_equal(got[t], o.values_at(coords)), t


def test_fp32_and_fp64_frames_are_contracted_in_fp64():
    shape = (30, 45, 20)
    a = _encoded(shape, F32, [12])[0]
    b = _encoded(shape, F64, [7])[0]
    objs = [a, b, a.astype(BF16)]
    wide = [o.astype(F64) for o in objs]
    coords = _points(shape)
    for key in _keys(shape):
        got = NDMPS.decode_regions(objs, key, as_torch=True)
        assert got.dtype == F64
        for t, w in enumerate(wide):
            assert torch.equal(got[t], w.decode_region(key, as_torch=True)), (key, t)
    got = NDMPS.values_at_many(objs, coords)
    assert got.dtype == np.float64
    for t, w in enumerate(wide):
        assert np.array_equal(got[t], w.values_at(coords)), t


# ------------------------------------------------------------------------------------------------ 4. DCT mode
@pytest.mark.parametrize("storage,tol", [(F32, 1e-5), (F64, 1e-12)], ids=["f32", "f64"])
def test_dct_series_matches_each_frames_own_decode(storage, tol):
    shape = (16, 16, 8, 32)
    objs = _encoded(shape, storage, [12, 5, 9], mode="DCT")
    T = len(objs)
    vols = [o.to_tensor() for o in objs]
    for key in _keys(shape):
        got = NDMPS.decode_regions(objs, key)
        got_t = NDMPS.decode_regions(objs, key, as_torch=True)
        for t, o in enumerate(objs):
            want = np.asarray(o.decode_region(key))
            want_t = o.decode_region(key, as_torch=True)
            assert got.dtype == want.dtype and got.shape == (T,) + want.shape, (key, got.shape)
            assert got_t.dtype == want_t.dtype and tuple(got_t.shape) == (T,) + tuple(want_t.shape) and got_t.is_cuda
            assert _rel(got[t], want, vols[t]) <= tol, (key, t)
            assert _rel(got_t[t].cpu().numpy(), want, vols[t]) <= tol, (key, t)
    coords = _points(shape)
    got = NDMPS.values_at_many(objs, coords)
    got_t = NDMPS.values_at_many(objs, coords, as_torch=True)
    for t, o in enumerate(objs):
        want = o.values_at(coords)
        assert got.dtype == want.dtype and got.shape == (T, 500) and tuple(got_t.shape) == (T, 500)
        assert got_t.dtype == o.values_at(coords, as_torch=True).dtype
        assert _rel(got[t], want, vols[t]) <= tol and _rel(got_t[t].cpu().numpy(), want, vols[t]) <= tol, t


# ------------------------------------------------------------------------------------------------ 5. chunking
def test_chunked_series_equals_the_unchunked_one(monkeypatch):
    objs, _ = _ragged(F32, PROFILES + [[8, 33, 33, 33, 8]], tag="chunks")
    bonds = [o.mps.bonds for o in objs]
    coords = _points(CUBE)
    key = (slice(5, 37),)
    whole = NDMPS.decode_regions(objs, key, as_torch=True)
    whole_pts = NDMPS.values_at_many(objs, coords, as_torch=True)
    for plan, run, ref in [
        (region.plan_outer(CUBE, region.normalize_key(key, CUBE)[0]),
         lambda: NDMPS.decode_regions(objs, key, as_torch=True), whole),
        (region.plan_points(CUBE, region.normalize_points(coords, CUBE)),
         lambda: NDMPS.values_at_many(objs, coords, as_torch=True), whole_pts),
    ]:
        lay = region.plan_series(bonds, plan, 4)
        assert lay.chunks == [(0, 5)]
        with monkeypatch.context() as m:
            m.setattr(region, "SERIES_WS_BYTES", 4 * lay.frame_stride * 4 + 512)  # both buffers of two frames
            assert region.plan_series(bonds, plan, 4).chunks == [(0, 2), (2, 4), (4, 5)]
            assert torch.equal(run(), ref)


# ------------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("storage", STORAGES, ids=STORAGE_IDS)
@pytest.mark.parametrize("shape", [(5,), (6, 4)], ids=["L1", "L2"])
def test_short_chains(shape, storage):
    objs = _encoded(shape, storage, [4, 2, 3])
    assert len(objs[0].mps.cores) == len(shape)
    keys = [(), (Ellipsis,), (-1,), ([4, 0, 0, 2],), (slice(None, None, -2),)]
    if len(shape) == 2:
        keys += [(2, slice(1, None)), ([5, 0, 5], [3, 3, 1]), (-6, -4)]
    for key in keys:
        got = NDMPS.decode_regions(objs, key, as_torch=True)
        for t, o in enumerate(objs):
            assert torch.equal(got[t], o.decode_region(key, as_torch=True)), (key, t)
    coords = _points(shape, 40)
    got = NDMPS.values_at_many(objs, coords, as_torch=True)
    for t, o in enumerate(objs):
        assert torch.equal(got[t], o.values_at(coords, as_torch=True)), t


def test_empty_selections_and_errors_launch_nothing(monkeypatch):
    shape = (30, 45, 20)
    objs = _encoded(shape, F32, [12, 5, 9])

    def _no_launch(*a, **k):
        raise AssertionError("the series contraction was reached")

    monkeypatch.setattr(readout, "region_series_values", _no_launch)
    monkeypatch.setattr(readout, "region_values", _no_launch)
    got = NDMPS.decode_regions(objs, (slice(3, 3),))
    assert got.shape == (3, 0, 45, 20) and got.dtype == np.float32
    got = NDMPS.decode_regions(objs, (2, Ellipsis, slice(7, 7)), as_torch=True)
    assert tuple(got.shape) == (3, 45, 0) and got.is_cuda
    got = NDMPS.values_at_many(objs, np.zeros((0, 3), dtype=np.int64))
    assert got.shape == (3, 0) and got.dtype == np.float32
    assert NDMPS.values_at_many([o.astype(F64) for o in objs], np.zeros((0, 3), dtype=np.int64)).dtype == np.float64
    for key in [(30,), (0, -46), (0, 0, 0, 0), ([0, 30],), (Ellipsis, 0, Ellipsis)]:
        with pytest.raises(IndexError):
            NDMPS.decode_regions(objs, key)
    for key in [(1.0,), (True,), (np.array([True, False]),), ([0.5],), (None,), (slice(0.5, 3),)]:
        with pytest.raises(TypeError):
            NDMPS.decode_regions(objs, key)
    with pytest.raises(IndexError):
        NDMPS.values_at_many(objs, [[0, 0]])
    with pytest.raises(IndexError):
        NDMPS.values_at_many(objs, [[0, 0, 20]])
    with pytest.raises(TypeError):
        NDMPS.values_at_many(objs, np.zeros((2, 3)))
    other_shape = _encoded((30, 45, 10), F32, [5])
    other_mode = _encoded(shape, F32, [5], mode="DCT")
    for call in (lambda lst: NDMPS.decode_regions(lst, (0,)), lambda lst: NDMPS.values_at_many(lst, [[0, 0, 0]])):
        with pytest.raises(TypeError):
            call([objs[0], "frame"])
        with pytest.raises(ValueError):
            call([])
        with pytest.raises(ValueError, match="shape"):
            call(objs + other_shape)
        with pytest.raises(ValueError, match="mode"):
            call(objs + other_mode)
        bare = NDMPS(objs[0].mps, objs[0].qubit_size, None, None, objs[0].norm, None, objs[0].mode, objs[0].dim)
        with pytest.raises(ValueError, match="the tensor shape is unknown"):
            call([bare])
    for o in objs:
        o.mode = "Other"
    assert NDMPS.decode_regions(objs, (0,)) is None and NDMPS.values_at_many(objs, [[0, 0, 0]]) is None


def _c_call(objs, plan, records=None, ws_bytes=None):
    """ndmps_region_series_contract_f32 on fp32 frames with NaN-filled output (a guard row on either side) and
    workspace (a guard slab behind it).  Returns (rc, output rows with the guards, workspace as fp32, layout)."""
    lib = _lib.load()
    T, L = len(objs), len(objs[0].mps.cores)
    bonds = np.array([o.mps.bonds for o in objs], dtype=np.int64)
    ptrs = np.array([[c.data_ptr() for c in o.mps.cores] for o in objs], dtype=np.int64)
    lay = region.plan_series(bonds, plan, 4)
    assert lay.chunks == [(0, T)]
    if records is None:
        records = np.concatenate([ptrs.ravel(), bonds.ravel()])
    d_rec = torch.from_numpy(records).to(DEV)
    tables = torch.from_numpy(plan.tables()).to(DEV)
    out = torch.full((T + 2, plan.n_out), NAN, dtype=F32, device=DEV)
    ws = torch.full((lay.ws_bytes // 4 + lay.frame_stride,), NAN, dtype=F32, device=DEV)
    rc = lib.ndmps_region_series_contract_f32(
        T, L, _lib.i64_array(objs[0].mps.dims), bonds.ctypes.data_as(_lib.p_i64), _lib.i64_array(plan.nodes),
        _lib.i64_array(plan.n_tiles), tables.data_ptr(), tables.numel(), d_rec.data_ptr(), plan.n_out,
        out[1].data_ptr(), ws.data_ptr(), lay.ws_bytes if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, ws, lay


@pytest.mark.parametrize("fault", ["bond_above_cap", "bond_zero", "null_core"])
def test_a_bad_frame_record_stays_inside_its_slab(fault):
    """The device record of frame 1 is wrong (the host bonds are right, so the call is accepted): the frame must read
    nothing, leave its slabs and everybody else's memory alone and come out as zeros; its neighbours come out as from
    their own single-object calls."""
    objs, _ = _ragged(F32, [[8, 33, 33, 33, 8], [3, 3, 3, 3, 3], [8, 40, 40, 40, 8]], tag="guard")
    T, L = 3, 6
    key = (slice(5, 37),)
    plan = region.plan_outer(CUBE, region.normalize_key(key, CUBE)[0])
    bonds = np.array([o.mps.bonds for o in objs], dtype=np.int64)
    ptrs = np.array([[c.data_ptr() for c in o.mps.cores] for o in objs], dtype=np.int64)
    caps = bonds.max(axis=0)
    if fault == "bond_above_cap":
        bonds[1, 3] = caps[3] + 1
    elif fault == "bond_zero":
        bonds[1, 2] = 0
    else:
        ptrs[1, 4] = 0
    rc, out, ws, lay = _c_call(objs, plan, records=np.concatenate([ptrs.ravel(), bonds.ravel()]))
    assert rc == _lib.OK, _lib.load().ndmps_last_error()
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[T + 1]).all())  # the rows around the output
    assert bool((out[2] == 0).all()), "the bad frame is not zeros"
    for t in (0, 2):
        assert torch.equal(out[1 + t], objs[t].decode_region(key, as_torch=True).reshape(-1)), t
    half = lay.ws_bytes // 8  # elements of one ping-pong buffer
    for buf in range(2):
        slab = ws[buf * half + lay.frame_stride: buf * half + 2 * lay.frame_stride]
        assert bool(torch.isnan(slab).all()), f"the bad frame wrote into its slab of buffer {buf}"
    assert bool(torch.isnan(ws[lay.ws_bytes // 4:]).all()), "something was written behind the workspace"


def test_a_short_workspace_is_refused_and_launches_nothing():
    objs, _ = _ragged(F32, PROFILES[:2], tag="guard")
    plan = region.plan_outer(CUBE, region.normalize_key((5,), CUBE)[0])
    need = region.plan_series([o.mps.bonds for o in objs], plan, 4).ws_bytes
    rc, out, ws, _ = _c_call(objs, plan, ws_bytes=need - 1)
    assert rc == _lib.EWORKSPACE
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    rc, out, _, _ = _c_call(objs, plan)
    assert rc == _lib.OK and not bool(torch.isnan(out[1:3]).any())


# ------------------------------------------------------------------------------------------------ 7. memory
def test_series_slice_memory_follows_the_layout():
    """T = 8 slices of (64, 64, 64): the allocator's peak above the inputs stays below the helper's workspace, the
    output and the tables, plus 1 MiB (the frame records, allocator rounding)."""
    objs = _encoded(CUBE, F32, [64, 40, 33, 64, 12, 64, 20, 64])
    key = (20,)
    plan = region.plan_outer(CUBE, region.normalize_key(key, CUBE)[0])
    lay = region.plan_series([o.mps.bonds for o in objs], plan, 4)
    allowed = lay.ws_bytes + 8 * plan.n_out * 4 + plan.tables().nbytes + 2**20
    want = torch.stack([o.decode_region(key, as_torch=True) for o in objs])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = NDMPS.decode_regions(objs, key, as_torch=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"8 slices of 64^3: peak {peak / 2**20:.2f} MiB, workspace {lay.ws_bytes / 2**20:.2f} MiB, "
          f"allowed {allowed / 2**20:.2f} MiB")
    assert peak < allowed
    assert torch.equal(got, want)
