"""The DCT-mode decoders on arbitrary cores, element by element, against the fp64 reference of dct_decode_cases.py.

Objects are built as ``_random_object`` of tests/test_gpu_decode_reference.py builds them, in DCT mode: encoded from a
synthetic volume at ``max_bond=12``, then their cores replaced by drawn ones (uniform, or {-1, 0, 1}), exact in the
storage type.  Every call that transforms the last axis -- ``to_tensor``, ``to_tensors``, ``decode_region``,
``values_at``, ``decode_regions``, ``values_at_many``, ``downsample``, ``sum``, ``mean`` -- and
``ndmps_pool_dct_basis_*`` itself is held to the bars derived in dct_decode_cases.py and checked on the CPU in
test_dct_decode_cases_host.py; none of them comes from what the device returns.  The per-axis level list is also run
on the Std-mode objects of test_gpu_decode_reference.py with that file's bars.

The largest error / bar per family (to_tensor, region, series, pooled, pick, basis, std levels) is printed when the
module finishes; it is reported, never asserted against.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import dct_decode_cases as dc  # noqa: E402
from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402
from test_gpu_decode_reference import SHAPE_IDS as STD_IDS  # noqa: E402
from test_gpu_decode_reference import SHAPES as STD_SHAPES  # noqa: E402
from test_gpu_decode_reference import (_block_reduce, _ix, _random_object, _region_keys,  # noqa: E402
                                       _stored_cores)

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TORCH_DT = {"f32": F32, "bf16": BF16, "f64": F64}
NAME_OF = {F32: "f32", BF16: "bf16", F64: "f64"}
NP_RESULT = {"f32": np.float32, "bf16": np.float32, "f64": np.float64}

CASES = [(s, f, t) for s in dc.SHAPES for f in dc.FAMILIES for t in dc.STORAGES]
CASE_IDS = [f"{'x'.join(map(str, s))}-{f}-{t}" for s, f, t in CASES]
WORST = {}   # family -> largest observed error / bar (report only)
_OBJECTS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")
    yield
    _OBJECTS.clear()
    for key in sorted(WORST):
        print(f"\n[dct-decode] largest error / bar, {key}: {WORST[key]:.3e}", end="")
    print()


# ------------------------------------------------------------------------------------------------ helpers
def _dct_object(shape, family, storage, max_bond=dc.MAX_BOND, salt=0):
    """(object, case): a DCT-mode object over ``shape`` whose cores are the drawn ones of the case, stored as
    ``storage``.  The bonds are those the capped sweep leaves; the case is drawn over them."""
    key = (shape, family, storage, max_bond, salt)
    if key not in _OBJECTS:
        obj = NDMPS.from_tensor(synthetic_mri(shape, seed=17), max_bond=max_bond, mode="DCT", device=DEV,
                                dtype=F64 if storage == "f64" else None)
        assert list(obj.mps.dims) == dc.site_dims(shape)
        cs = dc.case(shape, family, storage, bonds=tuple(int(b) for b in obj.mps.bonds), salt=salt)
        arrays = obj.mps.arrays
        obj.replace_tensordata([c.reshape(tuple(arrays[i].shape)) for i, c in enumerate(cs.cores)])
        if storage == "bf16":
            obj = obj.astype(BF16)
        assert obj.mode == "DCT" and obj.mps.dtype == TORCH_DT[storage]
        for got, want in zip(_stored_cores(obj), cs.cores):
            assert np.array_equal(got, want)
        _OBJECTS[key] = (obj, cs)
    return _OBJECTS[key]


def _within(got, ref, bar, family, label):
    """|got - ref| <= bar at every element, no NaN; records error / bar under ``family``."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    bar = np.asarray(bar, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape == bar.shape, (label, got.shape, ref.shape, bar.shape)
    assert not np.isnan(got).any(), f"{label}: {int(np.isnan(got).sum())} elements are NaN"
    err = np.abs(got - ref)
    pos = bar > 0
    ratio = float(np.max(err[pos] / bar[pos])) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[dct-decode] {label}: error / bar = {ratio:.3e}")
    bad = err > bar
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} elements outside the bar, worst ratio {ratio:.3e}, "
                           f"first {np.flatnonzero(bad)[:8]}")


def _pick_family(cs, kind, ref):
    """The report's family of a pooled result: the integer chain whose every site collapses is held to one rounding
    of the result, a bar that a correct device meets with a ratio of up to 1, so it is reported on its own."""
    if kind == "pick" and cs.family == "integer" and ref.size == 1:
        return "pick, one rounding"
    return kind


def _region_key_list(shape):
    return _region_keys(shape) + dc.extra_region_keys(shape)


# ------------------------------------------------------------------------------------------------ pooled basis
def _basis_call(n, Bk, w, f64, numel=None):
    """ndmps_pool_dct_basis_* into a NaN-filled buffer with 64 guard elements behind it; returns (rc, buffer)."""
    lib = _lib.load()
    numel = (n // Bk) * n if numel is None else numel
    buf = torch.full((numel + 64,), float("nan"), dtype=F64 if f64 else F32, device=DEV)
    fn = lib.ndmps_pool_dct_basis_f64 if f64 else lib.ndmps_pool_dct_basis_f32
    rc = fn(buf.data_ptr(), n, Bk, w, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n,Bk", dc.BASIS_CASES)
def test_pooled_dct_basis_against_the_fp64_basis(n, Bk, f64):
    for w in (1.0, 1.0 / Bk):
        rc, buf = _basis_call(n, Bk, w, f64)
        assert rc == _lib.OK, _lib.load().ndmps_last_error()
        numel = (n // Bk) * n
        assert bool(torch.isnan(buf[numel:]).all()), "wrote behind the (n / Bk, n) buffer"
        _within(buf[:numel].to(F64).cpu().numpy(), dc.pooled_basis(n, Bk, w), dc.basis_bar(n, Bk, w, not f64),
                "basis f64" if f64 else "basis f32 (one rounding of the entry included)",
                f"pool_dct_basis_{'f64' if f64 else 'f32'} n={n} Bk={Bk} w={w:.4g}")
        rc, again = _basis_call(n, Bk, w, f64)
        assert rc == _lib.OK and torch.equal(buf[:numel], again[:numel]), "a second call gives other bits"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_pooled_dct_basis_refuses_bad_sizes_and_writes_nothing(f64):
    # (n, Bk); 16385 is asked with one block of the whole axis, so the buffer covers all a wrong launch could write
    for n, Bk, numel in ((20, 3, 400), (680, 7, 680 * 98), (0, 1, 64), (16385, 16385, 16385)):
        rc, buf = _basis_call(n, Bk, 1.0, f64, numel=numel)
        assert rc == _lib.EINVAL, (n, Bk, rc)
        assert bool(torch.isnan(buf).all()), f"a refused call (n={n}, Bk={Bk}) wrote into its buffer"


# ------------------------------------------------------------------------------------------------ full decode
@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_to_tensor_and_to_tensors_against_the_reference(shape, family, storage):
    objs, cases = zip(*[_dct_object(shape, family, storage, salt=s) for s in range(3)])
    got = objs[0].to_tensor()
    assert got.shape == shape and got.dtype == NP_RESULT[storage]
    _within(got, cases[0].x, cases[0].decode_bar("to_tensor"), "to_tensor", f"{cases[0].label} to_tensor")
    recs = NDMPS.to_tensors(list(objs))
    assert len(recs) == 3
    for t, (rec, cs) in enumerate(zip(recs, cases)):
        assert rec.shape == shape and rec.dtype == NP_RESULT[storage]
        _within(rec, cs.x, cs.decode_bar("to_tensor"), "to_tensor", f"{cs.label} to_tensors[{t}]")
    assert np.array_equal(recs[0], got), "to_tensors differs from to_tensor on the same object"


# ------------------------------------------------------------------------------------------------ regions, points
@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_decode_region_against_the_reference(shape, family, storage):
    obj, cs = _dct_object(shape, family, storage)
    full = obj.to_tensor()
    bar = cs.decode_bar("wide")
    for key in _region_key_list(shape):
        want = _ix(cs.x, key, shape)
        like = _ix(full, key, shape)
        got = obj.decode_region(key)
        assert np.shape(got) == like.shape == want.shape, (key, np.shape(got), like.shape)
        assert np.asarray(got).dtype == full.dtype, (key, np.asarray(got).dtype)
        if want.ndim == 0:
            assert isinstance(got, np.generic), key  # all-int keys give a NumPy scalar, as to_tensor()[i, j, k]
        _within(got, want, _ix(bar, key, shape), "region", f"{cs.label} decode_region {key!r:.40}")


@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_values_at_against_the_reference(shape, family, storage):
    obj, cs = _dct_object(shape, family, storage)
    bar = cs.decode_bar("wide")
    for name, pts in (("500 points", dc.points(shape)), ("one row", dc.points_one_row(shape))):
        got = obj.values_at(pts)
        assert got.shape == (pts.shape[0],) and got.dtype == NP_RESULT[storage]
        _within(got, cs.x[tuple(pts.T)], bar[tuple(pts.T)], "region", f"{cs.label} values_at {name}")
        if name == "500 points":
            assert got[0] == got[1]  # two equal points


# ------------------------------------------------------------------------------------------------ series
SERIES_BONDS = (12, 7, 9)


def _check_series(frames, call, singles, label):
    """``frames``: [(object, case)]; ``call``: the bar every frame is held to; ``singles``: the objects whose own
    decode_region / values_at every frame must reproduce bit for bit."""
    objs = [o for o, _ in frames]
    shape = frames[0][1].shape
    for key in [(), (slice(None, None, 3),) * len(shape)] + dc.extra_region_keys(shape):
        got = NDMPS.decode_regions(objs, key)
        for t, ((_, cs), single) in enumerate(zip(frames, singles)):
            _within(got[t], _ix(cs.x, key, shape), _ix(cs.decode_bar(call), key, shape), "series",
                    f"{label} decode_regions[{t}] {key!r:.40}")
            own = single.decode_region(key)
            assert got[t].dtype == own.dtype and np.array_equal(got[t], own), (key, t)
    pts = dc.points(shape)
    got = NDMPS.values_at_many(objs, pts)
    assert got.shape == (len(objs), pts.shape[0])
    for t, ((_, cs), single) in enumerate(zip(frames, singles)):
        _within(got[t], cs.x[tuple(pts.T)], cs.decode_bar(call)[tuple(pts.T)], "series", f"{label} values_at_many[{t}]")
        own = single.values_at(pts)
        assert got[t].dtype == own.dtype and np.array_equal(got[t], own), t


@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_series_of_one_storage_type_against_each_frames_reference(shape, family, storage):
    frames = [_dct_object(shape, family, storage, max_bond=mb, salt=10 + t) for t, mb in enumerate(SERIES_BONDS)]
    assert len({tuple(o.mps.bonds) for o, _ in frames}) == len(frames), "the frames were to differ in their bonds"
    _check_series(frames, "wide", [o for o, _ in frames], f"{frames[0][1].label} series")


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=dc.SHAPE_IDS)
def test_series_of_mixed_storage_types_is_contracted_in_fp64(shape, family):
    frames = [_dct_object(shape, family, st, max_bond=mb, salt=10 + t)
              for t, (st, mb) in enumerate(zip(("f32", "bf16", "f64"), SERIES_BONDS))]
    # an fp64 frame makes the call contract and transform every frame in fp64, the other cores widened exactly
    _check_series(frames, "f64", [o.astype(F64) for o, _ in frames], f"{'x'.join(map(str, shape))}/{family}/mixed series")


# ------------------------------------------------------------------------------------------------ pooled
@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_downsample_against_the_reference(shape, family, storage):
    obj, cs = _dct_object(shape, family, storage)
    for lev in dc.level_list(shape):
        for op in ("mean", "sum"):
            kind, ref, bar = dc.pooled(cs, lev, op)
            got = obj.downsample(lev, op=op)
            assert got.shape == ref.shape and got.dtype == NP_RESULT[storage], (lev, op, got.shape, ref.shape)
            _within(got, ref, bar, _pick_family(cs, kind, ref), f"{cs.label} downsample({lev}, {op})")
            if kind == "pick" and family == "integer" and ref.size > 1:
                # beside kept axes every site's core is weighted by sqrt(f) or 1 / sqrt(f) and rounded, so the result
                # is more than one rounding away from the exact one: how far is reported, not asserted
                one = dc.U[dc.work_of(storage)] * np.abs(ref)
                r = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)[one > 0] / one[one > 0]))
                WORST["pick beside kept axes, integer cores, error / one rounding"] = max(
                    WORST.get("pick beside kept axes, integer cores, error / one rounding", 0.0), r)


@pytest.mark.parametrize("shape,family,storage", CASES, ids=CASE_IDS)
def test_sum_and_mean_against_the_reference(shape, family, storage):
    obj, cs = _dct_object(shape, family, storage)
    for axis in dc.axis_list(shape):
        for op in ("sum", "mean"):
            kind, ref, bar = dc.pooled(cs, dc.axis_levels(shape, axis), op)
            want = getattr(cs.x, op)(axis=axis)
            assert np.allclose(ref.reshape(want.shape), want, rtol=0, atol=1e-13 * np.abs(cs.x).sum())  # same reduction
            for keepdims in (False, True):
                got = getattr(obj, op)(axis=axis, keepdims=keepdims)
                assert np.shape(got) == np.shape(getattr(cs.x, op)(axis=axis, keepdims=keepdims)), (axis, keepdims)
                assert np.asarray(got).dtype == NP_RESULT[storage]
                _within(got, ref, bar, _pick_family(cs, kind, ref), f"{cs.label} {op}(axis={axis}, keepdims={keepdims})")


# ------------------------------------------------------------------------------------------------ Std mode, per axis
@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("sweep_from", ["right", "left"])
@pytest.mark.parametrize("shape", STD_SHAPES, ids=STD_IDS)
def test_std_mode_per_axis_levels_on_random_cores(shape, sweep_from, storage):
    obj = _random_object(shape, storage, sweep_from, seed=17)
    assert obj.mode == "Std"
    cores = _stored_cores(obj)
    dest = im.flat_destination(shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores), dest).reshape(shape)
    # pool widens bf16 cores to fp32 and contracts in fp32 (test_gpu_decode_reference.py: _check_derived)
    wide = cb.CHAIN_ROUNDOFF["f64" if storage == F64 else "f32"]
    wide_b = cb.to_volume(cb.chain_bound(cores, *wide), dest).reshape(shape)
    for lev in dc.level_list(shape):
        blocks = obj.block_shape(lev)
        assert blocks == dc.block_shape(shape, dc.normalize_levels(shape, lev))
        for op in ("mean", "sum"):
            got = obj.downsample(lev, op=op)
            want = _block_reduce(ref, blocks, op)
            assert got.shape == want.shape
            _within(got, want, _block_reduce(wide_b, blocks, op), "std levels",
                    f"Std {shape} {sweep_from} {NAME_OF[storage]} downsample({lev}, {op})")
