"""Statistics per label from the cores (LabelEpi in csrc/labelstat.hip, core/labelstat.py), on the GPU, against NumPy on
the fp64 contraction of oracle/mps.py through the bars of tests/labelstat_cases.py (which tests/test_labelstat_host.py
shows to accept the reference and to reject labels read in site order, a tile left out, padding counted, a run never
flushed, folded windows, NaN counted and outside voxels added to a label).

Integer cores: every number must equal NumPy's on the reference, bit for bit.  Real cores: the sandwich bar, every
figure printed before it is asserted.  The chains of oracle/chain_cases.py go through core/labelstat.py with the plan
of ``cc.factor_array``; the methods of NDMPS, which are thin over the same functions, are tested on encoded volumes at
the end.
"""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import labelstat_cases as lc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import labelstat as ls  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import chain_cases as cc  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
ARRAYS = ("count", "n_nan", "sum", "sumsq", "min", "max", "mean", "std")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _chain(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def _plan(c):
    return _plan_for(c.shape, 0, factor_arr=c.fa)


def _check_shape_of_result(got, n_labels):
    assert set(got) == set(ARRAYS) | {"outside", "s", "s2"}
    for key in ARRAYS:
        assert got[key].shape == (n_labels,) and got[key].dtype == (np.int64 if key in ("count", "n_nan") else np.float64), key
    assert all(isinstance(got[key], int) for key in ("outside", "s", "s2"))


def _check_derived(got):
    """mean and std are the stated functions of sum, sumsq and count."""
    filled = got["count"] > 0
    n = got["count"][filled]
    mean = got["sum"][filled] / n
    assert lc.same_bits(got["mean"][filled], mean)
    assert lc.same_bits(got["std"][filled], np.sqrt(np.maximum(got["sumsq"][filled] / n - mean * mean, 0.0)))
    for key in ("mean", "std", "min", "max"):
        assert np.all(np.isnan(got[key][~filled])), key
    assert np.all(got["sum"][~filled] == 0) and np.all(got["sumsq"][~filled] == 0)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_integer_cores_give_numpy_s_numbers_exactly(name, storage):
    c = vc.case(name, "integer", storage)
    chain, plan = _chain(c.cores, storage), _plan(c)
    whole = vs.value_stats(chain)
    want_scales = ls.scales(max(abs(whole["min"]), abs(whole["max"])), c.n)
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        volume = lab.reshape(c.shape)
        got = ls.label_stats(chain, plan, volume.astype(np.int32), n_labels)
        print(f"[labelstat] {name}/{storage} {kind}: L {n_labels}, outside {got['outside']}, s {got['s']}, s2 {got['s2']}, "
              f"count {got['count'][:4]}, sum {got['sum'][:4]}, min {got['min'][:4]}, max {got['max'][:4]}")
        _check_shape_of_result(got, n_labels)
        lc.exact_stats(got, c.ref, lab, n_labels)
        _check_derived(got)
        assert (got["s"], got["s2"]) == want_scales == lc.ref_scales(c.ref)
        assert int(got["count"].sum() + got["n_nan"].sum()) + got["outside"] == c.n
        if kind == "one":
            for key in ("min", "max", "sum", "sumsq"):
                assert got[key][0] == whole[key], key
            assert got["count"][0] == whole["count"] - whole["n_nan"] == c.n
        assert lc.same_dict(ls.label_stats(chain, plan, volume.astype(np.int32), n_labels), got), "two calls differ"
        # every label type, and a device tensor, give the same dict
        types = [np.int16, np.int64] + ([np.uint8] if lab.min() >= 0 and lab.max() < 256 else []) + \
                ([np.bool_] if n_labels <= 2 and lab.min() >= 0 else [])
        for dtype in types:
            assert lc.same_dict(ls.label_stats(chain, plan, volume.astype(dtype), n_labels), got), dtype
        for dtype in (torch.int32, torch.int64):
            on_device = torch.from_numpy(volume).to(DEV).to(dtype)
            assert lc.same_dict(ls.label_stats(chain, plan, on_device, n_labels), got), dtype
        if kind in ("blocks", "one"):  # n_labels from the labels
            assert lc.same_dict(ls.label_stats(chain, plan, volume), got)


def test_two_labels_as_bool():
    c = vc.case("int_wide", "integer", "f32")
    chain, plan = _chain(c.cores, "f32"), _plan(c)
    mask = (np.arange(c.n) % 3 == 1).reshape(c.shape)
    got = ls.label_stats(chain, plan, mask)
    lc.exact_stats(got, c.ref, mask.reshape(-1).astype(np.int64), 2)
    for other in (mask.astype(np.uint8), mask.astype(np.int64), torch.from_numpy(mask).to(DEV)):
        assert lc.same_dict(ls.label_stats(chain, plan, other), got)


# ------------------------------------------------------------------------------------------------ NaN, infinity
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_voxels_are_counted_per_label(name, storage):
    c = vc.case(name, "integer", storage)
    cores, ref = vc.with_nan(c)
    chain, plan = _chain(cores, storage), _plan(c)
    nan = np.isnan(ref)
    assert 0 < nan.sum() < c.n
    for kind in ("blocks", "scatter"):
        lab, n_labels = lc.labels(c, kind)
        got = ls.label_stats(chain, plan, lab.reshape(c.shape), n_labels)
        print(f"[labelstat] {name}/{storage} {kind} with NaN: n_nan {got['n_nan']}, count {got['count']}")
        lc.exact_stats(got, ref, lab, n_labels)
        assert np.array_equal(got["n_nan"], np.bincount(lab[nan], minlength=n_labels)) and got["n_nan"].sum() == nan.sum()
        _check_derived(got)
    # a label whose voxels are all NaN
    lab, _ = lc.labels(c, "blocks")
    lab = np.where(nan, 7, lab)
    got = ls.label_stats(chain, plan, lab.reshape(c.shape), 8)
    lc.exact_stats(got, ref, lab, 8)
    assert got["count"][7] == 0 and got["n_nan"][7] == nan.sum() and np.isnan(got["min"][7]) and np.isnan(got["max"][7])
    assert got["sum"][7] == 0 and got["sumsq"][7] == 0 and np.isnan(got["mean"][7])


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_an_infinite_voxel_is_refused_and_the_next_call_runs(storage):
    # bonds of 1 and no zero entry: a voxel is a product of six numbers, so the infinite entry gives infinite voxels
    # (behind a sum, inf - inf or inf * 0 would give NaN, which is counted and not refused)
    c = vc.case("L6_bonds_one", "uniform", storage)
    cores = [x.copy() for x in c.cores]
    cores[0][0, 1, 0] = np.inf
    dense = mps_to_dense(cores)
    assert np.isinf(dense).sum() == c.n // 4 and not np.isnan(dense).any()
    plan = _plan(c)
    lab, n_labels = lc.labels(c, "blocks")
    with pytest.raises(ValueError, match="finite voxels"):
        ls.label_stats(_chain(cores, storage), plan, lab.reshape(c.shape), n_labels)
    got = ls.label_stats(_chain(c.cores, storage), plan, lab.reshape(c.shape), n_labels)
    lc.sandwich_stats(got, c.ref, c.bound, lab, n_labels)


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_real_cores_within_the_sandwich(name, family, storage):
    c = vc.case(name, family, storage)
    chain, plan = _chain(c.cores, storage), _plan(c)
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(c, kind)
        got = ls.label_stats(chain, plan, lab.reshape(c.shape), n_labels)
        show = lambda *figures: print(f"[labelstat] {name}/{family}/{storage} {kind}:", *figures)  # noqa: E731
        show("s", got["s"], "s2", got["s2"])
        lc.sandwich_stats(got, c.ref, c.bound, lab, n_labels, show)
        _check_derived(got)
        whole = vs.value_stats(chain)
        assert (got["s"], got["s2"]) == ls.scales(max(abs(whole["min"]), abs(whole["max"])), c.n)
        assert lc.same_dict(ls.label_stats(chain, plan, lab.reshape(c.shape), n_labels), got), "two calls differ"


# ------------------------------------------------------------------------------------------------ series
SERIES_DIMS = cc.INTEGER_CHAINS["int_wide"][0]
SERIES = [([1, 8, 16, 10, 1], "f32"), ([1, 4, 8, 5, 1], "f32"), ([1, 2, 3, 2, 1], "f64"), ([1, 8, 12, 7, 1], "f32")]


def test_series_rows_equal_the_single_calls_and_upload_once():
    c = vc.case("int_wide", "integer", "f32")  # the shape, the plan and the index map of the frames
    plan = _plan(c)
    frames, refs = [], []
    for t, (bonds, storage) in enumerate(SERIES):
        cc.check_chain(SERIES_DIMS, bonds)
        cores = cc.draw_cores(f"labelstat_series_{t}", SERIES_DIMS, bonds, "integer", storage)
        frames.append(_chain(cores, storage))
        refs.append(cb.to_volume(mps_to_dense(cores).reshape(-1), c.dest))
    for kind in ("scatter", "window"):
        lab, n_labels = lc.labels(c, kind)
        volume = torch.from_numpy(lab.reshape(c.shape)).to(DEV).to(torch.int16)
        ls.label_stats(frames[0], plan, volume, n_labels)  # the plan's tables are built on first use and kept
        n_cols = vs._split_columns(frames[0])
        tables = [t.data_ptr() for t in plan.split_tables(n_cols, torch.device(DEV))]
        uploads = ls.LABEL_UPLOADS
        many = ls.label_stats_many(frames, plan, volume, n_labels)
        assert ls.LABEL_UPLOADS == uploads + 1, "the label volume went to the device more than once"
        assert [t.data_ptr() for t in plan.split_tables(n_cols, torch.device(DEV))] == tables
        assert set(many) == set(ARRAYS) | {"outside", "s", "s2"}
        for key in ARRAYS:
            assert many[key].shape == (len(frames), n_labels), key
        for key in ("outside", "s", "s2"):
            assert many[key].shape == (len(frames),), key
        for t, (frame, ref) in enumerate(zip(frames, refs)):
            one = ls.label_stats(frame, plan, volume, n_labels)
            row = {key: (many[key][t] if key in ARRAYS else int(many[key][t])) for key in many}
            assert lc.same_dict(row, one), t
            lc.exact_stats(one, ref, lab, n_labels)
    with pytest.raises(ValueError, match="at least one"):
        ls.label_stats_many([], plan, volume, n_labels)


# ------------------------------------------------------------------------------------------------ memory
def measure_memory():
    """Run in a fresh process (the fixture below): per storage type on the 2**21-voxel chain with 4096 labels, what
    torch.cuda.max_memory_allocated shows above the inputs (the label volume is one of them), the bytes asked of
    the allocator, and the workspace query; one JSON line."""
    out = {}
    for storage in vc.STORAGES:
        c = vc.case("int_8x7", "integer", storage)
        chain, plan = _chain(c.cores, storage), _plan(c)
        lab, n_labels = lc.labels(c, "max")
        volume = torch.from_numpy(lab.reshape(c.shape)).to(DEV).to(torch.int16)
        call = lambda: ls.label_stats(chain, plan, volume, n_labels)  # noqa: E731
        call()  # the plan's offset tables are built once and kept
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        asked_before = torch.cuda.memory_stats()["requested_bytes.all.current"]
        got = call()
        torch.cuda.synchronize()
        out[storage] = dict(above=int(torch.cuda.max_memory_allocated() - before),
                            asked=int(torch.cuda.memory_stats()["requested_bytes.all.peak"] - asked_before),
                            ws=ls.workspace_bytes(chain, n_labels), volume=c.n * (8 if storage == "f64" else 4),
                            voxels=int(got["count"].sum()))
        del chain, plan, volume, call
    print("MEMORY " + json.dumps(out))


@pytest.fixture(scope="module")
def memory_figures():
    """measure_memory() in one fresh child process for both storage types (this test is about a process's allocator)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(tests)!r}, {tests!r}]; "
            "import test_gpu_labelstat as t; t.measure_memory()")
    flags = ["-s"] if sys.flags.no_user_site else []
    run = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("MEMORY ")]
    assert len(line) == 1, run.stdout[-2000:]
    return json.loads(line[0][len("MEMORY "):])


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_device_memory_is_the_workspace_not_the_volume(memory_figures, storage):
    f = memory_figures[storage]
    print(f"[labelstat] int_8x7/{storage} 4096 labels: {f['above']} bytes held and {f['asked']} bytes asked for above the "
          f"inputs, workspace {f['ws']}, volume {f['volume']}")
    assert f["voxels"] == 2 ** 21
    assert f["above"] <= f["ws"] + 64 * 1024
    assert f["asked"] <= f["ws"] + 64 * 1024
    assert f["ws"] < f["volume"] // 4


# ------------------------------------------------------------------------------------------------ through the class
@pytest.fixture(scope="module")
def encoded():
    x = synthetic_mri((32, 48, 40), seed=7)
    return x, {
        "f32": NDMPS.from_tensor(x, max_bond=12, device=DEV),
        "f64": NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=torch.float64),
    }


def _atlas(shape):
    """Eight octants, a central ball (label 8) and -1 on one face."""
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    atlas = sum(((g >= n // 2).astype(np.int64) << a) for a, (g, n) in enumerate(zip(grid, shape)))
    r2 = sum(((g - (n - 1) / 2) / (n / 4)) ** 2 for g, n in zip(grid, shape))
    atlas[r2 <= 1.0] = 8
    atlas[0] = -1
    return atlas


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_methods_on_an_encoded_volume_within_the_sandwich(encoded, storage):
    x, objs = encoded
    obj = objs[storage]
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(x.shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), dest)
    bound = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest)
    atlas = _atlas(x.shape)
    lab = atlas.reshape(-1)
    assert set(np.unique(lab)) == set(range(-1, 9))
    got = obj.label_stats(atlas)
    show = lambda *figures: print(f"[labelstat] class/{storage}:", *figures)  # noqa: E731
    _check_shape_of_result(got, 9)
    lc.sandwich_stats(got, ref, bound, lab, 9, show)
    _check_derived(got)
    assert got["outside"] == x.shape[1] * x.shape[2]
    assert lc.same_dict(obj.label_stats(atlas, 9), got) and lc.same_dict(obj.label_stats(torch.from_numpy(atlas).to(DEV)), got)
    wider = obj.label_stats(atlas, n_labels=12)
    assert np.array_equal(wider["count"][:9], got["count"]) and np.all(wider["count"][9:] == 0)
    fewer = obj.label_stats(atlas, n_labels=8)  # the ball falls outside
    assert fewer["outside"] == got["outside"] + got["count"][8]


def test_series_through_the_class(encoded):
    x, objs = encoded
    atlas = _atlas(x.shape)
    frames = [objs["f32"], objs["f64"], objs["f32"]]
    many = NDMPS.label_stats_many(frames, atlas)
    assert many["mean"].shape == (3, 9) and many["s"].shape == (3,)
    for t, obj in enumerate(frames):
        one = obj.label_stats(atlas)
        assert lc.same_dict({k: (many[k][t] if k in ARRAYS else int(many[k][t])) for k in many}, one), t


def test_refusals(encoded):
    x, objs = encoded
    obj = objs["f32"]
    atlas = _atlas(x.shape)
    for call in (lambda o: o.label_stats(atlas), lambda o: NDMPS.label_stats_many([o], atlas)):
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(obj.astype(torch.bfloat16))
        unknown = NDMPS.from_tensor(x, max_bond=4, device=DEV)
        unknown._shape = None
        with pytest.raises(ValueError, match="shape is unknown"):
            call(unknown)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        obj.label_stats(atlas, 4097)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        NDMPS.label_stats_many([obj], atlas, 4097)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        obj.label_stats(atlas * 1000)
    other = NDMPS.from_tensor(synthetic_mri((32, 48, 20), seed=7), max_bond=4, device=DEV)
    with pytest.raises(ValueError, match="shape"):
        NDMPS.label_stats_many([obj, other], atlas)
    with pytest.raises(ValueError, match="shape"):
        obj.label_stats(atlas[:-1])
    with pytest.raises(TypeError, match="integers"):
        obj.label_stats(atlas.astype(np.float32))
    with pytest.raises(TypeError):
        NDMPS.label_stats_many([obj, "frame"], atlas)
    with pytest.raises(ValueError):
        NDMPS.label_stats_many([], atlas)
    assert obj.astype(torch.bfloat16).astype(torch.float32).label_stats(atlas)["count"].sum() == x.size - x.shape[1] * x.shape[2]
