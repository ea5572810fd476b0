"""Pair statistics per label from the cores (LabelPairEpi in csrc/labelpair.hip, core/labelpair.py), on the GPU, against
NumPy on the fp64 contractions of oracle/mps.py through the bars of tests/labelpair_cases.py (which
tests/test_labelpair_host.py shows to accept the reference and to reject labels or the original read in site order, b's
tile shifted, a and b swapped, a tile left out, padding counted, a run never flushed, folded windows, NaN of b ignored,
outside voxels added to a label and sum_ab scaled with the wrong exponent).

Integer cores: every number must equal NumPy's on the references, bit for bit.  Real cores: the sandwich bar, every
figure printed before it is asserted.  The chains of tests/pairstat_cases.py go through core/labelpair.py with the plan
of ``cc.factor_array``; the methods of NDMPS, which are thin over the same functions, are tested on encoded volumes at
the end.
"""
import gc
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import labelpair_cases as lpc  # noqa: E402
import labelstat_cases as lc  # noqa: E402
import pairstat_cases as pc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import labelpair as lp  # noqa: E402
from imgcompressionmps_amd.core import labelstat as ls  # noqa: E402
from imgcompressionmps_amd.core import pairstat as ps  # noqa: E402
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
ARRAYS = lp.ARRAYS
SAME_AS_LABEL_STATS = (("count", "count"), ("sum", "sum_{}"), ("sumsq", "sumsq_{}"), ("min", "min_{}"), ("max", "max_{}"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _chain(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def _plan(c):
    return _plan_for(c.shape, 0, factor_arr=c.fa)


def _check_shape_of_result(got, n_labels):
    assert set(got) == set(ARRAYS) | {"outside", "scales"}
    for key in ARRAYS:
        assert got[key].shape == (n_labels,) and got[key].dtype == (np.int64 if key in lp.COUNTS else np.float64), key
    assert isinstance(got["outside"], int) and set(got["scales"]) == set(lp.SCALES)
    assert all(isinstance(v, int) for v in got["scales"].values())


def _check_derived(got):
    """The derived fields are pairstat.derive's functions of the raw ones, label by label, bit for bit."""
    filled = got["count"] > 0
    for l in range(got["count"].size):
        if not filled[l]:
            assert all(np.isnan(got[key][l]) for key in lp.DERIVED + lp.EXTREMES), l
            assert all(got[key][l] == 0 for key, _ in lp.SUMS + lp.SQUARES), l
            continue
        one = ps.derive({k: (int(got[k][l]) if k in lp.COUNTS else float(got[k][l])) for k in lp.COUNTS + ps.RAW_FIELDS})
        for key in lp.DERIVED:
            assert lc.same_bits(np.float64(got[key][l]), np.float64(one[key])), (key, l, got[key][l], one[key])


def _check_equals_label_stats(got, chain_a, chain_b, plan, volume, n_labels):
    """Without NaN the fields and exponents of a and of b are label_stats's on that chain, bit for bit."""
    for x, chain in (("a", chain_a), ("b", chain_b)):
        single = ls.label_stats(chain, plan, volume, n_labels)
        for theirs, ours in SAME_AS_LABEL_STATS:
            assert lc.same_bits(single[theirs], got[ours.format(x)]), (x, theirs)
        assert (single["s"], single["s2"]) == (got["scales"]["s_" + x], got["scales"]["s2_" + x]), x
        assert single["outside"] == got["outside"] and not single["n_nan"].any()


def _show(got, head):
    print(f"{head}: outside {got['outside']}, scales {got['scales']}, count {got['count'][:4]}, sum_ab {got['sum_ab'][:4]}, "
          f"sse {got['sse'][:4]}, max_abs_diff {got['max_abs_diff'][:4]}, pearson {got['pearson'][:4]}")


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.INT_NAMES)
def test_integer_cores_give_numpy_s_numbers_exactly(name, storage):
    p = pc.pair(name, "integer", storage)
    a, b, plan = _chain(p.a.cores, storage), _chain(p.b.cores, storage), _plan(p.a)
    ra, rb = p.a.ref, p.b.ref
    whole = ps.pair_stats(a, b)
    x = torch.from_numpy(rb.reshape(p.a.shape)).to(DEV)  # the reference volume of b as an original (exact in fp32 too)
    whole_err = vs.error_to(a, plan, x)
    for kind in lc.kinds_for(name, p.n):
        lab, n_labels = lc.labels(p.a, kind)
        volume = lab.reshape(p.a.shape)
        got = lp.label_pair_stats(a, b, plan, volume.astype(np.int32), n_labels)
        _show(got, f"[labelpair] {name}/{storage} {kind} L {n_labels}")
        _check_shape_of_result(got, n_labels)
        lpc.exact_stats(got, ra, rb, lab, n_labels)
        _check_derived(got)
        assert got["scales"] == lpc.ref_scales(ra, rb) and min(got["scales"].values()) >= 0
        assert got["scales"] == dict(zip(lp.SCALES, lp.scales(max(abs(whole["min_a"]), abs(whole["max_a"])),
                                                              max(abs(whole["min_b"]), abs(whole["max_b"])),
                                                              whole["max_abs_diff"], p.n)))
        assert int(got["count"].sum() + got["n_nan"].sum()) + got["outside"] == p.n
        _check_equals_label_stats(got, a, b, plan, volume.astype(np.int32), n_labels)
        assert lpc.same_dict(lp.label_pair_stats(a, b, plan, volume.astype(np.int32), n_labels), got), "two calls differ"
        if kind == "one":
            for key in ("count",) + ps.RAW_FIELDS:
                assert got[key][0] == whole[key], key
        # every label type, and a device tensor, give the same dict
        types = [np.int16, np.int64] + ([np.uint8] if lab.min() >= 0 and lab.max() < 256 else [])
        for dtype in types:
            assert lpc.same_dict(lp.label_pair_stats(a, b, plan, volume.astype(dtype), n_labels), got), dtype
        for dtype in (torch.int32, torch.int64):
            on_device = torch.from_numpy(volume).to(DEV).to(dtype)
            assert lpc.same_dict(lp.label_pair_stats(a, b, plan, on_device, n_labels), got), dtype
        if kind in ("blocks", "one"):  # n_labels from the labels
            assert lpc.same_dict(lp.label_pair_stats(a, b, plan, volume), got)
        # the original front end: b's reference volume as x
        err = lp.label_error_to(a, plan, x, volume, n_labels)
        assert set(err) == set(lp.ERROR_ARRAYS) | {"outside", "peak"}
        for theirs, ours in (("sse", "sse"), ("max_abs", "max_abs_diff"), ("ref_sumsq", "sumsq_b"), ("ref_max", "max_b"),
                             ("count", "count"), ("n_nan", "n_nan"), ("mse", "mse"), ("rel_frob", "rel_frob")):
            assert lc.same_bits(err[theirs], got[ours]), (kind, theirs)
        assert err["outside"] == got["outside"] and err["peak"] == whole_err["ref_max"] == rb.max()
        want_psnr = lp.psnr_per_label(err["peak"], err["mse"])
        assert lc.same_bits(err["psnr"], want_psnr)
        if kind == "one":
            for key in ("max_abs", "ref_max", "n_nan", "sse", "ref_sumsq", "mse", "rel_frob"):
                assert err[key][0] == whole_err[key], key
            assert err["psnr"][0] == vs.psnr_from(whole_err)


def test_two_labels_as_bool():
    p = pc.pair("int_wide", "integer", "f32")
    a, b, plan = _chain(p.a.cores, "f32"), _chain(p.b.cores, "f32"), _plan(p.a)
    mask = (np.arange(p.n) % 3 == 1).reshape(p.a.shape)
    got = lp.label_pair_stats(a, b, plan, mask)
    lpc.exact_stats(got, p.a.ref, p.b.ref, mask.reshape(-1).astype(np.int64), 2)
    for other in (mask.astype(np.uint8), mask.astype(np.int64), torch.from_numpy(mask).to(DEV)):
        assert lpc.same_dict(lp.label_pair_stats(a, b, plan, other), got)


# ------------------------------------------------------------------------------------------------ NaN, infinity
@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_in_either_volume_is_counted_per_label(name, storage):
    p = pc.pair(name, "integer", storage)
    plan = _plan(p.a)
    cores_a, ra_nan = vc.with_nan(p.a)
    cores_b, rb_nan = vc.with_nan(p.b)
    for where, ca, cb_, ra, rb in (("a", cores_a, p.b.cores, ra_nan, p.b.ref), ("b", p.a.cores, cores_b, p.a.ref, rb_nan),
                                   ("both", cores_a, cores_b, ra_nan, rb_nan)):
        a, b = _chain(ca, storage), _chain(cb_, storage)
        nan = np.isnan(ra) | np.isnan(rb)
        assert 0 < nan.sum() < p.n
        for kind in ("blocks", "scatter"):
            lab, n_labels = lc.labels(p.a, kind)
            got = lp.label_pair_stats(a, b, plan, lab.reshape(p.a.shape), n_labels)
            print(f"[labelpair] {name}/{storage} {kind} NaN in {where}: n_nan {got['n_nan']}, count {got['count']}")
            lpc.exact_stats(got, ra, rb, lab, n_labels)
            assert np.array_equal(got["n_nan"], np.bincount(lab[nan], minlength=n_labels)) and got["n_nan"].sum() == nan.sum()
            _check_derived(got)
        # NaN in an original: the reference volume of b with its NaN, against chain a
        if where != "a":
            x = rb.reshape(p.a.shape)
            err = lp.label_error_to(_chain(p.a.cores, storage), plan, x, lab.reshape(p.a.shape), n_labels)
            want = lpc.stats_of(p.a.ref, rb, lab, n_labels)
            for theirs, ours in (("count", "count"), ("n_nan", "n_nan"), ("sse", "sse"), ("max_abs", "max_abs_diff"),
                                 ("ref_sumsq", "sumsq_b"), ("ref_max", "max_b")):
                assert np.array_equal(err[theirs], want[ours], equal_nan=True), theirs
            assert err["n_nan"].sum() == np.isnan(rb).sum() > 0
            assert err["peak"] == np.nanmax(rb)
        # a label whose voxels are all NaN
        lab, _ = lc.labels(p.a, "blocks")
        lab = np.where(nan, 7, lab)
        got = lp.label_pair_stats(a, b, plan, lab.reshape(p.a.shape), 8)
        lpc.exact_stats(got, ra, rb, lab, 8)
        assert got["count"][7] == 0 and got["n_nan"][7] == nan.sum()
        assert all(np.isnan(got[key][7]) for key in lp.EXTREMES + lp.DERIVED)
        assert all(got[key][7] == 0 for key, _ in lp.SUMS + lp.SQUARES)


@pytest.mark.parametrize("storage", pc.STORAGES)
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
    volume = lab.reshape(c.shape)
    good, bad = _chain(c.cores, storage), _chain(cores, storage)
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="finite voxels"):
            lp.label_pair_stats(a, b, plan, volume, n_labels)
    x = c.ref.reshape(c.shape).copy()
    x.reshape(-1)[c.n // 3] = -np.inf
    with pytest.raises(ValueError, match="finite voxels"):
        lp.label_error_to(good, plan, x, volume, n_labels)
    with pytest.raises(ValueError, match="finite voxels"):
        lp.label_error_to(bad, plan, c.ref.reshape(c.shape), volume, n_labels)
    got = lp.label_pair_stats(good, good, plan, volume, n_labels)
    lpc.sandwich_stats(got, c.ref, c.bound, c.ref, c.bound, lab, n_labels)
    assert np.all(got["sse"] == 0) and np.all(got["max_abs_diff"][got["count"] > 0] == 0)
    err = lp.label_error_to(good, plan, c.ref.reshape(c.shape), volume, n_labels)
    assert np.array_equal(err["count"], got["count"]) and np.all(err["psnr"][err["count"] > 0] > 60)


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.REAL_NAMES)
def test_real_cores_within_the_sandwich(name, storage):
    p = pc.pair(name, "uniform", storage)
    a, b, plan = _chain(p.a.cores, storage), _chain(p.b.cores, storage), _plan(p.a)
    whole = ps.pair_stats(a, b)
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(p.a, kind)
        volume = lab.reshape(p.a.shape)
        got = lp.label_pair_stats(a, b, plan, volume, n_labels)
        show = lambda *figures: print(f"[labelpair] {name}/{storage} {kind}:", *figures)  # noqa: E731
        show("scales", got["scales"])
        lpc.sandwich_stats(got, p.a.ref, p.a.bound, p.b.ref, p.b.bound, lab, n_labels, show)
        _check_derived(got)
        assert got["scales"] == dict(zip(lp.SCALES, lp.scales(max(abs(whole["min_a"]), abs(whole["max_a"])),
                                                              max(abs(whole["min_b"]), abs(whole["max_b"])),
                                                              whole["max_abs_diff"], p.n)))
        _check_equals_label_stats(got, a, b, plan, volume, n_labels)
        assert lpc.same_dict(lp.label_pair_stats(a, b, plan, volume, n_labels), got), "two calls differ"
    # one label: the extremes are pair_stats's exactly
    got = lp.label_pair_stats(a, b, plan, np.zeros(p.a.shape, dtype=np.uint8), 1)
    for key in ("count", "min_a", "max_a", "min_b", "max_b", "max_abs_diff"):
        assert got[key][0] == whole[key], key
    # the original front end: the same pass with the reference of b, in the element type, as the second value
    x = p.b.ref.reshape(p.a.shape).astype(pc.NP_TYPE[storage])
    lab, n_labels = lc.labels(p.a, "outside")
    err = lp.label_error_to(a, plan, x, lab.reshape(p.a.shape), n_labels)
    x64 = x.reshape(-1).astype(np.float64)
    want = lpc.stats_of(p.a.ref, x64, lab, n_labels)
    assert np.array_equal(err["count"], want["count"]) and err["outside"] == want["outside"]
    assert lc.same_bits(err["ref_max"], want["max_b"])  # the original is read, not computed
    whole_err = vs.error_to(a, plan, x)
    assert err["peak"] == whole_err["ref_max"]
    show = lambda *figures: print(f"[labelpair] {name}/{storage} original:", *figures)  # noqa: E731
    _sandwich_error(err, p.a.ref, p.a.bound, x64, lab, n_labels, show)


@pytest.mark.parametrize("name", ["L4_tail_last", "L5_ragged", "L1"])
def test_mixed_storage_equals_the_call_on_both_widened(name):
    p32, p64 = pc.pair(name, "uniform", "f32"), pc.pair(name, "uniform", "f64")
    plan = _plan(p32.a)
    lab, n_labels = lc.labels(p32.a, "scatter")
    volume = lab.reshape(p32.a.shape)
    a32, b64 = _chain(p32.a.cores, "f32"), _chain(p64.b.cores, "f64")
    a32_wide = _chain(p32.a.cores, "f64")  # the fp32 cores, cast
    a, b = ps.pair_chains(a32, b64)
    got = lp.label_pair_stats(a, b, plan, volume, n_labels)
    assert lpc.same_dict(got, lp.label_pair_stats(a32_wide, b64, plan, volume, n_labels))
    back = lp.label_pair_stats(*ps.pair_chains(b64, a32), plan, volume, n_labels)
    assert lc.same_bits(back["sum_a"], got["sum_b"]) and lc.same_bits(back["sse"], got["sse"])


# ------------------------------------------------------------------------------------------------ series
SERIES_DIMS = cc.INTEGER_CHAINS["int_wide"][0]
SERIES = [([1, 8, 16, 10, 1], "f32"), ([1, 4, 8, 5, 1], "f32"), ([1, 2, 3, 2, 1], "f64"), ([1, 8, 12, 7, 1], "f32")]


def test_series_rows_equal_the_single_calls_and_upload_once():
    p = pc.pair("int_wide", "integer", "f32")  # the shape, the plan, the index map and the reference object (b)
    plan = _plan(p.a)
    ref_chain, rb = _chain(p.b.cores, "f32"), p.b.ref
    frames, refs = [], []
    for t, (bonds, storage) in enumerate(SERIES):
        cc.check_chain(SERIES_DIMS, bonds)
        cores = cc.draw_cores(f"labelpair_series_{t}", SERIES_DIMS, bonds, "integer", storage)
        frames.append(_chain(cores, storage))
        refs.append(cb.to_volume(mps_to_dense(cores).reshape(-1), p.a.dest))
    for kind in ("scatter", "window"):
        lab, n_labels = lc.labels(p.a, kind)
        volume = torch.from_numpy(lab.reshape(p.a.shape)).to(DEV).to(torch.int16)
        lp.label_pair_stats(frames[0], ref_chain, plan, volume, n_labels)  # the plan's tables are built on first use
        n_cols = vs._split_columns(frames[0])
        tables = [t.data_ptr() for t in plan.split_tables(n_cols, torch.device(DEV))]
        uploads = ls.LABEL_UPLOADS
        many = lp.label_pair_stats_many(frames, ref_chain, plan, volume, n_labels)
        assert ls.LABEL_UPLOADS == uploads + 1, "the label volume went to the device more than once"
        assert [t.data_ptr() for t in plan.split_tables(n_cols, torch.device(DEV))] == tables
        assert set(many) == set(ARRAYS) | {"outside", "scales"}
        for key in ARRAYS:
            assert many[key].shape == (len(frames), n_labels), key
        assert many["outside"].shape == (len(frames),) and all(many["scales"][k].shape == (len(frames),) for k in lp.SCALES)
        for t, (frame, ref) in enumerate(zip(frames, refs)):
            one = lp.label_pair_stats(frame, ref_chain, plan, volume, n_labels)
            row = {key: many[key][t] for key in ARRAYS}
            row.update(outside=int(many["outside"][t]), scales={k: int(many["scales"][k][t]) for k in lp.SCALES})
            assert lpc.same_dict(row, one), t
            lpc.exact_stats(one, ref, rb, lab, n_labels)
    with pytest.raises(ValueError, match="at least one"):
        lp.label_pair_stats_many([], ref_chain, plan, volume, n_labels)


# ------------------------------------------------------------------------------------------------ memory
def measure_memory():
    """Run in a fresh process (the fixture below): per storage type on the 2**21-voxel pair with 4096 labels, what
    torch.cuda.max_memory_allocated shows above the inputs (the label volume is one of them), the bytes asked of
    the allocator, and the workspace query; one JSON line."""
    out = {}
    for storage in pc.STORAGES:
        p = pc.pair("int_8x7", "integer", storage)
        a, b, plan = _chain(p.a.cores, storage), _chain(p.b.cores, storage), _plan(p.a)
        lab, n_labels = lc.labels(p.a, "max")
        volume = torch.from_numpy(lab.reshape(p.a.shape)).to(DEV).to(torch.int16)
        call = lambda: lp.label_pair_stats(a, b, plan, volume, n_labels)  # noqa: E731
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
                            ws=lp.workspace_bytes(a, b, n_labels), volume=p.n * (8 if storage == "f64" else 4),
                            voxels=int(got["count"].sum()))
        del a, b, plan, volume, call
    print("MEMORY " + json.dumps(out))


@pytest.fixture(scope="module")
def memory_figures():
    """measure_memory() in one fresh child process for both storage types (this test is about a process's allocator)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(tests)!r}, {tests!r}]; "
            "import test_gpu_labelpair as t; t.measure_memory()")
    flags = ["-s"] if sys.flags.no_user_site else []
    run = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("MEMORY ")]
    assert len(line) == 1, run.stdout[-2000:]
    return json.loads(line[0][len("MEMORY "):])


@pytest.mark.parametrize("storage", pc.STORAGES)
def test_device_memory_is_the_workspace_not_the_volumes(memory_figures, storage):
    f = memory_figures[storage]
    print(f"[labelpair] int_8x7/{storage} 4096 labels: {f['above']} bytes held and {f['asked']} bytes asked for above the "
          f"inputs, workspace {f['ws']}, one volume {f['volume']}")
    assert f["voxels"] == 2 ** 21
    assert f["above"] <= f["ws"] + 64 * 1024
    assert f["asked"] <= f["ws"] + 64 * 1024


# ------------------------------------------------------------------------------------------------ through the class
@pytest.fixture(scope="module")
def encoded():
    x = synthetic_mri((32, 48, 40), seed=7)
    return x, {
        ("f32", 12): NDMPS.from_tensor(x, max_bond=12, device=DEV),
        ("f32", 6): NDMPS.from_tensor(x, max_bond=6, device=DEV),
        ("f64", 12): NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=torch.float64),
        ("f64", 6): NDMPS.from_tensor(x, max_bond=6, device=DEV, dtype=torch.float64),
    }


def _atlas(shape):
    """Eight octants, a central ball (label 8) and -1 on one face."""
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    atlas = sum(((g >= n // 2).astype(np.int64) << a) for a, (g, n) in enumerate(zip(grid, shape)))
    r2 = sum(((g - (n - 1) / 2) / (n / 4)) ** 2 for g, n in zip(grid, shape))
    atlas[r2 <= 1.0] = 8
    atlas[0] = -1
    return atlas


def _ref_and_bound(obj, shape, storage):
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), dest)
    return ref, cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest)


@pytest.mark.parametrize("storage", pc.STORAGES)
def test_methods_on_encoded_volumes_within_the_sandwich(encoded, storage):
    x, objs = encoded
    a, b = objs[(storage, 12)], objs[(storage, 6)]
    ra, ba = _ref_and_bound(a, x.shape, storage)
    rb, bb = _ref_and_bound(b, x.shape, storage)
    atlas = _atlas(x.shape)
    lab = atlas.reshape(-1)
    got = a.label_pair_stats(b, atlas)
    show = lambda *figures: print(f"[labelpair] class/{storage}:", *figures)  # noqa: E731
    _check_shape_of_result(got, 9)
    lpc.sandwich_stats(got, ra, ba, rb, bb, lab, 9, show)
    _check_derived(got)
    assert got["outside"] == x.shape[1] * x.shape[2]
    assert lpc.same_dict(a.label_pair_stats(b, atlas, 9), got)
    assert lpc.same_dict(a.label_pair_stats(b, torch.from_numpy(atlas).to(DEV)), got)
    single = a.label_stats(atlas)
    assert lc.same_bits(single["sum"], got["sum_a"]) and lc.same_bits(single["min"], got["min_a"])
    fewer = a.label_pair_stats(b, atlas, n_labels=8)  # the ball falls outside
    assert fewer["outside"] == got["outside"] + got["count"][8]
    # the error per region against the original
    err = a.label_error_to(x, atlas)
    assert set(err) == set(lp.ERROR_ARRAYS) | {"outside", "peak"}
    whole = a.error_to(x)
    show("psnr per label", err["psnr"], "global", a.psnr_to(x), "peak", err["peak"])
    assert err["peak"] == whole["ref_max"]
    assert np.all(np.isfinite(err["psnr"][err["count"] > 0])) and (err["count"] > 0).all()
    assert lc.same_bits(err["psnr"], lp.psnr_per_label(err["peak"], err["mse"]))
    assert lc.same_bits(err["mse"], err["sse"] / err["count"])
    xt = x.astype(pc.NP_TYPE[storage]).reshape(-1).astype(np.float64)
    want = lpc.stats_of(ra, xt, lab, 9)
    assert np.array_equal(err["count"], want["count"]) and lc.same_bits(err["ref_max"], want["max_b"])
    _sandwich_error(err, ra, ba, xt, lab, 9, show)


def _sandwich_error(err, ra, ba, x, lab, n_labels, show):
    """sse, max_abs and ref_sumsq of label_error_to within the sandwich of labelpair_cases for an exact second value;
    the exponents are not returned, so the rounding of a term to an integer is bounded with the smallest exponent the
    rule can give: with the largest term t of the whole volume below 2**e and at least 2**(e - 1), scale = 61 - nb - e and
    2**-(scale + 1) = 2**(e - 1) 2**-(61 - nb) <= t 2**-(61 - nb); the largest computed term is at most the largest
    (|ref - x| + bound)**2."""
    inside = (lab >= 0) & (lab < n_labels)
    which = lab[inside]
    over = lambda w: np.bincount(which, weights=w, minlength=n_labels)  # noqa: E731
    d, bd, r = np.abs(ra - x)[inside], ba[inside], np.abs(x)[inside]
    n_v = over(np.ones_like(d))
    nb = (ra.size - 1).bit_length()
    top_d, top_r = float(((np.abs(ra - x) + ba) ** 2).max()), float((x * x).max())  # over the whole volume, as the scales
    for key, ref, slack, top in (("sse", over(d * d), over(2 * d * bd + bd * bd) + 5 * 2.0 ** -53 * over((d + bd) ** 2), top_d),
                                 ("ref_sumsq", over(r * r), 2.0 ** -52 * over(r * r), top_r)):
        slack = slack + n_v * top * 2.0 ** -(61 - nb)
        show(key, err[key], ref, slack)
        assert np.all(np.abs(err[key] - ref) <= slack), (key, err[key], ref, slack)
    lo = lc.per_label(np.fmax, np.abs(ra - x) - ba, lab, n_labels)
    hi = lc.per_label(np.fmax, np.abs(ra - x) + ba, lab, n_labels)
    show("max_abs", err["max_abs"], lo, hi)
    assert np.all((lo - 2.0 ** -52 * hi <= err["max_abs"]) & (err["max_abs"] <= hi * (1 + 2.0 ** -52)))


def test_series_through_the_class(encoded):
    x, objs = encoded
    atlas = _atlas(x.shape)
    ref = objs[("f32", 12)]
    frames = [objs[("f32", 6)], objs[("f64", 6)], objs[("f32", 12)], objs[("f64", 12)]]
    many = NDMPS.label_pair_stats_many(frames, ref, atlas)
    assert many["pearson"].shape == (4, 9) and many["scales"]["s_ab"].shape == (4,)
    for t, obj in enumerate(frames):
        one = obj.label_pair_stats(ref, atlas)
        row = {key: many[key][t] for key in ARRAYS}
        row.update(outside=int(many["outside"][t]), scales={k: int(many["scales"][k][t]) for k in lp.SCALES})
        assert lpc.same_dict(row, one), t
    same = many["sse"][2]
    assert np.all(same == 0) and np.all(many["pearson"][2][many["count"][2] > 0] > 1 - 1e-6)


def test_refusals(encoded):
    x, objs = encoded
    obj = objs[("f32", 12)]
    atlas = _atlas(x.shape)
    calls = (lambda o: o.label_pair_stats(obj, atlas), lambda o: obj.label_pair_stats(o, atlas),
             lambda o: NDMPS.label_pair_stats_many([o], obj, atlas), lambda o: NDMPS.label_pair_stats_many([obj], o, atlas),
             lambda o: o.label_error_to(x, atlas))
    for call in calls:
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(obj.astype(torch.bfloat16))
        unknown = NDMPS.from_tensor(x, max_bond=4, device=DEV)
        unknown._shape = None
        with pytest.raises(ValueError, match="shape is unknown"):
            call(unknown)
    other = NDMPS.from_tensor(synthetic_mri((32, 48, 20), seed=7), max_bond=4, device=DEV)
    for call in calls[:4]:
        with pytest.raises(ValueError, match="shape"):
            call(other)
    for call in calls[1:4]:  # a non-NDMPS as the other object, as a frame and as the reference
        with pytest.raises(TypeError):
            call("frame")
    for call in (lambda *a: obj.label_pair_stats(obj, *a), lambda *a: NDMPS.label_pair_stats_many([obj], obj, *a),
                 lambda *a: obj.label_error_to(x, *a)):
        with pytest.raises(ValueError, match="at most 4096 labels"):
            call(atlas, 4097)
        with pytest.raises(ValueError, match="at most 4096 labels"):
            call(atlas * 1000)
        with pytest.raises(ValueError, match="shape"):
            call(atlas[:-1])
        with pytest.raises(TypeError, match="integers"):
            call(atlas.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        obj.label_error_to(x[:-1], atlas)
    with pytest.raises(ValueError):
        NDMPS.label_pair_stats_many([], obj, atlas)
    bad = x.copy()
    bad[3, 4, 5] = np.inf
    with pytest.raises(ValueError, match="finite voxels"):
        obj.label_error_to(bad, atlas)
    assert obj.label_error_to(x, atlas)["count"].sum() == x.size - x.shape[1] * x.shape[2]
    assert math.isfinite(obj.label_error_to(torch.from_numpy(x).to(DEV), atlas)["peak"])
