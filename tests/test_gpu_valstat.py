"""Value statistics and the error against an original from the cores (csrc/valstat.hip), on the GPU, against the fp64
contraction of oracle/mps.py through the bars of tests/valstat_cases.py (which tests/test_valstat_host.py shows to
accept the reference and to reject a tile left out, padding counted, an open last bin, shifted bins, an original read
in site order and NaN in a bin).

Integer cores: every number must equal NumPy's on the reference.  Real cores: the sandwich bar.  Each figure is
printed before it is asserted.  The chains of oracle/chain_cases.py are no ``get_factorlist`` chains, so they go through
core/valstat.py with the plan of ``cc.factor_array``; the methods of NDMPS, which are thin over the same functions,
are tested on encoded volumes at the end.
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

import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import compute_psnr, synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _chain(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def _plan(c):
    return _plan_for(c.shape, 0, factor_arr=c.fa)


def _original(c, y):
    return torch.from_numpy(y.reshape(c.shape)).to(DEV).to(TORCH_DT[c.storage])


def _hist(chain, edges):
    counts, used, out = vs.histogram(chain, edges, outliers=True)
    assert np.array_equal(used, edges) and used.dtype == edges.dtype and counts.dtype == np.int64
    return counts, out


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_integer_cores_give_numpy_s_numbers_exactly(name, storage):
    c = vc.case(name, "integer", storage)
    chain = _chain(c.cores, storage)
    got = vs.value_stats(chain)
    print(f"[valstat] {name}/{storage}: {got}")
    vc.exact_moments(got, c.ref)
    assert got["mean"] == got["sum"] / c.n and got["norm"] == np.sqrt(got["sumsq"])
    assert vs.value_stats(chain) == got, "two calls differ"

    for label, edges in vc.integer_edge_sets(c.ref, vc.NP_TYPE[storage]).items():
        counts, out = _hist(chain, edges)
        print(f"[valstat] {name}/{storage} {label}: {edges.size - 1} bins, outliers {out}")
        vc.exact_histogram(counts, out, c.ref, edges)
        again, out2 = _hist(chain, edges)
        assert np.array_equal(again, counts) and out2 == out, "two calls differ"
    # an int with a range is numpy's linspace, and None asks for min and max first
    lo, hi = c.ref.min(), c.ref.max()
    counts, edges = vs.histogram(chain, 16, range=(lo - 0.5, hi + 0.5))
    assert np.array_equal(counts, np.histogram(c.ref, 16, range=(lo - 0.5, hi + 0.5))[0])
    counts, edges = vs.histogram(chain, 7)
    assert (edges[0], edges[-1]) == (lo, hi) and np.array_equal(counts, np.histogram(c.ref, edges.astype(np.float64))[0])

    y = c.original()
    err = vs.error_to(chain, _plan(c), _original(c, y))
    print(f"[valstat] {name}/{storage}: {err}")
    vc.exact_error(err, c.ref, y)
    assert err["n_nan"] == 0 and err["mse"] == err["sse"] / c.n
    assert vs.error_to(chain, _plan(c), _original(c, y)) == err, "two calls differ"
    assert vs.error_to(chain, _plan(c), y.reshape(c.shape))["sse"] == err["sse"]  # a NumPy original
    assert vs.psnr_from(err) == 10 * math.log10(y.max() ** 2 / err["mse"])
    same = vs.error_to(chain, _plan(c), _original(c, c.ref))
    assert same["sse"] == 0 and same["max_abs"] == 0 and vs.psnr_from(same) == np.inf

    for q in (0, 0.25, 0.5, 0.999, 1):
        value, (a, b) = vs.quantile(chain, q)
        want = np.quantile(c.ref, q, method="inverted_cdf")
        print(f"[valstat] {name}/{storage} quantile({q}) = {value} in [{a}, {b}], numpy {want}")
        assert value == want and a <= value <= b
    assert vs.quantile(chain, 0.5) == vs.quantile(chain, 0.5)


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_in_a_core_is_counted_and_lands_in_no_bin(name, storage):
    c = vc.case(name, "integer", storage)
    cores, ref = vc.with_nan(c)
    chain = _chain(cores, storage)
    got = vs.value_stats(chain)
    print(f"[valstat] {name}/{storage} with NaN: {got}")
    vc.exact_moments(got, ref)
    assert 0 < got["n_nan"] < c.n
    edges = vc.integer_edge_sets(ref, vc.NP_TYPE[storage])["half_integers"]
    counts, out = _hist(chain, edges)
    vc.exact_histogram(counts, out, ref, edges)
    assert out[2] == got["n_nan"] and counts.sum() + out[0] + out[1] == c.n - got["n_nan"]
    value, _ = vs.quantile(chain, 0.5)
    assert value == np.quantile(ref[~np.isnan(ref)], 0.5, method="inverted_cdf")
    err = vs.error_to(chain, _plan(c), _original(c, c.ref))
    assert err["n_nan"] == got["n_nan"] and err["sse"] == 0


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_real_cores_within_the_sandwich(name, family, storage):
    c = vc.case(name, family, storage)
    chain = _chain(c.cores, storage)
    got = vs.value_stats(chain)
    print(f"[valstat] {name}/{family}/{storage}: {got}")
    vc.sandwich_moments(got, c.ref, c.bound)
    edges = c.edges64()
    counts, out = _hist(chain, edges)
    print(f"[valstat] {name}/{family}/{storage}: {edges.size - 1} bins, outliers {out}")
    vc.sandwich_histogram(counts, out, c.ref, c.bound, edges)
    y = c.original()
    err = vs.error_to(chain, _plan(c), _original(c, y))
    print(f"[valstat] {name}/{family}/{storage}: {err}")
    vc.sandwich_error(err, c.ref, c.bound, y)
    assert vs.value_stats(chain) == got and vs.error_to(chain, _plan(c), _original(c, y)) == err, "two calls differ"


# ------------------------------------------------------------------------------------------------ memory
MEMORY_CALLS = ("value_stats", "histogram(4096)", "error_to")


def measure_memory():
    """Run in a fresh process (the fixture below): per storage type and call on the 2**21-voxel chain, what
    torch.cuda.max_memory_allocated shows above the inputs, the bytes asked of the allocator, and the workspace query;
    one JSON line.  The caching allocator hands a free block of up to 1 MiB more than a request out unsplit and counts
    it whole, so inside the suite the first figure depends on what earlier tests left in the pool (2 MiB for the
    1.28 MiB fp64 workspace); a process of its own has no such blocks."""
    out = {}
    for storage in vc.STORAGES:
        c = vc.case("int_8x7", "integer", storage)
        chain, plan = _chain(c.cores, storage), _plan(c)
        y = _original(c, c.ref)  # the original counts as an input
        edges = np.linspace(c.ref.min(), c.ref.max(), 4097).astype(vc.NP_TYPE[storage])
        calls = dict(zip(MEMORY_CALLS, ((lambda: vs.value_stats(chain), 0), (lambda: vs.histogram(chain, edges), 4096),
                                        (lambda: vs.error_to(chain, plan, y), 0))))
        for label, (call, n_bins) in calls.items():
            call()  # the plan's offset tables are built once and kept
            torch.cuda.synchronize()
            gc.collect()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            asked_before = torch.cuda.memory_stats()["requested_bytes.all.current"]
            call()
            torch.cuda.synchronize()
            out[f"{storage}/{label}"] = dict(
                above=int(torch.cuda.max_memory_allocated() - before),
                asked=int(torch.cuda.memory_stats()["requested_bytes.all.peak"] - asked_before),
                ws=vs.workspace_bytes(chain, n_bins), volume=c.n * (8 if storage == "f64" else 4))
        del chain, plan, y, calls
    print("MEMORY " + json.dumps(out))


@pytest.fixture(scope="module")
def memory_figures():
    """measure_memory() in one fresh child process for both storage types (this test is about a process's allocator)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(tests)!r}, {tests!r}]; "
            "import test_gpu_valstat as t; t.measure_memory()")
    flags = ["-s"] if sys.flags.no_user_site else []
    run = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("MEMORY ")]
    assert len(line) == 1, run.stdout[-2000:]
    return json.loads(line[0][len("MEMORY "):])


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_device_memory_is_the_workspace_not_the_volume(memory_figures, storage):
    for label in MEMORY_CALLS:
        f = memory_figures[f"{storage}/{label}"]
        print(f"[valstat] int_8x7/{storage} {label}: {f['above']} bytes held and {f['asked']} bytes asked for above the "
              f"inputs, workspace {f['ws']}, volume {f['volume']}")
        # the result records live in the workspace
        assert f["above"] <= f["ws"] + 64 * 1024, label
        assert f["asked"] <= f["ws"] + 64 * 1024, label
        assert f["ws"] < f["volume"] // 4


# ------------------------------------------------------------------------------------------------ through the class
@pytest.fixture(scope="module")
def encoded():
    x = synthetic_mri((32, 48, 40), seed=7)
    return x, {
        "f32": NDMPS.from_tensor(x, max_bond=12, device=DEV),
        "f64": NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=torch.float64),
    }


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_methods_on_an_encoded_volume_within_the_sandwich(encoded, storage):
    """The methods of NDMPS on the object's own chain: the reference is the fp64 contraction of the stored cores through
    the index map of the shape, the bars are those of the chains above."""
    x, objs = encoded
    obj = objs[storage]
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(x.shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), dest)
    bound = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest)
    st = obj.value_stats()
    print(f"[valstat] class/{storage}: {st}")
    vc.sandwich_moments(st, ref, bound)
    assert (obj.min(), obj.max()) == (st["min"], st["max"])
    n = ref.size
    assert st["mean"] == st["sum"] / n and st["norm"] == np.sqrt(st["sumsq"])
    assert st["std"] == np.sqrt(max(st["sumsq"] / n - st["mean"] ** 2, 0.0))
    counts, edges, out = obj.histogram(bins=32, outliers=True)
    assert edges.size == 33 and (edges[0], edges[-1]) == (st["min"], st["max"]) and out == (0, 0, 0)
    vc.sandwich_histogram(counts, out, ref, bound, edges)
    counts, edges, out = obj.histogram(bins=8, range=(0.2, 0.6), outliers=True)
    assert out[0] > 0 and out[1] > 0
    vc.sandwich_histogram(counts, out, ref, bound, edges)
    plain = obj.histogram(bins=8, range=(0.2, 0.6))
    assert len(plain) == 2 and np.array_equal(plain[0], counts)
    # the voxel of rank k among values within `bound` of the reference lies between the rank-k voxels of ref -/+ bound
    for q in (0.0, 0.5, 0.9, 1.0):
        value, (lo, hi) = obj.quantile(q)
        k = min(max(int(np.ceil(n * q - 1)), 0), n - 1)
        least, most = np.sort(ref - bound)[k], np.sort(ref + bound)[k]
        print(f"[valstat] class/{storage} quantile({q}) = {value} in [{lo}, {hi}], rank voxel in [{least}, {most}]")
        assert lo <= value <= hi and lo <= most and hi >= least
        # two passes of 4096 bins, and the rounding of the edges to the element type
        assert hi - lo <= (st["max"] - st["min"]) / 4096 ** 2 + 4 * np.finfo(vc.NP_TYPE[storage]).eps * np.abs(ref).max()
    y = x.astype(vc.NP_TYPE[storage]).astype(np.float64).reshape(-1)
    err = obj.error_to(x)
    print(f"[valstat] class/{storage}: {err}")
    vc.sandwich_error(err, ref, bound, y)
    assert err["mse"] == err["sse"] / n and err["rel_frob"] == np.sqrt(err["sse"] / err["ref_sumsq"])
    psnr = obj.psnr_to(x)
    assert psnr == 10 * math.log10(err["ref_max"] ** 2 / err["mse"])
    assert obj.psnr_to(torch.from_numpy(x).to(DEV)) == psnr
    # the reference's formula on the decoded volume: the two mean squared errors differ by the sandwich's slack
    d = ref - y
    rel = (2 * np.abs(d) * bound + bound * bound).sum() / (d * d).sum()
    vol = np.asarray(obj.to_tensor(), dtype=np.float64).reshape(-1)
    assert abs(psnr - compute_psnr(y, vol)) <= 10 / np.log(10) * 2.1 * rel + 1e-9


def test_refusals(encoded):
    x, objs = encoded
    obj = objs["f32"]
    for call in (lambda o: o.value_stats(), lambda o: o.min(), lambda o: o.max(), lambda o: o.histogram(),
                 lambda o: o.quantile(0.5), lambda o: o.error_to(x), lambda o: o.psnr_to(x)):
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(obj.astype(torch.bfloat16))
        unknown = NDMPS.from_tensor(x, max_bond=4, device=DEV)
        unknown._shape = None
        with pytest.raises(ValueError, match="shape is unknown"):
            call(unknown)
    with pytest.raises(NotImplementedError):
        obj.min(axis=0)
    with pytest.raises(NotImplementedError):
        obj.max(axis=(0, 1))
    with pytest.raises(ValueError, match="at most 4096 bins"):
        obj.histogram(bins=4097)
    with pytest.raises(ValueError, match="at most 4096 bins"):
        obj.histogram(bins=np.linspace(0, 1, 4098))
    with pytest.raises(ValueError, match="ascending"):
        obj.histogram(bins=[0.0, 0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="ascending"):
        obj.histogram(bins=[0.0, float("nan"), 1.0])
    with pytest.raises(ValueError, match="ascending"):
        obj.histogram(bins=4, range=(1.0, 0.0))
    with pytest.raises(ValueError):
        obj.histogram(bins=0)
    with pytest.raises(ValueError):
        obj.quantile(1.5)
    with pytest.raises(ValueError, match="shape"):
        obj.error_to(x[:-1])
    # the library's own check of the edges, behind the Python one
    chain = obj.mps
    with pytest.raises(ValueError, match="ascending"):
        vs.bin_counts(chain, np.array([0.0, 2.0, 1.0], dtype=np.float32))
    assert obj.astype(torch.bfloat16).astype(torch.float32).value_stats()["count"] == x.size
