"""Extremes along axes and the place of the global extreme from the cores (csrc/axisext.hip, core/axisext.py), on the
GPU, against the fp64 contraction of oracle/mps.py through the bars of tests/axisext_cases.py (which
tests/test_axisext_host.py shows to accept the reference and to reject a tile left out, padding counted, the last
occurrence, a dropped column index, unpermuted columns and a NaN that wins).

Integer cores: values and indices must equal NumPy's on the reference, ties included.  Real cores: the sandwich bar.
The chains of the cases are no ``get_factorlist`` chains, so they go through core/axisext.py with the plan of their
factor array; the methods of NDMPS, which are thin over the same functions, are tested on encoded volumes at the end.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import axisext_cases as ac  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import axisext as ax  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
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


def _exact_everything(c, chain, plan, storage):
    """The exact bar on every projection of an integer case; returns what was computed, for the repeat."""
    np_type = vc.NP_TYPE[storage]
    got = {}
    for axes in ac.axis_sets(len(c.shape)):
        for op in ac.OPS:
            values = ax.reduce_values(chain, plan, op, axes)
            assert values.dtype == np_type
            ac.exact_values(values, c.ref, axes, op)
            got[axes, op] = values
            if len(axes) == 1:
                assert np.array_equal(ax.reduce_values(chain, plan, op, axes[0]), values, equal_nan=True)
                where = ax.reduce_index(chain, plan, op, axes[0])
                ac.exact_index(where, c.ref, axes[0], op)
                where2, values2 = ax.reduce_index(chain, plan, op, axes[0], return_values=True)
                assert values2.dtype == np_type
                assert np.array_equal(where2, where) and np.array_equal(values2, values, equal_nan=True)
                got[axes, op, "index"] = where
    for op in ac.OPS:
        flat = ax.reduce_index(chain, plan, op)
        flat2, value = ax.reduce_index(chain, plan, op, return_values=True)
        assert isinstance(flat, int) and isinstance(value, float) and flat2 == flat
        ac.exact_flat(flat, value, c.ref, op)
        got[op, "flat"] = (flat, value)
    return got


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ac.SIGNED_NAMES)
def test_integer_cores_give_numpy_s_extremes_and_places_exactly(name, storage):
    c = ac.int_case(name, storage)
    chain, plan = _chain(c.cores, storage), _plan(c)
    got = _exact_everything(c, chain, plan, storage)
    for op in ac.OPS:
        print(f"[axisext] {name}/{storage} arg{op}() = {got[op, 'flat']}")
    again = _exact_everything(c, chain, plan, storage)
    assert got.keys() == again.keys()
    for key in got:
        if isinstance(got[key], tuple):
            assert got[key] == again[key], f"two calls differ: {key}"
        else:
            assert got[key].tobytes() == again[key].tobytes(), f"two calls differ: {key}"


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_in_a_core_takes_no_part(name, storage):
    c = ac.int_case(name, storage).with_nan()
    nan = np.isnan(c.ref)
    assert any(nan.all(axis=a).any() for a in range(3)), "no ray of NaN only"
    assert any((nan.any(axis=a) & ~nan.all(axis=a)).any() for a in range(3)), "no partly NaN ray"
    chain, plan = _chain(c.cores, storage), _plan(c)
    got = _exact_everything(c, chain, plan, storage)  # np.fmax / np.fmin, and -1 for a ray of NaN only
    for a in range(3):
        assert np.array_equal(got[(a,), "max", "index"] == -1, nan.all(axis=a))
        assert np.array_equal(np.isnan(got[(a,), "min"]), nan.all(axis=a))
    # a volume of NaN only
    cores = [x.copy() for x in c.cores]
    cores[0][:] = np.nan
    chain = _chain(cores, storage)
    for op in ac.OPS:
        flat, value = ax.reduce_index(chain, plan, op, return_values=True)
        assert flat == -1 and np.isnan(value)
        where, values = ax.reduce_index(chain, plan, op, 1, return_values=True)
        assert (where == -1).all() and np.isnan(values).all()


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_real_cores_within_the_sandwich(name, family, storage):
    c = ac.real_case(name, family, storage)
    chain, plan = _chain(c.cores, storage), _plan(c)
    for axis in range(len(c.shape)):
        for op in ac.OPS:
            values = ax.reduce_values(chain, plan, op, axis)
            ac.sandwich_values(values, c.ref, c.bound, (axis,), op)
            where, values2 = ax.reduce_index(chain, plan, op, axis, return_values=True)
            assert np.array_equal(values2, values)
            share = ac.sandwich_index(where, c.ref, c.bound, axis, op)
            moved = int((where != ac.ref_index(c.ref, axis, op)).sum())
            print(f"[axisext] {name}/{family}/{storage} a{op}({axis}): {share:.4f} of the rays ambiguous, "
                  f"{moved} of {where.size} indices differ from the reference's")
            again, values3 = ax.reduce_index(chain, plan, op, axis, return_values=True)
            assert np.array_equal(again, where) and values3.tobytes() == values.tobytes(), "two calls differ"
    for op in ac.OPS:
        flat, value = ax.reduce_index(chain, plan, op, return_values=True)
        ac.sandwich_values(np.float64(value), c.ref, c.bound, tuple(range(len(c.shape))), op)
        s = 1.0 if op == "max" else -1.0
        r, b = s * c.ref.reshape(-1), c.bound.reshape(-1)
        assert 0 <= flat < r.size and r[flat] + b[flat] >= (r - b).max(), (op, flat)


# ------------------------------------------------------------------------------------------------ through the class
VOLUMES = {"mri": (30, 45, 20), "cube": (16, 16, 16)}


@pytest.fixture(scope="module")
def encoded():
    out = {}
    for label, shape in VOLUMES.items():
        x = synthetic_mri(shape, seed=11)
        out[label] = (x, {"f32": NDMPS.from_tensor(x, max_bond=8, device=DEV),
                          "f64": NDMPS.from_tensor(x, max_bond=8, device=DEV, dtype=torch.float64)})
    return out


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("label", sorted(VOLUMES))
def test_methods_on_an_encoded_volume_within_the_sandwich(encoded, label, storage):
    """The methods of NDMPS on the object's own chain: the reference is the fp64 contraction of the stored cores through
    the index map of the shape, the bars are those of the chains above."""
    x, objs = encoded[label]
    obj = objs[storage]
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(x.shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), dest).reshape(x.shape)
    bound = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest).reshape(x.shape)
    np_type = vc.NP_TYPE[storage]
    for op, values_of, index_of in (("max", obj.amax, obj.argmax), ("min", obj.amin, obj.argmin)):
        for axes in ac.axis_sets(3):
            values = values_of(axes)
            assert isinstance(values, np.ndarray) and values.dtype == np_type
            ac.sandwich_values(values, ref, bound, axes, op)
            assert np.array_equal(values_of(tuple(a - 3 for a in axes)), values)
            kept = values_of(axes, keepdims=True)
            assert kept.shape == tuple(1 if a in axes else n for a, n in enumerate(x.shape))
            assert np.array_equal(kept.reshape(values.shape), values)
            dev = values_of(axes, as_torch=True)
            assert dev.device.type == "cuda" and dev.dtype == TORCH_DT[storage] and np.array_equal(dev.cpu().numpy(), values)
        for axis in range(3):
            where = index_of(axis)
            ambiguous = ac.sandwich_index(where, ref, bound, axis, op)  # no cap here: the background of a scan ties
            assert np.array_equal(values_of(axis), values_of((axis,)))
            assert np.array_equal(index_of(axis - 3), where)
            where2, values = index_of(axis, return_values=True)
            assert np.array_equal(where2, where) and np.array_equal(values, values_of(axis))
            kept, kept_values = index_of(axis, keepdims=True, return_values=True)
            assert kept.shape == kept_values.shape == tuple(1 if a == axis else n for a, n in enumerate(x.shape))
            assert np.array_equal(kept.reshape(where.shape), where)
            dev, dev_values = index_of(axis, as_torch=True, return_values=True)
            assert dev.dtype == torch.int64 and dev.device.type == "cuda" and np.array_equal(dev.cpu().numpy(), where)
            assert dev_values.dtype == TORCH_DT[storage] and np.array_equal(dev_values.cpu().numpy(), values)
            print(f"[axisext] class/{label}/{storage} arg{op}({axis}): {ambiguous:.4f} of the rays ambiguous")
        # None and a tuple naming every axis: the scalar of value_stats
        whole = obj.max() if op == "max" else obj.min()
        assert values_of() == values_of((0, 1, 2)) == values_of((-1, 0, 1)) == whole
        assert values_of(keepdims=True).shape == (1, 1, 1) and values_of(keepdims=True)[0, 0, 0] == np_type(whole)
        flat, value = index_of(return_values=True)
        assert isinstance(flat, int) and flat == index_of() and value == whole
        s = 1.0 if op == "max" else -1.0
        r, b = s * ref.reshape(-1), bound.reshape(-1)
        assert r[flat] + b[flat] >= (r - b).max()
        if (r + b >= (r - b).max()).sum() == 1:
            assert flat == int(np.argmax(r))


def test_refusals(encoded):
    x, objs = encoded["mri"]
    obj = objs["f32"]
    calls = (lambda o: o.amax(0), lambda o: o.amin((0, 1)), lambda o: o.argmax(1), lambda o: o.argmin(),
             lambda o: o.amax(), lambda o: o.argmax(2, return_values=True))
    for call in calls:
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(obj.astype(torch.bfloat16))
        unknown = NDMPS.from_tensor(x, max_bond=4, device=DEV)
        unknown._shape = None
        with pytest.raises(ValueError, match="shape is unknown"):
            call(unknown)
    for method in (obj.amax, obj.amin, obj.argmax, obj.argmin):
        for bad in (3, -4):
            with pytest.raises(np.exceptions.AxisError):
                method(bad)
    for method in (obj.amax, obj.amin):
        with pytest.raises(np.exceptions.AxisError):
            method((0, 3))
        with pytest.raises(ValueError, match="duplicate"):
            method((0, 0))
        with pytest.raises(ValueError, match="duplicate"):
            method((1, -2))
    for method in (obj.argmax, obj.argmin):
        with pytest.raises(TypeError):
            method((0, 1))
        with pytest.raises(TypeError):
            method((0,))
    # min and max keep their behaviour
    with pytest.raises(NotImplementedError):
        obj.min(axis=0)
    with pytest.raises(NotImplementedError):
        obj.max(axis=(0, 1))
    assert obj.astype(torch.bfloat16).astype(torch.float32).amax(0).shape == (45, 20)
