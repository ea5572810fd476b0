"""Voxels selected by value from the cores (csrc/select.hip, core/select.py), on the GPU, against the fp64 contraction of
oracle/mps.py through the bars of tests/select_cases.py (which tests/test_select_cases_host.py shows to accept the
reference and to reject a tile left out, padding taken as data, an open right bound, site-order indices, NaN selected
by ``invert``, a duplicated slot and an unsorted result).

Integer cores: indices and values must equal NumPy's on the reference.  Real cores: the sandwich bar.  The chains of
the cases are no ``get_factorlist`` chains, so they go through core/select.py with the plan of their factor array; the
methods of NDMPS, which are thin over the same functions, are tested on an encoded volume at the end.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import select_cases as sc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import axisext as ax  # noqa: E402
from imgcompressionmps_amd.core import select as sel  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

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


def _one_bin(chain, lo, hi, np_type):
    counts, _ = vs.histogram(chain, bins=np.array([lo, hi], dtype=np_type))
    return int(counts[0])


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sc.INT_NAMES)
def test_integer_cores_give_numpy_s_selection_exactly(name, storage):
    c = sc.int_case(name, storage)
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    n = c.ref.size
    intervals = sc.int_intervals(c.ref)
    if name == "int_wrap":  # 4 M voxels: the three selections that walk every tile, not the whole volume as a list
        intervals = {k: intervals[k] for k in ("closed_ends", "max_only", "invert", "empty")}
    for key, (lo, hi, invert) in intervals.items():
        index, values = sel.find(chain, plan, lo, hi, invert, max_count=n)
        sc.exact_find(index, values, c.ref, lo, hi, invert, np_type)
        print(f"[select] {name}/{storage} {key}: {index.size} of {n}")
        assert sel.count_between(chain, lo, hi, invert) == index.size
        if key == "empty":
            assert index.size == 0 and values.size == 0
        if key == "everything":
            assert np.array_equal(index, np.arange(n))
        if lo is not None and hi is not None and not invert:
            assert _one_bin(chain, lo, hi, np_type) == index.size
        # two calls return identical bytes
        again, values2 = sel.find(chain, plan, lo, hi, invert, max_count=n)
        assert again.tobytes() == index.tobytes() and values2.tobytes() == values.tobytes(), f"two calls differ: {key}"
    # coordinates and device tensors of one selection
    lo, hi, _ = intervals["closed_ends"]
    index, values = sel.find(chain, plan, lo, hi, max_count=n)
    coords, values2 = sel.find(chain, plan, lo, hi, max_count=n, coords=True)
    assert coords.dtype == np.int64 and coords.shape == (index.size, len(c.shape))
    assert np.array_equal(coords, np.stack(np.unravel_index(index, c.shape), axis=1)) and np.array_equal(values2, values)
    d_coords, d_values = sel.find(chain, plan, lo, hi, max_count=n, coords=True, as_torch=True)
    assert d_coords.device.type == "cuda" and d_coords.dtype == torch.int64 and d_values.dtype == TORCH_DT[storage]
    assert np.array_equal(d_coords.cpu().numpy(), coords) and np.array_equal(d_values.cpu().numpy(), values)
    # the maximum through find is where argmax says
    top = float(c.ref.max())
    at, _ = sel.find(chain, plan, top, top, max_count=n)
    assert at[0] == ax.reduce_index(chain, plan, "max")
    # more matches than max_count: refused with the count, nothing truncated
    many = sc.ref_count(c.ref, lo, hi)
    with pytest.raises(ValueError, match=f"{many} voxels match"):
        sel.find(chain, plan, lo, hi, max_count=many - 1)
    assert sel.find(chain, plan, lo, hi, max_count=many)[0].size == many


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_a_padded_zero_is_never_selected(storage):
    """Every voxel of int_positive lies in [64, 2048] and every voxel of int_negative in [-2048, -64]: a padded row or
    column taken as data is a 0, which the two selections below would list."""
    for name, args in (("int_positive", (-1.0, 1.0, False)), ("int_negative", (-4096.0, -1.0, True))):
        c = sc.int_case(name, storage)
        assert c.m % sc.TILE or c.n % sc.TILE
        chain, plan = _chain(c.cores, storage), _plan(c)
        index, values = sel.find(chain, plan, *args)
        assert index.size == 0 and values.size == 0, (name, index[:8], values[:8])
        assert sel.count_between(chain, *args) == 0


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_voxels_are_listed_by_find_nan_and_by_nothing_else(name, storage):
    c = sc.int_case(name, storage).with_nan()
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    n, n_nan = c.ref.size, int(np.isnan(c.ref).sum())
    assert 0 < n_nan < n
    where = sel.find_nan(chain, plan, max_count=n)
    sc.exact_nan(where, c.ref)
    coords = sel.find_nan(chain, plan, max_count=n, coords=True)
    assert np.array_equal(coords, np.stack(np.unravel_index(where, c.shape), axis=1))
    assert vs.value_stats(chain)["n_nan"] == n_nan == where.size
    index, values = sel.find(chain, plan, -np.inf, np.inf, max_count=n)
    sc.exact_find(index, values, c.ref, None, None, False, np_type)
    assert index.size == n - n_nan == sel.count_between(chain) and not np.isnan(values).any()
    lo, hi, _ = sc.int_intervals(c.ref)["closed_ends"]
    index, values = sel.find(chain, plan, lo, hi, invert=True, max_count=n)
    sc.exact_find(index, values, c.ref, lo, hi, True, np_type)
    assert not np.isnan(values).any() and not np.isin(index, where).any()
    assert sel.count_between(chain, lo, hi) + index.size + n_nan == n
    with pytest.raises(ValueError, match=f"{n_nan} voxels match"):
        sel.find_nan(chain, plan, max_count=n_nan - 1)
    # a volume without NaN has none to list
    assert sel.find_nan(_chain(sc.int_case(name, storage).cores, storage), plan).size == 0


# ------------------------------------------------------------------------------------------------ the capacity guard
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_8x7"])
def test_capacity_guard_counts_every_match_and_writes_only_its_slots(name, storage):
    """The C entry with fewer slots than matches: the total still counts every match, the slots at and beyond
    ``capacity`` keep their sentinel, the first ``capacity`` hold distinct members of the reference set.  The buffers
    have 64 slots more than there are matches, so every access stays inside them whatever the guard does."""
    c = sc.int_case(name, storage)
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    lo, hi, _ = sc.int_intervals(c.ref)["closed_ends"]
    want_index, want_values = sc.ref_find(c.ref, lo, hi)
    count = want_index.size
    assert count > 64
    n_cols = vs._split_columns(chain)
    row_off, col_off, col_perm = plan.split_tables(n_cols, chain.device)
    call = vs._Call(chain)
    for capacity in (count - 1, 0, count):
        index = torch.full((count + 64,), -7, dtype=torch.int64, device=DEV)
        values = torch.full((count + 64,), -7.5, dtype=TORCH_DT[storage], device=DEV)
        total = C.c_int64(-1)
        _lib.check(call.entry("select")(*call.head(), sel.INSIDE, float(lo), float(hi), row_off.data_ptr(), col_off.data_ptr(),
                                        col_perm.data_ptr(), n_cols, capacity, index.data_ptr(), values.data_ptr(),
                                        C.byref(total), *call.tail()))
        assert total.value == count, (capacity, total.value, count)
        index, values = index.cpu().numpy(), values.cpu().numpy()
        assert (index[capacity:] == -7).all() and (values[capacity:] == -7.5).all(), f"a write beyond capacity {capacity}"
        got = index[:capacity]
        assert np.unique(got).size == capacity and np.isin(got, want_index).all()
        assert np.array_equal(values[:capacity].astype(np.float64), c.ref.reshape(-1)[got])
        assert values.dtype == np_type


# ------------------------------------------------------------------------------------------------ topk
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sc.INT_NAMES)
def test_topk_on_integer_cores_equals_lexsort(name, storage):
    c = sc.int_case(name, storage)
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    for largest in (True, False):
        for k in (1, 7, 100):
            index, values = sel.topk(chain, plan, k, largest)
            sc.exact_topk(index, values, c.ref, k, largest, np_type)
    index, values = sel.topk(chain, plan, 7, True)
    coords, _ = sel.topk(chain, plan, 7, True, coords=True)
    assert np.array_equal(coords, np.stack(np.unravel_index(index, c.shape), axis=1))
    d_index, d_values = sel.topk(chain, plan, 7, True, as_torch=True)
    assert d_index.device.type == "cuda" and np.array_equal(d_index.cpu().numpy(), index)
    assert np.array_equal(d_values.cpu().numpy(), values)
    again, values2 = sel.topk(chain, plan, 7, True)
    assert again.tobytes() == index.tobytes() and values2.tobytes() == values.tobytes()


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_topk_completes_ties_and_refuses_too_many(storage):
    c = sc.int_case("int_no_tail", storage)  # thousands of voxels share the maximum
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    flat = c.ref.reshape(-1)
    top = float(flat.max())
    ties = int((flat == top).sum())
    assert ties > 1000
    second = int((flat == np.unique(flat)[-2]).sum())
    # k beyond the ties at the maximum with room for the second value's ties only: the strictly better voxels, then the
    # first ties of the second value in C order
    k, room = ties + 5, max(ties, second)
    assert ties + second > room
    index, values = sel.topk(chain, plan, k, True, max_count=room)
    sc.exact_topk(index, values, c.ref, k, True, np_type)
    # room for exactly the ties at the maximum: one find; one slot less: refused
    index, values = sel.topk(chain, plan, 100, True, max_count=ties)
    sc.exact_topk(index, values, c.ref, 100, True, np_type)
    with pytest.raises(ValueError, match=f"{ties} voxels tie at the k-th value"):
        sel.topk(chain, plan, 100, True, max_count=ties - 1)
    # fewer than k voxels are not NaN: all of them
    small = sc.int_case("int_tail_all", storage).with_nan()
    chain, plan = _chain(small.cores, storage), _plan(small)
    n_ok = int((~np.isnan(small.ref)).sum())
    index, values = sel.topk(chain, plan, small.ref.size, False)
    assert index.size == n_ok
    sc.exact_topk(index, values, small.ref, small.ref.size, False, np_type)


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", sc.REAL_CASES, ids=sc.REAL_IDS)
def test_real_cores_within_the_sandwich(name, family, storage):
    c = sc.real_case(name, family, storage)
    chain, plan, np_type = _chain(c.cores, storage), _plan(c), vc.NP_TYPE[storage]
    for key, (lo, hi) in c.intervals.items():
        index, values = sel.find(chain, plan, lo, hi, max_count=c.ref.size)
        ambiguous = sc.sandwich_find(index, values, c.ref, c.bound, lo, hi, np_type)
        moved = np.setxor1d(index, sc.ref_find(c.ref, lo, hi)[0]).size
        print(f"[select] {name}/{family}/{storage} {key}: {index.size} selected, {ambiguous} of them ambiguous, "
              f"{moved} differ from the reference's selection")
        assert sel.count_between(chain, lo, hi) == index.size
        if hi is not None:
            assert _one_bin(chain, lo, hi, np_type) == index.size
        again, values2 = sel.find(chain, plan, lo, hi, max_count=c.ref.size)
        assert again.tobytes() == index.tobytes() and values2.tobytes() == values.tobytes(), "two calls differ"


# ------------------------------------------------------------------------------------------------ through the class
@pytest.mark.parametrize("storage", vc.STORAGES)
def test_methods_on_an_encoded_volume_equal_the_object_s_own_to_tensor(storage):
    """find, find_nan and topk through the NDMPS methods against ``to_tensor()`` of the same object: both come from the
    same cores.  The equality holds only while the last product of ``to_tensor`` and the tile of the statistics family
    compute a voxel identically (the same order of the k loop on the same operands)."""
    x = synthetic_mri((64, 64, 64), seed=11)
    obj = NDMPS.from_tensor(x, max_bond=16, device=DEV, **({"dtype": torch.float64} if storage == "f64" else {}))
    v = obj.to_tensor()
    flat = v.reshape(-1)
    np_type = vc.NP_TYPE[storage]
    assert flat.dtype == np_type
    for lo, hi in ((np_type(np.percentile(flat, 99.9)), None), (np_type(np.percentile(flat, 90)), np_type(np.percentile(flat, 92)))):
        index, values = obj.find(lo, hi)
        want = np.flatnonzero((flat >= lo) & (flat <= (np.inf if hi is None else hi)))
        print(f"[select] class/{storage} [{lo}, {hi}]: {index.size} selected, to_tensor has {want.size}, "
              f"{np.setxor1d(index, want).size} differ")
        assert np.array_equal(index, want) and np.array_equal(values, flat[want])
        assert obj.count_between(lo, hi) == index.size
        coords, _ = obj.find(lo, hi, coords=True)
        assert np.array_equal(coords, np.stack(np.unravel_index(want, v.shape), axis=1))
    assert obj.find_nan().size == 0 and obj.find_nan(coords=True).shape == (0, 3)
    for largest in (True, False):
        coords, values = obj.topk(50, largest, coords=True)
        s = -flat if largest else flat
        order = np.lexsort((np.arange(flat.size), s))[:50]
        assert np.array_equal(coords, np.stack(np.unravel_index(order, v.shape), axis=1))
        assert np.array_equal(values, flat[order])
    at, top = obj.find(obj.max(), obj.max())
    assert at[0] == obj.argmax() and top[0] == np_type(obj.max())
