"""The host side of the decoders' device layer (core/readout.py, core/plan.py), without a GPU: the result conversion,
the names core/ndmps.py re-exports, and the two region skeletons driven by a fake contraction on CPU tensors."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from imgcompressionmps_amd.core import ndmps, plan, readout, region

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


# ------------------------------------------------------------------------------------------------ as_result
@pytest.mark.parametrize("src, as_torch, dtype, bf16_std",
                         itertools.product([F32, BF16, F64], [False, True], [None, F32, BF16, F64], [False, True]))
def test_as_result_truth_table(src, as_torch, dtype, bf16_std):
    res = torch.arange(6, dtype=torch.float32).reshape(2, 3).to(src)
    got = readout.as_result(res, as_torch, dtype, bf16_std)
    if as_torch:
        want = dtype if dtype is not None else BF16 if bf16_std else src
        assert isinstance(got, torch.Tensor) and got.dtype == want and tuple(got.shape) == (2, 3)
        if dtype is None and not bf16_std:
            assert got is res  # nothing is copied when nothing is asked for
    else:  # dtype and bf16_std play no part in the NumPy result
        assert isinstance(got, np.ndarray) and got.shape == (2, 3)
        assert got.dtype == (np.float64 if src == F64 else np.float32)
    assert np.array_equal(np.asarray(got.to(F64) if as_torch else got, dtype=np.float64), np.arange(6.0).reshape(2, 3))


def test_as_result_bf16_only_from_the_flag_or_the_argument():
    """An fp32 / fp64 result turns bf16 only for as_torch=True, dtype=None, bf16_std=True (or an explicit dtype)."""
    for src, as_torch, bf16_std in itertools.product([F32, F64], [False, True], [False, True]):
        got = readout.as_result(torch.zeros(4, dtype=src), as_torch, None, bf16_std)
        assert (getattr(got, "dtype", None) == BF16) == (as_torch and bf16_std)


@pytest.mark.parametrize("src, np_type", [(F32, np.float32), (BF16, np.float32), (F64, np.float64)])
def test_as_result_zero_d_is_a_numpy_scalar(src, np_type):
    got = readout.as_result(torch.tensor(2.5, dtype=src), False, None, True)
    assert isinstance(got, np.generic) and not isinstance(got, np.ndarray) and got.dtype == np_type and got == 2.5
    kept = readout.as_result(torch.tensor(2.5, dtype=src), True, None, False)
    assert isinstance(kept, torch.Tensor) and kept.dim() == 0 and kept.dtype == src


# ------------------------------------------------------------------------------------------------ re-exports
def test_ndmps_reexports_are_the_objects_of_plan():
    for name in ("StageTimer", "set_stage_timer", "_plan_for", "_dct_basis"):
        assert getattr(ndmps, name) is getattr(plan, name), name


def test_stage_timer_set_through_ndmps_is_seen_by_plan():
    class Timer:
        def __init__(self):
            self.names = []

        def span(self, name):
            self.names.append(name)
            return ("context of", name)

    t = Timer()
    try:
        ndmps.set_stage_timer(t)
        assert plan._span("x") == ("context of", "x") and t.names == ["x"]
    finally:
        ndmps.set_stage_timer(None)
    assert isinstance(plan._span("x"), contextlib.nullcontext) and t.names == ["x"]


# ------------------------------------------------------------------------------------------------ skeletons
SHAPE = (6, 10)
OUTER = [  # key, shape of the result behind the leading axes
    ((), (6, 10)),
    ((2,), (10,)),
    ((-1, 3), ()),
    ((slice(1, 6, 2),), (3, 10)),
    ((slice(None), slice(None, None, -3)), (6, 4)),
    (([4, 0, 0], 7), (3,)),
    (([5, 1], [9, 9, 0, 2]), (2, 4)),
    ((slice(3, 3),), (0, 10)),
    ((1, slice(7, 7)), (0,)),
    (([], [1, 2]), (0, 2)),
]
POINTS = [([[0, 0], [5, 9], [-1, -10], [2, 3], [2, 3]], 5), ([[3, 4]], 1), (np.zeros((0, 2), dtype=np.int64), 0)]


class _Fake:
    """A contraction that returns ``arange`` values for the plan's n_out behind the leading axes, on the CPU."""

    def __init__(self, lead):
        self.lead, self.plans = lead, []

    def __call__(self, rplan):
        self.plans.append(rplan)
        lead_n = int(np.prod(self.lead, dtype=np.int64))
        return torch.arange(lead_n * rplan.n_out, dtype=F32).view(*self.lead, rplan.n_out)


@pytest.mark.parametrize("lead", [(), (3,)], ids=["single", "series"])
@pytest.mark.parametrize("key, want", OUTER, ids=[str(k) for k, _ in OUTER])
def test_region_outer_shapes_and_empty_selections(lead, key, want):
    idx, keep = region.normalize_key(key, SHAPE)
    fake = _Fake(lead)
    got = readout.region_outer(fake, lead, SHAPE, idx, keep, False, F32, torch.device("cpu"))
    assert tuple(got.shape) == lead + want and got.dtype == F32
    if 0 in want:
        assert fake.plans == []  # an empty selection never reaches the contraction
    else:
        n_out = int(np.prod([i.size for i in idx]))
        assert [p.n_out for p in fake.plans] == [n_out]
        assert torch.equal(got.reshape(-1), torch.arange(int(np.prod(lead, dtype=np.int64)) * n_out, dtype=F32))


@pytest.mark.parametrize("lead", [(), (3,)], ids=["single", "series"])
@pytest.mark.parametrize("coords, N", POINTS, ids=["five", "one", "none"])
def test_region_points_shapes_and_empty_selections(lead, coords, N):
    pts = region.normalize_points(coords, SHAPE)
    fake = _Fake(lead)
    got = readout.region_points(fake, lead, SHAPE, pts, False, F64, torch.device("cpu"))
    assert tuple(got.shape) == lead + (N,)
    if N == 0:
        assert fake.plans == [] and got.dtype == F64  # the empty result has the type the caller named
    else:
        assert [p.n_out for p in fake.plans] == [N]
        assert torch.equal(got.reshape(-1), torch.arange(int(np.prod(lead, dtype=np.int64)) * N, dtype=F32))
