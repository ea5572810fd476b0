"""Host side of the series region decode (NDMPS.decode_regions / values_at_many): the workspace layout and the
chunking of ``core.region.plan_series`` on hand-computed cases, against ``ndmps_region_series_workspace_bytes``, and
the declarations of the new entry points.  No GPU: the library loads without one (tests/test_host_logic.py).

(64, 64, 64) has L = 6 sites of d = 8 (one binary digit of every axis per site).  With axis 0 fixed, level s of a
slice holds the 4 ** (s + 1) prefixes of the two free axes: 4, 16, 64, 256, 1024 nodes."""
import os
import re

import numpy as np
import pytest

from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (64, 64, 64)
FULL = [1, 8, 64, 512, 64, 8, 1]
THIN = [1, 3, 3, 3, 3, 3, 1]
RAGGED = [1, 8, 33, 70, 40, 8, 1]


def _slice_plan():
    plan = region.plan_outer(SHAPE, region.normalize_key((5,), SHAPE)[0])
    assert plan.nodes == [4, 16, 64, 256, 1024]
    return plan


def _points_plan():
    """(0, 0, 0) and (0, 0, 1) share every prefix but the last digit; (63, 63, 63) shares none: two nodes a level."""
    pts = region.normalize_points([[0, 0, 0], [63, 63, 63], [0, 0, 1]], SHAPE)
    plan = region.plan_points(SHAPE, pts)
    assert plan.nodes == [2, 2, 2, 2, 2]
    return plan


def _c_workspace(bonds, plan, elem):
    b = np.ascontiguousarray(bonds, dtype=np.int64)
    return int(_lib.load().ndmps_region_series_workspace_bytes(b.shape[0], b.shape[1] - 1, b.ctypes.data_as(_lib.p_i64),
                                                               _lib.i64_array(plan.nodes), elem))


def test_caps_stride_and_workspace_of_a_slice():
    plan = _slice_plan()
    lay = region.plan_series([FULL, THIN], plan, 4)
    assert lay.caps == FULL
    # nodes_s * cap_{s+1}: 4 * 8, 16 * 64, 64 * 512, 256 * 64, 1024 * 8
    assert lay.frame_stride == 32768
    assert lay.ws_bytes == 2 * 2 * 32768 * 4 == 524288
    assert lay.chunks == [(0, 2)]
    assert lay.ws_bytes == _c_workspace([FULL, THIN], plan, 4)
    # the caps are per level, not per frame: no frame has both bond 2 = 33 ... and bond 3 = 512
    lay = region.plan_series([THIN, RAGGED, THIN], plan, 8)
    assert lay.caps == RAGGED
    # 4 * 8, 16 * 33, 64 * 70, 256 * 40, 1024 * 8
    assert lay.frame_stride == 10240
    assert lay.ws_bytes == 2 * 3 * 10240 * 8 == _c_workspace([THIN, RAGGED, THIN], plan, 8)
    mixed = [[1, 8, 3, 70, 3, 8, 1], [1, 3, 33, 3, 40, 3, 1]]
    assert region.plan_series(mixed, plan, 4).caps == RAGGED
    assert region.plan_series(mixed, plan, 4).ws_bytes == _c_workspace(mixed, plan, 4)


def test_workspace_is_rounded_to_256_bytes_per_buffer():
    plan = _points_plan()
    bonds = [1, 5, 7, 3, 2, 2, 1]
    lay = region.plan_series([bonds], plan, 8)
    assert lay.frame_stride == 14  # 2 * 7
    assert lay.ws_bytes == 2 * 256 == _c_workspace([bonds], plan, 8)  # 112 bytes a buffer
    lay = region.plan_series([bonds] * 3, plan, 8)
    assert lay.ws_bytes == 2 * 512 == _c_workspace([bonds] * 3, plan, 8)  # 336 bytes a buffer
    lay = region.plan_series([bonds] * 3, plan, 4)
    assert lay.ws_bytes == 2 * 256 == _c_workspace([bonds] * 3, plan, 4)  # 168 bytes a buffer


def test_chunks_follow_the_workspace_limit():
    plan = _slice_plan()
    frames = [FULL, THIN, THIN, FULL, THIN]
    # a frame's slab is 131072 bytes; 600000 bytes hold both buffers of two frames (524288), not of three (786432)
    lay = region.plan_series(frames, plan, 4, ws_limit=600000)
    assert lay.chunks == [(0, 2), (2, 4), (4, 5)]
    assert lay.ws_bytes == 524288 <= 600000
    assert lay.caps == FULL and lay.frame_stride == 32768  # caps of the whole series, whatever the chunk holds
    assert lay.ws_bytes >= max(_c_workspace(frames[a:b], plan, 4) for a, b in lay.chunks)
    assert region.plan_series(frames, plan, 4, ws_limit=786432).chunks == [(0, 3), (3, 5)]
    assert region.plan_series(frames, plan, 4, ws_limit=5 * 262144).chunks == [(0, 5)]
    # one frame alone above the limit: a chunk of its own, the only case that exceeds the limit
    lay = region.plan_series(frames, plan, 4, ws_limit=1000)
    assert lay.chunks == [(t, t + 1) for t in range(5)] and lay.ws_bytes == 262144


def test_module_limit_is_read_at_call_time(monkeypatch):
    plan = _slice_plan()
    assert region.SERIES_WS_BYTES >= 1 << 28
    assert region.plan_series([FULL] * 5, plan, 4).chunks == [(0, 5)]
    monkeypatch.setattr(region, "SERIES_WS_BYTES", 600000)
    assert region.plan_series([FULL] * 5, plan, 4).chunks == [(0, 2), (2, 4), (4, 5)]


def test_a_chunk_holds_at_most_65535_frames():
    plan = _points_plan()
    bonds = np.tile(np.array([1, 2, 2, 2, 2, 2, 1], dtype=np.int64), (70000, 1))
    lay = region.plan_series(bonds, plan, 4)
    assert region.MAX_SERIES_FRAMES == 65535
    assert lay.chunks == [(0, 65535), (65535, 70000)]
    assert lay.frame_stride == 4 and lay.ws_bytes == 2 * 1048576  # 65535 * 16 = 1048560 bytes a buffer
    assert lay.ws_bytes == _c_workspace(bonds[:65535], plan, 4)
    assert _c_workspace(bonds[:65536], plan, 4) == -1


def test_single_site_chain_needs_no_workspace():
    plan = region.plan_outer((5,), region.normalize_key((), (5,))[0])
    assert plan.nodes == []
    lay = region.plan_series([[1, 1]] * 3, plan, 4)
    assert (lay.caps, lay.frame_stride, lay.ws_bytes, lay.chunks) == ([1, 1], 1, 0, [(0, 3)])
    assert _c_workspace([[1, 1]] * 3, plan, 4) == 0


def test_bad_bond_lists_are_refused():
    plan = _slice_plan()
    for bonds in ([], [FULL[:-1]], [[2] + FULL[1:]], [FULL[:-1] + [2]], [[1, 8, 0, 8, 8, 8, 1]], FULL):
        with pytest.raises(ValueError):
            region.plan_series(bonds, plan, 4)
    lib = _lib.load()
    b, n = _lib.i64_array(FULL), _lib.i64_array(plan.nodes)
    assert lib.ndmps_region_series_workspace_bytes(0, 6, b, n, 4) == -1
    assert lib.ndmps_region_series_workspace_bytes(1, 6, b, n, 0) == -1
    assert lib.ndmps_region_series_workspace_bytes(1, 65, b, n, 4) == -1
    assert lib.ndmps_region_series_workspace_bytes(1, 6, None, n, 4) == -1


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ndmps_hip.h")).read()
    lib = _lib.load()
    for name, n_args in [("ndmps_region_series_workspace_bytes", 5), ("ndmps_region_series_contract_f32", 14),
                         ("ndmps_region_series_contract_f64", 14)]:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in include/ndmps_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
    assert "d_records" in header and "core pointers" in header  # the layout of the frame records is documented


def test_refused_arguments_launch_nothing():
    """Argument checks come before anything touches a device, so they answer on a machine without one."""
    lib = _lib.load()
    plan = _slice_plan()
    dims, nodes, tiles = _lib.i64_array([8] * 6), _lib.i64_array(plan.nodes), _lib.i64_array(plan.n_tiles)
    bonds = _lib.i64_array(FULL)
    args = (dims, bonds, nodes, tiles, None, plan.tables().size, None, plan.n_out, None, None, 0, None)
    for fn in (lib.ndmps_region_series_contract_f32, lib.ndmps_region_series_contract_f64):
        assert fn(1, 6, *args) == _lib.EINVAL  # null tables, records and output
        assert fn(0, 6, *args) == _lib.EINVAL
