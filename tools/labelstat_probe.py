"""Statistics per label from the cores against decode-then-scatter: label_stats on 256^3 chi=64 and 64^3 chi=16, fp32,
under five label volumes (one label; a box mask, 2 labels; a grid of 5^3 + 1 parcels, uint8; of 10^3 + 1 parcels,
int16; 1001 labels scattered voxel by voxel, so that no run survives), each against to_tensor(as_torch=True) followed
by the six numbers from torch: counts and the two sums by torch.bincount(weights=) or by scatter_reduce("sum") in fp64,
whichever is faster, the NaN count by bincount, and the extremes by scatter_reduce amin / amax, read back to the host.
Then a series: label_stats_many over 16 frames against the same decode loop.  Warm-up, then the median of REPS timed
calls each (of 3 for a side whose call takes longer than 50 ms), the sides interleaved, each call ended by a device
synchronise; the times are whole calls (host planning, launches, the read-back; the labels are on the device).  Memory: torch.cuda.max_memory_allocated
during one call above what was allocated before it (the cores and the label volume are inputs).  Prints one JSON
line per case and label volume.
usage: python tools/labelstat_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "small"]
assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to time without one"
DEV = "cuda:0"
FRAMES = 16
SLOW_MS, SLOW_REPS = 50.0, 3


def make(case):
    n, bond = (64, 16) if case == "small" else (256, 64)
    x = synthetic_mri((n,) * 3, seed=31)
    return NDMPS.from_tensor(x, max_bond=bond, device=DEV)


def grid_labels(shape, g):
    """g^3 parcels in the middle of the volume (labels 1 ... g^3) inside a background of label 0."""
    axes = []
    for n in shape:
        margin = n // 9
        cell = (n - 2 * margin) // g
        i = (np.arange(n) - margin) // cell
        axes.append(np.where((i >= 0) & (i < g), i, -1))
    a, b, c = np.meshgrid(*axes, indexing="ij")
    return np.where((a >= 0) & (b >= 0) & (c >= 0), 1 + (a * g + b) * g + c, 0)


def label_volumes(shape):
    n = int(np.prod(shape))
    box = np.zeros(shape, dtype=np.uint8)
    box[tuple(slice(s // 4, 3 * s // 4) for s in shape)] = 1
    return {
        "one": (np.zeros(shape, dtype=np.uint8), 1),
        "box": (box, 2),
        "grid126": (grid_labels(shape, 5).astype(np.uint8), 126),
        "grid1001": (grid_labels(shape, 10).astype(np.int16), 1001),
        "scatter1001": (np.random.default_rng(5).integers(0, 1001, n).astype(np.int16).reshape(shape), 1001),
    }


def decoded(obj, lab64, n_labels, sums):
    """The six numbers per label from the decoded volume, on the host."""
    v = obj.to_tensor(as_torch=True).reshape(-1)
    nan = torch.isnan(v)
    d = torch.where(nan, torch.zeros_like(v), v).double()
    if sums == "bincount":
        total = torch.bincount(lab64, weights=d, minlength=n_labels)
        squares = torch.bincount(lab64, weights=d * d, minlength=n_labels)
    else:
        total = torch.zeros(n_labels, dtype=torch.float64, device=v.device).scatter_reduce(0, lab64, d, "sum")
        squares = torch.zeros(n_labels, dtype=torch.float64, device=v.device).scatter_reduce(0, lab64, d * d, "sum")
    n_nan = torch.bincount(lab64, weights=nan.double(), minlength=n_labels)
    count = torch.bincount(lab64, minlength=n_labels) - n_nan.long()
    lo = torch.full((n_labels,), float("inf"), device=v.device).scatter_reduce(0, lab64, v, "amin")
    hi = torch.full((n_labels,), float("-inf"), device=v.device).scatter_reduce(0, lab64, v, "amax")
    return [t.cpu().numpy() for t in (count, n_nan, total, squares, lo, hi)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def race(sides):
    """name -> [median, smallest, largest in ms, timed calls]; one call of every side in turn per repetition.  A side
    whose warm-up call takes longer than SLOW_MS (torch's scatter into a handful of labels takes seconds) is timed
    SLOW_REPS times instead of `reps`."""
    left = {}
    for name, fn in sides.items():  # warm-up: code objects, allocator, plan tables
        slow = timed(fn) > SLOW_MS
        for _ in range(0 if slow else 2):
            fn()
        left[name] = SLOW_REPS if slow else reps
    times = {name: [] for name in sides}
    while any(left.values()):
        for name, fn in sides.items():
            if left[name]:
                times[name].append(timed(fn))
                left[name] -= 1
    return {name: [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4), len(t)] for name, t in times.items()}


for case in which:
    obj = make(case)
    shape = tuple(obj._shape)
    for layout, (lab, n_labels) in label_volumes(shape).items():
        on_device = torch.from_numpy(lab).to(DEV)           # the input of the route from the cores, in its own type
        lab64 = on_device.reshape(-1).long()                # the input torch's bincount and scatter_reduce take
        sides = {
            "cores": lambda: obj.label_stats(on_device, n_labels),
            "decode_bincount": lambda: decoded(obj, lab64, n_labels, "bincount"),
            "decode_scatter": lambda: decoded(obj, lab64, n_labels, "scatter"),
        }
        out = {"case": case, "layout": layout, "shape": list(shape), "bonds_max": max(obj.mps.bonds), "n_labels": n_labels,
               "reps": reps, "device": torch.cuda.get_device_name(0)}
        got = obj.label_stats(on_device, n_labels)
        again = obj.label_stats(on_device, n_labels)
        out["cores_same_bits"] = all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got)
        ref, other = decoded(obj, lab64, n_labels, "bincount"), decoded(obj, lab64, n_labels, "bincount")
        out["decode_same_bits"] = all(x.tobytes() == y.tobytes() for x, y in zip(ref, other))
        out["counts_equal"] = bool(np.array_equal(got["count"], ref[0]))
        out["sum_rel_diff"] = float(np.nanmax(np.abs(got["sum"] - ref[2]) / np.maximum(np.abs(ref[2]), 1e-300)))
        out["ms_median_min_max_calls"] = race(sides)
        out["peak_bytes"] = {name: peak_above(fn) for name, fn in sides.items()}
        print(json.dumps(out), flush=True)
        if layout == "grid126":
            frames = [obj] * FRAMES
            series = {
                "cores": lambda: NDMPS.label_stats_many(frames, on_device, n_labels),
                "decode_bincount": lambda: [decoded(o, lab64, n_labels, "bincount") for o in frames],
            }
            print(json.dumps({"case": case, "layout": f"{layout} x {FRAMES} frames", "ms_median_min_max_calls": race(series),
                              "peak_bytes": {name: peak_above(fn) for name, fn in series.items()}}), flush=True)
        del on_device, lab64
    del obj
    torch.cuda.empty_cache()
