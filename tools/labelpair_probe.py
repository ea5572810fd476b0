"""Pair statistics per label from the cores against decode-then-scatter: label_pair_stats (two encodings of one scan,
chi and chi / 2), label_error_to (the encoding against the original on the device) and label_pair_stats_many (16
frames against one reference), on 256^3 chi=64 and 64^3 chi=16, fp32, under four label volumes (one label; a box mask,
2 labels; a grid of 5^3 + 1 parcels, uint8; of 10^3 + 1 parcels, int16).  The competitor decodes both objects with
to_tensor(as_torch=True) (for label_error_to: one object, the original is on the device already) and takes the same
numbers from torch: counts and the six sums by torch.bincount(weights=) in fp64, the NaN count by bincount, the five
extremes by scatter_reduce amin / amax, read back to the host.  Warm-up, then the median of REPS timed calls each (of 3
for a side whose call takes longer than 50 ms), the sides interleaved, each call ended by a device synchronise; the
times are whole calls (host planning, launches, the read-back; the labels are on the device).  Memory:
torch.cuda.max_memory_allocated during one call above what was allocated before it (the cores, the label volume and
the original are inputs).  Prints one JSON line per case, label volume and call.
usage: python tools/labelpair_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
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
    return x, NDMPS.from_tensor(x, max_bond=bond, device=DEV), NDMPS.from_tensor(x, max_bond=bond // 2, device=DEV)


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
    box = np.zeros(shape, dtype=np.uint8)
    box[tuple(slice(s // 4, 3 * s // 4) for s in shape)] = 1
    return {
        "one": (np.zeros(shape, dtype=np.uint8), 1),
        "box": (box, 2),
        "grid126": (grid_labels(shape, 5).astype(np.uint8), 126),
        "grid1001": (grid_labels(shape, 10).astype(np.int16), 1001),
    }


def scattered(va, vb, lab64, n_labels):
    """The numbers of label_pair_stats per label from two decoded volumes, on the host."""
    nan = torch.isnan(va) | torch.isnan(vb)
    zero = torch.zeros((), dtype=va.dtype, device=va.device)
    a, b = torch.where(nan, zero, va).double(), torch.where(nan, zero, vb).double()
    d = a - b
    out = [torch.bincount(lab64, weights=w, minlength=n_labels) for w in (a, b, a * b, a * a, b * b, d * d)]
    n_nan = torch.bincount(lab64, weights=nan.double(), minlength=n_labels)
    out += [torch.bincount(lab64, minlength=n_labels) - n_nan.long(), n_nan]
    inf = float("inf")
    keep = lambda v, fill: torch.where(nan, torch.full_like(v, fill), v)  # noqa: E731
    for v in (va, vb):
        out.append(torch.full((n_labels,), inf, dtype=v.dtype, device=v.device).scatter_reduce(0, lab64, keep(v, inf), "amin"))
        out.append(torch.full((n_labels,), -inf, dtype=v.dtype, device=v.device).scatter_reduce(0, lab64, keep(v, -inf), "amax"))
    out.append(torch.full((n_labels,), -inf, dtype=torch.float64, device=va.device).scatter_reduce(0, lab64, d.abs(), "amax"))
    return [t.cpu().numpy() for t in out]


def decoded_pair(a, b, lab64, n_labels):
    return scattered(a.to_tensor(as_torch=True).reshape(-1), b.to_tensor(as_torch=True).reshape(-1), lab64, n_labels)


def decoded_error(a, x_flat, lab64, n_labels):
    return scattered(a.to_tensor(as_torch=True).reshape(-1), x_flat, lab64, n_labels)


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
    whose warm-up call takes longer than SLOW_MS is timed SLOW_REPS times instead of `reps`."""
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


def report(head, sides):
    print(json.dumps(dict(head, ms_median_min_max_calls=race(sides),
                          peak_bytes={name: peak_above(fn) for name, fn in sides.items()})), flush=True)


for case in which:
    x, obj, coarse = make(case)
    shape = tuple(obj._shape)
    x_dev = torch.from_numpy(x).to(DEV)
    x_flat = x_dev.reshape(-1)
    for layout, (lab, n_labels) in label_volumes(shape).items():
        on_device = torch.from_numpy(lab).to(DEV)           # the input of the route from the cores, in its own type
        lab64 = on_device.reshape(-1).long()                # the input torch's bincount and scatter_reduce take
        head = {"case": case, "layout": layout, "shape": list(shape), "bonds_max": [max(obj.mps.bonds), max(coarse.mps.bonds)],
                "n_labels": n_labels, "reps": reps, "device": torch.cuda.get_device_name(0)}
        got, again = obj.label_pair_stats(coarse, on_device, n_labels), obj.label_pair_stats(coarse, on_device, n_labels)
        ref = decoded_pair(obj, coarse, lab64, n_labels)
        same = all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got if k != "scales")
        checks = {"cores_same_bits": same, "scales": got["scales"], "counts_equal": bool(np.array_equal(got["count"], ref[6])),
                  "sse_rel_diff": float(np.nanmax(np.abs(got["sse"] - ref[5]) / np.maximum(np.abs(ref[5]), 1e-300)))}
        report(dict(head, call="label_pair_stats", **checks), {
            "cores": lambda: obj.label_pair_stats(coarse, on_device, n_labels),
            "decode_both_scatter": lambda: decoded_pair(obj, coarse, lab64, n_labels),
        })
        err = obj.label_error_to(x_dev, on_device, n_labels)
        ref = decoded_error(obj, x_flat, lab64, n_labels)
        checks = {"counts_equal": bool(np.array_equal(err["count"], ref[6])), "psnr_first_labels": [float(v) for v in err["psnr"][:4]],
                  "psnr_global": float(obj.psnr_to(x_dev)),
                  "sse_rel_diff": float(np.nanmax(np.abs(err["sse"] - ref[5]) / np.maximum(np.abs(ref[5]), 1e-300)))}
        report(dict(head, call="label_error_to", **checks), {
            "cores": lambda: obj.label_error_to(x_dev, on_device, n_labels),
            "decode_scatter": lambda: decoded_error(obj, x_flat, lab64, n_labels),
        })
        if layout == "grid126":
            frames = [coarse] * FRAMES
            report(dict(head, call=f"label_pair_stats_many x {FRAMES} frames"), {
                "cores": lambda: NDMPS.label_pair_stats_many(frames, obj, on_device, n_labels),
                "decode_both_scatter": lambda: [decoded_pair(o, obj, lab64, n_labels) for o in frames],
            })
        del on_device, lab64
    del obj, coarse, x_dev, x_flat
    torch.cuda.empty_cache()
