"""Histograms and medians per label from the cores against decode-then-torch: on 256^3 chi=64 and 64^3 chi=16, fp32,
label_histogram at 126 parcels x 64 bins (a grid of 5^3 + 1, uint8) and at 1001 parcels x 256 bins (10^3 + 1, int16),
label_median at the 126 parcels, and median(mask=box).  The other side is to_tensor(as_torch=True) followed by torch:
the histogram by torch.bincount of label * bins + bin (the bin from torch.bucketize against the same edges, the last
bin closed on the right, voxels outside the range dropped), the medians by one sort of (label, value) pairs and a
gather at each label's rank, the masked median by torch.quantile's sort of the masked voxels (a kthvalue), read back to
the host.  Warm-up, then the median of REPS timed calls each (of 3 for a side whose call takes longer than 50 ms), the
sides interleaved, each call ended by a device synchronise; the times are whole calls (host planning, launches, the
read-back; the labels are on the device).  Memory: torch.cuda.max_memory_allocated during one call above what was
allocated before it (the cores and the label volume are inputs).  Prints one JSON line per case and measurement, with
the number of launches a call of the route from the cores makes.
usage: python tools/labelhist_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import labelhist as lh  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "small"]
assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to time without one"
DEV = "cuda:0"
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


def decoded_histogram(obj, lab64, n_labels, edges):
    """(n_labels, bins) counts from the decoded volume: bucketize against the edges, bincount of label * bins + bin."""
    v = obj.to_tensor(as_torch=True).reshape(-1)
    bins = edges.numel() - 1
    b = torch.bucketize(v, edges, right=True) - 1
    b = torch.where(v == edges[-1], torch.full_like(b, bins - 1), b)
    ok = (b >= 0) & (b < bins)  # NaN lands beyond the last edge and is dropped with the voxels out of range
    cells = torch.bincount(lab64[ok] * bins + b[ok], minlength=n_labels * bins)
    return cells.reshape(n_labels, bins).cpu().numpy()


def decoded_medians(obj, lab64, n_labels):
    """The voxel of rank ceil(n / 2) of every label from the decoded volume: a sort by value, a stable sort by label."""
    v = obj.to_tensor(as_torch=True).reshape(-1)
    v, order = torch.sort(v)
    lab, order = torch.sort(lab64[order], stable=True)
    v = v[order]
    n = torch.bincount(lab, minlength=n_labels)
    start = torch.cumsum(n, 0) - n
    k = torch.clamp(torch.ceil(n.double() * 0.5 - 1).long(), min=0)
    out = torch.where(n > 0, v[torch.clamp(start + k, max=v.numel() - 1)], torch.full_like(v[:1], float("nan")))
    return out.cpu().numpy()


def decoded_masked_median(obj, mask):
    v = obj.to_tensor(as_torch=True)[mask]
    k = max(int(np.ceil(v.numel() * 0.5 - 1)), 0) + 1
    return float(torch.kthvalue(v, k).values)


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


def report(out, sides):
    out["ms_median_min_max_calls"] = race(sides)
    out["peak_bytes"] = {name: peak_above(fn) for name, fn in sides.items()}
    print(json.dumps(out), flush=True)


for case in which:
    obj = make(case)
    shape = tuple(obj._shape)
    head = {"case": case, "shape": list(shape), "bonds_max": max(obj.mps.bonds), "reps": reps,
            "device": torch.cuda.get_device_name(0)}
    lo, hi = obj.min(), obj.max()
    for name, g, dtype, bins in (("grid126", 5, np.uint8, 64), ("grid1001", 10, np.int16, 256)):
        n_labels = g ** 3 + 1
        on_device = torch.from_numpy(grid_labels(shape, g).astype(dtype)).to(DEV)
        lab64 = on_device.reshape(-1).long()
        counts, edges = obj.label_histogram(on_device, n_labels, bins, (lo, hi))
        edges_dev = torch.from_numpy(edges).to(DEV)
        ref = decoded_histogram(obj, lab64, n_labels, edges_dev)
        out = dict(head, what=f"label_histogram {name} x {bins} bins", n_labels=n_labels, bins=bins,
                   launches=lh.plan_query(np.float32, n_labels, bins, False)["launches"],
                   same_bits=bool(np.array_equal(obj.label_histogram(on_device, n_labels, bins, (lo, hi))[0], counts)),
                   cells_that_differ_from_decode=int((counts != ref).sum()), voxels=int(counts.sum()))
        report(out, {"cores": lambda: obj.label_histogram(on_device, n_labels, bins, (lo, hi)),
                     "decode_bincount": lambda: decoded_histogram(obj, lab64, n_labels, edges_dev)})
        if name == "grid126":
            got = obj.label_quantile(on_device, 0.5, n_labels)
            ref = decoded_medians(obj, lab64, n_labels)
            plan = lh.plan_query(np.float32, n_labels, 64, True)
            out = dict(head, what=f"label_median {name}", n_labels=n_labels, passes=2, bins=64,
                       launches=1 + 2 * plan["launches"] + lh.plan_query(np.float32, n_labels, 1, True)["launches"],
                       max_bracket=float(np.nanmax(got["hi"] - got["lo"])),
                       max_diff_from_decode=float(np.nanmax(np.abs(got["value"] - ref))))
            report(out, {"cores": lambda: obj.label_median(on_device, n_labels),
                         "decode_sort": lambda: decoded_medians(obj, lab64, n_labels)})
        del on_device, lab64
    box = torch.zeros(shape, dtype=torch.bool, device=DEV)
    box[tuple(slice(s // 4, 3 * s // 4) for s in shape)] = True
    value, bracket = obj.quantile(0.5, mask=box)
    out = dict(head, what="median(mask=box)", inside=int(box.sum()), bracket=[bracket[0], bracket[1]],
               diff_from_decode=abs(value - decoded_masked_median(obj, box)))
    report(out, {"cores": lambda: obj.median(mask=box), "decode_kthvalue": lambda: decoded_masked_median(obj, box)})
    del obj, box
    torch.cuda.empty_cache()
