"""Value statistics from the cores against decode-then-reduce: value_stats, histogram(256), histogram(4096) and
error_to on 256^3 chi=64 fp32, on the same volume thresholded so that most voxels are exactly zero (LDS-atomic
contention in the histogram) and on one small case (64^3 chi=16), each against to_tensor(as_torch=True) followed by
torch.aminmax / torch.histc / compute_psnr.  Warm-up, then the median of REPS timed calls each, the two sides of a
pair interleaved, each call ended by a device synchronise; the times are whole calls (host planning, launches, the
read-back).  Memory: torch.cuda.max_memory_allocated during one call above what was allocated before it (the cores
and the original are inputs).  Prints one JSON line per case.
usage: python tools/valstat_probe.py [reps] [case ...]   (cases: cube, zeros, small; default all)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.utils.metrics import compute_psnr  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "zeros", "small"]
assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to time without one"


def make(case):
    """(object, original on the device)."""
    if case == "small":
        x = synthetic_mri((64,) * 3, seed=31)
        return NDMPS.from_tensor(x, max_bond=16, device="cuda:0"), torch.from_numpy(x).to("cuda:0")
    x = synthetic_mri((256,) * 3, seed=31)
    obj = NDMPS.from_tensor(x, max_bond=64, device="cuda:0")
    if case == "zeros":
        # the decoded volume of a chain is never exactly zero over a region; a product chain is: the volume times a mask
        # of its first axis (bond 1), as chain[0] scaled per physical index, zeroes 7/8 of the voxels exactly
        core = obj.mps.cores[0]
        keep = torch.zeros(core.shape[1], device=core.device)
        keep[: max(core.shape[1] // 8, 1)] = 1
        core.mul_(keep[None, :, None])
    return obj, torch.from_numpy(x).to("cuda:0")


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


for case in which:
    obj, x = make(case)
    st = obj.value_stats()
    lo, hi = st["min"], st["max"]

    def decoded_histc(bins):
        v = obj.to_tensor(as_torch=True)
        return torch.histc(v, bins=bins, min=lo, max=hi)

    pairs = {
        "value_stats": (lambda: obj.value_stats(), lambda: torch.aminmax(obj.to_tensor(as_torch=True))),
        "histogram256": (lambda: obj.histogram(256, range=(lo, hi)), lambda: decoded_histc(256).cpu()),
        "histogram4096": (lambda: obj.histogram(4096, range=(lo, hi)), lambda: decoded_histc(4096).cpu()),
        "error_to": (lambda: obj.error_to(x), lambda: compute_psnr(x, obj.to_tensor(as_torch=True))),
    }
    for a, b in pairs.values():  # warm-up: code objects, allocator, plan tables
        for _ in range(3):
            a()
            b()
    out = {"case": case, "shape": list(x.shape), "bonds_max": max(obj.mps.bonds), "reps": reps,
           "zero_share": float((obj.to_tensor(as_torch=True) == 0).float().mean()),
           "device": torch.cuda.get_device_name(0)}
    # agreement at the size that is timed: the counts of the two histograms differ only where a voxel sits within the
    # decode's rounding of an edge (reported, not asserted), the moments and the PSNR to the last digits
    counts, _ = obj.histogram(256, range=(lo, hi))
    ref = decoded_histc(256).cpu().numpy().astype(np.int64)
    out["hist256_counts_moved"] = int(np.abs(np.cumsum(counts) - np.cumsum(ref)).max())
    mn, mx = (float(v) for v in torch.aminmax(obj.to_tensor(as_torch=True)))
    out["minmax_abs_diff"] = max(abs(mn - lo), abs(mx - hi))
    out["psnr_diff_db"] = abs(obj.psnr_to(x) - compute_psnr(x, obj.to_tensor(as_torch=True)))
    for name, (cores_fn, decode_fn) in pairs.items():
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(cores_fn))
            tb.append(timed(decode_fn))
        out[name] = {
            "cores_ms": round(statistics.median(ta), 4), "cores_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
            "decode_ms": round(statistics.median(tb), 4), "decode_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
            "cores_peak_bytes": peak_above(cores_fn), "decode_peak_bytes": peak_above(decode_fn),
        }
    print(json.dumps(out), flush=True)
    del obj, x
    torch.cuda.empty_cache()
