"""Voxels by value from the cores against decode-then-select: find at selections of about 1e-5, 1e-3 and 1e-1 of the
voxels (thresholds from quantile), find_nan on a volume with a NaN planted in one core entry, and topk(100), on 256^3
chi=64 and 64^3 chi=16, fp32, each against to_tensor(as_torch=True) followed by torch.nonzero and a gather, or
torch.topk.  Warm-up, then the median of REPS timed calls each, the two sides of a pair alternating, each call ended by
a device synchronise; the times are whole calls (the counting pass, the list pass, the sort of the pairs and the
read-backs of the counts on the one side, the decode and the selection on the other).  Both sides leave their result
on the device.  Memory: torch.cuda.max_memory_allocated during one call above what was allocated before it (the cores
and the plan's tables are inputs).  A NaN in a core entry reaches every voxel that shares the entry, so the planted
volume has numel / d_0 NaN voxels: fewer cannot be planted through the cores.  Prints one JSON line per case.
usage: python tools/select_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import valstat  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "small"]
assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to time without one"
CASES = {"cube": ((256,) * 3, 64), "small": ((64,) * 3, 16)}


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


def decode_find(obj, lo):
    v = obj.to_tensor(as_torch=True).reshape(-1)
    index = torch.nonzero(v >= lo).squeeze(1)
    return index, v[index]


def decode_nan(obj):
    return torch.nonzero(torch.isnan(obj.to_tensor(as_torch=True).reshape(-1))).squeeze(1)


def decode_topk(obj, k):
    values, index = torch.topk(obj.to_tensor(as_torch=True).reshape(-1), k)
    return index, values


for case in which:
    shape, chi = CASES[case]
    numel = shape[0] * shape[1] * shape[2]
    x = synthetic_mri(shape, seed=31)
    obj = NDMPS.from_tensor(x, max_bond=chi, device="cuda:0")
    holed = NDMPS.from_tensor(x, max_bond=chi, device="cuda:0")
    holed.mps.cores[0][0, 0, 0] = float("nan")
    del x
    thresholds = {share: obj.quantile(1.0 - share)[0] for share in (1e-5, 1e-3, 1e-1)}

    pairs = {f"find({share:g})": (lambda lo=lo: obj.find(lo, max_count=numel, as_torch=True), lambda lo=lo: decode_find(obj, lo))
             for share, lo in thresholds.items()}
    pairs["find_nan"] = (lambda: holed.find_nan(max_count=numel), lambda: decode_nan(holed).cpu())
    pairs["topk(100)"] = (lambda: obj.topk(100, as_torch=True), lambda: decode_topk(obj, 100))
    for a, b in pairs.values():  # warm-up: code objects, allocator, plan tables
        for _ in range(3):
            a()
            b()
    out = {"case": case, "shape": list(shape), "bonds_max": max(obj.mps.bonds), "reps": reps, "volume_bytes": 4 * numel,
           "workspace_bytes": valstat.workspace_bytes(obj.mps), "device": torch.cuda.get_device_name(0)}
    # agreement at the size that is timed (reported, not asserted): the two sides contract the chain with different
    # last products, so a voxel within the decode's rounding of the threshold may be selected by one side only
    for share, lo in thresholds.items():
        mine, theirs = obj.find(lo, max_count=numel, as_torch=True)[0], decode_find(obj, lo)[0]
        both = torch.isin(mine, theirs).sum().item()
        out[f"find({share:g})_selected"] = [int(mine.numel()), int(theirs.numel()), int(mine.numel() + theirs.numel() - 2 * both)]
    out["find_nan_selected"] = [int(holed.find_nan(max_count=numel).size), int(decode_nan(holed).numel())]
    out["topk100_same_indices"] = bool(torch.equal(obj.topk(100, as_torch=True)[0], decode_topk(obj, 100)[0]))
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
    del obj, holed
    torch.cuda.empty_cache()
