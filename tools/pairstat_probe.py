"""Statistics of two objects from the cores against decode-both-then-reduce: pair_stats, joint_histogram(64),
joint_histogram(128) and mutual_information(64) on two 256^3 chi=64 fp32 objects (a phantom and a nonlinear intensity
map of it) and on 64^3 chi=16, each against two to_tensor(as_torch=True) calls followed by torch (sums and extremes;
bucketize + bincount for the histogram; the same host formula for the mutual information).  Warm-up, then the median
of REPS timed calls each, the two sides of a pair interleaved, each call ended by a device synchronise; the times are
whole calls (host planning, launches, the read-back).  Memory: torch.cuda.max_memory_allocated during one call above
what was allocated before it (the cores are inputs).  Prints one JSON line per case.
usage: python tools/pairstat_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import pairstat as ps  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "small"]
assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to time without one"


def make(case):
    """Two objects of one shape: two modalities of one anatomy."""
    side, bond = (64, 16) if case == "small" else (256, 64)
    x = synthetic_mri((side,) * 3, seed=31)
    u = (x - x.min()) / (x.max() - x.min())
    y = (0.2 + np.sin(np.pi * u) ** 2 + 0.3 * u).astype(x.dtype)
    return (NDMPS.from_tensor(x, max_bond=bond, device="cuda:0"), NDMPS.from_tensor(y, max_bond=bond, device="cuda:0"))


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
    a, b = make(case)
    sa, sb = a.value_stats(), b.value_stats()
    ranges = ((sa["min"], sa["max"]), (sb["min"], sb["max"]))

    def decoded_stats():
        va, vb = a.to_tensor(as_torch=True).double().reshape(-1), b.to_tensor(as_torch=True).double().reshape(-1)
        d = va - vb
        return torch.stack([va.sum(), vb.sum(), (va * va).sum(), (vb * vb).sum(), (va * vb).sum(), (d * d).sum(), d.abs().max(),
                            va.min(), va.max(), vb.min(), vb.max()]).cpu()

    def decoded_joint(bins):
        va, vb = a.to_tensor(as_torch=True).reshape(-1), b.to_tensor(as_torch=True).reshape(-1)
        ea = torch.linspace(ranges[0][0], ranges[0][1], bins + 1, device=va.device)
        eb = torch.linspace(ranges[1][0], ranges[1][1], bins + 1, device=va.device)
        ia = (torch.bucketize(va, ea, right=True) - 1).clamp_(0, bins - 1)  # the closed last bin; nothing lies outside
        ib = (torch.bucketize(vb, eb, right=True) - 1).clamp_(0, bins - 1)
        return torch.bincount(ia * bins + ib, minlength=bins * bins).reshape(bins, bins).cpu().numpy()

    pairs = {
        "pair_stats": (lambda: a.pair_stats(b), decoded_stats),
        "joint_histogram64": (lambda: a.joint_histogram(b, 64, range=ranges), lambda: decoded_joint(64)),
        "joint_histogram128": (lambda: a.joint_histogram(b, 128, range=ranges), lambda: decoded_joint(128)),
        "mutual_information64": (lambda: a.mutual_information(b, 64, range=ranges),
                                 lambda: ps.mutual_information_from_counts(decoded_joint(64))),
    }
    for cores_fn, decode_fn in pairs.values():  # warm-up: code objects, allocator, plan tables
        for _ in range(3):
            cores_fn()
            decode_fn()
    out = {"case": case, "shape": list(a._shape), "bonds_max": [max(a.mps.bonds), max(b.mps.bonds)], "reps": reps,
           "device": torch.cuda.get_device_name(0)}
    # agreement at the size that is timed (reported, not asserted): cells differ only where a voxel sits within the
    # decode's rounding of an edge
    counts = a.joint_histogram(b, 64, range=ranges)[0]
    ref = decoded_joint(64)
    out["hist64_cells_differing"] = int((counts != ref).sum())
    out["hist64_voxels_moved"] = int(np.abs(counts - ref).sum() // 2)
    out["mi64"] = [a.mutual_information(b, 64, range=ranges), ps.mutual_information_from_counts(ref)]
    st = a.pair_stats(b)
    out["pearson"], out["max_abs_diff"] = st["pearson"], st["max_abs_diff"]
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
    del a, b
    torch.cuda.empty_cache()
