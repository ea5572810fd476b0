"""Block-averaged decode against the full decode: downsample(1), downsample(2), mean() and mean(axis=0) against
to_tensor(as_torch=True) followed by the same torch reduction, on 256^3 chi=64 fp32 and on BASELINE config 5's
128x128x64x256 chi=128 stored as bf16.  Warm-up, then the median of REPS timed calls each, interleaved, each ended
by a device synchronise; the times include the host planner and the table upload.
usage: python tools/downsample_probe.py [reps] [case ...]   (cases: cube, config5; default both)"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2:] or ["cube", "config5"]


def smooth_4d(shape, seed=5):
    """A smooth nonnegative 4-D volume built on the device (separable bumps, a slow modulation along the last axis,
    1% noise): the host generator would take minutes at 0.5 G voxels."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ax = [torch.linspace(-1, 1, n, device="cuda") for n in shape[:3]]
    vol = torch.zeros(shape[:3], device="cuda")
    for _ in range(6):
        c = torch.rand(3, generator=gen, device="cuda") * 1.2 - 0.6
        w = torch.rand(3, generator=gen, device="cuda") * 0.35 + 0.1
        f = [torch.exp(-0.5 * ((a - c[i]) / w[i]) ** 2) for i, a in enumerate(ax)]
        vol += f[0][:, None, None] * f[1][None, :, None] * f[2][None, None, :]
    t = torch.linspace(0, 1, shape[3], device="cuda")
    vol = vol[..., None] * (1 + 0.25 * torch.sin(2 * torch.pi * 2 * t))
    vol += 0.01 * torch.randn(shape, generator=gen, device="cuda")
    vol -= vol.min()
    return vol / vol.max()


def make(case):
    if case == "cube":
        return NDMPS.from_tensor(synthetic_mri((256,) * 3, seed=31), max_bond=64, device="cuda:0")
    obj = NDMPS.from_tensor(smooth_4d((128, 128, 64, 256)), max_bond=128, device="cuda:0")
    torch.cuda.empty_cache()
    return obj.astype(torch.bfloat16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pooled(t, B):
    inter = [v for n, b in zip(t.shape, B) for v in (n // b, b)]
    return t.float().reshape(inter).mean(dim=tuple(range(1, 2 * t.dim(), 2)))


results = []
for case in which:
    obj = make(case)
    B1, B2 = obj.block_shape(1), obj.block_shape(2)
    cases = {
        "to_tensor": lambda: obj.to_tensor(as_torch=True),
        "downsample1": lambda: obj.downsample(1, as_torch=True),
        "full_then_pool1": lambda: pooled(obj.to_tensor(as_torch=True), B1),
        "downsample2": lambda: obj.downsample(2, as_torch=True),
        "full_then_pool2": lambda: pooled(obj.to_tensor(as_torch=True), B2),
        "mean": lambda: obj.mean(as_torch=True),
        "full_then_mean": lambda: obj.to_tensor(as_torch=True).float().mean(),
        "mean_axis0": lambda: obj.mean(axis=0, as_torch=True),
        "full_then_mean_axis0": lambda: obj.to_tensor(as_torch=True).float().mean(dim=0),
    }
    for fn in cases.values():  # warm-up: code objects, allocator, plan / basis caches
        for _ in range(3):
            fn()
    err = {}
    for a, b in (("downsample1", "full_then_pool1"), ("downsample2", "full_then_pool2"), ("mean", "full_then_mean"),
                 ("mean_axis0", "full_then_mean_axis0")):
        x, y = cases[a]().double(), cases[b]().double()
        err[a] = float((x - y).norm() / y.norm())
    times = {name: [] for name in cases}
    for _ in range(reps):  # interleaved, so drift on a shared host touches every case alike
        for name, fn in cases.items():
            times[name].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"--- {case}: bonds {obj.bond_sizes()} storage {obj.mps.dtype}")
    for name in cases:
        print(f"{name:22s} median {med[name]:8.3f} ms  min {min(times[name]):8.3f}  max {max(times[name]):8.3f}"
              + (f"  rel err vs full {err[name]:.1e}" if name in err else ""))
    results.append({"case": case, "bonds": obj.bond_sizes(), "reps": reps,
                    "median_ms": {k: round(v, 4) for k, v in med.items()}, "rel_err": err})
    del obj, cases
    torch.cuda.empty_cache()
print(json.dumps(results))
