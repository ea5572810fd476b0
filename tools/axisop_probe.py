"""Axis operators on the cores against the dense path, on one 256^3 chi=64 fp32 object.

* roll: ``roll(1, axis=0, max_bond=64)`` against ``to_tensor``, ``torch.roll`` and ``from_tensor(max_bond=64)``.
* stencil: ``correlate1d([1, -2, 1], axis=0, max_bond=64)`` against ``to_tensor``, the same stencil written with torch
  slices (zero outside the volume) and ``from_tensor(max_bond=64)``.
Per path: the median wall time of REPS calls after a warm-up, each ended by a device synchronise; the allocator peak
above the inputs; the error of the result's ``to_tensor`` against the exact operator result on the object's own
``to_tensor`` (fp64), relative in the Frobenius norm; the result's bonds.
usage: python tools/axisop_probe.py [reps] [case ...]   (cases: roll, stencil; default both)"""
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
which = sys.argv[2:] or ["roll", "stencil"]
DEV = "cuda:0"
W = [1.0, -2.0, 1.0]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(workload, name, fn, ref):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms, out = timed(fn)
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    times = [ms] + [timed(fn)[0] for _ in range(reps - 1)]
    rec = out.to_tensor(as_torch=True).double()
    err = (torch.linalg.norm(rec - ref) / torch.linalg.norm(ref)).item()
    print(json.dumps(dict(workload=workload, case=name, median_ms=round(statistics.median(times), 3),
                          peak_mib=round(peak, 2), rel_err=float(f"{err:.3e}"), bonds=out.bond_sizes())), flush=True)


def stencil_dense(x):
    """out[i] = x[i - 1] - 2 x[i] + x[i + 1] along axis 0, zero outside."""
    out = -2.0 * x
    out[1:] += x[:-1]
    out[:-1] += x[1:]
    return out


obj = NDMPS.from_tensor(synthetic_mri((256,) * 3, seed=41), max_bond=64, device=DEV)
dense = obj.to_tensor(as_torch=True).double()

if "roll" in which:
    exact = torch.roll(dense, 1, 0)
    run("roll", "cores", lambda: obj.roll(1, 0, max_bond=64), exact)
    run("roll", "dense", lambda: NDMPS.from_tensor(torch.roll(obj.to_tensor(as_torch=True), 1, 0), max_bond=64, device=DEV),
        exact)
    del exact

if "stencil" in which:
    exact = stencil_dense(dense)
    run("stencil", "cores", lambda: obj.correlate1d(W, 0, max_bond=64), exact)
    run("stencil", "dense", lambda: NDMPS.from_tensor(stencil_dense(obj.to_tensor(as_torch=True)), max_bond=64, device=DEV),
        exact)
