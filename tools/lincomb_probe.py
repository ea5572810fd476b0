"""Linear combination and recompression on the cores against the dense path, on 256^3 chi=64 fp32 objects.

* mean8: the mean of 8 volumes.  NDMPS.linear_combination(max_bond=64) against decoding all 8 volumes, torch.mean
  and from_tensor(max_bond=64).  Wall time, allocator peak above the inputs, and the error against the exact dense
  mean of the 8 objects' to_tensor().
* reduce: one object reduced to chi=32.  recompress(max_bond=32), a copy's compress(0, max_bond=32) and
  from_tensor(x, max_bond=32) on the volume x the object was made from; time and error against x.
Warm-up, then the median of REPS timed calls each, each ended by a device synchronise.
usage: python tools/lincomb_probe.py [reps] [case ...]   (cases: mean8, reduce; default both)"""
import copy
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
which = sys.argv[2:] or ["mean8", "reduce"]
DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, fn, ref, extra):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms, out = timed(fn)
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    times = [ms] + [timed(fn)[0] for _ in range(reps - 1)]
    rec = out.to_tensor(as_torch=True).double()
    err = (torch.linalg.norm(rec - ref) / torch.linalg.norm(ref)).item()
    print(json.dumps(dict(extra, case=name, median_ms=round(statistics.median(times), 3), peak_mib=round(peak, 2),
                          rel_err=float(f"{err:.3e}"), bonds=out.bond_sizes())), flush=True)


if "mean8" in which:
    objs = [NDMPS.from_tensor(synthetic_mri((256,) * 3, seed=40 + s), max_bond=64, device=DEV) for s in range(8)]
    exact = sum(o.to_tensor(as_torch=True).double() for o in objs) / 8
    torch.cuda.empty_cache()

    def dense_path():
        vols = torch.stack([o.to_tensor(as_torch=True) for o in objs])
        return NDMPS.from_tensor(torch.mean(vols, dim=0), max_bond=64, device=DEV)

    run("lincomb", lambda: NDMPS.linear_combination(objs, [1 / 8] * 8, max_bond=64), exact, {"workload": "mean8"})
    run("dense", dense_path, exact, {"workload": "mean8"})
    del objs, exact
    torch.cuda.empty_cache()

if "reduce" in which:
    x = synthetic_mri((256,) * 3, seed=41)
    xt = torch.from_numpy(x).to(DEV).double()
    obj = NDMPS.from_tensor(x, max_bond=64, device=DEV)

    def via_compress():
        c = copy.deepcopy(obj)
        c.compress(0, max_bond=32)
        return c

    run("recompress", lambda: obj.recompress(max_bond=32), xt, {"workload": "reduce"})
    run("compress", via_compress, xt, {"workload": "reduce"})
    run("from_tensor", lambda: NDMPS.from_tensor(x, max_bond=32, device=DEV), xt, {"workload": "reduce"})
