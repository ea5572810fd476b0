"""The elementwise product on the cores against the dense path, on two 256^3 chi=64 fp32 objects.

* cores: ``a.multiply(b, max_bond=64)`` (sketch bond 128).
* dense: two ``to_tensor``, a torch product and ``from_tensor(max_bond=64)``.
Per path: the median wall time of REPS calls after a warm-up, each ended by a device synchronise; the allocator peak
above the inputs; the error of the result's ``to_tensor`` against the exact product of the two objects' own
``to_tensor`` (fp64), relative in the Frobenius norm; the result's bonds.  The sketch's workspace by the layout's
formula is printed first.
usage: python tools/hadamard_probe.py [reps] [n]   (n: edge of the cube, default 256)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import hadamard as hd  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
DEV = "cuda:0"
CHI = 64


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, fn, ref):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms, out = timed(fn)
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    times = [ms] + [timed(fn)[0] for _ in range(reps - 1)]
    rec = out.to_tensor(as_torch=True).double()
    err = (torch.linalg.norm(rec - ref) / torch.linalg.norm(ref)).item()
    print(json.dumps(dict(workload="multiply", case=name, median_ms=round(statistics.median(times), 3),
                          peak_mib=round(peak, 2), rel_err=float(f"{err:.3e}"), bonds=out.bond_sizes())), flush=True)


a = NDMPS.from_tensor(synthetic_mri((n,) * 3, seed=41), max_bond=CHI, device=DEV)
b = NDMPS.from_tensor(synthetic_mri((n,) * 3, seed=42), max_bond=CHI, device=DEV)
exact = a.to_tensor(as_torch=True).double() * b.to_tensor(as_torch=True).double()

dims = a.mps.dims
ell = hd.sketch_bonds(dims, a.mps.bonds, b.mps.bonds, CHI, CHI)
ws = C.c_int64(0)
total = _lib.load().ndmps_hadamard_layout(len(dims), _lib.i64_array(dims), _lib.i64_array(a.mps.bonds), _lib.i64_array(b.mps.bonds),
                                          _lib.i64_array(ell), None, C.byref(ws))
print(json.dumps(dict(workload="multiply", sketch_bonds=ell, arena_mib=round(total * 8 / 2**20, 2),
                      workspace_mib=round(ws.value / 2**20, 2))), flush=True)

run("cores", lambda: a.multiply(b, max_bond=CHI), exact)
run("dense", lambda: NDMPS.from_tensor(a.to_tensor(as_torch=True) * b.to_tensor(as_torch=True), max_bond=CHI, device=DEV), exact)
