"""Gram matrix of a series on the cores against the pair loop and the dense path, on 256^3 chi=64 fp32 objects.

For K = 8 and K = 64 frames (random mixtures of 8 synthetic_mri volumes plus noise, from_tensors(max_bond=64)):
* gram : NDMPS.gram(objs) (csrc/series.hip, one launch);
* loop : [[a.mps @ b.mps for b in objs[i:]] for i, a in enumerate(objs)], the only route before NDMPS.gram;
* dense: decode every frame, flatten, X @ X.T in fp64 with torch.
Wall time (warm-up, then the median of REPS timed calls, each ended by a device synchronise; the loop is timed at most
three times), allocator peak above the inputs, and max |gram - loop| / sqrt(G_aa G_bb).
usage: python tools/series_probe.py [reps] [case ...]   (cases: k8, k64, trace64 -- one gram call at K = 64 and nothing
else, for `rocprofv3 --kernel-trace --stats -- python tools/series_probe.py 1 trace64`)"""
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
which = sys.argv[2:] or ["k8", "k64"]
DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(name, fn, n, extra):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms, out = timed(fn)
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    times = [ms] + [timed(fn)[0] for _ in range(n - 1)]
    print(json.dumps(dict(extra, case=name, median_ms=round(statistics.median(times), 3), reps=n,
                          peak_mib=round(peak, 2))), flush=True)
    return np.asarray(out, dtype=np.float64)


def series(K):
    gen = torch.Generator(device=DEV).manual_seed(K)
    base = torch.stack([torch.from_numpy(synthetic_mri((256,) * 3, seed=60 + s)).to(DEV) for s in range(8)])
    frames = []
    for k in range(K):
        w = torch.rand(8, generator=gen, device=DEV) - 0.3
        frames.append(torch.tensordot(w, base, dims=1) + 1e-3 * torch.randn((256,) * 3, generator=gen, device=DEV))
    del base
    objs = []
    for k0 in range(0, K, 8):
        objs += NDMPS.from_tensors(frames[k0:k0 + 8], max_bond=64, device=DEV)
    del frames
    torch.cuda.empty_cache()
    return objs


def loop(objs):
    K = len(objs)
    G = np.zeros((K, K))
    for i, a in enumerate(objs):
        for j in range(i, K):
            G[i, j] = G[j, i] = a.mps @ objs[j].mps
    return G


def dense(objs):
    X = torch.stack([o.to_tensor(as_torch=True).reshape(-1) for o in objs]).double()
    return (X @ X.T).cpu().numpy()


for case in which:
    K = {"k8": 8, "k64": 64, "trace64": 64}[case]
    objs = series(K)
    extra = {"K": K, "bonds": objs[0].bond_sizes(), "route": NDMPS.gram_route(objs)}
    if case == "trace64":
        NDMPS.gram(objs)
        torch.cuda.synchronize()
        continue
    G = run("gram", lambda: NDMPS.gram(objs), reps, extra)
    Gl = run("loop", lambda: loop(objs), min(reps, 3), extra)
    Gd = run("dense", lambda: dense(objs), min(reps, 3), extra)
    nrm = np.sqrt(np.outer(np.diag(Gl), np.diag(Gl)))
    print(json.dumps(dict(extra, case="agreement", gram_vs_loop=float(f"{np.max(np.abs(G - Gl) / nrm):.3e}"),
                          gram_vs_dense=float(f"{np.max(np.abs(G - Gd) / nrm):.3e}"))), flush=True)
    del objs
    torch.cuda.empty_cache()
