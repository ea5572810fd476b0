"""Region decode against the full decode on one 256^3 chi=64 fp32 volume: one axial slice, one 32^3 block and 1000
random points (decode_region / values_at) against to_tensor.  Warm-up, then the median of REPS timed calls, each
ended by a device synchronise; the times include the host planner and the table upload.
usage: python tools/region_probe.py [reps] [edge] [chi]"""
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
edge = int(sys.argv[2]) if len(sys.argv) > 2 else 256
chi = int(sys.argv[3]) if len(sys.argv) > 3 else 64
obj = NDMPS.from_tensor(synthetic_mri((edge,) * 3, seed=31), max_bond=chi, device="cuda:0")
rng = np.random.default_rng(0)
points = np.stack([rng.integers(0, edge, 1000) for _ in range(3)], axis=1)
b0 = edge // 3
cases = {
    "to_tensor": lambda: obj.to_tensor(as_torch=True),
    "axial_slice": lambda: obj.decode_region((edge // 2,), as_torch=True),
    "block_32": lambda: obj.decode_region((slice(b0, b0 + 32),) * 3, as_torch=True),
    "points_1000": lambda: obj.values_at(points, as_torch=True),
}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for fn in cases.values():  # warm-up: code objects, allocator, DCT / plan caches
    for _ in range(3):
        fn()
full = obj.to_tensor(as_torch=True)
err = {
    "axial_slice": float((cases["axial_slice"]() - full[edge // 2]).norm() / full[edge // 2].norm()),
    "block_32": float((cases["block_32"]() - full[b0:b0 + 32, b0:b0 + 32, b0:b0 + 32]).norm()
                      / full[b0:b0 + 32, b0:b0 + 32, b0:b0 + 32].norm()),
}
ref_pts = full[tuple(torch.from_numpy(points.T).cuda())]
err["points_1000"] = float((cases["points_1000"]() - ref_pts).norm() / ref_pts.norm())
del full
times = {name: [] for name in cases}
for _ in range(reps):  # interleaved, so drift on a shared host touches every case alike
    for name, fn in cases.items():
        times[name].append(timed(fn))
med = {k: statistics.median(v) for k, v in times.items()}
for name in cases:
    speed = med["to_tensor"] / med[name]
    print(f"{name:12s} median {med[name]:8.3f} ms  min {min(times[name]):8.3f}  max {max(times[name]):8.3f}"
          f"  x{speed:6.1f} vs to_tensor" + (f"  rel err {err[name]:.1e}" if name in err else ""))
print(json.dumps({"edge": edge, "chi": chi, "bonds": obj.bond_sizes(), "reps": reps,
                  "median_ms": {k: round(v, 4) for k, v in med.items()}, "rel_err": err}))
