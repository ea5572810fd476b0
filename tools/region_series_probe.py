"""Region decode of a series against the loop over its frames: T frames of one 256^3 chi=64 fp32 series, T = 8 and
T = 64 (four encoded volumes and their rescaled copies); one axial slice, one 32^3 block and 1000 random points, by the loop over decode_region / values_at and by
decode_regions / values_at_many.  Warm-up, then REPS interleaved reps of every case, each ended by a device
synchronise; the median is reported.  The times include the host planner and the uploads of both paths.
usage: python tools/region_series_probe.py [reps] [edge] [chi]"""
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
T_MAX = 64
# a series: four encoded volumes, the later frames their rescaled copies (same bonds, other values: cheap to build)
seeds = NDMPS.from_tensors([synthetic_mri((edge,) * 3, seed=31 + t) for t in range(4)], max_bond=chi, device="cuda:0")
frames = [seeds[t % 4] * (1.0 + 0.01 * (t // 4)) for t in range(T_MAX)]
rng = np.random.default_rng(0)
points = np.stack([rng.integers(0, edge, 1000) for _ in range(3)], axis=1)
b0 = edge // 3
slice_key, block_key = (edge // 2,), (slice(b0, b0 + 32),) * 3
cases = {}
for T in (8, T_MAX):
    objs = frames[:T]
    cases[f"axial_slice/T{T}/loop"] = lambda objs=objs: [o.decode_region(slice_key, as_torch=True) for o in objs]
    cases[f"axial_slice/T{T}/series"] = lambda objs=objs: NDMPS.decode_regions(objs, slice_key, as_torch=True)
    cases[f"block_32/T{T}/loop"] = lambda objs=objs: [o.decode_region(block_key, as_torch=True) for o in objs]
    cases[f"block_32/T{T}/series"] = lambda objs=objs: NDMPS.decode_regions(objs, block_key, as_torch=True)
    cases[f"points_1000/T{T}/loop"] = lambda objs=objs: [o.values_at(points, as_torch=True) for o in objs]
    cases[f"points_1000/T{T}/series"] = lambda objs=objs: NDMPS.values_at_many(objs, points, as_torch=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for fn in cases.values():  # warm-up: code objects, allocator
    for _ in range(2):
        fn()
same = {name[:-7]: bool(torch.equal(torch.stack(cases[name[:-7] + "/loop"]()), cases[name]()))
        for name in cases if name.endswith("/series")}
times = {name: [] for name in cases}
for _ in range(reps):  # interleaved, so drift on a shared host touches every case alike
    for name, fn in cases.items():
        times[name].append(timed(fn))
med = {k: statistics.median(v) for k, v in times.items()}
for name in cases:
    if name.endswith("/series"):
        loop = name[:-7] + "/loop"
        print(f"{name[:-7]:20s} loop {med[loop]:8.3f} ms  series {med[name]:8.3f} ms (min {min(times[name]):8.3f}, "
              f"max {max(times[name]):8.3f})  series / loop {med[name] / med[loop]:6.3f}  bit-equal {same[name[:-7]]}")
print(json.dumps({"edge": edge, "chi": chi, "reps": reps,
                  "bonds": sorted({tuple(o.bond_sizes()) for o in frames}),
                  "median_ms": {k: round(v, 4) for k, v in med.items()},
                  "series_over_loop": {k[:-7]: round(med[k] / med[k[:-7] + "/loop"], 4)
                                       for k in med if k.endswith("/series")},
                  "bit_equal": same}))
