"""Extremes along axes from the cores against decode-then-reduce: amax(0), amax(2), amax((0, 1)), argmax(0,
return_values=True) and argmax() on 256^3 chi=64 and 64^3 chi=16, fp32, each against to_tensor(as_torch=True) followed
by torch.amax / torch.max(dim) / torch.argmax.  Warm-up, then the median of REPS timed calls each, the two sides of a
pair alternating, each call ended by a device synchronise; the times are whole calls (host planning, launches, and for
argmax() the read-back).  Both sides leave their result on the device.  Memory: torch.cuda.max_memory_allocated during
one call above what was allocated before it (the cores and the plan's tables are inputs).  Prints one JSON line per
case.
usage: python tools/axisext_probe.py [reps] [case ...]   (cases: cube, small; default both)"""
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


for case in which:
    shape, chi = CASES[case]
    x = synthetic_mri(shape, seed=31)
    obj = NDMPS.from_tensor(x, max_bond=chi, device="cuda:0")
    del x

    def decoded():
        return obj.to_tensor(as_torch=True)

    pairs = {
        "amax(0)": (lambda: obj.amax(0, as_torch=True), lambda: torch.amax(decoded(), 0)),
        "amax(2)": (lambda: obj.amax(2, as_torch=True), lambda: torch.amax(decoded(), 2)),
        "amax((0,1))": (lambda: obj.amax((0, 1), as_torch=True), lambda: torch.amax(decoded(), (0, 1))),
        "argmax(0,values)": (lambda: obj.argmax(0, as_torch=True, return_values=True), lambda: torch.max(decoded(), 0)),
        "argmax()": (lambda: obj.argmax(), lambda: int(torch.argmax(decoded()))),
    }
    for a, b in pairs.values():  # warm-up: code objects, allocator, plan tables
        for _ in range(3):
            a()
            b()
    out = {"case": case, "shape": list(shape), "bonds_max": max(obj.mps.bonds), "reps": reps,
           "volume_bytes": 4 * shape[0] * shape[1] * shape[2], "device": torch.cuda.get_device_name(0)}
    # agreement at the size that is timed (reported, not asserted): the two sides contract the chain with different
    # last products, so values differ by the decode's rounding and an index may move where two voxels nearly tie
    v = decoded()
    out["amax0_abs_diff"] = float((obj.amax(0, as_torch=True) - torch.amax(v, 0)).abs().max())
    where, _ = obj.argmax(0, as_torch=True, return_values=True)
    out["argmax0_indices_moved"] = int((where != torch.max(v, 0).indices).sum())
    out["argmax_flat_same"] = bool(obj.argmax() == int(torch.argmax(v)))
    del v, where
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
    del obj
    torch.cuda.empty_cache()
