"""Digests of what the statistics family returns (core/valstat.py, axisext.py, labelstat.py, pairstat.py over
csrc/valstat.hip, axisext.hip, labelstat.hip, pairstat.hip) on the chains of the existing case tables, in fp32 and fp64.
One line per case, `name sha256(dtype, shape and raw bytes of every array, scalar and string a call returns)`; a refused
call hashes the type and the message of what it raises.  It hashes and does not judge: two builds compute the same
thing iff their lines agree, and a line that differs between two runs of ONE build says nothing.

The chains: every integer chain of tests/valstat_cases.py (rows and columns that are no multiples of 64, the 512 tiles
of int_8x7) and the 626-tile pair of tests/pairstat_cases.py (more tiles than workgroups), and real chains of one
site (the unit operand), with a k below and beside the k-tile, with a pre-contracted tail (a gathered right operand)
and without one (the column order read in the kernel).  NaN is planted where tests/valstat_cases.with_nan plants it.
usage: python tools/stat_digest.py [group ...]     (groups: value extreme label pair)"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import axisext_cases as ac  # noqa: E402
import pairstat_cases as pc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd.core import axisext as ax  # noqa: E402
from imgcompressionmps_amd.core import labelstat as ls  # noqa: E402
from imgcompressionmps_amd.core import pairstat as ps  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_cases as cc  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
INT_NAMES = sorted(vc.INT_CHAINS)
REAL_NAMES = ["L1", "L2_maxbond", "L4_tail_last", "L6_tail_all", "L5_ragged", "L4_no_tail", "L5_mid_tail_65"]
NAN_NAMES = ["int_tail_all", "int_no_tail"]


def feed(h, x):
    if isinstance(x, dict):
        for key in sorted(x):
            feed(h, key)
            feed(h, x[key])
    elif isinstance(x, (tuple, list)):
        h.update(f"seq{len(x)}".encode())
        for v in x:
            feed(h, v)
    elif isinstance(x, torch.Tensor):
        feed(h, x.cpu().numpy())
    elif isinstance(x, str):
        h.update(x.encode())
    elif x is None:
        h.update(b"None")
    else:
        a = np.ascontiguousarray(x)
        h.update(f"{type(x).__name__ if a.ndim == 0 else 'array'}/{a.dtype}/{a.shape}".encode())
        h.update(a.tobytes())


def emit(name, call):
    h = hashlib.sha256()
    try:
        feed(h, call())
        torch.cuda.synchronize()
    except (ValueError, TypeError) as e:  # a refusal; anything else (a HIP error) stops the tool
        feed(h, (type(e).__name__, str(e)))
    print(f"{name} {h.hexdigest()[:32]}", flush=True)


def cores_of(name, storage, nan=False):
    """(cores, factor array) of a chain of the case tables: three volume axes where tests/axisext_cases.py has them."""
    family = "integer" if name.startswith("int_") else "uniform"
    dims, bonds = pc.CHAINS[name]
    cores = [c.copy() for c in cc.draw_cores(name, dims, bonds, family, storage)]
    if nan:
        i = min(1, len(cores) - 1)
        cores[i][0, cores[i].shape[1] // 2, 0] = np.nan
    fa = np.array(ac.FACTORS[name], dtype=np.int64) if name in ac.FACTORS else cc.factor_array(dims)
    return cores, fa


def chain_of(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def each_chain(names=None, with_nan=True):
    """(tag, chain, plan, shape) over the chains, both element types, and the NaN variants."""
    for storage in vc.STORAGES:
        for name in names or INT_NAMES + REAL_NAMES:
            for nan in (False, True) if with_nan and name in NAN_NAMES else (False,):
                cores, fa = cores_of(name, storage, nan)
                shape = tuple(int(v) for v in np.prod(fa, axis=0))
                yield f"{name}{'+nan' if nan else ''}/{storage}", chain_of(cores, storage), _plan_for(shape, 0, factor_arr=fa), shape


def run_value():
    for tag, chain, plan, shape in each_chain():
        emit(f"value/moments/{tag}", lambda: vs.moments(chain))
        for lo, hi in ((-1.5, 2.0), (-1e-3, 2e-3)):  # a part of the integer voxels, a part of the real ones
            emit(f"value/moments_clip{hi}/{tag}", lambda: vs.moments(chain, clip=(lo, hi)))
        emit(f"value/value_stats/{tag}", lambda: vs.value_stats(chain))
        for bins in (1, 256, 4096):  # over the volume's own range
            emit(f"value/histogram{bins}/{tag}", lambda: vs.histogram(chain, bins, outliers=True))
        emit(f"value/histogram_range/{tag}", lambda: vs.histogram(chain, 7, range=(-2.5, 1e-3), outliers=True))
        emit(f"value/quantile/{tag}", lambda: vs.quantile(chain, 0.25))
        rng = np.random.default_rng(len(tag))
        x = rng.integers(-3, 4, size=shape).astype(np.float64)
        emit(f"value/error_to/{tag}", lambda: vs.error_to(chain, plan, x))
        emit(f"value/error_to_shape/{tag}", lambda: vs.error_to(chain, plan, x.reshape(-1)))
    emit("value/refused_bins", lambda: vs.histogram(chain, 4097))


def run_extreme():
    for tag, chain, plan, shape in each_chain():
        for op in ax.OPS:
            emit(f"extreme/arg/{op}/{tag}", lambda: ax.arg_extreme(chain, plan, op))
            for axes in ac.axis_sets(len(shape)):
                name = "".join(map(str, axes))
                emit(f"extreme/axes{name}/{op}/{tag}", lambda: ax.extreme(chain, plan, axes, op))
                emit(f"extreme/axes{name}/index/{op}/{tag}", lambda: ax.extreme(chain, plan, axes, op, index=True))


def run_label():
    for tag, chain, plan, shape in each_chain():
        n = int(np.prod(shape))
        index = np.arange(n, dtype=np.int64).reshape(shape)
        volumes = {"uint8": ((index * 7) % 251).astype(np.uint8), "int16": ((index % 300) - 5).astype(np.int16),
                   "int32": (index % 1500).astype(np.int32)}  # 1500 labels: two windows
        for kind, n_labels in (("uint8", 251), ("int16", 290), ("int32", 1500)):
            emit(f"label/{kind}/{tag}", lambda: ls.label_stats(chain, plan, volumes[kind], n_labels))
        emit(f"label/many/{tag}", lambda: ls.label_stats_many([chain, chain], plan, volumes["uint8"]))
    emit("label/refused_labels", lambda: ls.label_stats(chain, plan, volumes["int32"], 4097))


def run_pair():
    for storage in vc.STORAGES:
        for name in sorted(pc.INT_PAIRS) + sorted(pc.REAL_PAIRS):
            for nan in (False, True) if name in NAN_NAMES else (False,):
                family, table = ("integer", pc.INT_PAIRS) if name in pc.INT_PAIRS else ("uniform", pc.REAL_PAIRS)
                dims = pc.CHAINS[name][0]
                a = chain_of(cores_of(name, storage, nan)[0], storage)
                b = chain_of(cc.draw_cores(name + "/b", dims, table[name], family, storage), storage)
                tag = f"{name}{'+nan' if nan else ''}/{storage}"
                emit(f"pair/stats/{tag}", lambda: ps.pair_stats(a, b))
                emit(f"pair/joint8/{tag}", lambda: ps.joint_histogram(a, b, 8, outliers=True))  # over the volumes' own ranges
                emit(f"pair/joint128/{tag}", lambda: ps.joint_histogram(a, b, 128, outliers=True))  # above 64 KB of LDS
                emit(f"pair/joint_range/{tag}", lambda: ps.joint_histogram(a, b, (5, 1024), ((-2.5, 1e-3), (-1e-3, 3.0)), outliers=True))
                emit(f"pair/mi/{tag}", lambda: ps.mutual_information(a, b, 16))
    emit("pair/refused_cells", lambda: ps.joint_histogram(a, b, (1024, 17)))


GROUPS = {"value": run_value, "extreme": run_extreme, "label": run_label, "pair": run_pair}

if __name__ == "__main__":
    for group in sys.argv[1:] or list(GROUPS):
        GROUPS[group]()
