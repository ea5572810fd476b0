"""Digests of the pair-product family's results (csrc/series.hip, wgram.hip, hadamard.hip, sumsketch.hip) on a fixed
case list: the smallest shapes that reach every branch of their kernels and both routes (a single tile, a ragged tile,
a full tile, a second k-tile, a split of the frames, every storage type).  One line per case,
`name sha256(raw output bytes, then ranks / zero flags / return code where the call gives them)`.  It hashes and does
not judge: two builds compute the same thing iff their lines agree, and a line that differs between two runs of ONE
build says nothing.  Inputs come from tests/series_cases.py, tests/wgram_cases.py, tests/sumsketch_cases.py or a fixed
seed; outputs start as zeros.  Uses only the C entry points, so the same script runs against any build that has them.
usage: python tools/pair_digest.py [group ...]     (groups: series wgram sandwich hadamard step sketch)"""
import ctypes as C
import hashlib
import itertools
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import hadamard_cases as hc  # noqa: E402
import series_cases as sc  # noqa: E402
import sumsketch_cases as ssc  # noqa: E402
import wgram_cases as wc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402
from imgcompressionmps_amd.core import hadamard as hd  # noqa: E402
from imgcompressionmps_amd.core import sumsketch as ss  # noqa: E402

DEV = "cuda:0"
CODE = {"f32": 0, "bf16": 1, "f64": 2}
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
WS_LIMIT = 1 << 31


def dev(a, storage="f64"):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV).to(DTYPE[storage]).contiguous()


def zeros(n):
    return torch.zeros(max(int(n), 1), dtype=torch.float64, device=DEV)


def workspace(nbytes):
    return torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=DEV)


def emit(name, *parts):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)).tobytes())
    print(f"{name} {h.hexdigest()[:32]}", flush=True)


def chain_list(lists, storages):
    """(device cores kept alive, bonds, codes, pointers) of a list of chains given as fp64 arrays."""
    keep = [[dev(c, s) for c in cores] for cores, s in zip(lists, storages)]
    bonds = _lib.i64_array([b for cores in lists for b in hc.bonds_of(cores)])
    codes = (C.c_int * len(lists))(*[CODE[s] for s in storages])
    ptrs = (C.c_void_p * sum(len(k) for k in keep))(*[t.data_ptr() for k in keep for t in k])
    return keep, bonds, codes, ptrs


def run_series(lib):
    for name, case in sc.CASES.items():
        la, lb = sc.cores_of(name)
        sym = int(lb is None)
        ka, ba, ca, pa = chain_list(la, case["storage_a"])
        kb, bb, cb, pb = (ka, ba, ca, pa) if sym else chain_list(lb, case["storage_b"])
        Ka, Kb, L = len(la), len(la if sym else lb), len(la[0])
        dims = _lib.i64_array([c.shape[1] for c in la[0]])
        ws = workspace(_lib.check(lib.ndmps_series_gram_workspace_bytes(Ka, Kb, L, dims, ba, bb)))
        G = zeros(Ka * Kb)
        _lib.check(lib.ndmps_series_gram(Ka, Kb, sym, L, dims, ba, ca, pa, bb, cb, pb, G.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr()))
        emit(f"series/{name}", G)


def run_wgram(lib):
    for name, case in wc.CASES.items():
        la, lb, w = wc.cores_of(name)
        sym = int(lb is None)
        ka, ba, ca, pa = chain_list(la, case["storage_a"])
        kb, bb, cb, pb = (ka, ba, ca, pa) if sym else chain_list(lb, case["storage_b"])
        kw, bw, _, pw = chain_list([w], [case["storage_w"]])
        Ka, Kb, L = len(la), len(la if sym else lb), len(w)
        dims = _lib.i64_array([c.shape[1] for c in w])
        query = lambda cap: lib.ndmps_series_wgram_workspace_bytes(Ka, Kb, sym, L, dims, ba, bb, bw, cap)
        caps = {"": WS_LIMIT}
        if name in ("ragged_mixed", "five"):  # the caps that leave room for one pair and for two
            query(0)
            one = int(re.search(r"one pair needs (\d+) bytes", lib.ndmps_last_error().decode()).group(1))
            lo, hi = one, query(WS_LIMIT)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if query(mid) > query(one) else (mid, hi)
            caps.update({"/chunk1": one, "/chunk2": hi})
        for tag, cap in caps.items():
            ws = workspace(_lib.check(query(cap)))
            G = zeros(Ka * Kb)
            _lib.check(lib.ndmps_series_wgram(Ka, Kb, sym, L, dims, ba, ca, pa, bb, cb, pb, bw, CODE[case["storage_w"]], pw,
                                              G.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
            emit(f"wgram/{name}{tag}", G)


def run_sandwich(lib):
    shapes = [(1, 1, 1, 1), (7, 13, 9, 16), (64, 64, 64, 64), (16, 80, 16, 7)]  # the last takes the general route
    for form, (ca, ca2, cb, cb2), d, n, st in itertools.product((0, 1), shapes, (1, 5), (1, 3), ("f32", "bf16", "f64")):
        rng = np.random.default_rng([form, ca, ca2, cb, cb2, d, n])
        A, B = dev(rng.standard_normal((ca, d, ca2)), st), dev(rng.standard_normal((cb, d, cb2)), st)
        E = dev(rng.standard_normal((n * d, ca2, cb2) if form else (n, ca, cb)))
        out = zeros(n * ca * cb if form else n * d * ca2 * cb2)
        ws = workspace(8 * (ca * d * ca2 + cb * d * cb2 + n * ca * d * cb2) + 1024)
        _lib.check(lib.ndmps_hadamard_sandwich(form, ca, d, ca2, cb, cb2, CODE[st], A.data_ptr(), CODE[st], B.data_ptr(), n,
                                               E.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        emit(f"sandwich/form{form}/{ca}x{ca2}x{cb}x{cb2}/d{d}/n{n}/{st}", out)


def run_hadamard(lib):
    rng = np.random.default_rng(77)
    dims = [8] * 4
    pa = hc.gaussian_cores(dims, [1, 2, 10, 10, 1], rng)   # product bonds 4, 100, 100 under sketch bonds 4, 16, 8:
    pb = hc.gaussian_cores(dims, [1, 2, 10, 10, 1], rng)   # bond 1 is an identity
    za = hc.gaussian_cores(dims, [1, 3, 3, 3, 1], rng)
    zb = hc.gaussian_cores(dims, [1, 4, 4, 4, 1], rng)
    za[0][:, 4:, :] = 0.0                        # a lives on the first half of site 0, b on the second: a zero product
    zb[0][:, :4, :] = 0.0
    cases = {
        "planted": (dims, pa, pb, 8, 8, "f32", "f64"),
        "zero": (dims, za, zb, 8, 8, "f32", "f32"),
        "bond64": ([4] * 4, hc.gaussian_cores([4] * 4, [1, 4, 64, 4, 1], rng), hc.gaussian_cores([4] * 4, [1, 4, 64, 4, 1], rng),
                   8, 8, "bf16", "f32"),
        "bond65": ([4] * 4, hc.gaussian_cores([4] * 4, [1, 4, 65, 4, 1], rng), hc.gaussian_cores([4] * 4, [1, 4, 3, 4, 1], rng),
                   8, 8, "f32", "bf16"),
    }
    for name, (dims, a, b, max_bond, over, sa, sb) in cases.items():
        L = len(dims)
        ba, bb = hc.bonds_of(a), hc.bonds_of(b)
        ell = hd.sketch_bonds(dims, ba, bb, max_bond, over)
        R = np.ascontiguousarray(np.concatenate([r.ravel() for r in hd.sketch_cores(dims, ell, 5)]))
        c_dims, c_ba, c_bb, c_ell = (_lib.i64_array(v) for v in (dims, ba, bb, ell))
        off, nbytes = (C.c_int64 * (L + 1))(), C.c_int64(0)
        total = _lib.check(lib.ndmps_hadamard_layout(L, c_dims, c_ba, c_bb, c_ell, off, C.byref(nbytes)))
        ka, kb = [dev(c, sa) for c in a], [dev(c, sb) for c in b]
        ptr = lambda keep: (C.c_void_p * L)(*[t.data_ptr() for t in keep])
        out, ws, ranks = zeros(total), workspace(nbytes.value), (C.c_int64 * (L + 1))()
        rc = _lib.check(lib.ndmps_hadamard_sketch(L, c_dims, c_ba, CODE[sa], ptr(ka), c_bb, CODE[sb], ptr(kb), c_ell,
                                                  R.ctypes.data_as(_lib.p_f64), R.size, out.data_ptr(), out.numel(), ranks,
                                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        emit(f"hadamard/{name}/ell{'-'.join(map(str, ell))}", out, list(ranks), [rc])


def run_step(lib):
    sizes = (1, 17, 64, 65)
    for form, T, d, l0, l1 in itertools.product((0, 1, 2), (1, 5, 20), (1, 3), sizes, sizes):
        rng = np.random.default_rng([form, T, d, l0, l1])
        chi, chi2 = rng.integers(1, 65, T), rng.integers(1, 65, T)
        chi[0], chi2[0] = 64, 33
        if T > 1:
            chi2[T // 2] = 65   # one frame on the general route
        st = [("f32", "bf16", "f64")[a % 3] for a in range(T)]
        keep = [dev(rng.standard_normal((chi[a], d, chi2[a])), st[a]) for a in range(T)]
        M = dev(rng.standard_normal(l0 * int(chi.sum())))      # M_a (l0 x chi_a), frame after frame
        Wn = dev(rng.standard_normal(int(chi2.sum()) * l1))    # W_{a,k+1} (chi2_a x l1)
        mat = dev(rng.standard_normal(l0 * d * l1))            # env: R_k;  project: Q
        d_in, d_in2, n_out = {0: (Wn, None, int(chi.sum()) * l0), 1: (M, Wn, l0 * d * l1), 2: (M, None, l1 * int(chi2.sum()))}[form]
        out, ws = zeros(n_out), workspace(16 << 20)
        _lib.check(lib.ndmps_sumsketch_step(form, T, d, _lib.i64_array(chi), _lib.i64_array(chi2), (C.c_int * T)(*[CODE[s] for s in st]),
                                            (C.c_void_p * T)(*[t.data_ptr() for t in keep]), l0, l1, d_in.data_ptr(),
                                            None if d_in2 is None else d_in2.data_ptr(), mat.data_ptr(), out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        emit(f"step/form{form}/T{T}/d{d}/l{l0}x{l1}", out)


def run_sketch(lib):
    rng = np.random.default_rng(99)
    frames_p, w_p = ssc.planted(0)
    dims_r, frames_r, w_r = ssc.ragged(0)
    lists = {"planted": (ssc.PLANTED_DIMS, frames_p + [hc.gaussian_cores(ssc.PLANTED_DIMS, [1, 8, 65, 65, 8, 1], rng)],
                         np.concatenate([w_p, rng.standard_normal((2, 1))], axis=1)),
             "ragged": (dims_r, frames_r + [hc.gaussian_cores(dims_r, [1, 8, 65, 8, 1], rng)],
                        np.concatenate([w_r, rng.standard_normal((2, 1))], axis=1))}
    for name, (dims, frames, w2) in lists.items():
        T, K, L = len(frames), 3, len(dims)
        w = np.concatenate([w2, np.zeros((1, T))])   # K = 3: the last row is zero,
        w[:, 1] = 0.0                                  # frame 1 is used by no row, and the last frame is wide
        st = [("f32", "bf16", "f64")[a % 3] for a in range(T)]
        keep, bonds, codes, ptrs = chain_list(frames, st)
        ell = ss.sketch_bonds(dims, [hc.bonds_of(f) for f in frames], 8, 8)
        R = np.ascontiguousarray(np.concatenate([r.ravel() for r in hd.sketch_cores(dims, ell, 3)]))
        c_dims, c_ell = _lib.i64_array(dims), _lib.i64_array(ell)
        off, nbytes = (C.c_int64 * (L + 1))(), C.c_int64(0)
        total = _lib.check(lib.ndmps_sumsketch_layout(T, K, L, c_dims, bonds, c_ell, off, C.byref(nbytes)))
        out, ws = zeros(total), workspace(nbytes.value)
        ranks, zero = (C.c_int64 * (K * (L + 1)))(), (C.c_int * K)()
        weights = np.ascontiguousarray(w, dtype=np.float64)
        _lib.check(lib.ndmps_sumsketch_sketch(T, K, L, c_dims, bonds, codes, ptrs, weights.ctypes.data_as(_lib.p_f64), c_ell,
                                              R.ctypes.data_as(_lib.p_f64), R.size, out.data_ptr(), out.numel(), ranks, zero,
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        emit(f"sketch/{name}/ell{'-'.join(map(str, ell))}", out, list(ranks), list(zero))


GROUPS = {"series": run_series, "wgram": run_wgram, "sandwich": run_sandwich, "hadamard": run_hadamard, "step": run_step,
          "sketch": run_sketch}

if __name__ == "__main__":
    library = _lib.load()
    for group in sys.argv[1:] or list(GROUPS):
        GROUPS[group](library)
