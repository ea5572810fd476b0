"""Digests of the direct eigen-solver's results on a fixed case list: one case per route kind and per switch of the
host driver (csrc/eig_tridiag.hip, trd_route), at the smallest order that reaches the kind.  Each case runs
ndmps_syevd_topk_values_f64 + _vectors_f64 and, where k <= 128, values + _vectors_auto_f64 on the same matrices, and
prints one line  `name sha256(w, V) sha256(w, V, ranks)`.  Two builds compute the same thing iff the lines agree; a case
whose line differs between two runs of ONE build is not repeatable and says nothing.  Inputs are made on the host from a
fixed seed.  Uses only entry points every build has; the route is printed too where the build can tell it.
usage: python tools/solver_digest.py [case ...]        (rocprofv3 --kernel-trace -- python tools/solver_digest.py)"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imgcompressionmps_amd import _lib  # noqa: E402

PANEL = {"NDMPS_TRD_PANEL_MIN": "513", "NDMPS_TRD_TEAM_MAX": "512"}
# name: (orders, k, environment, streamed, team enabled)
CASES = {
    "tail_128": ([128], 16, {}, 0, 1),
    "team_130": ([130], 16, {}, 0, 1),
    "team_260": ([260], 64, {}, 0, 1),
    "team_260_mixed": ([260, 131, 40], 40, {}, 0, 1),
    "team_130x17_lds_tail": ([130] * 17, 8, {}, 0, 1),
    "team_260x20_blocks32": ([260] * 20, 16, {}, 0, 1),
    "team_260x8_streamed": ([260] * 8, 16, {}, 1, 1),
    "team_260x8_streamed_narrow": ([260] * 8, 16, {"NDMPS_TRD_TEAM_NARROW": "1"}, 1, 1),
    "team_260_wide": ([260], 16, {"NDMPS_TRD_TEAM_WIDE": "1"}, 0, 1),
    "team_260x20_half": ([260] * 20, 16, {"NDMPS_TRD_TEAM_HALF": "1"}, 0, 1),
    "team_260x30_sym": ([260] * 30, 8, {"NDMPS_TRD_SYM": "1"}, 0, 1),
    "team_260_no_xcd": ([260] * 2, 16, {"NDMPS_TRD_XCD": "0"}, 0, 1),
    "team_260_no_pair": ([260] * 2, 16, {"NDMPS_TRD_PAIR": "0"}, 0, 1),
    "team_260_full_turn": ([260], 16, {"NDMPS_TEAM_FULL_TURN": "1"}, 0, 1),
    "team_260_tail_lds": ([260], 16, {"NDMPS_TRD_TAIL": "lds"}, 0, 1),
    "team_130x17_tail_regs": ([130] * 17, 8, {"NDMPS_TRD_TAIL": "regs"}, 0, 1),
    "band2_260": ([260] * 3, 64, {"NDMPS_TRD_BAND": "2"}, 0, 1),
    "band4_260": ([260] * 3, 64, {"NDMPS_TRD_BAND": "4"}, 0, 1),
    "columns_260_no_team": ([260], 64, {"NDMPS_TRD_NO_TEAM": "1"}, 0, 1),
    "columns_260_team_off": ([260], 64, {}, 0, 0),
    "columns_260_wide": ([260], 16, {"NDMPS_TRD_NO_TEAM": "1", "NDMPS_TRD_WIDE": "1"}, 0, 1),
    "ortho_blocks_260": ([260], 100, {}, 0, 1),
    "ortho_columns_260": ([260], 100, {"NDMPS_ORTHO_COLUMNS": "1"}, 0, 1),
    "wide_k200_260": ([260], 200, {}, 0, 1),
    "wide_k200_260_back_narrow": ([260], 200, {"NDMPS_BACK_NARROW": "1"}, 0, 1),
    "bigteam_600": ([600], 64, {}, 0, 1),
    "bigteam_777x3": ([777, 600, 650], 50, {}, 0, 1),
    "hybrid512_640": ([640], 64, PANEL, 0, 1),
    "panel_777": ([777], 64, PANEL, 0, 1),
    "panel_640_no_hybrid": ([640], 64, dict(PANEL, NDMPS_TRD_NO_HYBRID="1"), 0, 1),
    "panel_640_graph": ([640], 64, dict(PANEL, NDMPS_TRD_NO_HYBRID="1", NDMPS_TRD_PANEL_GRAPH="1"), 0, 1),
    "panel_1100_777": ([1100, 777], 96, PANEL, 0, 1),
    "columns_640_no_panel": ([640], 64, dict(PANEL, NDMPS_TRD_NO_PANEL="1"), 0, 1),
    "columns_640_default_min": ([640], 64, {"NDMPS_TRD_TEAM_MAX": "512"}, 0, 1),
    "hybrid1024_1100": ([1100], 64, {"NDMPS_TRD_TEAM_MAX": "1024"}, 0, 1),
    "bigteam_1024_wide_phase2": ([1024], 128, {}, 0, 1),
    "bigteam_1024x2_wide_phase2": ([1024, 1024], 100, {}, 0, 1),
    "bigteam_1024x3_narrow_phase2": ([1024] * 3, 100, {}, 0, 1),
    "bigteam_1024_ortho_narrow": ([1024], 128, {"NDMPS_ORTHO_NARROW": "1"}, 0, 1),
    "bigteam_1024_back_narrow": ([1024], 128, {"NDMPS_BACK_NARROW": "1"}, 0, 1),
    "bigteam_1024_no_side_stream": ([1024], 128, {"NDMPS_NO_SIDE_STREAM": "1"}, 0, 1),
    "bigteam_1024_k300": ([1024], 300, {}, 0, 1),
    "bigteam_2048": ([2048], 128, {}, 0, 1),
}
SWITCHES = sorted({name for case in CASES.values() for name in case[2]} |
                  {"NDMPS_INVIT_DBG", "NDMPS_INVIT_CB"})


def matrices(orders, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in orders:
        a = rng.standard_normal((n + 16, n)) * np.logspace(0, -4, n)[None, :]
        out.append(a.T @ a)
    return out


def solve(lib, mats, k, auto):
    """(w, V, ranks) of one values + vectors (auto: values + vectors_auto, cutoff 1e-3) call, as host arrays."""
    sizes = [m.shape[0] for m in mats]
    n, B = max(sizes), len(mats)
    g = np.zeros((B, n * n))
    for b, m in enumerate(mats):
        g[b, : m.size] = m.reshape(-1)
    tg = torch.from_numpy(g).to("cuda:0")
    tv = torch.zeros_like(tg)
    tw = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
    nbytes = lib.ndmps_syevd_topk_workspace_bytes(n, B, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    n_arr, sp = _lib.i64_array(sizes), _lib.stream_ptr()
    _lib.check(lib.ndmps_syevd_topk_values_f64(B, tg.data_ptr(), n * n, n_arr, tv.data_ptr(), n * n, tw.data_ptr(), n, k,
                                               ws.data_ptr(), nbytes, sp))
    ranks = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    if auto:
        status = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        _lib.check(lib.ndmps_syevd_topk_vectors_auto_f64(B, n_arr, k, 1e-3, ranks.data_ptr(), None, 0, status.data_ptr(),
                                                         ws.data_ptr(), nbytes, sp))
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * B, status
    else:
        status = (C.c_int * B)()
        ks = [min(k, s) for s in sizes]
        _lib.check(lib.ndmps_syevd_topk_vectors_f64(B, n_arr, _lib.i64_array(ks), k, ws.data_ptr(), nbytes, status, sp))
        assert list(status) == [0] * B, list(status)
    return tw.cpu().numpy(), tv.cpu().numpy(), ranks.cpu().numpy()


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()[:16]


def route_text(lib, orders, k, team, streamed):
    if not hasattr(lib, "ndmps_syevd_topk_route_query"):
        return ""
    out = (C.c_int64 * 64)()
    if lib.ndmps_syevd_topk_route_query(len(orders), _lib.i64_array(orders), k, team, streamed, None, out) != 0:
        return " route=?"
    return " route=" + ",".join(str(v) for v in list(out)[:4])


def main(names):
    lib = _lib.load()
    for name in SWITCHES:
        os.environ.pop(name, None)
    for name in names:
        orders, k, env, streamed, team = CASES[name]
        mats = matrices(orders, int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
        os.environ.update(env)
        lib.ndmps_syevd_topk_set_streamed(streamed)
        lib.ndmps_syevd_topk_set_team(team)
        try:
            two_phase = digest(solve(lib, mats, k, auto=False)[:2])
            auto = digest(solve(lib, mats, k, auto=True)) if k <= 128 else "-" * 16
            route = route_text(lib, orders, k, team, streamed)
        finally:
            lib.ndmps_syevd_topk_set_streamed(0)
            lib.ndmps_syevd_topk_set_team(1)
            for key in env:
                del os.environ[key]
        print(f"{name} {two_phase} {auto}{route}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
