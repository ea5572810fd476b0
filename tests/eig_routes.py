"""ndmps_syevd_topk_route_query for the tests: the slot names of include/ndmps_hip.h, the kinds by name, and the
resident-slot counts of the MI355X that the host table of tests/test_eig_route_host.py is built on (the GPU suite
asserts that the device reports exactly these).  ctypes only."""
import ctypes as C

from imgcompressionmps_amd import _lib

# ndmps_syevd_topk_team_slots(512 / 1024 / 2048) on the MI355X: two 256-thread workgroups per CU on 256 CUs, one of the
# kernel with 8 rows per thread (read on the device; tests/test_gpu_robustness.py keeps it honest)
MI355X_TEAM_SLOTS = (512, 512, 256)

SLOTS = ("reduce", "handover", "kernel", "team_order", "team_size", "per_launch", "lds", "xcd", "pair", "half_turn",
         "col_width", "col_rows", "col_launches", "tail_cols", "tail_lower", "tail", "graph", "invit_cb", "invit_dbg",
         "ortho", "back", "seg", "r", "rb", "wyb", "t_factors", "bytes", "stamps", "off_desc", "off_desc2", "kw", "wpart")
COLUMNS, BAND2, BAND4, TEAM, BIG_TEAM, PANEL, PANEL_HYBRID = range(7)                      # reduce
K_NONE, K_TAGGED2, K_MEET2, K_SYM, K_TAGGED4, K_TAGGED8, K_BAND2, K_BAND4 = range(8)      # kernel
TAIL_NONE, TAIL_REGS, TAIL_LDS = range(3)                                                 # tail
ORTHO_WIDE_AUTO, ORTHO_WIDE, ORTHO_SMALL, ORTHO_BLOCKS, ORTHO_COLUMNS = range(5)          # ortho
BACK_LANES, BACK_ROWS, BACK_WIDE = range(3)                                               # back
RESIDENT = (TEAM, BIG_TEAM)


def route(lib, orders, k, team=-1, streamed=-1, slots=None):
    """The plan of a solve as a dict over SLOTS.  slots=None asks the device (needs a GPU); team / streamed -1: the
    calling thread's current settings."""
    assert len(SLOTS) == 32
    out = (C.c_int64 * len(SLOTS))()
    h_slots = (C.c_int * 3)(*slots) if slots is not None else None
    _lib.check(lib.ndmps_syevd_topk_route_query(len(orders), _lib.i64_array(list(orders)), k, team, streamed, h_slots, out))
    return dict(zip(SLOTS, out))
