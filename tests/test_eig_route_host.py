"""The eigen-solver's host side, pinned (no GPU): the workspace layout and the launches trd_route plans
(csrc/eig_tridiag.hip), through ndmps_syevd_topk_route_query with the MI355X's resident-slot counts as inputs.

PINNED was recorded from the build before the driver was moved onto TrdSwitches / trd_route / one carve: callers
allocate by these numbers and a recovery reuses the workspace, so a changed number is a changed layout.  It hits n = 1,
128/129 (kTail), 512/513, 1023/1024 (kWideOrthoMinOrder), 2048/2049, 4096; batch 1, 2/3 (kWideOrthoMaxBatch), 8, 16/17,
32, 4096; k = 1, 64, 128/129 (kMaxK), n; and the switches that move the layout.  ROUTES states, per case, what the
driver launched before the move, worked out from its code with those slot counts: every kind of reduction and every
boundary between two kinds."""
import os
import re

import pytest

import eig_routes as er
from eig_routes import route
from imgcompressionmps_amd import _lib

SWITCHES = ("NDMPS_TRD_BAND", "NDMPS_TRD_SYM", "NDMPS_TRD_NO_TEAM", "NDMPS_TRD_TEAM_MAX", "NDMPS_TRD_NO_HYBRID",
            "NDMPS_TRD_PANEL_MIN", "NDMPS_TRD_NO_PANEL", "NDMPS_TRD_PANEL_GRAPH", "NDMPS_TRD_TEAM_NARROW",
            "NDMPS_TRD_TEAM_WIDE", "NDMPS_TRD_TEAM_HALF", "NDMPS_TRD_XCD", "NDMPS_TRD_PAIR", "NDMPS_TRD_WIDE",
            "NDMPS_TRD_TAIL", "NDMPS_TEAM_FULL_TURN", "NDMPS_INVIT_DBG", "NDMPS_ORTHO_NARROW", "NDMPS_ORTHO_COLUMNS",
            "NDMPS_BACK_NARROW", "NDMPS_NO_SIDE_STREAM")
S = er.MI355X_TEAM_SLOTS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (switch, n_max, batch, k_max, ndmps_syevd_topk_workspace_bytes, ndmps_syevd_topk_stamps_offset)
PINNED = [
    ('', 1, 1, 1, 6656, 5888), ('', 2, 1, 1, 7168, 6400), ('', 2, 1, 2, 7168, 6400), ('', 17, 1, 1, 23808, 22528),
    ('', 17, 1, 17, 34816, 33536), ('', 128, 1, 1, 370176, 365568), ('', 128, 1, 64, 622080, 617472),
    ('', 128, 1, 128, 957952, 953344), ('', 129, 1, 1, 380416, 375552), ('', 129, 1, 64, 634112, 629248),
    ('', 129, 1, 128, 972544, 967680), ('', 129, 1, 129, 2728704, 1052416), ('', 260, 1, 1, 1300736, 1291776),
    ('', 260, 1, 64, 1812224, 1803264), ('', 260, 1, 128, 2494464, 2485504), ('', 260, 1, 129, 4795392, 2656256),
    ('', 260, 1, 260, 9272832, 4020736), ('', 512, 1, 1, 4618752, 4601856), ('', 512, 1, 64, 5626368, 5609472),
    ('', 512, 1, 128, 6969856, 6952960), ('', 512, 1, 129, 10124032, 7288832), ('', 512, 1, 512, 31283968, 15013888),
    ('', 513, 1, 1, 4966656, 4630272), ('', 513, 1, 64, 5976064, 5639680), ('', 513, 1, 128, 7322112, 6985728),
    ('', 513, 1, 129, 10706432, 7322368), ('', 513, 1, 513, 37559296, 15399168), ('', 777, 1, 1, 10824448, 10291456),
    ('', 777, 1, 64, 12353536, 11820544), ('', 777, 1, 128, 14392320, 13859328),
    ('', 777, 1, 129, 18867456, 14369280), ('', 777, 1, 777, 67665664, 34757632),
    ('', 1023, 1, 1, 18297600, 17573376), ('', 1023, 1, 64, 20310784, 19586560),
    ('', 1023, 1, 128, 22995200, 22270976), ('', 1023, 1, 129, 28516352, 22942208),
    ('', 1023, 1, 1023, 100160000, 59851776), ('', 1024, 1, 1, 19009536, 17590272),
    ('', 1024, 1, 64, 21805056, 19605504), ('', 1024, 1, 128, 26195968, 22292480),
    ('', 1024, 1, 129, 29128704, 22964224), ('', 1024, 1, 1024, 104413184, 59910144),
    ('', 2048, 1, 1, 71764992, 68732928), ('', 2048, 1, 64, 77294592, 72763392),
    ('', 2048, 1, 128, 85748736, 78137344), ('', 2048, 1, 129, 91089920, 79480832),
    ('', 2048, 1, 2048, 377908224, 239355904), ('', 2049, 1, 1, 71938048, 68835072),
    ('', 2049, 1, 64, 77549312, 72867328), ('', 2049, 1, 128, 86137088, 78243840),
    ('', 2049, 1, 129, 91593728, 79588096), ('', 2049, 1, 2049, 389238784, 240885504),
    ('', 4096, 1, 1, 278731776, 271681536), ('', 4096, 1, 64, 289729536, 279742464),
    ('', 4096, 1, 128, 306310144, 290490368), ('', 4096, 1, 129, 316468224, 293177344),
    ('', 4096, 1, 4096, 1503456256, 956860416), ('', 129, 2, 129, 3879936, 2100992),
    ('', 512, 2, 64, 11251712, 11218176), ('', 512, 2, 512, 46575872, 30027008),
    ('', 1024, 2, 128, 50260480, 44584192), ('', 1024, 2, 129, 53930496, 45927680),
    ('', 2048, 2, 128, 167694848, 156273920), ('', 129, 3, 129, 5031424, 3149568),
    ('', 512, 3, 64, 16877312, 16826880), ('', 512, 3, 512, 61868032, 45040128),
    ('', 1024, 3, 128, 69049344, 66875904), ('', 1024, 3, 129, 76963072, 68891136),
    ('', 2048, 3, 128, 239548672, 234410496), ('', 129, 8, 129, 10789120, 8393472),
    ('', 512, 8, 64, 45005056, 44870912), ('', 512, 8, 512, 138328576, 120106240),
    ('', 1024, 8, 128, 184130304, 178334976), ('', 1024, 8, 129, 198024192, 183708928),
    ('', 2048, 8, 128, 638795008, 625093888), ('', 129, 16, 129, 20002304, 16784128),
    ('', 512, 16, 64, 90009344, 89741056), ('', 512, 16, 512, 260665344, 240211712),
    ('', 1024, 16, 128, 368259840, 356669184), ('', 1024, 16, 129, 391721984, 367417088),
    ('', 2048, 16, 128, 1277589248, 1250187008), ('', 129, 17, 129, 21155840, 17834496),
    ('', 512, 17, 64, 95634944, 95349760), ('', 512, 17, 512, 275957504, 255224832),
    ('', 1024, 17, 128, 391276288, 378960896), ('', 1024, 17, 129, 415934464, 390380544),
    ('', 2048, 17, 128, 1357438720, 1328323584), ('', 129, 32, 129, 38429440, 33566208),
    ('', 512, 32, 64, 180017920, 179481344), ('', 512, 32, 512, 505338880, 480422656),
    ('', 1024, 32, 128, 736518912, 713337600), ('', 1024, 32, 129, 779117568, 734833408),
    ('', 8, 4096, 8, 38371328, 35749888), ('', 16, 4096, 1, 77955072, 74285056),
    ('', 1023, 2, 128, 45988864, 44540928), ('', 1023, 3, 128, 68983040, 66811136),
    ('', 4096, 2, 4096, 2534003456, 1913720064), ('', 4096, 3, 128, 884914688, 871469568),
    ('NDMPS_TRD_BAND=2', 128, 1, 16, 534016, 365568), ('NDMPS_TRD_BAND=2', 260, 3, 64, 7252224, 5403648),
    ('NDMPS_TRD_BAND=2', 512, 1, 128, 9198080, 6952960), ('NDMPS_TRD_BAND=2', 512, 32, 64, 251321088, 179481344),
    ('NDMPS_TRD_BAND=2', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_BAND=2', 1024, 2, 128, 50260480, 44584192),
    ('NDMPS_TRD_BAND=4', 128, 1, 16, 534016, 365568), ('NDMPS_TRD_BAND=4', 260, 3, 64, 7252224, 5403648),
    ('NDMPS_TRD_BAND=4', 512, 1, 128, 9198080, 6952960), ('NDMPS_TRD_BAND=4', 512, 32, 64, 251321088, 179481344),
    ('NDMPS_TRD_BAND=4', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_BAND=4', 1024, 2, 128, 50260480, 44584192),
    ('NDMPS_TRD_SYM=1', 128, 1, 16, 386560, 365568), ('NDMPS_TRD_SYM=1', 260, 3, 64, 5529856, 5403648),
    ('NDMPS_TRD_SYM=1', 512, 1, 128, 7035392, 6952960), ('NDMPS_TRD_SYM=1', 512, 32, 64, 182115072, 179481344),
    ('NDMPS_TRD_SYM=1', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_SYM=1', 1024, 2, 128, 50260480, 44584192),
    ('NDMPS_TRD_BAND=0', 128, 1, 16, 370176, 365568), ('NDMPS_TRD_BAND=0', 260, 3, 64, 5430016, 5403648),
    ('NDMPS_TRD_BAND=0', 512, 1, 128, 6969856, 6952960), ('NDMPS_TRD_BAND=0', 512, 32, 64, 180017920, 179481344),
    ('NDMPS_TRD_BAND=0', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_BAND=0', 1024, 2, 128, 50260480, 44584192),
    ('NDMPS_TRD_BAND=3', 128, 1, 16, 534016, 365568), ('NDMPS_TRD_BAND=3', 260, 3, 64, 7252224, 5403648),
    ('NDMPS_TRD_BAND=3', 512, 1, 128, 9198080, 6952960), ('NDMPS_TRD_BAND=3', 512, 32, 64, 251321088, 179481344),
    ('NDMPS_TRD_BAND=3', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_BAND=3', 1024, 2, 128, 50260480, 44584192),
    ('NDMPS_TRD_SYM=0', 128, 1, 16, 370176, 365568), ('NDMPS_TRD_SYM=0', 260, 3, 64, 5430016, 5403648),
    ('NDMPS_TRD_SYM=0', 512, 1, 128, 6969856, 6952960), ('NDMPS_TRD_SYM=0', 512, 32, 64, 180017920, 179481344),
    ('NDMPS_TRD_SYM=0', 513, 1, 64, 5976064, 5639680), ('NDMPS_TRD_SYM=0', 1024, 2, 128, 50260480, 44584192),
]


@pytest.fixture
def lib(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def _setenv(monkeypatch, env):
    for item in env.split():
        monkeypatch.setenv(*item.split("="))


def test_solver_size_queries_are_pinned(lib, monkeypatch):
    assert len(PINNED) >= 60
    got = []
    for env, n, batch, k, _, _ in PINNED:
        with monkeypatch.context() as m:
            _setenv(m, env)
            got.append((env, n, batch, k, lib.ndmps_syevd_topk_workspace_bytes(n, batch, k),
                        lib.ndmps_syevd_topk_stamps_offset(n, batch, k)))
    assert got == PINNED


def test_vector_phase_and_layout_agree_on_every_pinned_row(lib, monkeypatch):
    """The query is answered from the layout and the route the calls use: its sizes are the size queries', and the
    chip-wide kinds of phase 2 are planned exactly where the layout reserved their buffers -- more than kMaxK = 128
    vectors, or at most kWideOrthoMaxBatch = 2 matrices of order >= kWideOrthoMinOrder = 1024."""
    for env, n, batch, k, nbytes, stamps in PINNED:
        with monkeypatch.context() as m:
            _setenv(m, env)
            r = route(lib, [n] * batch, k, 1, 0, S)
        row = (env, n, batch, k)
        assert (r["bytes"], r["stamps"]) == (nbytes, stamps), row
        assert 0 < r["off_desc"] < r["off_desc2"] < r["stamps"] < nbytes and r["off_desc"] % 256 == r["off_desc2"] % 256 == 0
        many, big = k > 128, n >= 1024 and batch <= 2
        kp = -(-k // 16) * 16
        assert r["kw"] == (-(-kp // 64) * 64 if many or big else 0), row
        assert (r["kw"] > 0) == (r["ortho"] in (er.ORTHO_WIDE_AUTO, er.ORTHO_WIDE)), row
        assert r["ortho"] == (er.ORTHO_WIDE if many else er.ORTHO_WIDE_AUTO if big else
                              er.ORTHO_SMALL if k <= 64 else er.ORTHO_BLOCKS), row
        assert (r["wpart"] > 0) == big and (r["back"] == er.BACK_ROWS) == (big and not many), row
        assert (r["back"] == er.BACK_WIDE) == many, row
        assert r["t_factors"] == (0 if r["back"] == er.BACK_LANES else 2), row
        assert (r["seg"] * r["r"] >= n and r["rb"] > 0 and r["wyb"] > 0) == (r["back"] == er.BACK_LANES), row


def _phase1(reduce, handover=0, kernel=0, team_order=0, team_size=0, per_launch=0, lds=0, xcd=0, pair=0, half_turn=0,
            col_width=0, col_rows=0, col_launches=0, tail_cols=0, tail_lower=0, tail=er.TAIL_REGS, graph=0):
    return dict(reduce=reduce, handover=handover, kernel=kernel, team_order=team_order, team_size=team_size,
                per_launch=per_launch, lds=lds, xcd=xcd, pair=pair, half_turn=half_turn, col_width=col_width,
                col_rows=col_rows, col_launches=col_launches, tail_cols=tail_cols, tail_lower=tail_lower, tail=tail,
                graph=graph)


def _narrow(n, per_launch, half_turn, pair=1, **kw):   # 8-column tagged blocks, placed XCD by XCD
    return _phase1(er.TEAM, kernel=er.K_TAGGED2, team_order=n, team_size=-(-n // 8), per_launch=per_launch, lds=16384,
                   xcd=1, pair=pair, half_turn=half_turn, **kw)


def _blocks32(n, half_turn, per_launch=None, **kw):   # 32-column blocks that meet at a counter
    size = -(-n // 32)
    return _phase1(er.TEAM, kernel=er.K_MEET2, team_order=n, team_size=size, per_launch=per_launch or 512 // size,
                   lds=16384, xcd=1, pair=int(32 % size == 0 or size % 32 == 0), half_turn=half_turn, **kw)


def _big(n, per_launch, reduce=er.BIG_TEAM, **kw):   # 8-column tagged blocks, 4 or 8 rows per thread, 2-D grid, whole turn
    rows8 = n > 1024
    return _phase1(reduce, kernel=er.K_TAGGED8 if rows8 else er.K_TAGGED4, team_order=n, team_size=-(-n // 8),
                   per_launch=per_launch, lds=65536 if rows8 else 32768, **kw)


def _hybrid(handover, per_launch, **kw):
    return _big(handover, per_launch, reduce=er.PANEL_HYBRID, handover=handover, tail_cols=handover, **kw)


def _columns(n, width, rows, **kw):
    return _phase1(er.COLUMNS, col_width=width, col_rows=rows, col_launches=max(n - 128, 0), **kw)


_PANEL = _phase1(er.PANEL, tail_cols=128, tail_lower=1)
_PANEL_ENV = "NDMPS_TRD_TEAM_MAX=512 NDMPS_TRD_PANEL_MIN=513"

# (orders, switches, team_enabled, streamed, the phase-1 fields)
ROUTES = [
    # no reduction launches up to kTail = 128: the tail kernel takes the whole matrix
    ([1], "", 1, 0, _columns(1, 8, 2)),
    ([128], "", 1, 0, _columns(128, 8, 2)),
    ([128] * 16, "", 1, 0, _columns(128, 8, 2, tail=er.TAIL_LDS)),
    # orders 129 .. 512: the resident kernel; 8-column blocks while batch * n / 8 fits the 512 slots (half of them for a
    # streamed caller), half a turn while a launch fits 256 slots
    ([129], "", 1, 0, _narrow(129, 30, 1, pair=0)),
    ([130] * 15, "", 1, 0, _narrow(130, 30, 1, pair=0)),
    ([130] * 16, "", 1, 0, _narrow(130, 30, 0, pair=0, tail=er.TAIL_LDS)),
    ([256], "", 1, 0, _narrow(256, 16, 1)),
    ([512], "", 1, 0, _narrow(512, 8, 1)),
    ([512] * 4, "", 1, 0, _narrow(512, 8, 1)),
    ([512] * 5, "", 1, 0, _narrow(512, 8, 0)),
    ([512] * 8, "", 1, 0, _narrow(512, 8, 0)),
    ([512] * 4, "", 1, 1, _narrow(512, 8, 1)),
    ([512] * 5, "", 1, 1, _blocks32(512, 1)),
    ([512] * 8, "", 1, 1, _blocks32(512, 1)),
    ([512] * 9, "", 1, 0, _blocks32(512, 1)),
    ([512] * 16, "", 1, 0, _blocks32(512, 1, tail=er.TAIL_LDS)),
    ([512] * 17, "", 1, 0, _blocks32(512, 0, tail=er.TAIL_LDS)),
    ([512] * 32, "", 1, 0, _blocks32(512, 0, tail=er.TAIL_LDS)),
    ([260] * 20, "", 1, 0, _blocks32(260, 1, tail=er.TAIL_LDS)),
    ([512, 40, 300], "", 1, 0, _narrow(512, 8, 1)),
    # half storage: opt-in, only beyond the narrow teams and beyond half the slots (batch * 16 > 256)
    ([512] * 16, "NDMPS_TRD_SYM=1", 1, 0, _blocks32(512, 1, tail=er.TAIL_LDS)),
    ([512] * 17, "NDMPS_TRD_SYM=1", 1, 0,
     _phase1(er.TEAM, kernel=er.K_SYM, team_order=512, team_size=8, per_launch=64, xcd=1, half_turn=1, tail_lower=1,
             tail=er.TAIL_LDS)),
    ([512] * 32, "NDMPS_TRD_SYM=1", 1, 0,
     _phase1(er.TEAM, kernel=er.K_SYM, team_order=512, team_size=8, per_launch=64, xcd=1, half_turn=1, tail_lower=1,
             tail=er.TAIL_LDS)),
    # two-stage: orders 129 .. 512, widths 2 and 4 only, resident launches on
    ([260] * 3, "NDMPS_TRD_BAND=2", 1, 0,
     _phase1(er.BAND2, kernel=er.K_BAND2, team_order=260, team_size=9, per_launch=56, tail=er.TAIL_NONE)),
    ([512], "NDMPS_TRD_BAND=4", 1, 0,
     _phase1(er.BAND4, kernel=er.K_BAND4, team_order=512, team_size=16, per_launch=32, tail=er.TAIL_NONE)),
    ([512], "NDMPS_TRD_BAND=3", 1, 0, _narrow(512, 8, 1)),
    ([128], "NDMPS_TRD_BAND=2", 1, 0, _columns(128, 8, 2)),
    ([513], "NDMPS_TRD_BAND=2", 1, 0, _big(513, 7)),
    ([512], "NDMPS_TRD_BAND=2", 0, 0, _columns(512, 8, 2)),
    ([512], "NDMPS_TRD_BAND=2 NDMPS_TRD_NO_TEAM=1", 1, 0, _columns(512, 8, 2)),
    # orders 513 .. 2048 whose teams are all resident at once
    ([513], "", 1, 0, _big(513, 7)),
    ([777], "", 1, 0, _big(777, 5)),
    ([1024], "", 1, 0, _big(1024, 4)),
    ([1024] * 4, "", 1, 0, _big(1024, 4)),
    ([1025], "", 1, 0, _big(1025, 1)),
    ([2048], "", 1, 0, _big(2048, 1)),
    ([1024, 600, 100, 1000], "", 1, 0, _big(1024, 4)),
    # the hand-over: the widest of 2048 / 1024 / 512 that leaves 64 panel columns and fits the slots in one launch
    ([1024] * 5, "", 1, 0,
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, tail_cols=512)),
    ([1024] * 8, "", 1, 0,
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, tail_cols=512)),
    ([1024] * 9, "", 1, 0, _columns(1024, 32, 4)),   # no hand-over fits: below the 1536 of the plain panels
    ([2048] * 2, "", 1, 0, _hybrid(1024, 4)),
    ([2050], "", 1, 0, _hybrid(1024, 4)),
    ([2100], "", 1, 0, _hybrid(1024, 4)),
    ([2110], "", 1, 0, _hybrid(1024, 4)),
    ([2112], "", 1, 0, _hybrid(2048, 1)),
    ([4096], "", 1, 0, _hybrid(2048, 1)),
    ([4096] * 2, "", 1, 0, _hybrid(1024, 4)),
    ([2112], "NDMPS_TRD_TEAM_MAX=1024", 1, 0, _hybrid(1024, 4)),
    ([2112], "NDMPS_TRD_TEAM_MAX=100", 1, 0,   # clamped to 512
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, half_turn=1, tail_cols=512)),
    ([640], _PANEL_ENV, 1, 0,
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, half_turn=1, tail_cols=512)),
    ([574], _PANEL_ENV, 1, 0, _PANEL),   # 62 columns before the hand-over: fewer than a tile
    ([576], _PANEL_ENV, 1, 0,
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, half_turn=1, tail_cols=512)),
    ([640], "NDMPS_TRD_TEAM_MAX=512", 1, 0, _columns(640, 8, 4)),   # a hand-over is there, but the order is below 1024
    ([640], _PANEL_ENV + " NDMPS_TRD_NO_HYBRID=1", 1, 0, _PANEL),
    ([640], _PANEL_ENV + " NDMPS_TRD_NO_PANEL=1", 1, 0, _columns(640, 8, 4)),
    ([640], _PANEL_ENV + " NDMPS_TRD_NO_HYBRID=1 NDMPS_TRD_PANEL_GRAPH=1", 1, 0, dict(_PANEL, graph=1)),
    ([1100, 777], _PANEL_ENV, 1, 0, _PANEL),   # not hybrid: the batch is not uniform
    ([640], "NDMPS_TRD_TEAM_MAX=512 NDMPS_TRD_PANEL_MIN=100", 1, 0,   # clamped to 513
     _phase1(er.PANEL_HYBRID, handover=512, kernel=er.K_TAGGED2, team_order=512, team_size=64, per_launch=8, lds=16384,
             xcd=1, pair=1, half_turn=1, tail_cols=512)),
    # the plain panels: odd orders, mixed batches, resident launches off -- from order 1536 on
    ([2049], "", 1, 0, _PANEL),
    ([3001], "", 1, 0, _PANEL),
    ([4096], "", 0, 0, _PANEL),
    ([1536], "", 0, 0, _PANEL),
    ([1535], "", 0, 0, _columns(1535, 8, 8)),
    ([2048, 1300], "", 1, 0, _PANEL),   # 2 x 256 workgroups > 256 slots, and no hand-over for mixed orders
    # column launches: 8-column blocks while batch * n / 8 <= 512 workgroups; 2 / 4 / 8 / 16 rows per thread
    ([1200], "NDMPS_TRD_NO_TEAM=1", 1, 0, _columns(1200, 8, 8)),
    ([1200], "", 0, 0, _columns(1200, 8, 8)),
    ([512] * 8, "", 0, 0, _columns(512, 8, 2)),
    ([512] * 9, "", 0, 0, _columns(512, 32, 2)),
    ([512], "NDMPS_TRD_WIDE=1", 0, 0, _columns(512, 32, 2)),
    ([513], "", 0, 0, _columns(513, 8, 4)),
    ([1024], "", 0, 0, _columns(1024, 8, 4)),
    ([1025], "", 0, 0, _columns(1025, 8, 8)),
    ([2048], "NDMPS_TRD_NO_PANEL=1", 0, 0, _columns(2048, 8, 8)),
    ([2049], "NDMPS_TRD_NO_PANEL=1", 0, 0, _columns(2049, 8, 16)),
    ([4096] * 2, "NDMPS_TRD_NO_PANEL=1", 0, 0, _columns(4096, 32, 16)),
    # the tail kernel by the batch, or as told
    ([512], "NDMPS_TRD_TAIL=lds", 1, 0, _narrow(512, 8, 1, tail=er.TAIL_LDS)),
    ([512] * 32, "NDMPS_TRD_TAIL=regs", 1, 0, _blocks32(512, 0)),
]


@pytest.mark.parametrize("index", range(len(ROUTES)))
def test_reduction_route(lib, monkeypatch, index):
    orders, env, team, streamed, want = ROUTES[index]
    _setenv(monkeypatch, env)
    r = route(lib, orders, min(64, max(orders)), team, streamed, S)
    assert {k: r[k] for k in want} == want, (orders, env, team, streamed)


def test_route_table_reaches_every_kind():
    assert {row[4]["reduce"] for row in ROUTES} == set(range(7))
    assert {row[4]["kernel"] for row in ROUTES} == set(range(8))
    assert {row[4]["tail"] for row in ROUTES} == set(range(3))
    assert {row[4]["handover"] for row in ROUTES} == {0, 512, 1024, 2048}


# (orders, k, streamed, invit_cb, ortho, back, (SEG, R, RB, WYB), t_factors)
VECTORS = [
    ([1], 1, 128, er.ORTHO_SMALL, er.BACK_LANES, (32, 4, 8, 4), 0),
    ([128], 64, 128, er.ORTHO_SMALL, er.BACK_LANES, (32, 4, 8, 4), 0),
    ([129], 65, 128, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 8, 8, 4), 0),
    ([256], 128, 128, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 8, 8, 4), 0),
    ([257], 129, 128, er.ORTHO_WIDE, er.BACK_WIDE, (0, 0, 0, 0), 2),
    ([512] * 32, 128, 128, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 16, 8, 4), 0),
    ([513], 64, 128, er.ORTHO_SMALL, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1023], 128, 128, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024], 128, 16, er.ORTHO_WIDE_AUTO, er.BACK_ROWS, (0, 0, 0, 0), 2),
    ([1024] * 2, 128, 16, er.ORTHO_WIDE_AUTO, er.BACK_ROWS, (0, 0, 0, 0), 2),
    ([1024] * 3, 128, 16, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024] * 32, 128, 16, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024] * 33, 128, 32, er.ORTHO_BLOCKS, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024] * 65, 16, 16, er.ORTHO_SMALL, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024] * 257, 16, 128, er.ORTHO_SMALL, er.BACK_LANES, (32, 32, 4, 2), 0),
    ([1024], 1024, 16, er.ORTHO_WIDE, er.BACK_WIDE, (0, 0, 0, 0), 2),
    ([1025] * 3, 128, 16, er.ORTHO_BLOCKS, er.BACK_LANES, (64, 32, 2, 2), 0),
    ([2048] * 3, 64, 16, er.ORTHO_SMALL, er.BACK_LANES, (64, 32, 2, 2), 0),
    ([2049] * 3, 64, 16, er.ORTHO_SMALL, er.BACK_LANES, (64, 64, 1, 1), 0),
    ([4096], 128, 16, er.ORTHO_WIDE_AUTO, er.BACK_ROWS, (0, 0, 0, 0), 2),
]


@pytest.mark.parametrize("index", range(len(VECTORS)))
def test_vector_phase_route(lib, index):
    """Inverse iteration in blocks of 128 columns below order 1024, from there on halved while batch * blocks <= 256
    (16 at least); one workgroup per matrix up to 64 / 128 vectors, the chip for more or for one or two big matrices;
    the lane-dealt back-transformation by the first (SEG, R) with SEG * R >= n."""
    orders, k, cb, ortho, back, lanes, t_factors = VECTORS[index]
    r = route(lib, orders, k, 1, 0, S)
    assert (r["invit_cb"], r["invit_dbg"], r["ortho"], r["back"], (r["seg"], r["r"], r["rb"], r["wyb"]), r["t_factors"]) == \
        (cb, 0, ortho, back, lanes, t_factors)


# switch -> (value, orders, k, team_enabled, streamed, the fields it moves: {name: (without, with)})
WIRING = {
    "NDMPS_TRD_BAND": ("2", [260], 64, 1, 0, dict(reduce=(er.TEAM, er.BAND2), kernel=(er.K_TAGGED2, er.K_BAND2),
                                                   team_size=(33, 9), per_launch=(15, 56), lds=(16384, 0), xcd=(1, 0),
                                                   half_turn=(1, 0), tail=(er.TAIL_REGS, er.TAIL_NONE))),
    "NDMPS_TRD_SYM": ("1", [512] * 32, 64, 1, 0, dict(kernel=(er.K_MEET2, er.K_SYM), team_size=(16, 8), per_launch=(32, 64),
                                                      lds=(16384, 0), pair=(1, 0), half_turn=(0, 1), tail_lower=(0, 1))),
    "NDMPS_TRD_NO_TEAM": ("1", [512], 64, 1, 0, dict(reduce=(er.TEAM, er.COLUMNS), kernel=(er.K_TAGGED2, 0),
                                                     team_order=(512, 0), team_size=(64, 0), per_launch=(8, 0),
                                                     lds=(16384, 0), xcd=(1, 0), pair=(1, 0), half_turn=(1, 0),
                                                     col_width=(0, 8), col_rows=(0, 2), col_launches=(0, 384))),
    "NDMPS_TRD_TEAM_MAX": ("1024", [2112], 64, 1, 0, dict(handover=(2048, 1024), kernel=(er.K_TAGGED8, er.K_TAGGED4),
                                                          team_order=(2048, 1024), team_size=(256, 128), per_launch=(1, 4),
                                                          lds=(65536, 32768), tail_cols=(2048, 1024))),
    "NDMPS_TRD_NO_HYBRID": ("1", [2112], 64, 1, 0, dict(reduce=(er.PANEL_HYBRID, er.PANEL), handover=(2048, 0),
                                                        kernel=(er.K_TAGGED8, 0), team_order=(2048, 0), team_size=(256, 0),
                                                        per_launch=(1, 0), lds=(65536, 0), tail_cols=(2048, 128),
                                                        tail_lower=(0, 1))),
    "NDMPS_TRD_PANEL_MIN": ("513", [600], 64, 0, 0, dict(reduce=(er.COLUMNS, er.PANEL), col_width=(8, 0), col_rows=(4, 0),
                                                         col_launches=(472, 0), tail_cols=(0, 128), tail_lower=(0, 1))),
    "NDMPS_TRD_NO_PANEL": ("1", [3001], 64, 1, 0, dict(reduce=(er.PANEL, er.COLUMNS), col_width=(0, 8), col_rows=(0, 16),
                                                       col_launches=(0, 2873), tail_cols=(128, 0), tail_lower=(1, 0))),
    "NDMPS_TRD_PANEL_GRAPH": ("1", [3001], 64, 1, 0, dict(graph=(0, 1))),
    "NDMPS_TRD_TEAM_NARROW": ("1", [512] * 8, 64, 1, 1, dict(kernel=(er.K_MEET2, er.K_TAGGED2), team_size=(16, 64),
                                                             per_launch=(32, 8), half_turn=(1, 0))),
    "NDMPS_TRD_TEAM_WIDE": ("1", [512], 64, 1, 0, dict(kernel=(er.K_TAGGED2, er.K_MEET2), team_size=(64, 16),
                                                       per_launch=(8, 32))),
    "NDMPS_TRD_TEAM_HALF": ("1", [512] * 32, 64, 1, 0, dict(per_launch=(32, 16), half_turn=(0, 1))),
    "NDMPS_TRD_XCD": ("0", [512], 64, 1, 0, dict(xcd=(1, 0), pair=(1, 0))),
    "NDMPS_TRD_PAIR": ("0", [512], 64, 1, 0, dict(pair=(1, 0))),
    "NDMPS_TRD_WIDE": ("1", [512], 64, 0, 0, dict(col_width=(8, 32))),
    "NDMPS_TRD_TAIL": ("lds", [512], 64, 1, 0, dict(tail=(er.TAIL_REGS, er.TAIL_LDS))),
    "NDMPS_TEAM_FULL_TURN": ("1", [512], 64, 1, 0, dict(half_turn=(1, 0))),
    "NDMPS_INVIT_DBG": ("2", [512], 64, 1, 0, dict(invit_dbg=(0, 2))),
    "NDMPS_ORTHO_NARROW": ("1", [1024], 128, 1, 0, dict(ortho=(er.ORTHO_WIDE_AUTO, er.ORTHO_BLOCKS),
                                                        back=(er.BACK_ROWS, er.BACK_LANES), seg=(0, 32), r=(0, 32), rb=(0, 4),
                                                        wyb=(0, 2), t_factors=(2, 0))),
    "NDMPS_ORTHO_COLUMNS": ("1", [512], 128, 1, 0, dict(ortho=(er.ORTHO_BLOCKS, er.ORTHO_COLUMNS))),
    "NDMPS_BACK_NARROW": ("1", [1024], 128, 1, 0, dict(back=(er.BACK_ROWS, er.BACK_LANES), seg=(0, 32), r=(0, 32), rb=(0, 4),
                                                       wyb=(0, 2), t_factors=(2, 0))),
    "NDMPS_NO_SIDE_STREAM": ("1", [1024], 128, 1, 0, dict(t_factors=(2, 1))),
}
MOVES_THE_LAYOUT = {"NDMPS_TRD_BAND", "NDMPS_TRD_SYM"}


def test_every_switch_has_a_wiring_case():
    assert set(WIRING) == set(SWITCHES)


@pytest.mark.parametrize("name", SWITCHES)
def test_switch_moves_exactly_the_fields_it_governs(lib, monkeypatch, name):
    """Each switch of TrdSwitches, on a case where it matters: the plan differs from the default's in the fields the
    switch governs and in no other, every other switch's case is untouched by it being spelled differently (a mistyped
    name would leave the plan unchanged), and the workspace changes size only for NDMPS_TRD_BAND and NDMPS_TRD_SYM.
    NDMPS_INVIT_CB is latched by its first use and cannot be flipped inside a process: not in this table."""
    value, orders, k, team, streamed, moved = WIRING[name]
    before = route(lib, orders, k, team, streamed, S)
    monkeypatch.setenv(name, value)
    after = route(lib, orders, k, team, streamed, S)
    sizes = {"bytes"} if name in MOVES_THE_LAYOUT else set()
    assert {f: (before[f], after[f]) for f in er.SLOTS if before[f] != after[f] and f not in sizes} == moved
    assert (before["bytes"] != after["bytes"]) == (name in MOVES_THE_LAYOUT)
    assert (before["stamps"], before["off_desc"], before["off_desc2"]) == (after["stamps"], after["off_desc"], after["off_desc2"])
    monkeypatch.delenv(name)
    assert route(lib, orders, k, team, streamed, S) == before   # read per call: nothing is latched


def test_query_follows_the_threads_settings_and_checks_its_arguments(lib):
    """team_enabled / streamed = -1 plan for what ndmps_syevd_topk_set_team / _set_streamed last set on this thread."""
    assert route(lib, [512] * 8, 64, -1, -1, S) == route(lib, [512] * 8, 64, 1, 0, S)
    assert lib.ndmps_syevd_topk_set_streamed(1) == 0
    try:
        assert route(lib, [512] * 8, 64, -1, -1, S) == route(lib, [512] * 8, 64, 1, 1, S)
    finally:
        lib.ndmps_syevd_topk_set_streamed(0)
    assert lib.ndmps_syevd_topk_set_team(0) == 1
    try:
        assert route(lib, [512], 64, -1, -1, S) == route(lib, [512], 64, 0, 0, S)
        assert route(lib, [512], 64, 1, -1, S)["reduce"] == er.TEAM
    finally:
        lib.ndmps_syevd_topk_set_team(1)
    import ctypes as C
    out, slots, n = (C.c_int64 * 32)(), (C.c_int * 3)(*S), _lib.i64_array([512])
    q = lib.ndmps_syevd_topk_route_query
    assert q(1, n, 64, 1, 0, slots, out) == 0
    assert q(0, n, 64, 1, 0, slots, out) == _lib.EINVAL and q(1, None, 64, 1, 0, slots, out) == _lib.EINVAL
    assert q(1, n, 0, 1, 0, slots, out) == _lib.EINVAL and q(1, n, 4097, 1, 0, slots, out) == _lib.EINVAL
    assert q(1, n, 64, 1, 0, slots, None) == _lib.EINVAL and q(1, _lib.i64_array([4097]), 64, 1, 0, slots, out) == _lib.EINVAL
    assert q(1, n, 64, 1, 0, (C.c_int * 3)(512, 0, 256), out) == _lib.EINVAL


def _body(src, signature):
    """The text of the function that starts at `signature`, up to the first line that closes it at column 0."""
    start = src.index(signature)
    return src[start:src.index("\n}\n", start)]


def test_environment_is_read_in_one_function_and_the_route_is_pure():
    """getenv appears in trd_switches and in the latched NDMPS_INVIT_CB and nowhere else in the solver; trd_route and
    the geometry it calls make no HIP call, read no thread-local and call neither of those two."""
    csrc = os.path.join(ROOT, "img-compression-mps_amd", "csrc")
    src = open(os.path.join(csrc, "eig_tridiag.hip")).read()
    for inc in ("eig_band.inc", "eig_sym.inc", "eig_panel.inc", "eig_wide.inc"):
        assert "getenv" not in open(os.path.join(csrc, inc)).read()
    switches, latched = _body(src, "TrdSwitches trd_switches() {"), _body(src, "int invit_cb_forced() {")
    readers = switches + latched
    code = "\n".join(line.split("//")[0] for line in src.replace(switches, "").replace(latched, "").splitlines())
    assert "getenv" not in code and readers.count("getenv") >= 5
    for name in SWITCHES + ("NDMPS_INVIT_CB",):
        assert readers.count('"' + name + '"') >= 1, name
    for signature in ("TrdRoute trd_route(const TrdCase& c, const TrdLayout& l) {", "TeamGeom team_geometry(",
                      "int band_width_for("):
        body = "\n".join(line.split("//")[0] for line in _body(src, signature).splitlines())
        assert not re.search(r"\bhip[A-Z_]|getenv|g_team_|g_route|trd_switches|invit_cb_forced|NDMPS_CHECK|NDMPS_TRY", body), signature
