"""The decode's plan (csrc/chain_plan.h), on the host (no GPU).  Three nets:

* the size queries of every chain of oracle/chain_cases.py, pinned from the build before the chain was moved onto
  the plan: callers allocate by them, so a changed number is a changed workspace layout;
* ndmps_chain_plan_query against a model written here from ``cc.tail_start`` and the schedule (tail right to left,
  cumulative left products, one final product): the products, their operands, and the invariants that make the
  ping-pong between the buffers sound;
* the refusals every entry makes before its first launch, exercised with pointers that are never dereferenced.
"""
import ctypes as C

import numpy as np
import pytest

from imgcompressionmps_amd import _lib
from oracle import chain_cases as cc

ALL = dict(cc.CHAINS, **cc.INTEGER_CHAINS)
BATCHES = (1, 2, 64, 65, 130)

# name -> (workspace_bytes, workspace_bytes_f64, tail_columns, batched_workspace_bytes at BATCHES with equal bonds)
PINNED = {
    'L1': (1536, 1792, 0, 1536, 3072, 98304, 98304, 98304),
    'L2_maxbond': (27392, 49408, 65, 27392, 54784, 1753088, 1753088, 1753088),
    'L3_tail_all': (5888, 9728, 55, 5888, 11776, 376832, 376832, 376832),
    'L4_tail_4096': (657408, 1182720, 4096, 657408, 1314816, 42074112, 42074112, 42074112),
    'L5_ragged': (94208, 168704, 1320, 94208, 188416, 6029312, 6029312, 6029312),
    'L6_tail_all': (104960, 188160, 3456, 104960, 209920, 6717440, 6717440, 6717440),
    'L7_tail_all': (8448, 14336, 216, 8448, 16896, 540672, 540672, 540672),
    'L5_nonmonotone': (1620480, 2917376, 4032, 1620480, 3240960, 103710720, 103710720, 103710720),
    'L5_primes_maxbond': (25088, 44288, 770, 25088, 50176, 1605632, 1605632, 1605632),
    'L5_unit_dims': (4608, 7424, 63, 4608, 9216, 294912, 294912, 294912),
    'L6_bonds_one': (35840, 63744, 3456, 35840, 71680, 2293760, 2293760, 2293760),
    'L3_tail_last': (124672, 215296, 41, 124672, 249344, 7979008, 7979008, 7979008),
    'L4_tail_last': (121088, 219136, 64, 121088, 242176, 7749632, 7749632, 7749632),
    'L5_tail_last': (562944, 1094656, 64, 562944, 1125888, 36028416, 36028416, 36028416),
    'L6_tail_last': (696832, 1318912, 64, 696832, 1393664, 44597248, 44597248, 44597248),
    'L7_tail_last': (691712, 1326592, 64, 691712, 1383424, 44269568, 44269568, 44269568),
    'L5_mid_tail_129': (5332992, 9624576, 4096, 5332992, 10665984, 341311488, 341311488, 341311488),
    'L5_mid_tail_65': (1140224, 2056192, 1716, 1140224, 2280448, 72974336, 72974336, 72974336),
    'L2_no_tail': (197632, 328704, 0, 197632, 395264, 12648448, 12648448, 12648448),
    'L3_no_tail': (738304, 1229824, 0, 738304, 1476608, 47251456, 47251456, 47251456),
    'L4_no_tail': (508928, 902144, 0, 508928, 1017856, 32571392, 32571392, 32571392),
    'L4_large': (66986496, 132915200, 65, 66986496, 133972992, 4287135744, 4287135744, 4287135744),
    'int_tail_all': (11520, 19968, 504, 11520, 23040, 737280, 737280, 737280),
    'int_tail_last': (18176, 32256, 41, 18176, 36352, 1163264, 1163264, 1163264),
    'int_no_tail': (427008, 820224, 0, 427008, 854016, 27328512, 27328512, 27328512),
    'int_wide': (116480, 208896, 1440, 116480, 232960, 7454720, 7454720, 7454720),
}
# a batch of 3 over the sites of L4_tail_last with one differing bond profile: one slice that fits the largest
MIXED = ([[1, 3, 13, 13, 1], [1, 3, 13, 13, 1], [1, 2, 5, 33, 1]], 271104)

# name -> (j0, cumulative left products), as noted beside the cases in oracle/chain_cases.py (j0 == L: no tail)
NOTED = {
    'L1': (1, 0), 'L2_maxbond': (1, 0), 'L3_tail_all': (1, 0), 'L4_tail_4096': (1, 0), 'L5_ragged': (1, 0),
    'L6_tail_all': (1, 0), 'L7_tail_all': (1, 0), 'L5_nonmonotone': (1, 0), 'L5_primes_maxbond': (1, 0),
    'L5_unit_dims': (1, 0), 'L6_bonds_one': (1, 0),
    'L3_tail_last': (2, 1), 'L4_tail_last': (3, 2), 'L5_tail_last': (4, 3), 'L6_tail_last': (5, 4), 'L7_tail_last': (6, 5),
    'L5_mid_tail_129': (2, 1), 'L5_mid_tail_65': (2, 1),
    'L2_no_tail': (2, 1), 'L3_no_tail': (3, 2), 'L4_no_tail': (4, 3), 'L4_large': (3, 2),
    'int_tail_all': (1, 0), 'int_tail_last': (2, 1), 'int_no_tail': (4, 3), 'int_wide': (1, 0),
}

TAIL, LEFT, FINAL = 0, 1, 2
WS_LEFT, WS_TAIL0, WS_TAIL1, OUT, NONE = -1, -2, -3, -4, -5
ELEMS = {"f32": 0, "bf16": 1, "f64": 2}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _prod(xs):
    return int(np.prod(xs, dtype=np.int64)) if len(xs) else 1


def _plan(lib, dims, bonds, elem="f32"):
    L = len(dims)
    out = (C.c_int64 * (6 + 8 * (L - 1)))()
    assert lib.ndmps_chain_plan_query(ELEMS[elem], L, _lib.i64_array(dims), _lib.i64_array(bonds), out) == _lib.OK
    head = dict(zip(("j0", "tail_cols", "n_products", "left_elems", "tail_elems", "bytes"), out[:6]))
    products = [dict(zip(("kind", "m", "n", "k", "a", "b", "c", "spare"), out[6 + 8 * q:14 + 8 * q]))
                for q in range(head["n_products"])]
    return head, products


def test_the_cases_and_the_tables_here_cover_each_other():
    assert set(PINNED) == set(NOTED) == set(ALL)
    for name, (dims, bonds) in ALL.items():
        cc.check_chain(dims, bonds)
        assert cc.tail_start(dims) == NOTED[name][0], name


def test_hand_checked_size():
    """L3_tail_last in fp32, by the formula: left = max(6 * 5, 600 * 33) = 19800 -> 19840, tail = 33 * 41 = 1353 ->
    1408, largest right operand 5 * 100 * 33 = 16500 elements of two bytes -> 33024, + 1024."""
    assert PINNED["L3_tail_last"][0] == (19840 + 2 * 1408) * 4 + 33024 + 1024 == 124672


@pytest.mark.parametrize("name", sorted(ALL))
def test_size_queries_are_pinned(lib, name):
    dims, bonds = ALL[name]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    got = (lib.ndmps_chain_workspace_bytes(L, d, b), lib.ndmps_chain_workspace_bytes_f64(L, d, b),
           lib.ndmps_chain_tail_columns(L, d))
    got += tuple(lib.ndmps_chain_batched_workspace_bytes(n, L, d, _lib.i64_array(list(bonds) * n)) for n in BATCHES)
    assert got == PINNED[name]


def test_batched_size_with_one_differing_bond_profile(lib):
    rows, nbytes = MIXED
    dims = cc.CHAINS["L4_tail_last"][0]
    flat = _lib.i64_array([x for r in rows for x in r])
    assert lib.ndmps_chain_batched_workspace_bytes(len(rows), len(dims), _lib.i64_array(dims), flat) == nbytes
    each = [lib.ndmps_chain_workspace_bytes(len(dims), _lib.i64_array(dims), _lib.i64_array(r)) for r in rows]
    assert nbytes == -(-max(each) // 256) * 256


@pytest.mark.parametrize("name", sorted(ALL))
def test_plan_against_the_model(lib, name):
    dims, bonds = ALL[name]
    L = len(dims)
    j0 = cc.tail_start(dims)
    has_tail = j0 < L
    head, products = _plan(lib, dims, bonds)
    assert head["j0"] == j0 == NOTED[name][0]
    assert head["tail_cols"] == (_prod(dims[j0:]) if has_tail else 0) == PINNED[name][2]

    # ---- the model's schedule: tail sites L-2 .. j0, left sites 1 .. (j0 - 1 with a tail, L - 1 without), final
    tail_sites = list(range(L - 2, j0 - 1, -1)) if has_tail else []
    left_sites = list(range(1, j0 if has_tail else L))
    kinds = [p["kind"] for p in products]
    assert kinds == [TAIL] * len(tail_sites) + [LEFT] * len(left_sites) + [FINAL] * int(has_tail)
    assert len(left_sites) == NOTED[name][1]
    assert len(products) == L - 1

    R, left = L - 1, 0  # what holds the tail matrix / the cumulative left product so far
    for p, i in zip(products, tail_sites):
        assert (p["m"], p["n"], p["k"]) == (bonds[i] * dims[i], _prod(dims[i + 1:]), bonds[i + 1])
        assert (p["a"], p["b"]) == (i, R) and p["c"] in (WS_TAIL0, WS_TAIL1) and p["spare"] == NONE
        R = p["c"]
    for p, i in zip(products[len(tail_sites):], left_sites):
        assert (p["m"], p["n"], p["k"]) == (_prod(dims[:i]), dims[i] * bonds[i + 1], bonds[i])
        assert (p["a"], p["b"]) == (left, i) and p["c"] in (WS_LEFT, OUT) and p["spare"] == NONE
        left = p["c"]
    if has_tail:
        p = products[-1]
        assert (p["m"], p["n"], p["k"]) == (_prod(dims[:j0]), _prod(dims[j0:]), bonds[j0])
        assert (p["a"], p["b"], p["c"]) == (left, R, OUT)
        # the spare buffer is the tail buffer that does not hold R
        assert p["spare"] in (WS_TAIL0, WS_TAIL1) and p["spare"] != R
        assert p["k"] * p["n"] <= head["tail_elems"]

    # ---- the invariants of the ping-pong
    capacity = {WS_LEFT: head["left_elems"], WS_TAIL0: head["tail_elems"], WS_TAIL1: head["tail_elems"],
                OUT: _prod(dims)}
    written = set(range(L))  # the cores
    for q, p in enumerate(products):
        assert p["a"] in written and p["b"] in written, f"product {q} reads a buffer nothing wrote"
        assert p["c"] not in (p["a"], p["b"]), f"product {q} writes a buffer it reads"
        assert p["c"] < 0 and p["m"] * p["n"] <= capacity[p["c"]], f"product {q} does not fit its destination"
        if q and products[q - 1]["kind"] == p["kind"]:
            assert products[q - 1]["c"] != p["c"], f"products {q - 1} and {q} do not alternate"
        written.add(p["c"])
    if products:
        assert products[-1]["c"] == OUT
        assert len(products) < 2 or products[-2]["c"] != OUT


@pytest.mark.parametrize("name", sorted(ALL))
def test_query_and_size_queries_agree(lib, name):
    dims, bonds = ALL[name]
    f32, f64, tail_cols = PINNED[name][:3]
    plans = {elem: _plan(lib, dims, bonds, elem) for elem in ELEMS}
    assert plans["f32"][0]["bytes"] == plans["bf16"][0]["bytes"] == f32
    assert plans["f64"][0]["bytes"] == f64
    assert plans["f32"] == plans["bf16"] and plans["f32"][1] == plans["f64"][1]
    assert all(h["tail_cols"] == tail_cols for h, _ in plans.values())
    if cc.tail_start(dims) == len(dims):
        assert tail_cols == 0 and plans["f32"][0]["tail_elems"] == 0


def test_refusals_before_any_launch(lib):
    """Every refusal below returns before the first HIP call: the pointers are fakes."""
    dims, bonds = cc.CHAINS["L4_tail_last"]
    L, d, b = len(dims), _lib.i64_array(dims), _lib.i64_array(bonds)
    fake = (C.c_void_p * L)(*[64] * L)
    p64 = C.c_void_p(64)
    need = lib.ndmps_chain_workspace_bytes(L, d, b)
    out = (C.c_int64 * (6 + 8 * (L - 1)))()
    assert lib.ndmps_chain_plan_query(0, L, d, b, None) == _lib.EINVAL
    assert lib.ndmps_chain_plan_query(3, L, d, b, out) == _lib.EINVAL
    assert lib.ndmps_chain_plan_query(-1, L, d, b, out) == _lib.EINVAL
    for fn, need_s in ((lib.ndmps_chain_contract_f32, need), (lib.ndmps_chain_contract_bf16, need),
                       (lib.ndmps_chain_contract_f64, lib.ndmps_chain_workspace_bytes_f64(L, d, b))):
        assert fn(L, d, b, fake, p64, p64, need_s - 1, None) == _lib.EWORKSPACE
        assert fn(L, d, b, fake, p64, None, 1 << 30, None) == _lib.EWORKSPACE
        assert fn(0, d, b, fake, p64, p64, 1 << 30, None) == _lib.EINVAL
        assert fn(L, d, b, fake, None, p64, 1 << 30, None) == _lib.EINVAL
        assert fn(L, d, b, None, p64, p64, 1 << 30, None) == _lib.EINVAL
        for bad in ([1, 4, 13, 13, 1], [1, 3, 13, 65, 1], [1, 3, 0, 13, 1]):
            assert fn(L, d, _lib.i64_array(bad), fake, p64, p64, 1 << 30, None) == _lib.EINVAL, bad
            assert b"exceeds" in lib.ndmps_last_error()
        for bad in ([2, 3, 13, 13, 1], [1, 3, 13, 13, 2]):
            assert fn(L, d, _lib.i64_array(bad), fake, p64, p64, 1 << 30, None) == _lib.EINVAL, bad
            assert b"boundary" in lib.ndmps_last_error()
    # the scatter entries: tables for another number of columns, a chain without a tail, NULL tables
    n_cols = lib.ndmps_chain_tail_columns(L, d)
    scatter = lib.ndmps_chain_contract_scatter_f32
    assert scatter(L, d, b, fake, p64, p64, p64, p64, n_cols * dims[-2], p64, 1 << 30, None) == _lib.EINVAL
    assert b"tail columns" in lib.ndmps_last_error()
    assert scatter(L, d, b, fake, p64, p64, p64, p64, n_cols, p64, need - 1, None) == _lib.EWORKSPACE
    assert scatter(L, d, b, fake, p64, None, p64, p64, n_cols, p64, 1 << 30, None) == _lib.EINVAL
    nt_dims, nt_bonds = cc.CHAINS["L3_no_tail"]
    assert scatter(3, _lib.i64_array(nt_dims), _lib.i64_array(nt_bonds), fake, p64, p64, p64, p64, nt_dims[-1], p64,
                   1 << 30, None) == _lib.EINVAL
    batched = lib.ndmps_chain_contract_scatter_batched_f32
    for batch in (1, 3):  # in turn / together
        cores, outs = (C.c_void_p * (batch * L))(*[64] * (batch * L)), (C.c_void_p * batch)(*[64] * batch)
        flat = _lib.i64_array(list(bonds) * batch)
        assert batched(batch, L, d, flat, cores, outs, p64, p64, p64, n_cols + 1, p64, 1 << 30, None) == _lib.EINVAL
        assert b"tail columns" in lib.ndmps_last_error()
        bad = _lib.i64_array([1, 4, 13, 13, 1] * batch)
        assert batched(batch, L, d, bad, cores, outs, p64, p64, p64, n_cols, p64, 1 << 30, None) == _lib.EINVAL
        assert b"exceeds" in lib.ndmps_last_error()
        assert batched(batch, L, d, flat, cores, outs, p64, p64, p64, n_cols, p64, need - 1, None) == _lib.EWORKSPACE
    outs = (C.c_void_p * 3)(64, None, 64)
    cores = (C.c_void_p * (3 * L))(*[64] * (3 * L))
    flat = _lib.i64_array(list(bonds) * 3)
    assert batched(3, L, d, flat, cores, outs, p64, p64, p64, n_cols, p64, 1 << 30, None) == _lib.EINVAL
    assert batched(0, L, d, flat, cores, outs, p64, p64, p64, n_cols, p64, 1 << 30, None) == _lib.EINVAL
