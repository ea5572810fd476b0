"""The cases and bars of tests/pairstat_cases.py, on the host (no GPU): the table holds the cases the kernel's paths
need, the bars accept the reference, and every modelled fault is rejected on every case it can occur on (each can
occur on at least one).
"""
import numpy as np
import pytest

import pairstat_cases as pc
import valstat_cases as vc
from oracle import chain_cases as cc


def _rejects(fault, case, bar, *args):
    with pytest.raises(AssertionError):
        bar(*args)
    print(f"[pairstat] {case}: {fault} rejected")


def test_the_table_holds_the_cases_the_kernel_needs():
    ks = {}
    for name, bonds_b in list(pc.REAL_PAIRS.items()) + list(pc.INT_PAIRS.items()):
        dims, bonds_a = pc.CHAINS[name]
        cc.check_chain(dims, bonds_a)
        cc.check_chain(dims, bonds_b)
        assert len(bonds_b) == len(bonds_a)
        ks[name] = (pc.last_k(dims, bonds_a), pc.last_k(dims, bonds_b))
    real = {n: ks[n] for n in pc.REAL_PAIRS}
    assert any(a < b for a, b in real.values()) and any(a > b for a, b in real.values())
    # the k of a pair on either side of a multiple of the k-tile, in both element types, both ways round
    for kt in pc.K_TILE.values():
        tiles = lambda k: -(-k // kt)  # noqa: E731
        assert any(tiles(a) < tiles(b) and (a % kt or b % kt) for a, b in real.values()), kt
        assert any(tiles(a) > tiles(b) and (a % kt or b % kt) for a, b in real.values()), kt
    assert ks["L4_tail_last"] == (13, 40) and ks["L5_tail_last"] == (33, 16)
    assert any(min(pc.REAL_PAIRS[n]) == max(pc.REAL_PAIRS[n]) == 1 and max(pc.CHAINS[n][1]) > 1 for n in real)
    shapes = {n: vc.last_product_shape(pc.CHAINS[n][0]) for n in ks}
    assert shapes["L4_no_tail"] == shapes["int_no_tail"] == (12, 8192)
    assert shapes["L5_ragged"][0] % 64 and shapes["L5_ragged"][1] % 64
    assert shapes["L4_tail_4096"][1] == 4096 and cc.tail_start(pc.CHAINS["L4_tail_4096"][0]) == 1
    assert cc.tail_start(pc.CHAINS["L4_tail_last"][0]) == 3
    assert {len(pc.CHAINS[n][0]) for n in real} >= {1, 2}
    assert set(pc.INT_PAIRS) == set(cc.INTEGER_CHAINS) | {"int_8x7", "int_many_tiles"}
    for name, bonds_b in pc.INT_PAIRS.items():
        assert int(np.prod(bonds_b, dtype=np.int64)) < 2 ** 24 and int(np.prod(pc.CHAINS[name][1], dtype=np.int64)) < 2 ** 24
    m, n = shapes["int_8x7"]
    # 512 tiles: one per workgroup of the 512 a launch has at most, two per workgroup of the 256 that a joint histogram
    # above 64 KiB of LDS (the 1024 x 16 edge pair) is held to
    assert m * n == 2 ** 21 and (m // 64) * (n // 64) == 512
    m, n = shapes["int_many_tiles"]
    assert -(-m // 64) * -(-n // 64) > 512 and n % 64  # a second tile for some workgroups of every launch, the last ragged
    # the faults that cannot occur everywhere can occur somewhere, among the real and among the integer pairs (the bar
    # tests below reject every fault wherever it occurs): unequal k at the last product, padded tiles
    for names in (pc.REAL_PAIRS, pc.INT_PAIRS):
        assert any(ks[n][0] != ks[n][1] and len(pc.CHAINS[n][0]) > 1 for n in names)
        assert any(shapes[n][0] % pc.TILE or shapes[n][1] % pc.TILE for n in names)


@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.REAL_NAMES)
def test_sandwich_bar_on_the_reference_and_on_modelled_faults(name, storage):
    p = pc.pair(name, "uniform", storage)
    a, b = p.a, p.b
    ea, eb = a.edges64(), b.edges64()
    assert vc.near_edge_fraction(a.ref, a.bound, ea) <= 0.01 and vc.near_edge_fraction(b.ref, b.bound, eb) <= 0.01
    bars = (a.ref, a.bound, b.ref, b.bound)

    def stats_bar(ra, rb):
        pc.sandwich_pair_stats(pc.ref_pair_stats(ra, rb), *bars)

    def joint_bar(ra, rb):
        pc.sandwich_joint(*pc.ref_joint(ra, rb, ea, eb), *bars, ea, eb)

    stats_bar(a.ref, b.ref)
    joint_bar(a.ref, b.ref)
    case = f"{name}/{storage}"
    for fault, volumes in (("wrong_k", pc.fault_wrong_k(p)), ("swapped", pc.fault_swapped(p)),
                           ("b_tile_shifted", pc.fault_b_tile_shifted(p)), ("padding_counted", pc.fault_padding_counted(p)),
                           ("tile_left_out", pc.fault_tile_left_out(p))):
        if volumes is None:
            continue
        _rejects(fault + "/stats", case, stats_bar, *volumes)
        _rejects(fault + "/joint", case, joint_bar, *volumes)
    assert (pc.fault_wrong_k(p) is None) == (p.k_a == p.k_b or len(p.dims) == 1)
    assert (pc.fault_padding_counted(p) is None) == (p.m % pc.TILE == 0 and p.cols % pc.TILE == 0)


@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.INT_NAMES)
def test_exact_bar_on_the_reference_and_on_modelled_faults(name, storage):
    p = pc.pair(name, "integer", storage)
    ra, rb = p.a.ref, p.b.ref
    for r in (ra, rb):
        assert np.array_equal(r, np.round(r)) and np.abs(r).max() < 2 ** 24
    # every sum the record holds is a sum of integers that stays below 2**53: exact in any order
    assert p.n * max(np.abs(ra).max(), np.abs(rb).max(), np.abs(ra - rb).max()) ** 2 < 2 ** 53
    pc.exact_pair_stats(pc.ref_pair_stats(ra, rb), ra, rb)
    case = f"{name}/{storage}"
    volume_faults = [(f, v) for f, v in (("wrong_k", pc.fault_wrong_k(p)), ("swapped", pc.fault_swapped(p)),
                                         ("b_tile_shifted", pc.fault_b_tile_shifted(p)),
                                         ("padding_counted", pc.fault_padding_counted(p)),
                                         ("tile_left_out", pc.fault_tile_left_out(p))) if v is not None]
    for fault, volumes in volume_faults:
        _rejects(fault + "/stats", case, pc.exact_pair_stats, pc.ref_pair_stats(*volumes), ra, rb)
    _, rb_nan = vc.with_nan(p.b)
    k = int(np.isnan(rb_nan).sum())
    assert 0 < k < p.n
    pc.exact_pair_stats(pc.ref_pair_stats(ra, rb_nan), ra, rb_nan)
    sets = pc.integer_edge_pairs(ra, rb, pc.NP_TYPE[storage])
    assert [tuple(e.size - 1 for e in sets[s]) for s in ("1x1", "1x1024", "1024x16")] == [(1, 1), (1, 1024), (1024, 16)]
    assert float(sets["last_edges"][1][-1]) == rb.max()
    for label, (ea, eb) in sets.items():
        assert ea.size - 1 <= 1024 and eb.size - 1 <= 1024 and (ea.size - 1) * (eb.size - 1) <= 16384, label
        assert np.all(np.diff(ea.astype(np.float64)) >= 0) and np.all(np.diff(eb.astype(np.float64)) >= 0), label
        pc.exact_joint(*pc.ref_joint(ra, rb, ea, eb), ra, rb, ea, eb)
        # a fault that moves voxels between values shows where the bins are fine (one cell holds whatever it is given)
        for fault, volumes in volume_faults if label == "128x128" else ():
            _rejects(fault + "/joint", case, pc.exact_joint, *pc.ref_joint(*volumes, ea, eb), ra, rb, ea, eb)
        pc.exact_joint(*pc.ref_joint(ra, rb_nan, ea, eb), ra, rb_nan, ea, eb)
        for fault, report in (("nan_of_b_ignored", pc.fault_nan_of_b_ignored(ra, rb_nan, ea, eb)),):
            assert report is not None
            _rejects(fault, case, pc.exact_joint, *report, ra, rb_nan, ea, eb)
        for fault, report in (("outside_on_a_alone", pc.fault_outside_on_a_alone(ra, rb, ea, eb)),
                              ("last_bin_open_on_b", pc.fault_last_bin_open_on_b(ra, rb, ea, eb))):
            if report is not None:
                _rejects(fault, case, pc.exact_joint, *report, ra, rb, ea, eb)
    assert pc.fault_outside_on_a_alone(ra, rb, *sets["1024x16"]) is not None, "the excluding range excludes nothing"
    assert pc.fault_last_bin_open_on_b(ra, rb, *sets["last_edges"]) is not None, "no voxel on the last edge"
