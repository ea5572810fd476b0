"""CPU tests of tests/sweep_cases.py: the planted-rank cases for the TT-SVD sweep are well posed BEFORE any GPU is
involved.  Per case and member: the fp64 reference finds the planted bonds (min(planted, cap) where a cap cuts);
every rank decision sits in a relative gap of at least 1e-2; the sweep emulated at the storage precision decides the same
ranks; the gauge-free comparisons detect what they are meant to detect; and, where the library has a host query, the
case reaches the route it names.  If a check fails for a case, the case (its seed, its tail) changes, not the check.
"""
import ctypes as C

import numpy as np
import pytest

import sweep_cases as sc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.utils import core as hc

NAMES = list(sc.CASES)
GAP = 1e-2


@pytest.mark.parametrize("name", NAMES)
def test_reference_finds_the_planted_bonds(name):
    for b, (_, ref, _) in enumerate(sc.sweeps(name)):
        assert ref["bonds"] == sc.expected_bonds(name, b), (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_every_rank_decision_sits_in_a_gap(name):
    """A condition on the cases, not a measurement: behind the last kept value of EVERY bond the reference's spectrum
    drops by at least 1e-2 s_0 -- (s_k - s_{k+1}) / s_0 where a cap or the cutoff cuts, s_k / s_0 where nothing follows
    (relative_gap takes s_{k+1} = 0 there) -- and what the cutoff drops is below the storage type's cutoff floor."""
    case = sc.CASES[name]
    for b, (_, ref, _) in enumerate(sc.sweeps(name)):
        for i, k in enumerate(ref["bonds"], start=1):
            s = ref["spectra"][i]
            assert sc.relative_gap(s, k) >= GAP, (name, b, i, k, sc.relative_gap(s, k))
            if k < len(s) and not (case["cap"] and k == case["cap"]):  # cut by the cutoff: exactly the planted rank
                assert s[k] <= 1e-3 * sc.CUTOFF_FLOOR[case["storage"]] * s[0], (name, b, i, s[k] / s[0])


@pytest.mark.parametrize("name", NAMES)
def test_emulated_sweep_decides_the_same_ranks(name):
    for b, (_, ref, emu) in enumerate(sc.sweeps(name)):
        assert emu["bonds"] == ref["bonds"], (name, b)
        assert [c.shape for c in emu["cores"]] == [c.shape for c in ref["cores"]]


@pytest.mark.parametrize("name", NAMES)
def test_reference_cores_are_isometries_and_yardsticks_are_small(name):
    case = sc.CASES[name]
    sf, u = case["sweep_from"], sc.U[case["storage"]]
    for b, (x, ref, emu) in enumerate(sc.sweeps(name)):
        L = len(ref["cores"])
        inner = range(1, L) if sf == "right" else range(L - 1)
        for i in inner:
            assert sc.isometry_defect(ref["cores"][i], sf) <= 1e-14, (name, b, i)
            # rounded once: 2 u by Cauchy-Schwarz, headroom 2; truncation to bf16 errs by up to 2 u per entry; fp64 is
            # LAPACK's own orthogonality
            bound = {"f32": 4 * u, "bf16": 8 * u, "f64": 1e-14}[case["storage"]]
            assert sc.isometry_defect(emu["cores"][i], sf) <= bound, (name, b, i)
        end, w_end = (0, 1) if sf == "right" else (L - 1, L - 1)
        assert sc.site0_defect(ref["cores"][end], ref["bases"][w_end], x, sf) <= 1e-14
        for i in range(1, L):
            # the yardstick of a GPU comparison: the emulated sweep against the reference, far from an unrelated subspace
            s, k = ref["spectra"][i], ref["bonds"][i - 1]
            theta = sc.max_sin_theta(emu["bases"][i], ref["bases"][i])
            assert theta <= 64 * u / sc.relative_gap(s, k) + 1e-14, (name, b, i, theta)


def test_planted_volume_has_unit_rms_and_the_planted_ranks():
    x = sc.planted_volume((12, 44, 18), [5, 4], 3)
    assert x.shape == (12, 44, 18) and abs(np.sqrt(np.mean(x * x)) - 1.0) <= 1e-12
    dims = sc.site_dims(x.shape)
    assert dims == [int(q) for q in hc.get_factorlist(x.shape)[0].prod(axis=1)] == [44, 12, 18]
    t = sc.to_site_order(x).reshape(dims)
    assert np.linalg.matrix_rank(t.reshape(44, -1), tol=1e-9) == 5
    assert np.linalg.matrix_rank(t.reshape(-1, 18), tol=1e-9) == 4
    assert np.array_equal(sc.from_site_order(sc.to_site_order(x), x.shape), x)
    y = sc.planted_volume((12, 44, 18), [5, 4], 3, tail=([9, 9], 1e-2))
    s = np.linalg.svd(sc.to_site_order(y).reshape(-1, 18), compute_uv=False)
    # 4 planted values, a gap, then the 9 of the tail (ranks add: 13 of the 18 possible), then nothing
    assert s[3] / s[0] > 0.05 > 0.02 > s[4] / s[0] and s[12] / s[0] > 1e-5 > 1e-12 > s[13] / s[0]


def test_bases_are_the_products_of_the_cores():
    x = sc.planted_volume((16, 16, 16), [5, 11, 6], 7)
    for sf in ("right", "left"):
        ref = sc.reference_sweep(x, sweep_from=sf)
        dense = sc.to_site_order(x)
        for i in range(1, 4):
            w = ref["bases"][i]
            assert np.abs(w @ w.T - np.eye(w.shape[0])).max() <= 1e-14
            # the volume lies in the kept subspace of every bond (exact ranks): projecting changes nothing
            mat = dense.reshape(-1, w.shape[1]) if sf == "right" else dense.reshape(w.shape[1], -1).T
            assert np.linalg.norm(mat - (mat @ w.T) @ w) <= 1e-12 * np.linalg.norm(dense)
    assert sc.reference_sweep(x, sweep_from="left")["bonds"] == sc.reference_sweep(x)["bonds"] == [5, 11, 6]


def test_max_sin_theta_ignores_gauge_and_sees_a_tilt():
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((40, 9)))[0].T  # 9 orthonormal rows
    w, perp = q[:6], q[6:]
    signs = np.diag([1, -1, -1, 1, -1, 1.0])
    rot = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    assert sc.max_sin_theta(signs @ w, w) <= 1e-15
    assert sc.max_sin_theta(rot @ w, w) <= 1e-15
    for angle in (1e-10, 1e-6, 1e-3, 0.3):
        tilted = w.copy()
        tilted[5] = np.cos(angle) * w[5] + np.sin(angle) * perp[1]  # one vector leaves the subspace by `angle`
        got = sc.max_sin_theta(rot @ tilted, signs @ w)
        assert abs(got - np.sin(angle)) <= 1e-6 * np.sin(angle) + 1e-16, (angle, got)
        # ... and it is the definition: sqrt(1 - sigma_min(Wa Wb^T)^2), where that form has the digits
        if angle >= 1e-3:
            smin = np.linalg.svd(tilted @ w.T, compute_uv=False)[-1]
            assert abs(got - np.sqrt(1 - smin ** 2)) <= 1e-10
    swapped = np.vstack([w[:5], perp[:1]])  # a wrong trailing vector: orthogonal to the right one
    assert sc.max_sin_theta(swapped, w) >= 1 - 1e-12
    assert sc.max_sin_theta(w[:5], w) == 1.0  # different ranks never agree


def test_isometry_and_site0_defects_see_a_wrong_core():
    x = sc.planted_volume((16, 16, 16), [8, 8, 8], 5)
    ref = sc.reference_sweep(x, max_bond=8)
    core = ref["cores"][2].copy()
    assert sc.isometry_defect(core) <= 1e-14
    core[3] *= 1 + 1e-5
    assert 1.9e-5 <= sc.isometry_defect(core) <= 2.1e-5
    c0 = ref["cores"][0].copy()
    assert sc.site0_defect(c0, ref["bases"][1], x) <= 1e-14
    c0[0, 2, 5] += 1e-4 * np.linalg.norm(sc.to_site_order(x))
    assert 0.99e-4 <= sc.site0_defect(c0, ref["bases"][1], x) <= 1.01e-4
    left = sc.reference_sweep(x, max_bond=8, sweep_from="left")
    assert sc.isometry_defect(left["cores"][1], "left") <= 1e-14 < sc.isometry_defect(left["cores"][3], "left")
    assert sc.site0_defect(left["cores"][3], left["bases"][3], x, "left") <= 1e-14


def test_round_to_and_unit_roundoffs():
    a = np.random.default_rng(1).standard_normal(4096)
    for storage, worst in (("f32", sc.U["f32"]), ("bf16", 2 * sc.U["bf16"]), ("f64", 0.0)):
        err = np.abs(sc.round_to(a, storage) - a) / np.abs(a)
        assert err.max() <= worst and (storage == "f64" or err.max() >= worst / 4)
    assert np.all(sc.round_to(a, "bf16").astype(np.float32).view(np.uint32) & 0xFFFF == 0)


# ------------------------------------------------------------------------------------------------ routes
def _layout(dims, cap):
    lib = _lib.load()
    L = len(dims)
    mb, co, so = ((C.c_int64 * (L + 1))() for _ in range(3))
    _lib.check(lib.ndmps_tt_layout(L, _lib.i64_array(dims), cap or 0, mb, co, so, None))
    return [int(v) for v in mb]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_route(name, monkeypatch):
    """The host queries of the library (no GPU needed), per case: bond caps of the layout, the merge width of the fused
    encode, whether the ranks are decided on the device, whether the permutation plan is tiled."""
    for env in sc.SWITCHES + ("NDMPS_EXACT_JACOBI", "NDMPS_NO_FUSED_ENCODE"):
        monkeypatch.delenv(env, raising=False)
    lib = _lib.load()
    case = sc.CASES[name]
    dims = sc.site_dims(case["shape"])
    if case["sweep_from"] == "left":
        dims = dims[::-1]
    L, cap, cd = len(dims), case["cap"] or 0, _lib.i64_array(dims)
    numel = int(np.prod(dims))
    caps = _layout(dims, cap)
    for b in range(len(case["members"])):
        bonds = sc.expected_bonds(name, b)
        if case["sweep_from"] == "left":
            bonds = bonds[::-1]
        assert all(k <= c for k, c in zip(bonds, caps[1:L])), (name, bonds, caps)
    merge_n = int(lib.ndmps_tt_merge_columns(L, cd, cap))
    pads = int(lib.ndmps_tt_sweep_pads_cores(L, cd, cap))
    start = sc.merge_start(dims, cap)
    route = case["route"]
    if "fused encode" in route:
        three = "three-site" in route
        assert case["storage"] == "f32" and merge_n == int(np.prod(dims[start:])) == (512 if three else 64)
        assert start == (L - 3 if three else L - 2)
        # the streamed gathered projection serves a merge width of 64 with k = 32 or 64; anything else the tile kernel
        assert ("gathered projection" in route) == (merge_n == 64 and cap in (32, 64))
    elif "unfused" in route:
        # a merged run on the site-order tensor: too few rows for the fused encode (16^3), or not fp32 storage
        assert start == L - 2 and (merge_n == 0 or case["storage"] != "f32")
    if "no merged run" in route or "exact" in route:
        assert merge_n == 0 and start == L
    if "generic permutation" in route:
        f = np.ascontiguousarray(hc.get_factorlist(case["shape"])[0], dtype=np.int64)
        out = np.empty(numel, dtype=np.int64)
        shp = _lib.i64_array(case["shape"])
        assert lib.ndmps_plan_emulate(len(case["shape"]), shp, f.shape[0], f.ctypes.data_as(_lib.p_i64), 2,
                                      out.ctypes.data_as(_lib.p_i64)) == 0
    if "host rank decision" in route:
        assert cap > sc.TOPK_MAX_K == lib.ndmps_syevd_topk_max_k() and pads == 0 and start == L - 2 and merge_n == 0
        assert max(caps) > sc.TOPK_MAX_K  # a bond beyond 128 is possible, and one member plants it
        assert max(max(sc.expected_bonds(name, b)) for b in range(len(case["members"]))) > sc.TOPK_MAX_K
    elif cap:
        assert pads == 1  # ranks decided on the device, cap-shaped cores
    else:
        assert pads == 0
    if "padded cores" in route:  # some member stays below the cap at a bond the cap could bind
        assert any(k < c for b in range(len(case["members"])) for k, c in zip(sc.expected_bonds(name, b), caps[1:L]))
    if name == "cap32_f32":  # site 3 (the first behind the merged run) has order d_3 * cap = 256
        assert dims[3] * caps[4] == 256 and numel // int(np.prod(dims[3:])) >= 256
    # The switches the case is also run under, where a host query shows their effect: each must change the answer, so a
    # switch the library ignored would fail here.  NDMPS_SWEEP_JACOBI without a cap and NDMPS_EXACT_JACOBI only choose
    # the eigen-solver of an exact sweep; no host query depends on that, and only the GPU suite sees them.
    members = len(case["members"])
    ws_default = lib.ndmps_tt_sweep_batched_workspace_bytes(members, L, cd, cap)
    for env in case["routes"]:
        monkeypatch.setenv(env, "1")
        if env == "NDMPS_SWEEP_NO_MERGE":  # no merged run: no fused encode, none of the run's buffers in the workspace
            assert start < L and lib.ndmps_tt_merge_columns(L, cd, cap) == 0
            assert 0 < lib.ndmps_tt_sweep_batched_workspace_bytes(members, L, cd, cap) < ws_default
        elif env in ("NDMPS_SWEEP_HOST_RANK", "NDMPS_SWEEP_JACOBI") and cap:  # ranks decided on the host, compact cores
            assert pads == 1 and lib.ndmps_tt_sweep_pads_cores(L, cd, cap) == 0
        else:
            assert not cap and env in ("NDMPS_SWEEP_JACOBI", "NDMPS_EXACT_JACOBI")
        monkeypatch.delenv(env)


def test_the_cases_cover_what_they_must():
    by = lambda word: [n for n, c in sc.CASES.items() if word in c["route"]]  # noqa: E731
    assert by("fused encode") and by("gathered projection") and by("unfused") and by("no merged run") and by("exact")
    assert by("host rank decision") and by("mirrored") and by("padded cores") and by("three-site merged run")
    # every route switch has a case that is run under it
    assert {e for c in sc.CASES.values() for e in c["routes"]} == set(sc.SWITCHES) | {"NDMPS_EXACT_JACOBI"}
    # a tail's rank adds to the planted rank; every bond of a member with a tail is cut by the cap or by the shape
    for n, c in sc.CASES.items():
        dims = sc.site_dims(c["shape"])
        for b, m in enumerate(c["members"]):
            if m["tail"] is not None:
                full = [min(int(np.prod(dims[:i])), int(np.prod(dims[i:]))) for i in range(1, len(dims))]
                assert sc.expected_bonds(n, b) == [min(f, c["cap"]) for f in full], (n, b)
    assert {sc.CASES[n]["storage"] for n in NAMES} == {"f32", "f64", "bf16"}
    assert all(len(sc.site_dims(sc.CASES[n]["shape"])) >= 3 for n in NAMES)
    members = sc.CASES["nonuniform_group"]["members"]
    assert len(members) == 3
    b = [sc.expected_bonds("nonuniform_group", i) for i in range(3)]
    cap = sc.CASES["nonuniform_group"]["cap"]
    assert b[0][1] < cap == b[1][1] == b[2][1] and members[2]["ranks"][1] == cap + 1 and members[1]["ranks"][1] == cap
