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


# ------------------------------------------------------------------------------------------------ the model family
def test_carry_product_sums_in_the_accumulator_in_steps():
    """``"steps"`` against a plain loop written out here: fp32 running sum over exact pairs (f32), over exact runs of 16
    with one rounding to bf16 at the end (bf16), fp64 over runs of 4 (f64); ``reverse`` walks the same chunks backwards;
    ``"exact"`` is the fp64 product rounded once."""
    rng = np.random.default_rng(5)
    for storage, acc_t, step in (("f32", np.float32, 2), ("bf16", np.float32, 16), ("f64", np.float64, 4)):
        assert sc.KSTEP[storage] == step
        mat = sc.round_to(rng.standard_normal((7, 37)), storage)  # 37: the last chunk is short
        core = sc.round_to(rng.standard_normal((3, 37)), storage)
        assert np.array_equal(sc.carry_product(mat, core, storage), sc.round_to(mat @ core.T, storage))
        for reverse in (False, True):
            want = np.zeros((7, 3), dtype=acc_t)
            starts = list(range(0, 37, step))
            for c in (starts[::-1] if reverse else starts):
                chunk = np.zeros((7, 3))
                for kk in range(c, min(c + step, 37)):
                    chunk += np.outer(mat[:, kk], core[:, kk])
                want = (want.astype(np.float64) + chunk).astype(acc_t)
            got = sc.carry_product(mat, core, storage, "steps", reverse)
            # the chunk itself is summed by BLAS here and term by term above: both exact for fp32 / bf16 data
            assert np.array_equal(got, sc.round_to(want, storage)) or storage == "f64"
            assert np.abs(got - sc.round_to(want, storage)).max() <= 4 * sc.U["f64"] * np.abs(mat).max() * np.abs(core).max() * 37
        fwd, bwd = (sc.carry_product(mat, core, storage, "steps", r) for r in (False, True))
        assert storage == "bf16" or not np.array_equal(fwd, bwd)  # two orders, two roundings
        if storage == "f32":  # the running fp32 sum is NOT the product rounded once
            assert not np.array_equal(fwd, sc.carry_product(mat, core, storage))


def test_gram_route_restates_the_header_of_tt_hip():
    rng = np.random.default_rng(6)
    tall, wide = rng.standard_normal((40, 12)), rng.standard_normal((9, 30))
    for mat in (tall, wide):
        s, rows, u = sc._site_gram(mat)
        s_ref, vh = sc._site_svd(mat)
        r = min(mat.shape)
        assert np.abs(s[:r] - s_ref).max() <= 1e-13 * s_ref[0]
        assert np.abs(np.abs(rows[:r] @ vh.T) - np.eye(r)).max() <= 1e-10  # the same vectors up to sign
        if mat.shape[1] <= mat.shape[0]:
            assert u is None
        else:  # core = diag(1/s) U^T A, carry = U diag(s): their product is A
            assert np.array_equal(rows, (1.0 / s)[:, None] * (u.T @ mat))
            assert np.abs((u * s) @ rows - mat).max() <= 1e-13 * s[0]
    x = sc.volumes("merged16_f64")[0]
    emu = sc.emulated_sweep(x, max_bond=8, storage="f64", route="gram")
    ref = sc.sweeps("merged16_f64")[0][1]
    assert emu["bonds"] == ref["bonds"]
    # site 1 is the n > m site (8 x 64): carry U_k s_k, so site 0 has orthogonal columns of norms s
    c0 = emu["cores"][0].reshape(8, 8)
    assert np.abs(c0.T @ c0 - np.diag(emu["spectra"][1][:8] ** 2)).max() <= 1e-12 * emu["spectra"][1][0] ** 2


@pytest.mark.parametrize("name", NAMES)
def test_every_model_of_the_family_decides_the_reference_ranks(name):
    """``yardstick`` raises when a model decides other bonds than the reference; here also: every model is there, every
    (member, bond) and every inner core has a yardstick, and no value lies below its floor."""
    case = sc.CASES[name]
    u, sf = sc.U[case["storage"]], case["sweep_from"]
    yards = sc.yardstick(name)
    assert len(yards) == len(case["members"])
    for b, (yard, (_, ref, _)) in enumerate(zip(yards, sc.sweeps(name))):
        L = len(ref["cores"])
        assert set(yard["models"]) == set(sc.MODELS) and len(sc.MODELS) == 6
        assert sorted(yard["theta"]) == sorted(yard["spec"]) == list(range(1, L))
        assert sorted(yard["iso"]) == (list(range(1, L)) if sf == "right" else list(range(L - 1)))
        assert min(yard["theta"].values()) >= u and min(yard["iso"].values()) >= u and yard["site0"] >= u <= yard["recon"]
        for i in range(1, L):
            assert len(yard["spec"][i]) == ref["bonds"][i - 1] and yard["spec"][i].min() >= u * ref["spectra"][i][0]
        for q in yard["models"].values():  # the maximum over the family
            assert all(yard["theta"][i] >= q["theta"][i] for i in q["theta"]) and yard["recon"] >= q["recon"]


def test_accumulating_in_steps_exceeds_rounding_once_on_cap32_f32():
    """Why the family exists: the fp32 running sum of the carry product moves the kept subspace several times further
    than one rounding of an fp64 product does."""
    worst = 0.0
    for yard in sc.yardstick("cap32_f32"):
        once, steps = yard["models"][("svd", "exact", False)], yard["models"][("svd", "steps", False)]
        worst = max([worst] + [steps["theta"][i] / once["theta"][i] for i in once["theta"]]
                    + [steps["site0"] / once["site0"]])
    assert worst > 4.0, worst
    for yard in sc.yardstick("cap32_bf16"):  # one rounding to bf16 behind an fp32 sum: the order hardly shows
        once, steps = yard["models"][("svd", "exact", False)], yard["models"][("svd", "steps", False)]
        assert max(steps["theta"][i] / once["theta"][i] for i in once["theta"]) < 1.5


def test_gram_route_loses_orthogonality_at_the_wide_sites_of_cap32_f64():
    for b, yard in enumerate(sc.yardstick("cap32_f64")):
        svd, gram = yard["models"][("svd", "exact", False)]["iso"], yard["models"][("gram", "exact", False)]["iso"]
        wide = [site for _, (site, m, n) in sc._swept_sites("cap32_f64", b).items() if n > m]
        assert wide == [1, 2]
        assert max(gram[i] for i in wide) > 4 * max(svd.values()), (b, gram, svd)
        assert all(gram[i] <= 8 * sc.U["f64"] for i in gram if i not in wide)  # eigenvectors, polished: a few u


def test_summation_order_spread_sets_the_margin():
    """R: the largest ratio of one quantity between the "steps" model summed forwards and backwards, over all cases,
    members, sites and both routes.  MARGIN = max(4, 2 R rounded up to a power of two) and R stays below MARGIN / 2."""
    spread = {}
    for name in NAMES:
        for yard in sc.yardstick(name):
            for q, v in yard["spread"].items():
                spread[q] = max(spread.get(q, 1.0), v)
    r = max(spread.values())
    print("R per quantity:", {q: round(v, 3) for q, v in spread.items()}, "margin", sc.MARGIN)
    assert set(spread) == {"theta", "iso", "site0", "spec", "recon"}
    assert r < sc.MARGIN / 2, spread
    assert sc.MARGIN == max(4.0, 2.0 ** np.ceil(np.log2(2 * r))), (r, sc.MARGIN)


def test_no_subspace_bar_is_vacuous():
    assert sum(yard["vacuous"] for name in NAMES for yard in sc.yardstick(name)) == 0
    worst = max(sc.MARGIN * v + sc.solver_terms(name, b)["theta"][i]
                for name in NAMES for b, yard in enumerate(sc.yardstick(name)) for i, v in yard["theta"].items())
    assert worst < sc.VACUOUS == 0.1, worst


def test_solver_terms_follow_the_solver_contract():
    assert sc.solver_eps(8) == sc.solver_eps(50) == 1e-13 and sc.solver_eps(256) == 2e-15 * 256
    for name in NAMES:
        u = sc.U[sc.CASES[name]["storage"]]
        for b, (_, ref, _) in enumerate(sc.sweeps(name)):
            sol = sc.solver_terms(name, b)
            assert sol["site0"] == 0.0 == sol["recon"]
            sites = sc._swept_sites(name, b)
            for i, (site, m, n) in sites.items():
                s, k = ref["spectra"][i], ref["bonds"][i - 1]
                eps = sc.solver_eps(min(m, n))
                gap2 = (s[k - 1] ** 2 - (s[k] ** 2 if k < len(s) else 0.0)) / s[0] ** 2
                assert sol["theta"][i] == eps / gap2 and np.array_equal(sol["spec"][i], eps * s[0] ** 2 / s[:k])
                assert sol["iso"][site] == (eps if n <= m else eps * (s[0] / s[k - 1]) ** 2)
                if u > 1e-10:  # f32 and bf16: far below u
                    assert max(sol["theta"][i], sol["iso"][site], sol["spec"][i].max() / s[0]) <= 0.1 * u
    sol = sc.solver_terms("cap32_f64", 0)
    assert 1e-12 < max(sol["theta"].values()) < 1e-9  # about 1e4 u: legitimate for fp64 storage


# ------------------------------------------------------------------------------------------------ the comparator
MUTATED = ["cap32_f32", "nonuniform_group", "cap32_f64", "cap32_bf16"]
_STEPS = {}


def _steps(name, member, tamper=None):
    """The "steps" model's own output (SVD route, forwards) for a member; untampered ones are cached."""
    case = sc.CASES[name]
    if tamper is None and (name, member) in _STEPS:
        return _STEPS[(name, member)]
    x = sc.sweeps(name)[member][0]
    emu = sc.emulated_sweep(x, case["cutoff"], case["cap"], case["sweep_from"], case["storage"], "steps", "svd", tamper=tamper,
                            polish=case["storage"] == "f64")
    if tamper is None:
        _STEPS[(name, member)] = emu
    return emu


def _check(name, member, cores, spectra, recon=None, **kw):
    """check_sweep without solver terms: the models' vectors come from LAPACK, not from the device's solver."""
    x, ref, _ = sc.sweeps(name)[member]
    recon = sc.reconstruction(cores, x.shape) if recon is None else recon
    return sc.check_sweep(cores, spectra, recon, x, ref, sc.yardstick(name)[member], (name, member), sc.MARGIN, None, **kw)


def _raises(check, name, member, *args, **kw):
    with pytest.raises(sc.SweepCheckError) as err:
        _check(name, member, *args, **kw)
    assert err.value.check == check, str(err.value)
    assert f"{name}[{member}]" in str(err.value)
    return str(err.value)


@pytest.mark.parametrize("name", MUTATED)
def test_check_sweep_passes_on_the_models_own_output(name):
    for member in range(len(sc.CASES[name]["members"])):
        emu = _steps(name, member)
        got = _check(name, member, emu["cores"], emu["spectra"])
        assert set(got) == {"theta", "iso", "site0", "spec", "recon"}
        cores = emu["cores"]
        end = 0 if sc.CASES[name]["sweep_from"] == "right" else len(cores) - 1
        _check(name, member, cores, emu["spectra"], boundary=[[c.min(), c.max()] for c in cores],
               norm_value=np.linalg.norm(cores[end]))


@pytest.mark.parametrize("name", [n for n in MUTATED if n.startswith("cap32")])
def test_check_sweep_sees_a_term_left_out_of_one_carry_product(name):
    """Site 3 of the cap32 cases is the site of order 256 (512 x 256, k = 32): its carry product without the term
    k = 100.  What it carries to the left is then not the volume on the kept basis: the end of the chain is off it."""
    def drop(i, mat, core, carry):
        if i != 3:
            return carry
        assert mat.shape == (512, 256) and core.shape == (32, 256)
        return sc.round_to(carry - np.outer(mat[:, 100], core[:, 100]), sc.CASES[name]["storage"])

    emu = _steps(name, 0, tamper={"carry": drop})
    x, ref, _ = sc.sweeps(name)[0]
    assert emu["bonds"] == ref["bonds"]
    # what is decomposed to the left of site 3 is another matrix: the first check that meets it is the subspace of the
    # bonds 1 and 2; bonds 3 .. 5 were finished before and stay within the bar
    msg = _raises("theta", name, 0, emu["cores"], emu["spectra"])
    assert "bond 1" in msg or "bond 2" in msg
    yard = sc.yardstick(name)[0]
    got = sc.sweep_quantities(emu["cores"], emu["spectra"], sc.reconstruction(emu["cores"], x.shape), x, ref, "right")
    assert all(got["theta"][i] <= sc.MARGIN * yard["theta"][i] for i in (3, 4, 5))
    assert got["theta"][2] > 100 * yard["theta"][2] or name == "cap32_bf16"
    # and the volume is not the reference's (one term of 256 is inside bf16's own bar: there only the subspace shows it)
    assert got["recon"] > sc.MARGIN * yard["recon"] or name == "cap32_bf16"


@pytest.mark.parametrize("name", MUTATED)
def test_check_sweep_sees_a_wrong_trailing_vector(name):
    """The last kept vector of bond 3 replaced by the first dropped one, in the member whose bond the cap cuts; the
    sweep goes on consistently from it, so cores stay isometries and only the subspace (and what follows) is off."""
    member = 2 if name == "nonuniform_group" else 1
    storage = sc.CASES[name]["storage"]

    def swap(i, rows, k, core):
        if i != 3:
            return core
        assert k < len(rows)
        core = core.copy()
        core[k - 1] = sc.round_to(rows[k], storage)
        return core

    emu = _steps(name, member, tamper={"core": swap})
    msg = _raises("theta", name, member, emu["cores"], emu["spectra"])
    assert "bond 1" in msg
    x, ref, _ = sc.sweeps(name)[member]
    yard = sc.yardstick(name)[member]
    got = sc.sweep_quantities(emu["cores"], emu["spectra"], sc.reconstruction(emu["cores"], x.shape), x, ref, "right")
    assert got["theta"][3] > 0.9 and all(got["theta"][i] <= sc.MARGIN * yard["theta"][i] for i in range(4, len(ref["cores"])))
    assert all(v <= sc.MARGIN * yard["iso"][i] for i, v in got["iso"].items()) and got["site0"] <= sc.MARGIN * yard["site0"]


@pytest.mark.parametrize("name", MUTATED)
def test_check_sweep_sees_a_core_row_scaled_by_64_u(name):
    u = sc.U[sc.CASES[name]["storage"]]
    emu = _steps(name, 0)
    cores = [c.copy() for c in emu["cores"]]
    cores[3][2] *= 1 + 64 * u  # site 3: a tall unfolding on every one of these cases
    msg = _raises("isometry", name, 0, cores, emu["spectra"])
    assert "site 3" in msg


@pytest.mark.parametrize("name", MUTATED)
def test_check_sweep_sees_a_bond_one_short(name):
    members = range(len(sc.CASES[name]["members"]))
    for member in members:
        emu = _steps(name, member)
        cores = [c.copy() for c in emu["cores"]]
        k = cores[2].shape[0]
        cores[1], cores[2] = cores[1][:, :, : k - 1], cores[2][: k - 1]
        _raises("bonds", name, member, cores, emu["spectra"])
        spectra = list(emu["spectra"])
        spectra[2] = spectra[2][: k - 1]  # one value short where the bond is right
        _raises("spectra", name, member, emu["cores"], spectra)


def test_check_sweep_sees_a_non_zero_behind_the_rank():
    """nonuniform_group member 0 keeps 6 of 8 at bond 3: its cores in cap shape, one value written behind the rank
    BEFORE they are cut.  The cut cores and a decode from them are unaffected, so only the padded cores can show it."""
    name, member = "nonuniform_group", 0
    emu = _steps(name, member)
    assert emu["bonds"] == [7, 7, 6, 7]
    caps = [1, 8, 8, 8, 8, 1]
    padded = []
    for i, c in enumerate(emu["cores"]):
        p = np.zeros((caps[i], c.shape[1], caps[i + 1]))
        p[: c.shape[0], :, : c.shape[2]] = c
        padded.append(p)
    _check(name, member, emu["cores"], emu["spectra"], padded=padded)
    padded[3][6, 0, 0] = 1e-30
    cut = [p[: c.shape[0], :, : c.shape[2]].copy() for p, c in zip(padded, emu["cores"])]
    msg = _raises("padding", name, member, cut, emu["spectra"], padded=padded)
    assert "{3: (1, 1e-30)}" in msg
    padded[3][6, 0, 0] = 0.0
    padded[2][1, 1, 1] *= 1 + 2.0 ** -20  # the cut core is not the padded core's leading block
    _raises("padding", name, member, cut, emu["spectra"], padded=padded)


@pytest.mark.parametrize("name", MUTATED)
def test_check_sweep_sees_two_members_exchanged(name):
    a, b = (1, 2) if name == "nonuniform_group" else (0, 1)  # two members with the same bonds
    ea, eb = _steps(name, a), _steps(name, b)
    assert ea["bonds"] == eb["bonds"]
    _raises("theta", name, a, eb["cores"], eb["spectra"], recon=sc.reconstruction(eb["cores"], sc.CASES[name]["shape"]))
    # its own cores with the other member's spectra, and with the other member's reconstruction
    _raises("spectra", name, a, ea["cores"], eb["spectra"])
    _raises("recon", name, a, ea["cores"], ea["spectra"], recon=sc.reconstruction(eb["cores"], sc.CASES[name]["shape"]))


def test_check_sweep_sees_wrong_state():
    name = "rank_below_cap"
    emu = _steps(name, 0)
    cores, u = emu["cores"], sc.U["f32"]
    bl = np.array([[c.min(), c.max()] for c in cores])
    norm = np.linalg.norm(cores[0])
    _check(name, 0, cores, emu["spectra"], boundary=bl, norm_value=norm * (1 + 3 * u))
    _raises("state", name, 0, cores, emu["spectra"], boundary=bl, norm_value=norm * (1 + 6 * u))
    bl[2, 1] = np.nextafter(bl[2, 1], 1.0)
    _raises("state", name, 0, cores, emu["spectra"], boundary=bl)
    bad = [c.copy() for c in cores]
    bad[1][0, 0, 0] = np.nan
    _raises("shape", name, 0, bad, emu["spectra"])
