"""Host side of the weighted Gram matrix (core/wgram.py, csrc/wgram.hip) and its error bar, checked on the CPU before
any kernel is held to it (the pattern of tests/test_series_host.py).

The bar of an entry: ``|G_w[a, b] - sum a * w * b| <= weighted_bound(a, w, b) = 1.01 * 2**-53 * N * S`` with
``N = sum_j (chi_a + chi_b + chi_w d + 4)`` and ``S`` the same sum over the absolute values of the cores: the forward
error bound of the three nested products per site in the shipped order.  For EVERY case of tests/wgram_cases.py:

* sound: ``core.wgram.emulate``, the fp64 restatement of that order, is inside the bar of the dense reference;
* teeth: a restatement with one modelled fault -- the weight's core read with w and w' swapped, the last w dropped, the
  weight's physical index shifted by one against the objects', ``A`` read untransposed, fp32 accumulation -- is
  outside it wherever the fault changes the sum at all (integer cases: differs, since equality is their bar);
* where S = 0 the result is exactly 0, and the integer cases come out equal.

No tolerance here or in tests/test_gpu_wgram.py comes from a kernel's output.
"""
import os
import re

import numpy as np
import pytest

import wgram_cases as wc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import series as se
from imgcompressionmps_amd.core import wgram as wg

FAULTS = ("swap_w", "drop_w", "shift_i", "a_untransposed", "fp32")


def _site(cores, pred):
    """The site nearest the middle of the chain that satisfies ``pred`` (None: no such site)."""
    L = len(cores)
    return next((j for j in sorted(range(L), key=lambda j: abs(j - L // 2)) if pred(cores[j])), None)


def faulty(a, w, b, fault):
    """The contraction of core.wgram.emulate with one modelled fault at one site; None where the chains leave the
    fault no room (no square core, no bond above 1, no physical index to shift)."""
    dt = np.float32 if fault == "fp32" else np.float64
    at = {"swap_w": _site(w, lambda c: c.shape[0] == c.shape[2] > 1), "drop_w": _site(w, lambda c: c.shape[0] > 1),
          "shift_i": _site(w, lambda c: c.shape[1] > 1), "a_untransposed": _site(a, lambda c: c.shape[0] == c.shape[2] > 1),
          "fp32": 0}[fault]
    if at is None:
        return None
    E = np.ones((1, 1, 1), dtype=dt)
    for j, (A, W, B) in enumerate(zip(a, w, b)):
        A, W, B = A.astype(dt), W.astype(dt), B.astype(dt)
        hit = j == at
        if hit and fault == "swap_w":
            W = W.transpose(2, 1, 0)
        if hit and fault == "shift_i":
            W = np.roll(W, 1, axis=1)
        cw, d, cw2 = W.shape
        n_w = cw - 1 if hit and fault == "drop_w" else cw
        P = np.zeros((cw, d, A.shape[2], B.shape[2]), dtype=dt)
        for v in range(n_w):
            for i in range(d):
                Ai = A[:, i, :] if hit and fault == "a_untransposed" else A[:, i, :].T
                P[v, i] = Ai @ (E[v] @ B[:, i, :])
        E = (W.reshape(cw * d, cw2).T @ P.reshape(cw * d, -1)).reshape(cw2, A.shape[2], B.shape[2])
    return float(E[0, 0, 0])


def check_case(name, case, la, lb, w, ref):
    integer = case["family"] == "integer"
    caught = dict.fromkeys(FAULTS, 0)
    for i, k, a, b in wc.pairs_of(la, lb):
        want, tol = ref[i, k], wg.weighted_bound(a, w, b)
        got = wg.emulate(a, w, b)
        if integer:  # every partial sum is an integer of magnitude <= S < 2**53: nothing rounds
            S = wg.emulate([np.abs(c) for c in a], [np.abs(c) for c in w], [np.abs(c) for c in b])
            assert S < 2.0 ** 53 and got == want, (name, i, k, got, want, S)
        assert abs(got - want) <= tol, (name, i, k, got, want, tol)
        if tol == 0.0:
            assert got == 0.0 and want == 0.0, (name, i, k)
            continue
        for fault in FAULTS:
            bad = faulty(a, w, b, fault)
            if bad is None or bad == got:  # the fault has no room here, or does not change the sum
                continue
            caught[fault] += 1
            if integer:
                assert bad != want, (name, i, k, fault)
            else:
                assert abs(bad - want) > tol, (name, i, k, fault, bad, want, tol)
    return caught


@pytest.mark.parametrize("name", list(wc.CASES))
def test_bar_is_sound_and_has_teeth(name):
    case = wc.CASES[name]
    la, lb, w, ref = wc.reference(name)
    caught = check_case(name, case, la, lb, w, ref)
    if case["family"] == "pos":  # positive draws: a shifted physical index and fp32 accumulation always show
        assert caught["shift_i"] > 0 and caught["fp32"] > 0, (name, caught)
    if name in ("uniform64", "ragged_f32", "five"):
        assert caught["drop_w"] > 0, (name, caught)  # square cores, for the other two faults: the many-pairs case


def test_bar_is_sound_and_has_teeth_on_the_many_pairs_case():
    la, lb, w, ref = wc.reference("many", wc.MANY)
    assert len(la) * (len(la) + 1) // 2 == 820
    caught = check_case("many", wc.MANY, la, lb, w, ref)
    assert all(caught[f] > 0 for f in FAULTS), caught


def test_disjoint_case_has_exact_zeros():
    la, lb, w, ref = wc.reference("disjoint")
    for k in range(3):
        assert wg.weighted_bound(la[0], w, la[k]) == 0.0 and ref[0, k] == 0.0 and wg.emulate(la[0], w, la[k]) == 0.0
    assert ref[1, 2] > 0.0 and wg.weighted_bound(la[1], w, la[2]) > 0.0


def test_all_ones_weight_reduces_to_the_plain_gram():
    from oracle.mps import mps_overlap

    la, _, _, _ = wc.reference("uniform64")
    ones = [np.ones((1, d, 1)) for d in wc.CASES["uniform64"]["dims"]]
    for i, k, a, b in wc.pairs_of(la, None):
        assert abs(wg.emulate(a, ones, b) - mps_overlap(a, b)) <= 2 * wg.weighted_bound(a, ones, b)


def test_emulate_rejects_mismatched_chains():
    la, _, w, _ = wc.reference("K1")
    with pytest.raises(ValueError):
        wg.emulate(la[0], w[:-1], la[0])
    with pytest.raises(ValueError):
        wg.emulate(la[0], [np.ones((1, 4, 1))] * 4, la[0])
    with pytest.raises(ValueError):
        wg.emulate([np.ones((2, 8, 1))], [np.ones((1, 8, 1))], [np.ones((1, 8, 1))])
    assert wg.WS_LIMIT_BYTES == 1 << 30


def test_wgram_module_needs_no_torch():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "img-compression-mps_amd", "core", "wgram.py")
    code = ("import sys, importlib.util as u\n"
            f"spec = u.spec_from_file_location('wgram', {path!r})\n"
            "m = u.module_from_spec(spec); spec.loader.exec_module(m)\n"
            "import numpy as np\n"
            "c = [np.full((1, 2, 1), 2.0)]\n"
            "assert 'torch' not in sys.modules; print(m.emulate(c, c, c))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out.strip() == "16.0"


# ------------------------------------------------------------------------------------------------ the library
def _flat(bl):
    return _lib.i64_array([v for row in bl for v in row])


def _route(lib, dims, ba, bb, bw):
    return lib.ndmps_series_wgram_route(len(ba), len(bb), len(dims), _lib.i64_array(dims), _flat(ba), _flat(bb),
                                        _lib.i64_array(bw))


def test_routes_need_no_device():
    lib = _lib.load()
    for name, case in list(wc.CASES.items()) + [("many", wc.MANY)]:
        if case["family"] == "swept":
            continue
        got = _route(lib, case["dims"], case["bonds_a"], case["bonds_b"] or case["bonds_a"], case["bonds_w"])
        assert se.ROUTES[got] == case["route"], name
    # the weight's bonds do not decide the route; one bond of either list above 64 does
    assert se.ROUTES[_route(lib, [8, 8, 8], [[1, 8, 8, 1]], [[1, 8, 8, 1]], [1, 200, 300, 1])] == "resident"
    assert se.ROUTES[_route(lib, [16] * 3, [[1, 16, 64, 1]], [[1, 16, 65, 1]], [1, 2, 2, 1])] == "per-pair"
    assert se.ROUTES[_route(lib, [16] * 3, [[1, 16, 65, 1]] * 2, [[1, 16, 65, 1]] * 2, [1, 1, 1, 1])] == "per-pair"


def test_argument_errors_return_einval_and_launch_nothing():
    lib = _lib.load()
    dims, ba, bw = _lib.i64_array([4, 4]), _lib.i64_array([1, 4, 1]), _lib.i64_array([1, 3, 1])
    route, query, run = lib.ndmps_series_wgram_route, lib.ndmps_series_wgram_workspace_bytes, lib.ndmps_series_wgram
    assert route(1, 1, 2, dims, ba, ba, bw) == 0
    assert route(0, 1, 2, dims, ba, ba, bw) == _lib.EINVAL
    assert route(1, 1, 0, dims, ba, ba, bw) == _lib.EINVAL
    assert route(1, 1, 2, dims, ba, ba, None) == _lib.EINVAL
    assert route(1, 1, 2, dims, _lib.i64_array([2, 4, 1]), ba, bw) == _lib.EINVAL
    assert route(1, 1, 2, dims, ba, ba, _lib.i64_array([1, 3, 2])) == _lib.EINVAL  # the weight's outer bond
    assert b"outer bonds" in lib.ndmps_last_error()
    assert route(1, 1, 2, dims, ba, ba, _lib.i64_array([1, 0, 1])) == _lib.EINVAL
    assert b"bond" in lib.ndmps_last_error()
    assert route(1, 1, 2, _lib.i64_array([4, 0]), ba, ba, bw) == _lib.EINVAL
    assert query(1, 1, 1, 2, dims, ba, ba, bw, 1 << 30) > 0
    assert query(1, 0, 0, 2, dims, ba, ba, bw, 1 << 30) == _lib.EINVAL
    assert query(2, 1, 1, 2, dims, _lib.i64_array([1, 4, 1] * 2), ba, bw, 1 << 30) == _lib.EINVAL  # symmetric, two lengths
    # the run itself: every refusal comes before anything touches a device (there is none here)
    vp, C = _lib.vp, _lib.C
    null = C.cast(None, C.POINTER(vp))
    codes = (C.c_int * 1)(0)
    some = (vp * 2)(64, 64)  # non-NULL addresses that nothing may dereference
    hole = (vp * 2)(64, None)
    assert run(1, 1, 1, 2, dims, ba, None, null, ba, None, null, bw, 0, null, None, None, 0, None) == _lib.EINVAL
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, some, bw, 0, null, 64, None, 0, None) == _lib.EINVAL
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, some, bw, 3, some, 64, None, 0, None) == _lib.EINVAL
    assert b"weight" in lib.ndmps_last_error()
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, some, bw, 0, hole, 64, None, 0, None) == _lib.EINVAL
    assert b"NULL core" in lib.ndmps_last_error()
    assert run(1, 1, 1, 2, dims, ba, codes, hole, ba, codes, hole, bw, 0, some, 64, None, 0, None) == _lib.EINVAL
    assert run(1, 1, 1, 2, dims, ba, (C.c_int * 1)(7), some, ba, codes, some, bw, 0, some, 64, None, 0, None) == _lib.EINVAL
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, (vp * 2)(64, 128), bw, 0, some, 64, None, 0, None) == _lib.EINVAL
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, some, _lib.i64_array([1, 3, 5]), 0, some, 64, None, 0,
               None) == _lib.EINVAL
    # good arguments, no workspace: refused as too small, still before any launch
    assert run(1, 1, 1, 2, dims, ba, codes, some, ba, codes, some, bw, 0, some, 64, None, 0, None) == _lib.EWORKSPACE


def test_workspace_query_is_monotone_in_its_cap_and_refuses_less_than_one_pair():
    lib = _lib.load()
    case = wc.CASES["five"]
    dims, ba, bw = _lib.i64_array(case["dims"]), _flat(case["bonds_a"]), _lib.i64_array(case["bonds_w"])
    K, L = len(case["bonds_a"]), len(case["dims"])
    q = lambda cap: lib.ndmps_series_wgram_workspace_bytes(K, K, 1, L, dims, ba, ba, bw, cap)  # noqa: E731
    full = q(1 << 30)
    assert 0 < full < 1 << 30 and q(full) == full and q(1 << 40) == full
    lo = next(c for c in range(0, full + 1, 256) if q(c) > 0)  # the smallest cap (in 256-byte steps) that fits one pair
    assert q(lo - 256) == _lib.EWORKSPACE and q(0) == _lib.EWORKSPACE and q(-5) == _lib.EWORKSPACE
    assert b"one pair" in lib.ndmps_last_error()
    prev, sizes = 0, set()
    for cap in np.linspace(lo, full, 40).astype(np.int64):
        got = q(int(cap))
        assert prev <= got <= cap, (cap, got, prev)
        prev = got
        sizes.add(got)
    assert len(sizes) >= 10 and prev == full  # 15 pairs: the chunk grows with the cap
    # per-pair route: one pair at a time, the same rule
    wide = wc.CASES["wide"]
    wdims, wba, wbw = _lib.i64_array(wide["dims"]), _flat(wide["bonds_a"]), _lib.i64_array(wide["bonds_w"])
    need = lib.ndmps_series_wgram_workspace_bytes(2, 2, 1, 4, wdims, wba, wba, wbw, 1 << 30)
    assert need > 0 and lib.ndmps_series_wgram_workspace_bytes(2, 2, 1, 4, wdims, wba, wba, wbw, need - 256) == _lib.EWORKSPACE


# ------------------------------------------------------------------------------------------------ NDMPS, no device
def _cpu_object(dims, bonds, mode="Std", value=1.0):
    torch = pytest.importorskip("torch")
    from imgcompressionmps_amd import NDMPS
    from imgcompressionmps_amd.core.mps import DeviceMPS

    cores = [torch.full((bonds[j], d, bonds[j + 1]), value, dtype=torch.float32) for j, d in enumerate(dims)]
    return NDMPS(DeviceMPS(cores), np.array(dims), None, None, False, None, mode, 3)


def test_weight_errors_need_no_device():
    from imgcompressionmps_amd import NDMPS

    a, m = _cpu_object([4, 4], [1, 4, 1]), _cpu_object([4, 4], [1, 2, 1])
    for call in (lambda w: NDMPS.gram([a], weight=w), lambda w: a.inner(a, weight=w), lambda w: NDMPS.gram_route([a], weight=w),
                 lambda w: NDMPS.pca([a, a], weight=w), lambda w: NDMPS.gram([a], [a], weight=w)):
        for bad in (3, "mask", np.ones((4, 4))):
            with pytest.raises(TypeError, match="weight must be an NDMPS"):
                call(bad)
        with pytest.raises(ValueError, match="differs from object 0"):
            call(_cpu_object([4, 8], [1, 2, 1]))
        with pytest.raises(ValueError, match="mode"):
            call(_cpu_object([4, 4], [1, 2, 1], mode="DCT"))
    da, dm = _cpu_object([4, 4], [1, 4, 1], mode="DCT"), _cpu_object([4, 4], [1, 2, 1], mode="DCT")
    with pytest.raises(ValueError) as e1:
        NDMPS.gram([da], weight=dm)
    with pytest.raises(ValueError) as e2:
        da.multiply(dm, max_bond=4)
    assert str(e1.value) == str(e2.value) and "DCT" in str(e1.value)
    assert NDMPS.gram_route([a], weight=m) == "resident"
    assert NDMPS.gram_route([_cpu_object([16, 16], [1, 65, 1])], weight=_cpu_object([16, 16], [1, 2, 1])) == "per-pair"
    # one pair above the workspace limit: 64 matrices E of 2048 x 2048 doubles
    big, wbig = _cpu_object([8, 8], [1, 2048, 1]), _cpu_object([8, 8], [1, 64, 1])
    with pytest.raises(ValueError, match="workspace"):
        NDMPS.gram([big], weight=wbig)


def test_wgram_site_kernel_does_not_spill():
    """Like test_resident_series_kernel_does_not_spill: the site kernel of the weighted Gram matrix keeps P's tile,
    Z's tile and the operands in registers, and fits two workgroups per CU: at most 80 KiB of LDS and 256 registers."""
    import shutil
    import subprocess
    import tempfile

    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no ROCm LLVM tools on this host")
    tmp = tempfile.mkdtemp()
    seen = {}
    try:
        shutil.copy(_lib.LIB_PATH, os.path.join(tmp, "g.so"))
        subprocess.run([objdump, "--offloading", "g.so"], cwd=tmp, capture_output=True, check=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", f], cwd=tmp, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if name and "series_wgram_site_kernel" in name.group(1):
                    seen[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                           for k in ("vgpr_spill_count", "vgpr_count", "group_segment_fixed_size",
                                                     "private_segment_fixed_size")}
    finally:
        shutil.rmtree(tmp)
    print(seen)
    assert len(seen) >= 1, seen
    for name, v in seen.items():
        assert v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256 and v["group_segment_fixed_size"] <= 80 * 1024, (name, v)
