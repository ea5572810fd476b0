"""Host side of NDMPS.gram / pca (core/series.py) and the error bar of the Gram matrix, checked on the CPU before any
kernel is held to it (the pattern of tests/test_decode_bound_host.py).

The bar of an entry: ``|G[a, b] - mps_overlap(a, b)| <= max(overlap_bound(a, b), overlap_bound(b, a))`` with
``u_acc = u_store = 2**-53`` (oracle/chain_bound.py; the kernels associate ``E B`` first, whose inner extents are those
of the swapped pair).  For EVERY case of tests/series_cases.py:

* sound: a NumPy fp64 restatement of the kernels' association, ``E' = sum_i A_i^T (E B_i)``, is inside the bar;
* teeth: the same restatement with one physical index of one site dropped, and with one core of b read with its two
  (equal) bond axes transposed, is outside it (integer cases: differs, since equality is their bar);
* the integer cases satisfy the precondition under which the result must be exact (|a| . |b| < 2**53).

``pca_weights`` is checked against numpy.linalg.svd of the centred series.  No tolerance here or in
tests/test_gpu_series.py comes from a kernel's output.
"""
import os
import re

import numpy as np
import pytest

import series_cases as sc
from imgcompressionmps_amd import _lib
from imgcompressionmps_amd.core import series as se
from oracle import chain_bound as cb
from oracle.mps import mps_overlap


def restated(a, b, drop=None, transpose=None):
    """``E_{j+1} = sum_i A_j[:, i, :]^T (E_j B_j[:, i, :])`` in fp64.  ``drop = j``: the last physical index of site j
    is left out; ``transpose = j``: the core of b at site j is read with its bond axes swapped."""
    E = np.ones((1, 1))
    for j, (A, B) in enumerate(zip(a, b)):
        if transpose == j:
            B = B.transpose(2, 1, 0)
        d = A.shape[1] - (1 if drop == j else 0)
        E = sum(A[:, i, :].T @ (E @ B[:, i, :]) for i in range(d))
    return float(E[0, 0])


def square_site(b):
    """A site of b with equal bonds > 1 (None: the chain has none)."""
    return next((j for j, c in enumerate(b) if c.shape[0] == c.shape[2] > 1), None)


def drop_site(a):
    """The site whose last physical index the mistake leaves out: the middle one with d > 1."""
    L = len(a)
    return next(j for j in sorted(range(L), key=lambda j: abs(j - L // 2)) if a[j].shape[1] > 1)


def bar(a, b):
    return max(cb.overlap_bound(a, b), cb.overlap_bound(b, a))


def pairs_of(la, lb):
    if lb is None:
        return [(i, k, la[i], la[k]) for i in range(len(la)) for k in range(i, len(la))]
    return [(i, k, la[i], lb[k]) for i in range(len(la)) for k in range(len(lb))]


def check_case(name, case, la, lb):
    integer = case["family"] == "integer"
    n_drop = n_tr = n_tr_possible = n_pos = 0
    for i, k, a, b in pairs_of(la, lb):
        ref, tol = mps_overlap(a, b), bar(a, b)
        got = restated(a, b)
        if integer:
            assert cb.abs_overlap(a, b) < 2.0 ** 53 and got == ref, (name, i, k)
        assert abs(got - ref) <= tol, (name, i, k, got, ref, tol)
        if tol == 0.0:
            assert got == 0.0
            continue
        n_pos += 1
        n_drop += abs(restated(a, b, drop=drop_site(a)) - ref) > tol
        j = square_site(b)
        if j is not None:
            n_tr_possible += 1
            n_tr += abs(restated(a, b, transpose=j) - ref) > tol
    # non-negative and swept cores: EVERY entry with a non-zero bar catches the dropped index; integers: at least one
    assert n_drop == n_pos if not integer else n_drop >= 1, (name, n_drop, n_pos)
    if n_tr_possible:
        assert n_tr >= max(1, n_tr_possible // 2), (name, n_tr, n_tr_possible)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_bar_is_sound_and_has_teeth(name):
    case = sc.CASES[name]
    la, lb = sc.cores_of(name)
    check_case(name, case, la, lb)


def test_bar_is_sound_and_has_teeth_on_the_many_pairs_case():
    la, _ = sc.cores_of("many", sc.MANY)
    assert len(la) * (len(la) + 1) // 2 == 65703
    check_case("many", sc.MANY, la, None)


def test_disjoint_case_has_an_exact_zero():
    la, _ = sc.cores_of("disjoint")
    assert cb.abs_overlap(la[0], la[1]) == 0.0 and cb.abs_overlap(la[0], la[2]) > 0.0


def test_signed_uniform_cores_at_bond_64_would_be_toothless():
    """Why the cases are non-negative: with oracle.chain_cases' signed uniform draw at the headline shape the bar
    exceeds the change a dropped physical index makes."""
    from oracle import chain_cases as cc

    a = cc.draw_cores("x", [8] * 8, sc.U64, "uniform", "f32", salt=1)
    b = cc.draw_cores("x", [8] * 8, sc.U64, "uniform", "f32", salt=2)
    assert abs(restated(a, b, drop=4) - mps_overlap(a, b)) < bar(a, b)
    pa, pb = [np.abs(c) for c in a], [np.abs(c) for c in b]
    assert abs(restated(pa, pb, drop=4) - mps_overlap(pa, pb)) > 1e6 * bar(pa, pb)


# ------------------------------------------------------------------------------------------------ pca_weights
def _svd_centred(X, center=True):
    Xc = X - X.mean(axis=0, keepdims=True) if center else X
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    return Xc, U, s, Vt


@pytest.mark.parametrize("center", [True, False])
def test_pca_weights_reproduce_the_svd(center):
    rng = np.random.default_rng(5)
    K, N = 9, 400
    X = rng.standard_normal((K, 4)) @ rng.standard_normal((4, N)) + 1e-2 * rng.standard_normal((K, N)) + 3.0
    sigma, U, W = se.pca_weights(X @ X.T, None, center, 1e-8)
    Xc, Us, s, Vt = _svd_centred(X, center)
    r = len(sigma)
    assert r == (K - 1 if center else K)
    np.testing.assert_allclose(sigma, s[:r], rtol=0, atol=1e-12 * s[0])
    V = W.T @ X  # the components: weights on the ORIGINAL rows
    for k in range(r):
        if s[k] < 1e-3 * s[0]:
            continue
        sign = np.sign(Us[np.argmax(np.abs(Us[:, k])), k])
        assert U[np.argmax(np.abs(U[:, k])), k] > 0
        np.testing.assert_allclose(V[k], sign * Vt[k], rtol=0, atol=1e-9)
        np.testing.assert_allclose(U[:, k] * sigma[k], sign * Us[:, k] * s[k], rtol=0, atol=1e-9 * s[0])
    np.testing.assert_allclose(se.explained_variance(sigma, K, center), s[:r] ** 2 / (K - 1 if center else K),
                               rtol=0, atol=1e-11 * s[0] ** 2)


def test_pca_weights_rank_deficient_series_keep_only_values_above_the_floor():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((6, 200))
    X[4] = X[1]                                    # two equal rows: rank 5, centred rank 4
    sigma, U, W = se.pca_weights(X @ X.T, None, True, 1e-6)
    assert len(sigma) == 4 and np.all(sigma > 1e-6 * sigma[0])
    const = np.tile(rng.standard_normal(200), (5, 1))   # a constant series: nothing is left after centring
    sigma, U, W = se.pca_weights(const @ const.T, None, True, 1e-6)
    assert len(sigma) == 0 and U.shape == (5, 0) and W.shape == (5, 0)
    sigma, U, W = se.pca_weights(const @ const.T, None, False, 1e-6)
    assert len(sigma) == 1
    np.testing.assert_allclose(W[:, 0] @ const, const[0] / np.linalg.norm(const[0]), atol=1e-12)


def test_pca_weights_edges():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 50))
    sigma, U, W = se.pca_weights(x @ x.T, None, True, 1e-6)      # K = 1 centred: empty
    assert len(sigma) == 0 and se.explained_variance(sigma, 1, True).shape == (0,)
    sigma, U, W = se.pca_weights(x @ x.T, None, False, 1e-6)     # K = 1 uncentred: the frame itself
    np.testing.assert_allclose(sigma, [np.linalg.norm(x)])
    assert U[0, 0] == 1.0
    X = rng.standard_normal((5, 80))
    s_all = se.pca_weights(X @ X.T, None, True, 1e-6)[0]
    s_big = se.pca_weights(X @ X.T, 50, True, 1e-6)[0]          # n_components above the rank
    s_two = se.pca_weights(X @ X.T, 2, True, 1e-6)[0]
    assert len(s_all) == len(s_big) == 4 and len(s_two) == 2
    with pytest.raises(ValueError):
        se.pca_weights(X @ X.T, 0)
    with pytest.raises(ValueError):
        se.pca_weights(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        se.check_lists(0)
    with pytest.raises(ValueError):
        se.check_lists(2, 0)
    G = X @ X.T
    H = np.eye(5) - np.ones((5, 5)) / 5
    np.testing.assert_allclose(se.centre(G), H @ G @ H, atol=1e-12 * np.abs(G).max())


def test_series_module_needs_no_torch():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path.insert(0, {root!r})\n"
            "import importlib.util as u\n"
            f"spec = u.spec_from_file_location('series', {os.path.join(root, 'img-compression-mps_amd', 'core', 'series.py')!r})\n"
            "m = u.module_from_spec(spec); spec.loader.exec_module(m)\n"
            "assert 'torch' not in sys.modules; print(m.pca_weights([[4.0]], None, False)[0][0])")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out.strip() == "2.0"


# ------------------------------------------------------------------------------------------------ the library
def _route(lib, dims, ba, bb):
    flat = lambda bl: _lib.i64_array([v for row in bl for v in row])  # noqa: E731
    return lib.ndmps_series_gram_route(len(ba), len(bb), len(dims), _lib.i64_array(dims), flat(ba), flat(bb))


def test_routes_and_argument_errors_need_no_device():
    lib = _lib.load()
    for name, case in sc.CASES.items():
        if case["family"] == "swept":
            continue
        got = _route(lib, case["dims"], case["bonds_a"], case["bonds_b"] or case["bonds_a"])
        assert se.ROUTES[got] == case["route"], name
    assert se.ROUTES[_route(lib, [8, 8, 8], [[1, 8, 8, 1]], [[1, 8, 8, 1]])] == "resident"
    assert se.ROUTES[_route(lib, [16, 16, 16], [[1, 16, 65, 1]] * 2, [[1, 16, 65, 1]] * 2)] == "batched"
    assert se.ROUTES[_route(lib, [16, 16, 16], [[1, 16, 65, 1]], [[1, 16, 64, 1]])] == "per-pair"
    dims, ba = _lib.i64_array([4, 4]), _lib.i64_array([1, 4, 1])
    assert lib.ndmps_series_gram_route(0, 1, 2, dims, ba, ba) == _lib.EINVAL
    assert lib.ndmps_series_gram_route(1, 1, 0, dims, ba, ba) == _lib.EINVAL
    assert lib.ndmps_series_gram_route(1, 1, 2, dims, _lib.i64_array([2, 4, 1]), ba) == _lib.EINVAL  # outer bond
    assert lib.ndmps_series_gram_route(1, 1, 2, dims, _lib.i64_array([1, 0, 1]), ba) == _lib.EINVAL
    assert b"bond" in lib.ndmps_last_error()
    assert lib.ndmps_series_gram_workspace_bytes(1, 1, 2, dims, ba, ba) > 0
    assert lib.ndmps_series_gram_workspace_bytes(1, 0, 2, dims, ba, ba) == _lib.EINVAL
    # nothing is launched for a bad argument: NULL lists, a symmetric call with two lengths
    null = _lib.C.cast(None, _lib.C.POINTER(_lib.vp))
    rc = lib.ndmps_series_gram(1, 1, 1, 2, dims, ba, None, null, ba, None, null, None, None, 0, None)
    assert rc == _lib.EINVAL


def test_resident_series_kernel_does_not_spill():
    """Like test_resident_kernels_keep_their_state_in_registers: the resident Gram kernel keeps E', Z's tile and the
    operands of the next phase in registers; a build that spills a vector register pays scratch round trips inside
    the MFMA loop.  It must also fit two workgroups per CU: 64 KiB of LDS, at most 256 registers."""
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
                if name and "series_gram_resident_kernel" in name.group(1):
                    seen[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                           for k in ("vgpr_spill_count", "vgpr_count", "group_segment_fixed_size")}
    finally:
        shutil.rmtree(tmp)
    assert len(seen) >= 1, seen
    for name, v in seen.items():
        assert v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256 and v["group_segment_fixed_size"] <= 80 * 1024, (name, v)
