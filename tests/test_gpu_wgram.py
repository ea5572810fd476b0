"""NDMPS.gram / inner / pca with ``weight=`` on the MI355X (csrc/wgram.hip, core/wgram.py).

Bars, and where they come from:

* Element bar of G_w on arbitrary cores: ``|G_w[a, b] - sum a * w * b| <= weighted_bound(a, w, b)`` (core/wgram.py:
  ``1.01 * 2**-53 * N * S``, the forward error bound of the three nested fp64 products per site; the inputs are widened
  exactly) against the fp64 sum over the three dense site-order tensors (``oracle.mps.mps_to_dense``), on the cores as
  stored, for both routes, through the C ABI and through ``NDMPS.gram``.  Where the bound is 0 the entry is exactly 0;
  the integer cases come out equal.  tests/test_wgram_host.py proves on the CPU that this bar holds for the fp64
  restatement of the shipped order and rejects the modelled faults on every case used here (tests/wgram_cases.py).
* Bits: the symmetric result is exactly symmetric; a second call, a workspace filled with 0xFF bytes and a workspace
  cap that forces several chunks all give the same bits.
* PCA under a weight: the singular values are functions of ``G_w`` alone (``|sigma_k**2 - lambda_k| <= 1e-12 lambda_0``:
  two backward-stable symmetric eigen-solvers on one matrix); the components are orthonormal in the weighted inner
  product within ``e_k + e_l + e_k e_l``, ``e_k = tol * sum_a |c_{a,k}| norm_value_a`` with ``tol = 1e-5``: the bar and
  the constant of tests/test_gpu_series.py for unweighted components.  It carries over because the weight used is an
  indicator (0 <= w <= 1), under which the weighted norm of a component's rounding error is at most its plain norm.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import wgram_cases as wc  # noqa: E402
from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core import oncore  # noqa: E402
from imgcompressionmps_amd.core import series as se  # noqa: E402
from imgcompressionmps_amd.core import wgram as wg  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"f32": F32, "bf16": BF16, "f64": F64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _object(cores, st):
    """An NDMPS around the given fp64 cores, stored as ``st`` (the values are representable: exact)."""
    dev = [torch.from_numpy(np.ascontiguousarray(c)).to(device=DEV, dtype=DT[st]) for c in cores]
    return NDMPS(DeviceMPS(dev), np.array([c.shape[1] for c in cores]), None, None, False, None, "Std", 3)


def _objects(name, case=None):
    case = case or wc.CASES[name]
    la, lb, w, ref = wc.reference(name, case)
    objs = [_object(c, s) for c, s in zip(la, case["storage_a"])]
    others = None if lb is None else [_object(c, s) for c, s in zip(lb, case["storage_b"])]
    return objs, others, _object(w, case["storage_w"]), (la, lb, w, ref)


def _abi(objs, others, weight, cap=None, fill=None):
    """G_w through the C ABI: the workspace the query asks for under ``cap``, optionally pre-filled with a byte."""
    lib = _lib.load()
    cols, c_dims = objs if others is None else others, _lib.i64_array(objs[0].mps.dims)
    sa = oncore.chain_list_args([o.mps for o in objs])
    sb = sa if others is None else oncore.chain_list_args([o.mps for o in others])
    bonds_w, codes_w, ptrs_w = oncore.chain_list_args([weight.mps])
    sw = (bonds_w, codes_w[0], ptrs_w)
    Ka, Kb, L, sym = len(objs), len(cols), objs[0].mps.L, 1 if others is None else 0
    nbytes = _lib.check(lib.ndmps_series_wgram_workspace_bytes(Ka, Kb, sym, L, c_dims, sa[0], sb[0], sw[0],
                                                               wg.WS_LIMIT_BYTES if cap is None else cap))
    assert cap is None or nbytes <= cap
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    G = torch.full((Ka, Kb), float("nan"), dtype=F64, device=DEV)
    _lib.check(lib.ndmps_series_wgram(Ka, Kb, sym, L, c_dims, sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], sw[0], sw[1], sw[2],
                                      G.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return G.cpu().numpy()


def _check_entries(G, la, lb, w, ref, integer=False, transposed=False):
    worst = 0.0
    for i, k, a, b in wc.pairs_of(la, lb):
        got = G[k, i] if transposed else G[i, k]
        tol = wg.weighted_bound(a, w, b)
        if integer:
            assert got == ref[i, k], (i, k, got, ref[i, k])
        if tol == 0.0:
            assert got == 0.0, (i, k, got)
            continue
        worst = max(worst, abs(got - ref[i, k]) / tol)
        assert abs(got - ref[i, k]) <= tol, (i, k, got, ref[i, k], tol)
    print(f"worst |G_w - ref| / bar = {worst:.3g}")


@pytest.mark.parametrize("name", list(wc.CASES))
def test_weighted_gram_entries_against_the_dense_reference(name):
    case = wc.CASES[name]
    objs, others, weight, (la, lb, w, ref) = _objects(name)
    integer = case["family"] == "integer"
    assert NDMPS.gram_route(objs, others, weight=weight) == case["route"]
    G = NDMPS.gram(objs, others, weight=weight)
    assert G.dtype == np.float64 and G.shape == ref.shape and np.all(np.isfinite(G))
    _check_entries(G, la, lb, w, ref, integer)
    Gc = _abi(objs, others, weight)
    _check_entries(Gc, la, lb, w, ref, integer)
    assert np.array_equal(G, Gc), "the C ABI and NDMPS.gram are one computation"
    assert np.array_equal(G, NDMPS.gram(objs, others, weight=weight)), "two calls must give identical bits"
    if others is None:
        assert np.array_equal(G, G.T), "G_w[b, a] is a copy of G_w[a, b]"
        # the rectangular call on the same list computes [b, a] itself: same bar, both triangles
        Gr = NDMPS.gram(objs, list(objs), weight=weight)
        _check_entries(Gr, la, None, w, ref, integer)
        _check_entries(Gr, la, None, w, ref, integer, transposed=True)
        assert objs[0].inner(objs[-1], weight=weight) == Gr[0, -1]
    else:
        assert objs[0].inner(others[-1], weight=weight) == G[0, -1]
        assert objs[-1].inner(others[0], weight=weight) == G[-1, 0]
    t = NDMPS.gram(objs, others, as_torch=True, weight=weight)
    assert t.dtype == F64 and t.is_cuda and np.array_equal(t.cpu().numpy(), G)


def test_weighted_gram_of_40_tiny_chains_entry_by_entry():
    objs, _, weight, (la, lb, w, ref) = _objects("many", wc.MANY)
    assert NDMPS.gram_route(objs, weight=weight) == "resident" and len(objs) * (len(objs) + 1) // 2 == 820
    G = NDMPS.gram(objs, weight=weight)
    assert np.array_equal(G, G.T)
    _check_entries(G, la, lb, w, ref)
    assert np.array_equal(_abi(objs, None, weight), G)


@pytest.mark.parametrize("name", ["ragged_mixed", "rect_2x3", "wide"])
def test_garbage_in_the_workspace_reaches_no_result(name):
    objs, others, weight, _ = _objects(name)
    fresh = _abi(objs, others, weight, fill=0)
    dirty = _abi(objs, others, weight, fill=0xFF)  # every double a NaN
    assert np.all(np.isfinite(dirty)) and np.array_equal(fresh, dirty)


def test_chunked_workspace_changes_no_bit():
    lib = _lib.load()
    case = wc.CASES["five"]
    objs, _, weight, (la, lb, w, ref) = _objects("five")
    dims, bw = _lib.i64_array(case["dims"]), _lib.i64_array(case["bonds_w"])
    ba = _lib.i64_array([v for row in case["bonds_a"] for v in row])
    q = lambda cap: lib.ndmps_series_wgram_workspace_bytes(5, 5, 1, 4, dims, ba, ba, bw, int(cap))  # noqa: E731
    full = q(wg.WS_LIMIT_BYTES)
    sizes = sorted({q(c) for c in np.linspace(0, full, 600)} - {_lib.EWORKSPACE})
    assert len(sizes) == 15 and sizes[-1] == full  # 15 pairs: sizes[n - 1] holds a chunk of n pairs
    one = _abi(objs, None, weight)
    _check_entries(one, la, lb, w, ref)
    for n in (5, 4, 1):  # 3 chunks; 4 chunks, the last of 3 pairs; 15 chunks
        assert -(-15 // n) >= 3
        assert np.array_equal(_abi(objs, None, weight, cap=sizes[n - 1]), one), n
    with pytest.raises(_lib.NdmpsHipError):
        _abi(objs, None, weight, cap=sizes[0] - 256)


def test_all_ones_weight_agrees_with_the_plain_gram():
    objs, _, _, (la, _, _, _) = _objects("ragged_mixed")
    ones = [np.ones((1, 8, 1))] * 6
    G1 = NDMPS.gram(objs, weight=_object(ones, "f32"))
    G0 = NDMPS.gram(objs)
    for i, k, a, b in wc.pairs_of(la, None):  # both are inside their own bars around one exact value
        assert abs(G1[i, k] - G0[i, k]) <= 2 * wg.weighted_bound(a, ones, b), (i, k)


def _stored(obj):
    return [c.to(F64).cpu().numpy() for c in obj.mps.cores]


def _masks(shape):
    z, y, x = np.indices(shape)
    # a box of whole dyadic blocks, z in [8, 16), y in [16, 24): a product over the binary digits, so its bond is 1
    box = ((z // 8 == 1) & (y // 8 == 2) & (x >= 0)).astype(np.float32)
    c = (np.array(shape) - 1) / 2
    ball = ((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 12.0 ** 2).astype(np.float32)
    return box, ball


def test_end_to_end_through_the_public_encoders():
    shape = (32, 32, 32)
    objs = [NDMPS.from_tensor(synthetic_mri(shape, seed=s), max_bond=16, device=DEV) for s in (21, 22, 23, 24)]
    box_x, ball_x = _masks(shape)
    box = NDMPS.from_tensor(box_x, device=DEV)
    ball = NDMPS.from_tensor(ball_x, max_bond=8, device=DEV)
    assert max(box.bond_sizes()) == 1 and 1 < max(ball.bond_sizes()) <= 8
    la = [_stored(o) for o in objs]
    for m in (box, ball):
        w = _stored(m)
        ref = wc.dense_reference(la, None, w)
        G = NDMPS.gram(objs, weight=m)
        assert np.array_equal(G, G.T)
        _check_entries(G, la, None, w, ref)
        Gr = NDMPS.gram(objs[:2], objs[1:], weight=m)
        _check_entries(Gr, la[:2], la[1:], w, ref[:2, 1:])
    # the box is exactly representable: its second moments are those of the decoded volumes inside the box
    X = np.stack([np.asarray(o.to_tensor(), dtype=np.float64).reshape(-1) for o in objs])
    want = (X * box_x.reshape(-1).astype(np.float64)) @ X.T
    nrm = np.sqrt(np.diag(X @ X.T))
    G = NDMPS.gram(objs, weight=box)
    assert np.all(np.abs(G - want) <= 1e-5 * np.outer(nrm, nrm))  # the decoder's fp32 rounding: tests/test_gpu_series.py


def test_pca_under_a_weight():
    rng = np.random.default_rng(42)
    shape, K, tol = (32, 32, 32), 8, 1e-5
    base = np.stack([synthetic_mri(shape, seed=s) for s in (1, 2, 3)]).astype(np.float64)
    mix = rng.uniform(-1.0, 1.0, size=(K, 3)) + np.array([2.0, 0.0, 0.0])
    frames = np.tensordot(mix, base, axes=1) + 1e-4 * rng.standard_normal((K,) + shape)
    objs = [NDMPS.from_tensor(f.astype(np.float32), max_bond=16, device=DEV) for f in frames]
    m = NDMPS.from_tensor(_masks(shape)[0], device=DEV)
    assert max(m.bond_sizes()) == 1
    res = NDMPS.pca(objs, weight=m)
    G = NDMPS.gram(objs, weight=m)
    lam = np.linalg.eigvalsh(se.centre(G))[::-1]
    r = len(res.singular_values)
    assert 3 <= r <= K - 1 and len(res.components) == r and res.scores.shape == (K, r)
    assert np.all(np.abs(res.singular_values ** 2 - lam[:r]) <= 1e-12 * lam[0])
    np.testing.assert_allclose(res.explained_variance, res.singular_values ** 2 / (K - 1), rtol=1e-15)
    s = res.singular_values
    strong = [k for k in range(r) if s[k] >= 1e-3 * s[0]]  # beyond that 1 / sigma_k amplifies storage noise
    assert len(strong) >= 3
    comps = [res.components[k] for k in strong]
    Gc = NDMPS.gram(comps, weight=m)
    norms = np.array([float(o.norm_value) for o in objs])
    e = np.array([tol * float(np.abs(res.weights[:, k]) @ norms) for k in strong])
    for i in range(len(strong)):
        for j in range(len(strong)):
            assert abs(Gc[i, j] - (i == j)) <= e[i] + e[j] + e[i] * e[j], (i, j, Gc[i, j], e[i], e[j])
            assert comps[i].inner(comps[j], weight=m) == NDMPS.gram([comps[i]], [comps[j]], weight=m)[0, 0]
    # without the weight the same objects give another PCA: the keyword is not ignored
    assert abs(NDMPS.pca(objs).singular_values[0] - s[0]) > 1e-3 * s[0]
