"""Statistics of two chains from the cores (csrc/pairstat.hip), on the GPU, against the fp64 contractions of
oracle/mps.py through the bars of tests/pairstat_cases.py (which tests/test_pairstat_cases_host.py shows to accept the
reference and to reject a wrong k, swapped accumulators, a shifted tile of b, padding counted, a tile left out, NaN of
one object ignored, ``outside`` decided on a alone and an open last bin).

Integer cores: every number equals NumPy's on the references.  Real cores: the sandwich bar, and bit for bit the
identities that tie the joint histogram and the pair record to the single-chain calls of core/valstat.py.  Each figure
is printed before it is asserted.  The chains of oracle/chain_cases.py go through core/pairstat.py; the methods of
NDMPS, thin over the same functions, are tested on encoded volumes at the end.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import pairstat_cases as pc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import pairstat as ps  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _chain(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def _joint(a, b, ea, eb):
    counts, ua, ub, out = ps.joint_histogram(a, b, (ea, eb), outliers=True)
    assert np.array_equal(ua, ea) and np.array_equal(ub, eb) and ua.dtype == ea.dtype and counts.dtype == np.int64
    assert counts.shape == (ea.size - 1, eb.size - 1)
    return counts, out[0], out[1]


def _swapped(st):
    """A pair_stats dict with the _a and _b fields exchanged."""
    out = dict(st)
    for key in st:
        if key.endswith("_a"):
            out[key], out[key[:-2] + "_b"] = st[key[:-2] + "_b"], st[key]
    return out


def _check_swap(back, got):
    """pair_stats(b, a) against pair_stats(a, b): the _a / _b fields exchanged and everything else equal, bit for bit
    (products and squared differences are symmetric in the two values); rel_frob divides by the other norm."""
    want = _swapped(got)
    for key in got:
        assert key == "rel_frob" or back[key] == want[key], (key, back[key], want[key])
    assert back["rel_frob"] == np.sqrt(got["sse"] / got["sumsq_a"])


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.INT_NAMES)
def test_integer_cores_give_numpy_s_numbers_exactly(name, storage):
    p = pc.pair(name, "integer", storage)
    a, b = _chain(p.a.cores, storage), _chain(p.b.cores, storage)
    ra, rb = p.a.ref, p.b.ref
    got = ps.pair_stats(a, b)
    print(f"[pairstat] {name}/{storage}: {got}")
    pc.exact_pair_stats(got, ra, rb)
    n = got["count"]
    assert got["mean_a"] == got["sum_a"] / n and got["mse"] == got["sse"] / n
    assert got["cov"] == got["sum_ab"] / n - got["mean_a"] * got["mean_b"]
    assert got["rel_frob"] == np.sqrt(got["sse"] / got["sumsq_b"])
    assert abs(got["pearson"] - np.corrcoef(ra, rb)[0, 1]) <= 1e-12
    assert ps.pair_stats(a, b) == got, "two calls differ"
    _check_swap(ps.pair_stats(b, a), got)

    for label, (ea, eb) in pc.integer_edge_pairs(ra, rb, pc.NP_TYPE[storage]).items():
        counts, outside, nan = _joint(a, b, ea, eb)
        print(f"[pairstat] {name}/{storage} {label}: {counts.shape} cells, {int(counts.sum())} binned, outside {outside}, nan {nan}")
        pc.exact_joint(counts, outside, nan, ra, rb, ea, eb)
        again = _joint(a, b, ea, eb)
        assert np.array_equal(again[0], counts) and again[1:] == (outside, nan), "two calls differ"
        flipped = _joint(b, a, eb, ea)
        assert np.array_equal(flipped[0], counts.T) and flipped[1:] == (outside, nan), "swapped arguments do not transpose"
    # ints with a range are numpy's linspace per axis, and None asks each object for its own min and max
    rng = ((ra.min() - 0.5, ra.max() + 0.5), (rb.min() - 0.5, rb.max() + 0.5))
    counts, ea, eb = ps.joint_histogram(a, b, (16, 8), range=rng)
    assert np.array_equal(counts, np.histogram2d(ra, rb, (16, 8), range=rng)[0])
    counts, ea, eb = ps.joint_histogram(a, b, 7)
    assert (ea[0], ea[-1], eb[0], eb[-1]) == (ra.min(), ra.max(), rb.min(), rb.max())
    assert np.array_equal(ea, vs.histogram(a, 7)[1]) and np.array_equal(eb, vs.histogram(b, 7)[1])
    want = np.histogram2d(ra, rb, (ea.astype(np.float64), eb.astype(np.float64)))[0]
    assert np.array_equal(counts, want)
    mi = ps.mutual_information(a, b, 7)
    assert mi == ps.mutual_information_from_counts(want.astype(np.int64)) and mi >= 0


@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_in_one_object_only_is_counted_and_the_rest_is_over_the_other_voxels(name, storage):
    p = pc.pair(name, "integer", storage)
    cores_nan, rb_nan = vc.with_nan(p.b)
    a, b = _chain(p.a.cores, storage), _chain(cores_nan, storage)
    ra = p.a.ref
    got = ps.pair_stats(a, b)
    print(f"[pairstat] {name}/{storage} with NaN in b: {got}")
    pc.exact_pair_stats(got, ra, rb_nan)
    assert 0 < got["n_nan"] == int(np.isnan(rb_nan).sum()) < p.n and got["count"] + got["n_nan"] == p.n
    pc.exact_pair_stats(ps.pair_stats(b, a), rb_nan, ra)
    ea, eb = pc.integer_edge_pairs(ra, p.b.ref, pc.NP_TYPE[storage])["1024x16"]  # NaN wins over out of range
    counts, outside, nan = _joint(a, b, ea, eb)
    pc.exact_joint(counts, outside, nan, ra, rb_nan, ea, eb)
    assert nan == got["n_nan"] and outside > 0 and counts.sum() + outside + nan == p.n


# ------------------------------------------------------------------------------------------------ sandwich, identities
@pytest.mark.parametrize("storage", pc.STORAGES)
@pytest.mark.parametrize("name", pc.REAL_NAMES)
def test_real_cores_within_the_sandwich_and_tied_to_the_single_calls(name, storage):
    p = pc.pair(name, "uniform", storage)
    a, b = _chain(p.a.cores, storage), _chain(p.b.cores, storage)
    bars = (p.a.ref, p.a.bound, p.b.ref, p.b.bound)
    got = ps.pair_stats(a, b)
    print(f"[pairstat] {name}/{storage}: {got}")
    pc.sandwich_pair_stats(got, *bars)
    ea, eb = p.a.edges64(), p.b.edges64()
    counts, outside, nan = _joint(a, b, ea, eb)
    print(f"[pairstat] {name}/{storage}: {counts.shape} cells, {int(counts.sum())} binned, outside {outside}, nan {nan}")
    pc.sandwich_joint(counts, outside, nan, *bars, ea, eb)
    assert ps.pair_stats(a, b) == got, "two calls differ"
    again = _joint(a, b, ea, eb)
    assert np.array_equal(again[0], counts) and again[1:] == (outside, nan), "two calls differ"
    flipped = _joint(b, a, eb, ea)
    assert np.array_equal(flipped[0], counts.T) and flipped[1:] == (outside, nan), "swapped arguments do not transpose"
    _check_swap(ps.pair_stats(b, a), got)

    # the marginals are the single-chain histograms, bit for bit.  Edges narrower than the range, so that each object
    # puts voxels outside that the other keeps.  three(e): below, inside and above the range of e as three bins (the
    # last edge of e belongs inside), which tells per bin of one object the voxels that only the other put outside
    def inner(e):
        return e[e.size // 8: e.size - e.size // 8] if e.size >= 16 else e

    def three(e):
        inf = e.dtype.type(np.inf)
        return np.array([-inf, e[0], np.nextafter(e[-1], inf), inf], dtype=e.dtype)

    ia, ib = inner(ea), inner(eb)
    counts, outside, nan = _joint(a, b, ia, ib)
    ha, _, (below_a, above_a, nan_a) = vs.histogram(a, ia, outliers=True)
    hb, _, (below_b, above_b, nan_b) = vs.histogram(b, ib, outliers=True)
    assert nan == nan_a == nan_b == 0
    by_b = _joint(a, b, ia, three(ib))
    by_a = _joint(a, b, three(ia), ib)
    print(f"[pairstat] {name}/{storage}: marginals, {outside} outside, {below_a + above_a} by a, {below_b + above_b} by b")
    assert np.array_equal(by_b[0][:, 1], counts.sum(axis=1)) and np.array_equal(by_a[0][1], counts.sum(axis=0))
    assert np.array_equal(counts.sum(axis=1) + by_b[0][:, 0] + by_b[0][:, 2], ha) and by_b[1] == below_a + above_a
    assert np.array_equal(counts.sum(axis=0) + by_a[0][0] + by_a[0][2], hb) and by_a[1] == below_b + above_b
    assert outside == below_a + above_a + int(by_b[0][:, 0].sum() + by_b[0][:, 2].sum())

    # an object against itself: a diagonal table with its histogram on it, and a record that is the single record
    diag, outside, nan = _joint(a, a, ia, ia)
    assert np.array_equal(diag, np.diag(ha)) and outside == below_a + above_a and nan == 0
    same, single = ps.pair_stats(a, a), vs.value_stats(a)
    print(f"[pairstat] {name}/{storage}: against itself {same}")
    assert same["sse"] == 0 and same["max_abs_diff"] == 0 and same["sum_ab"] == same["sumsq_a"] == same["sumsq_b"]
    assert (same["min_a"], same["max_a"], same["sum_a"], same["sumsq_a"]) == (single["min"], single["max"], single["sum"], single["sumsq"])
    assert (same["min_b"], same["max_b"], same["sum_b"]) == (single["min"], single["max"], single["sum"])
    assert same["count"] == single["count"] and same["mse"] == 0 and same["rel_frob"] == 0


@pytest.mark.parametrize("name", ["L4_tail_last", "L5_ragged", "L1"])
def test_mixed_storage_is_the_fp64_call(name):
    p32, p64 = pc.pair(name, "uniform", "f32"), pc.pair(name, "uniform", "f64")
    a32, b64 = _chain(p32.a.cores, "f32"), _chain(p64.b.cores, "f64")
    a_as_64 = _chain(p32.a.cores, "f64")  # the fp32 cores, cast
    got = ps.pair_stats(a32, b64)
    assert got == ps.pair_stats(a_as_64, b64)
    assert ps.pair_stats(b64, a32) == ps.pair_stats(b64, a_as_64)
    pc.sandwich_pair_stats(got, p32.a.ref, cb.to_volume(cb.chain_bound(p32.a.cores, *cb.CHAIN_ROUNDOFF["f64"]).reshape(-1), p32.a.dest),
                           p64.b.ref, p64.b.bound)
    mixed = ps.joint_histogram(a32, b64, 16, outliers=True)
    wide = ps.joint_histogram(a_as_64, b64, 16, outliers=True)
    assert mixed[1].dtype == np.float64 and all(np.array_equal(x, y) for x, y in zip(mixed[:3], wide[:3])) and mixed[3] == wide[3]


# ------------------------------------------------------------------------------------------------ through the class
SHIFTS = (-2, -1, 0, 1, 2)


@pytest.fixture(scope="module")
def encoded():
    """Two modalities of one anatomy: the phantom, and a nonlinear (non-monotone) intensity map of it."""
    x = synthetic_mri((32, 32, 32), seed=11)
    lo, hi = float(x.min()), float(x.max())
    u = (x - lo) / (hi - lo)
    y = (0.2 + np.sin(np.pi * u) ** 2 + 0.3 * u).astype(x.dtype)
    objs = {}
    for storage, dt in TORCH_DT.items():
        ox = NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=dt)
        oy = NDMPS.from_tensor(y, max_bond=12, device=DEV, dtype=dt)
        objs[storage] = (ox, oy)
    return x, y, objs


def _reference(obj, shape, storage):
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), dest)
    return ref, cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest)


@pytest.mark.parametrize("storage", pc.STORAGES)
def test_methods_on_encoded_volumes(encoded, storage):
    x, y, objs = encoded
    ox, oy = objs[storage]
    rx, bx = _reference(ox, x.shape, storage)
    st = ox.pair_stats(oy)
    print(f"[pairstat] class/{storage}: {st}")
    ry, by = _reference(oy, x.shape, storage)
    pc.sandwich_pair_stats(st, rx, bx, ry, by)
    counts, ea, eb, out = ox.joint_histogram(oy, bins=(16, 12), outliers=True)
    assert counts.shape == (16, 12) and np.array_equal(ea, ox.histogram(16)[1]) and np.array_equal(eb, oy.histogram(12)[1])
    pc.sandwich_joint(counts, out[0], out[1], rx, bx, ry, by, ea, eb)
    plain = ox.joint_histogram(oy, bins=(16, 12))
    assert len(plain) == 3 and np.array_equal(plain[0], counts)
    counts, ea, eb, out = ox.joint_histogram(oy, bins=8, range=((0.2, 0.6), (0.3, 0.9)), outliers=True)
    assert out[0] > 0 and np.array_equal(ea, np.linspace(0.2, 0.6, 9).astype(ea.dtype))
    pc.sandwich_joint(counts, out[0], out[1], rx, bx, ry, by, ea, eb)

    # mutual information against NumPy on the decoded pair, through the sandwich.  The bar in counts: a voxel can leave
    # its reference's cell only if it lies within its bound of an edge on either axis, so at most `moved` voxels differ
    # between the computed table and NumPy's on the references (out of range included: then it leaves the table).  With
    # H = ln N - (1 / N) sum c ln c, and (c + 1) ln(c + 1) - c ln c <= ln N + 1, one voxel moved between two cells
    # changes an entropy by at most (ln N + 1) / N and one voxel removed by at most (ln N + 2) / (N - 1); MI is
    # H(a) + H(b) - H(a, b): at most 3 (ln N + 2) / (N - moved) per voxel
    bins = 16
    ea, eb = ox.histogram(bins)[1], oy.histogram(bins)[1]
    got = ox.mutual_information(oy, bins=(ea, eb))
    want = ps.mutual_information_from_counts(pc.ref_joint(rx, ry, ea, eb)[0])
    near = lambda r, b, e: np.abs(r[:, None] - np.asarray(e, dtype=np.float64)[None, :]).min(axis=1) <= b  # noqa: E731
    moved = int((near(rx, bx, ea) | near(ry, by, eb)).sum())
    n = rx.size
    slack = moved * 3 * (np.log(n) + 2) / (n - moved)
    print(f"[pairstat] class/{storage}: MI {got} against {want} on the references, {moved} voxels near an edge, slack {slack}")
    assert moved <= 0.02 * n and abs(got - want) <= slack + 1e-12
    dx, dy = np.asarray(ox.to_tensor(), dtype=np.float64).reshape(-1), np.asarray(oy.to_tensor(), dtype=np.float64).reshape(-1)
    decoded = ps.mutual_information_from_counts(np.histogram2d(dx, dy, (ea.astype(np.float64), eb.astype(np.float64)))[0].astype(np.int64))
    print(f"[pairstat] class/{storage}: MI {decoded} from NumPy on the decoded pair")
    assert abs(got - decoded) <= 2 * slack + 1e-12
    nmi = ox.mutual_information(oy, bins=(ea, eb), normalized=True)
    assert 1.0 < nmi <= 2.0 + 1e-12

    # registration by mutual information: the other modality rolled along an axis, scored against the fixed one
    fixed_edges = ox.histogram(bins)[1]
    moving = [oy.roll(s, axis=1) for s in SHIFTS]
    scores = [m.mutual_information(ox, bins=(bins, fixed_edges)) for m in moving]
    print(f"[pairstat] class/{storage}: MI over shifts {SHIFTS}: {scores}")
    assert int(np.argmax(scores)) == SHIFTS.index(0)
    many = NDMPS.mutual_information_many(moving, ox, bins=bins)
    assert many.shape == (len(SHIFTS),) and many.dtype == np.float64
    for t, m in enumerate(moving):
        assert many[t] == m.mutual_information(ox, bins=(bins, fixed_edges)), t


def test_refusals(encoded):
    x, y, objs = encoded
    ox, oy = objs["f32"]
    other_shape = NDMPS.from_tensor(x[:, :, :16].copy(), max_bond=4, device=DEV)
    for call in (lambda a, b: a.pair_stats(b), lambda a, b: a.joint_histogram(b), lambda a, b: a.mutual_information(b),
                 lambda a, b: NDMPS.mutual_information_many([a], b)):
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"), oy)
        with pytest.raises(ValueError, match="DCT"):
            call(ox, NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(ox, oy.astype(torch.bfloat16))
        with pytest.raises(ValueError, match="shape"):
            call(ox, other_shape)
        with pytest.raises(TypeError):
            call(ox, y)
    with pytest.raises(ValueError, match="1024 bins per axis"):
        ox.joint_histogram(oy, bins=(1025, 2))
    with pytest.raises(ValueError, match="16384 cells"):
        ox.joint_histogram(oy, bins=(1024, 17))
    with pytest.raises(ValueError, match="ascending"):
        ox.joint_histogram(oy, bins=([0.0, 0.5, 0.25], 4))
    with pytest.raises(ValueError):
        ox.joint_histogram(oy, bins=(0, 4))
    with pytest.raises(ValueError):
        ox.joint_histogram(oy, bins=(4, 4, 4))
    counts, _, _ = ox.joint_histogram(ox, bins=(1024, 16))  # the largest table
    assert counts.sum() == x.size
