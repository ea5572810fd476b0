"""Histograms, quantiles and medians per label from the cores (LabelHistEpi in csrc/labelhist.hip, core/labelhist.py), on
the GPU, against NumPy on the fp64 contraction of oracle/mps.py through the bars of tests/labelhist_cases.py (which
tests/test_labelhist_host.py shows to accept the reference and to reject labels read in site order, a tile left out,
padding counted, folded windows, the shared row used for per-label rows, an open last bin, NaN in a bin, outside
voxels added to a label and a voxel on a repeated last edge lost).

Integer cores: every number must equal NumPy's on the reference, bit for bit.  Real cores: the sandwich bar, every
figure printed before it is asserted.  The chains of oracle/chain_cases.py go through core/labelhist.py with the plan
of ``cc.factor_array``; the methods of NDMPS, which are thin over the same functions, are tested on an encoded volume
at the end, against NumPy on the object's own ``to_tensor()``: the decoded voxel and the voxel the reducing product
computes each lie within the chain's element bound of the exact contraction, so the bars run with twice that bound.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import labelhist_cases as hc  # noqa: E402
import labelstat_cases as lc  # noqa: E402
import valstat_cases as vc  # noqa: E402
from imgcompressionmps_amd import NDMPS  # noqa: E402
from imgcompressionmps_amd.core import labelhist as lh  # noqa: E402
from imgcompressionmps_amd.core import labelstat as ls  # noqa: E402
from imgcompressionmps_amd.core import valstat as vs  # noqa: E402
from imgcompressionmps_amd.core.mps import DeviceMPS  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import chain_cases as cc  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_to_dense  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
BINS = 64  # of the quantile passes: label_quantile's default, which serves 4096 labels


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


def _chain(cores, storage):
    return DeviceMPS([torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]) for c in cores])


def _plan(c):
    return _plan_for(c.shape, 0, factor_arr=c.fa)


def _hist(chain, plan, volume, n_labels, edges):
    """The result dict of the bars from ``label_histogram`` with explicit edges, which come back as they went in."""
    counts, used, out = lh.label_histogram(chain, plan, volume, n_labels, edges, outliers=True)
    assert np.array_equal(used, edges) and used.dtype == edges.dtype
    assert counts.shape[1] == edges.size - 1 and counts.dtype == np.int64 and isinstance(out["outside"], int)
    assert n_labels is None or counts.shape[0] == n_labels
    assert set(out) == {"below", "above", "n_nan", "outside"}
    plain = lh.label_histogram(chain, plan, volume, n_labels, edges)
    assert len(plain) == 2 and np.array_equal(plain[0], counts)
    return dict(counts=counts, **out)


def _rows(chain, plan, volume, n_labels, rows):
    """The same dict from one edge row per label, through the frame the quantile passes use."""
    labels, n_labels = ls.check_labels(volume, plan.shape, n_labels)
    with torch.cuda.device(chain.device):
        frame = lh._frames([chain], plan, labels, n_labels, [(rows.shape[1] - 1, True)])[0]
        cells, lo, hi, outside = frame.run(rows)
    bins = rows.shape[1] - 1
    return dict(counts=cells[:, :bins].copy(), below=cells[:, bins].copy(), above=cells[:, bins + 1].copy(),
                n_nan=cells[:, bins + 2].copy(), outside=outside), lo, hi


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_integer_cores_give_numpy_s_histograms_exactly(name, storage):
    c = vc.case(name, "integer", storage)
    np_type = vc.NP_TYPE[storage]
    chain, plan = _chain(c.cores, storage), _plan(c)
    sets = vc.integer_edge_sets(c.ref, np_type)
    whole = {label: vs.histogram(chain, edges, outliers=True) for label, edges in sets.items()}
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        volume = lab.reshape(c.shape).astype(np.int32)
        stats = ls.label_stats(chain, plan, volume, n_labels)
        ran = []
        for label, edges in sets.items():
            want_plan = hc.window_rule(np.dtype(np_type).itemsize, n_labels, edges.size - 1, False)
            if want_plan is None:  # more than 64 launches: refused, with the two remedies
                with pytest.raises(ValueError, match="fewer bins or split the atlas"):
                    lh.label_histogram(chain, plan, volume, n_labels, edges)
                continue
            assert lh.plan_query(np_type, n_labels, edges.size - 1, False) == want_plan
            got = _hist(chain, plan, volume, n_labels, edges)
            ran.append(label)
            print(f"[labelhist] {name}/{storage} {kind} {label}: L {n_labels}, {edges.size - 1} bins, {want_plan['launches']} "
                  f"launches of {want_plan['window']} labels, outside {got['outside']}, below {got['below'][:4]}, "
                  f"above {got['above'][:4]}")
            hc.exact_histogram(got, c.ref, lab, n_labels, edges)
            # pinned to what exists: the whole-volume histogram and the label statistics
            counts, _, (below, above, nan) = whole[label]
            if kind == "one":
                assert lc.same_bits(got["counts"][0], counts)
                assert (got["below"][0], got["above"][0], got["n_nan"][0]) == (below, above, nan)
            if got["outside"] == 0:
                assert np.array_equal(got["counts"].sum(axis=0), counts)
                assert (got["below"].sum(), got["above"].sum(), got["n_nan"].sum()) == (below, above, nan)
            assert np.array_equal(got["counts"].sum(axis=1) + got["below"] + got["above"], stats["count"])
            assert np.array_equal(got["n_nan"], stats["n_nan"]) and got["outside"] == stats["outside"]
            if label == "bins_4096" and n_labels == 7:  # a window of one or two labels: the call spans several launches
                assert want_plan["window"] == (2 if storage == "f32" else 1) and want_plan["launches"] == -(-7 // want_plan["window"])
            if label == "range_excludes":
                assert got["below"].sum() > 0 and got["above"].sum() > 0
                assert hc.same_result(_hist(chain, plan, volume, n_labels, edges), got), "two calls differ"
        assert {"one_bin", "one_bin_inside", "range_excludes"} <= set(ran), (kind, ran)
        if kind == "outside":
            assert got["outside"] == 3
        if kind in ("window", "max"):  # more labels than one launch holds, for some table that ran
            assert any(hc.window_rule(np.dtype(np_type).itemsize, n_labels, sets[label].size - 1, False)["launches"] > 1
                       for label in ran), ran


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", sorted(vc.INT_CHAINS))
def test_integer_cores_give_numpy_s_quantiles_exactly(name, storage):
    c = vc.case(name, "integer", storage)
    np_type = vc.NP_TYPE[storage]
    chain, plan = _chain(c.cores, storage), _plan(c)
    passes = hc.passes_for(c.ref, BINS)
    for kind in lc.kinds_for(name, c.n):
        lab, n_labels = lc.labels(c, kind)
        volume = lab.reshape(c.shape).astype(np.int32)
        assert lh.plan_query(np_type, n_labels, BINS, True) == hc.window_rule(np.dtype(np_type).itemsize, n_labels, BINS, True)
        many = lh.label_quantile(chain, plan, volume, list(hc.QS), n_labels, passes, BINS)
        assert many["value"].shape == (n_labels, len(hc.QS))
        print(f"[labelhist] {name}/{storage} {kind}: L {n_labels}, {passes} passes of {BINS} bins, outside {many['outside']}, "
              f"quantiles of label 0 {many['value'][0]}")
        for j, q in enumerate(hc.QS):
            column = dict(many, value=many["value"][:, j].copy(), lo=many["lo"][:, j].copy(), hi=many["hi"][:, j].copy())
            hc.exact_quantile(column, c.ref, lab, n_labels, q)
            if n_labels <= 9:  # a sequence of q equals the scalar calls, bit for bit
                one = lh.label_quantile(chain, plan, volume, q, n_labels, passes, BINS)
                assert one["value"].shape == (n_labels,) and hc.same_result(one, column), q
            if kind == "one":  # the whole volume's quantile, in value and bracket
                value, (lo, hi) = vs.quantile(chain, q, passes, BINS)
                assert (column["value"][0], column["lo"][0], column["hi"][0]) == (value, lo, hi), q
        if kind == "empty":
            assert np.isnan(many["value"][7:]).all() and np.all(many["count"][7:] == 0)
        if kind == "blocks":
            median = lh.label_median(chain, plan, volume, n_labels, passes, BINS)
            assert lc.same_bits(median, many["value"][:, hc.QS.index(0.5)].copy())


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_wide", "int_tail_all"])
def test_one_edge_row_per_label_exactly(name, storage):
    """Rows over each label's own range, short rows padded with their last edge, on which some voxel sits."""
    c = vc.case(name, "integer", storage)
    np_type = vc.NP_TYPE[storage]
    chain, plan = _chain(c.cores, storage), _plan(c)
    for kind in [k for k in ("blocks", "scatter", "outside", "window") if k in lc.kinds_for(name, c.n)]:
        lab, n_labels = lc.labels(c, kind)
        bins = 16 if kind != "window" else 255
        rows = hc.per_label_rows(c.ref, lab, n_labels, bins, np_type)
        query = lh.plan_query(np_type, n_labels, bins, True)
        got, lo, hi = _rows(chain, plan, lab.reshape(c.shape), n_labels, rows)
        print(f"[labelhist] {name}/{storage} {kind} rows: {query}, below {got['below'][:4]}, above {got['above'][:4]}")
        hc.exact_histogram(got, c.ref, lab, n_labels, rows)
        if kind == "window":
            assert query["launches"] > 1
        inside = (lab >= 0) & (lab < n_labels)
        row_of = np.where(inside, lab, 0)
        assert np.all(rows[:, -2] == rows[:, -1])  # every row is padded, and the label's largest voxel sits on the padding
        on_padding = np.bincount(lab[inside & (c.ref == rows[row_of, -1])], minlength=n_labels)
        assert np.all(on_padding[np.bincount(lab[inside], minlength=n_labels) > 0] > 0) and got["above"].sum() == 0
        assert got["below"].sum() > 0
        # the extremes of the voxels inside each row's range
        taken = inside & (c.ref >= rows[row_of, 0]) & (c.ref <= rows[row_of, -1])
        want_lo = lc.per_label(np.fmin, c.ref[taken], lab[taken], n_labels)
        want_hi = lc.per_label(np.fmax, c.ref[taken], lab[taken], n_labels)
        assert lc.same_bits(lo, want_lo) and lc.same_bits(hi, want_hi)


@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name", ["int_tail_all", "int_no_tail"])
def test_nan_voxels_are_counted_per_label_and_land_in_no_bin(name, storage):
    c = vc.case(name, "integer", storage)
    cores, ref = vc.with_nan(c)
    chain, plan = _chain(cores, storage), _plan(c)
    nan = np.isnan(ref)
    assert 0 < nan.sum() < c.n
    passes = hc.passes_for(ref, BINS)
    for kind in ("blocks", "scatter"):
        lab, n_labels = lc.labels(c, kind)
        for label in ("half_integers", "range_excludes"):
            edges = vc.integer_edge_sets(ref, vc.NP_TYPE[storage])[label]
            got = _hist(chain, plan, lab.reshape(c.shape), n_labels, edges)
            print(f"[labelhist] {name}/{storage} {kind} {label} with NaN: n_nan {got['n_nan']}")
            hc.exact_histogram(got, ref, lab, n_labels, edges)
            assert np.array_equal(got["n_nan"], np.bincount(lab[nan], minlength=n_labels))
        quant = lh.label_quantile(chain, plan, lab.reshape(c.shape), 0.5, n_labels, passes, BINS)
        hc.exact_quantile(quant, ref, lab, n_labels, 0.5)
    lab = np.where(nan, 7, lc.labels(c, "blocks")[0])  # a label whose voxels are all NaN
    quant = lh.label_quantile(chain, plan, lab.reshape(c.shape), [0.0, 1.0], 8, passes, BINS)
    assert np.isnan(quant["value"][7]).all() and quant["count"][7] == 0 and quant["n_nan"][7] == nan.sum()
    hc.exact_quantile(dict(quant, value=quant["value"][:, 1].copy(), lo=quant["lo"][:, 1].copy(), hi=quant["hi"][:, 1].copy()),
                      ref, lab, 8, 1.0)


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_an_infinite_voxel_is_binned_not_refused(storage):
    c = vc.case("L6_bonds_one", "uniform", storage)
    cores = [x.copy() for x in c.cores]
    cores[0][0, 1, 0] = np.inf
    ref = cb.to_volume(mps_to_dense(cores).reshape(-1), c.dest)
    assert np.isinf(ref).sum() == c.n // 4 and not np.isnan(ref).any()
    chain, plan = _chain(cores, storage), _plan(c)
    lab, n_labels = lc.labels(c, "blocks")
    edges = np.array([-np.inf, -1.0, 0.0, 1.0, np.inf], dtype=vc.NP_TYPE[storage])
    got = _hist(chain, plan, lab.reshape(c.shape), n_labels, edges)
    want = hc.hist_of(ref, lab, n_labels, edges)
    # the two outer bins hold the infinite voxels and whatever else lies beyond -1 and 1; the sign of a voxel is exact
    assert np.array_equal(got["counts"][:, [0, 1]].sum(axis=1), want["counts"][:, [0, 1]].sum(axis=1))
    assert np.array_equal(got["counts"].sum(axis=1), want["counts"].sum(axis=1)) and got["below"].sum() == got["above"].sum() == 0
    # the largest voxel of a label: +inf where it has one, and within the bound of the reference's elsewhere
    top = lh.label_quantile(chain, plan, lab.reshape(c.shape), 1.0, n_labels)
    want = hc.quantile_of(ref, lab, n_labels, 1.0)
    assert np.isposinf(want).any() and not np.isposinf(want).all()
    assert np.array_equal(np.isposinf(top["value"]), np.isposinf(want)) and np.array_equal(np.isposinf(top["hi"]), np.isposinf(want))
    finite = ~np.isposinf(want)
    assert np.all(np.abs(top["hi"][finite] - want[finite]) <= c.bound.max())
    bottom = lh.label_quantile(chain, plan, lab.reshape(c.shape), 0.0, n_labels)
    assert np.array_equal(np.isneginf(bottom["lo"]), np.isneginf(hc.quantile_of(ref, lab, n_labels, 0.0)))


# ------------------------------------------------------------------------------------------------ sandwich
@pytest.mark.parametrize("storage", vc.STORAGES)
@pytest.mark.parametrize("name,family", vc.REAL_CASES, ids=vc.REAL_IDS)
def test_real_cores_within_the_sandwich(name, family, storage):
    c = vc.case(name, family, storage)
    chain, plan = _chain(c.cores, storage), _plan(c)
    edges = c.edges64()
    for kind in lc.REAL_KINDS:
        lab, n_labels = lc.labels(c, kind)
        volume = lab.reshape(c.shape)
        show = lambda *figures: print(f"[labelhist] {name}/{family}/{storage} {kind}:", *figures)  # noqa: E731
        got = _hist(chain, plan, volume, n_labels, edges)
        hc.sandwich_histogram(got, c.ref, c.bound, lab, n_labels, edges, show)
        assert hc.same_result(_hist(chain, plan, volume, n_labels, edges), got), "two calls differ"
        many = lh.label_quantile(chain, plan, volume, [0.0, 0.5, 0.9, 1.0], n_labels)
        for j, q in enumerate((0.0, 0.5, 0.9, 1.0)):
            column = dict(many, value=many["value"][:, j], lo=many["lo"][:, j], hi=many["hi"][:, j])
            hc.sandwich_quantile(column, c.ref, c.bound, lab, n_labels, q, show)
        stats = ls.label_stats(chain, plan, volume, n_labels)
        assert np.array_equal(many["count"], stats["count"]) and many["outside"] == stats["outside"]
        # the bracket of q = 0 starts at the label's smallest voxel and that of q = 1 ends at its largest
        assert np.array_equal(many["lo"][:, 0], stats["min"]) and np.array_equal(many["hi"][:, 3], stats["max"])


# ------------------------------------------------------------------------------------------------ label types, series
def test_every_label_type_gives_the_same_result():
    c = vc.case("int_wide", "integer", "f32")
    chain, plan = _chain(c.cores, "f32"), _plan(c)
    edges = vc.integer_edge_sets(c.ref, np.float32)["range_excludes"]
    for kind in ("scatter", "outside", "window"):
        lab, n_labels = lc.labels(c, kind)
        volume = lab.reshape(c.shape)
        got = _hist(chain, plan, volume.astype(np.int32), n_labels, edges)
        quant = lh.label_quantile(chain, plan, volume.astype(np.int32), 0.25, n_labels)
        others = [volume.astype(np.int16), volume.astype(np.int64), torch.from_numpy(volume).to(DEV).to(torch.int32),
                  torch.from_numpy(volume).to(DEV).to(torch.int64), torch.from_numpy(volume).to(DEV).to(torch.int16)]
        if lab.min() >= 0 and lab.max() < 256:
            others += [volume.astype(np.uint8), torch.from_numpy(volume.astype(np.uint8)).to(DEV)]
        for other in others:
            assert hc.same_result(_hist(chain, plan, other, n_labels, edges), got), other.dtype
            assert hc.same_result(lh.label_quantile(chain, plan, other, 0.25, n_labels), quant), other.dtype
        if kind == "scatter":  # n_labels from the labels
            assert hc.same_result(_hist(chain, plan, volume, None, edges), got)
    mask = (np.arange(c.n) % 3 == 1).reshape(c.shape)
    got = _hist(chain, plan, mask, None, edges)
    hc.exact_histogram(got, c.ref, mask.reshape(-1).astype(np.int64), 2, edges)
    for other in (mask.astype(np.uint8), mask.astype(np.int64), torch.from_numpy(mask).to(DEV)):
        assert hc.same_result(_hist(chain, plan, other, None, edges), got), other.dtype


SERIES_DIMS = cc.INTEGER_CHAINS["int_wide"][0]
SERIES = [([1, 8, 16, 10, 1], "f32"), ([1, 4, 8, 5, 1], "f32"), ([1, 8, 12, 7, 1], "f32")]


def test_series_rows_equal_the_single_calls_and_upload_once():
    c = vc.case("int_wide", "integer", "f32")  # the shape, the plan and the index map of the frames
    plan = _plan(c)
    frames, refs = [], []
    for t, (bonds, storage) in enumerate(SERIES):
        cc.check_chain(SERIES_DIMS, bonds)
        cores = cc.draw_cores(f"labelhist_series_{t}", SERIES_DIMS, bonds, "integer", storage)
        frames.append(_chain(cores, storage))
        refs.append(cb.to_volume(mps_to_dense(cores).reshape(-1), c.dest))
    lo, hi = min(r.min() for r in refs), max(r.max() for r in refs)
    for kind in ("scatter", "window"):
        lab, n_labels = lc.labels(c, kind)
        volume = torch.from_numpy(lab.reshape(c.shape)).to(DEV).to(torch.int16)
        lh.label_histogram(frames[0], plan, volume, n_labels, 16)  # the plan's tables are built on first use and kept
        uploads = ls.LABEL_UPLOADS
        counts, edges, out = lh.label_histogram_many(frames, plan, volume, n_labels, 16, outliers=True)
        assert ls.LABEL_UPLOADS == uploads + 1, "the label volume went to the device more than once"
        # one edge table over the minimum and the maximum of all frames
        assert edges.dtype == np.float32 and np.array_equal(edges, np.linspace(lo, hi, 17).astype(np.float32))
        assert counts.shape == (3, n_labels, 16) and out["below"].shape == (3, n_labels) and out["outside"].shape == (3,)
        assert len(lh.label_histogram_many(frames, plan, volume, n_labels, 16)) == 2
        for t, (frame, ref) in enumerate(zip(frames, refs)):
            one = _hist(frame, plan, volume, n_labels, edges)
            row = dict(counts=counts[t].copy(), below=out["below"][t].copy(), above=out["above"][t].copy(),
                       n_nan=out["n_nan"][t].copy(), outside=int(out["outside"][t]))
            assert hc.same_result(row, one), t
            hc.exact_histogram(one, ref, lab, n_labels, edges)
    with pytest.raises(ValueError, match="at least one"):
        lh.label_histogram_many([], plan, volume, n_labels)


# ------------------------------------------------------------------------------------------------ through the class
@pytest.fixture(scope="module")
def encoded():
    x = synthetic_mri((32, 48, 40), seed=7)
    return x, {
        "f32": NDMPS.from_tensor(x, max_bond=12, device=DEV),
        "f64": NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=torch.float64),
    }


def _atlas(shape):
    """Eight octants, a central ball (label 8) and -1 on one face."""
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    atlas = sum(((g >= n // 2).astype(np.int64) << a) for a, (g, n) in enumerate(zip(grid, shape)))
    r2 = sum(((g - (n - 1) / 2) / (n / 4)) ** 2 for g, n in zip(grid, shape))
    atlas[r2 <= 1.0] = 8
    atlas[0] = -1
    return atlas


@pytest.mark.parametrize("storage", vc.STORAGES)
def test_methods_on_an_encoded_volume_against_numpy_on_its_own_decode(encoded, storage):
    x, objs = encoded
    obj = objs[storage]
    cores = [t.to(torch.float64).cpu().numpy() for t in obj.mps.cores]
    dest = im.flat_destination(x.shape).reshape(-1)
    # the decode and the reducing product each lie within the chain's bound of the exact contraction
    bound = 2 * cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]).reshape(-1), dest)
    ref = np.asarray(obj.to_tensor(), dtype=np.float64).reshape(-1)
    atlas = _atlas(x.shape)
    lab = atlas.reshape(-1)
    show = lambda *figures: print(f"[labelhist] class/{storage}:", *figures)  # noqa: E731

    counts, edges, out = obj.label_histogram(atlas, bins=32, outliers=True)
    whole_counts, whole_edges = obj.histogram(bins=32)
    assert np.array_equal(edges, whole_edges) and edges.dtype == vc.NP_TYPE[storage] and counts.shape == (9, 32)
    assert out["outside"] == x.shape[1] * x.shape[2]
    hc.sandwich_histogram(dict(counts=counts, **out), ref, bound, lab, 9, edges, show)
    counts, edges, out = obj.label_histogram(atlas, 9, 8, (0.2, 0.6), True)
    assert out["below"].sum() > 0 and out["above"].sum() > 0
    hc.sandwich_histogram(dict(counts=counts, **out), ref, bound, lab, 9, edges, show)
    assert np.array_equal(obj.label_histogram(torch.from_numpy(atlas).to(DEV), 9, 8, (0.2, 0.6))[0], counts)

    quant = obj.label_quantile(atlas, 0.5)
    hc.sandwich_quantile(quant, ref, bound, lab, 9, 0.5, show)
    assert lc.same_bits(obj.label_median(atlas), quant["value"])
    wide = obj.label_quantile(atlas, [0.01, 0.99], passes=3)
    for j, q in enumerate((0.01, 0.99)):
        hc.sandwich_quantile(dict(wide, value=wide["value"][:, j], lo=wide["lo"][:, j], hi=wide["hi"][:, j]), ref, bound, lab, 9,
                             q, show)
    # three passes of 64 bins inside a label's range, which the volume's contains, and the rounding of the edges
    span = obj.max() - obj.min()
    assert np.all(wide["hi"] - wide["lo"] <= span / 64 ** 3 + 4 * np.finfo(vc.NP_TYPE[storage]).eps * np.abs(ref).max())

    # a mask: two labels, row 1
    mask = atlas == 8
    inside = mask.reshape(-1).astype(np.int64)
    counts, edges, outliers = obj.histogram(bins=8, range=(0.2, 0.6), outliers=True, mask=mask)
    assert counts.shape == (8,) and counts.sum() + sum(outliers) == mask.sum()
    both = lh.label_histogram(obj.mps, _plan_for(x.shape, 0), mask, 2, 8, (0.2, 0.6), True)
    assert np.array_equal(both[0][1], counts) and np.array_equal(both[1], edges)
    got = dict(counts=both[0], **both[2])
    hc.sandwich_histogram(got, ref, bound, inside, 2, edges, show)
    assert len(obj.histogram(bins=8, range=(0.2, 0.6), mask=mask)) == 2
    for other in (mask.astype(np.uint8) * 7, torch.from_numpy(mask).to(DEV), atlas * mask):
        assert np.array_equal(obj.histogram(bins=8, range=(0.2, 0.6), mask=other)[0], counts)
    n = int(mask.sum())
    for q in (0.0, 0.5, 1.0):
        value, (lo, hi) = obj.quantile(q, mask=mask)
        k = min(max(int(np.ceil(n * q - 1)), 0), n - 1)
        least, most = np.sort((ref - bound)[mask.reshape(-1)])[k], np.sort((ref + bound)[mask.reshape(-1)])[k]
        show("quantile", q, "mask", value, (lo, hi), "rank voxel in", (least, most))
        assert lo <= value <= hi and lo <= most and hi >= least
    assert obj.median(mask=mask) == obj.quantile(0.5, mask=mask)[0]
    assert obj.median() == obj.quantile(0.5)[0]
    everything = np.ones(x.shape, dtype=bool)
    assert obj.quantile(0.5, mask=everything) == obj.quantile(0.5)  # every voxel inside: the whole volume's answer
    assert np.isnan(obj.median(mask=np.zeros(x.shape, dtype=bool)))


def test_without_a_mask_histogram_and_quantile_are_unchanged(encoded):
    x, objs = encoded
    for obj in objs.values():
        for args in ((32, None), (8, (0.2, 0.6))):
            got, want = obj.histogram(*args, outliers=True), vs.histogram(obj.mps, *args, outliers=True)
            assert lc.same_bits(got[0], want[0]) and lc.same_bits(got[1], want[1]) and got[2] == want[2]
            assert lc.same_bits(obj.histogram(*args, mask=None)[0], want[0])
        for q in (0.0, 0.3, 1.0):
            assert obj.quantile(q) == obj.quantile(q, mask=None) == vs.quantile(obj.mps, q)
        assert obj.quantile(0.3, 1, 64) == vs.quantile(obj.mps, 0.3, 1, 64)


def test_refusals(encoded):
    x, objs = encoded
    obj = objs["f32"]
    atlas = _atlas(x.shape)
    mask = atlas == 8
    calls = (lambda o: o.label_histogram(atlas), lambda o: NDMPS.label_histogram_many([o], atlas),
             lambda o: o.label_quantile(atlas, 0.5), lambda o: o.label_median(atlas), lambda o: o.median(mask=mask),
             lambda o: o.median(), lambda o: o.histogram(mask=mask), lambda o: o.quantile(0.5, mask=mask))
    for call in calls:
        with pytest.raises(ValueError, match="DCT"):
            call(NDMPS.from_tensor(x, max_bond=4, device=DEV, mode="DCT"))
        with pytest.raises(ValueError, match=r"astype\(torch.float32\)"):
            call(obj.astype(torch.bfloat16))
        unknown = NDMPS.from_tensor(x, max_bond=4, device=DEV)
        unknown._shape = None
        with pytest.raises(ValueError, match="shape is unknown"):
            call(unknown)
    for call in (lambda a: obj.label_histogram(a), lambda a: obj.label_quantile(a, 0.5), lambda a: obj.label_median(a),
                 lambda a: obj.histogram(mask=a), lambda a: obj.quantile(0.5, mask=a), lambda a: obj.median(mask=a)):
        with pytest.raises(ValueError, match="shape"):
            call(atlas[:-1])
        with pytest.raises(TypeError):
            call(atlas.astype(np.float32))
    with pytest.raises(ValueError, match="at most 4096 labels"):
        obj.label_histogram(atlas, 4097)
    with pytest.raises(ValueError, match="at most 4096 labels"):
        obj.label_quantile(atlas * 1000, 0.5)
    with pytest.raises(ValueError, match="at most 4096 bins"):
        obj.label_histogram(atlas, bins=4097)
    with pytest.raises(ValueError, match="at most 4096 bins"):
        obj.histogram(bins=4097, mask=mask)
    with pytest.raises(ValueError, match="ascending"):
        obj.label_histogram(atlas, bins=[0.0, 0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="fewer bins or split the atlas"):
        obj.label_histogram(atlas, 4096, 4096)
    with pytest.raises(ValueError, match="fewer bins or split the atlas"):
        obj.label_quantile(atlas, 0.5, 4096, bins=4096)
    with pytest.raises(ValueError, match=r"\[1, 4096\]"):
        obj.label_quantile(atlas, 0.5, bins=0)
    for q in (1.5, -0.1, [0.5, 2.0], [[0.5]], []):
        with pytest.raises(ValueError, match="q must"):
            obj.label_quantile(atlas, q)
    with pytest.raises(ValueError):
        obj.quantile(1.5, mask=mask)
    other = NDMPS.from_tensor(synthetic_mri((32, 48, 20), seed=7), max_bond=4, device=DEV)
    with pytest.raises(ValueError, match="shape"):
        NDMPS.label_histogram_many([obj, other], atlas)
    with pytest.raises(ValueError):
        NDMPS.label_histogram_many([], atlas)
    many = NDMPS.label_histogram_many([objs["f32"], objs["f64"]], atlas, bins=8)
    assert many[0].shape == (2, 9, 8)
    assert np.array_equal(many[0][0], objs["f32"].label_histogram(atlas, bins=many[1])[0])
