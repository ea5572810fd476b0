"""Every decoder on arbitrary cores against one fp64 contraction (oracle/mps.py), element by element.

The bar is ``oracle.chain_bound``: the textbook forward error bound of a product of L matrices,
``1.01 * (u_acc * sum(chi) + u_store * (L - 1)) * |A_0| ... |A_{L-1}|``, which holds for every association and
order of summation and therefore owes nothing to what the kernels return (tests/test_decode_bound_host.py checks it
on the CPU, and that a dropped term, two swapped columns or a transposed core leave it, on the same cases).
Roundoffs (u_acc / u_store): fp32 chain 2**-24 / 2**-24, fp64 chain 2**-53 / 2**-53, bf16 chain 2**-24 / 2**-8
(fp32 accumulator, bf16 intermediates), overlap 2**-53 / 2**-53.  decode_region / values_at and downsample / sum /
mean widen bf16 cores to fp32, contract in fp32 and reduce in fp64, so for bf16 storage their u_store is 2**-24, not
2**-8; for the reductions the bound is the same reduction of the element bounds.

Outputs are pre-filled with NaN, so an element no kernel wrote fails.  Integer chains ({-1, 0, 1} cores whose
partial products stay below 2**24 / 2**53 / 257) must come out bit for bit.  The largest error / bound per storage
type is printed when the module finishes; it is reported, never asserted against.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS, _lib  # noqa: E402
from imgcompressionmps_amd.core.ndmps import _plan_for  # noqa: E402
from oracle import chain_bound as cb  # noqa: E402
from oracle import chain_cases as cc  # noqa: E402
from oracle import index_map as im  # noqa: E402
from oracle.metrics import synthetic_mri  # noqa: E402
from oracle.mps import mps_overlap, mps_to_dense  # noqa: E402

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TORCH_DT = {"f32": F32, "bf16": BF16, "f64": F64}
NAME_OF = {F32: "f32", BF16: "bf16", F64: "f64"}
NAN = float("nan")

ALL = dict(cc.CHAINS, **cc.INTEGER_CHAINS)
FAMILIES = ([(n, "uniform") for n in cc.CHAINS] + [(n, "graded") for n in cc.GRADED]
            + [(n, "integer") for n in cc.INTEGER_CHAINS])
FAMILY_IDS = [f"{n}-{f}" for n, f in FAMILIES]
WITH_TAIL = [(n, f) for n, f in FAMILIES if cc.tail_start(ALL[n][0]) < len(ALL[n][0])]
NO_TAIL = [n for n in cc.CHAINS if len(cc.CHAINS[n][0]) > 1 and cc.tail_start(cc.CHAINS[n][0]) == len(cc.CHAINS[n][0])]

WORST = {}  # storage / entry -> largest observed error / bound (report only)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")
    yield
    for key in sorted(WORST):
        print(f"\n[decode-reference] largest error / bound, {key}: {WORST[key]:.3e}", end="")
    print()


# ------------------------------------------------------------------------------------------------ helpers
def _lib_():
    return _lib.load()


def _device_cores(cores, storage):
    """fp64 host cores (values exact in `storage`) -> contiguous device tensors of that type."""
    return [torch.from_numpy(np.ascontiguousarray(c)).to(DEV).to(TORCH_DT[storage]).contiguous() for c in cores]


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _nan(numel, dtype):
    return torch.full((int(numel),), NAN, dtype=dtype, device=DEV)


def _host(t):
    return t.to(torch.float64).cpu().numpy().reshape(-1)


def _ws(dims, bonds, storage):
    lib = _lib_()
    d, b = _lib.i64_array(dims), _lib.i64_array(bonds)
    fn = lib.ndmps_chain_workspace_bytes_f64 if storage == "f64" else lib.ndmps_chain_workspace_bytes
    return int(fn(len(dims), d, b))


def _chain(dims, bonds, dev_cores, storage, ws_bytes=None, out=None):
    """ndmps_chain_contract_<storage> into a NaN-filled buffer; returns (rc, out)."""
    lib = _lib_()
    fn = {"f32": lib.ndmps_chain_contract_f32, "bf16": lib.ndmps_chain_contract_bf16,
          "f64": lib.ndmps_chain_contract_f64}[storage]
    need = _ws(dims, bonds, storage)
    ws = torch.empty(max(need, ws_bytes or 0, 1), dtype=torch.uint8, device=DEV)  # never smaller than claimed
    if out is None:
        out = _nan(np.prod(dims, dtype=np.int64), TORCH_DT[storage])
    rc = fn(len(dims), _lib.i64_array(dims), _lib.i64_array(bonds), _ptrs(dev_cores), out.data_ptr(), ws.data_ptr(),
            need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


class _Tables:
    """A two-axis volume whose site dims are `dims` (oracle.chain_cases.factor_array), its permutation plan and the
    scatter tables the fused decode takes, columns sorted as DeviceMPS.to_volume passes them."""

    def __init__(self, dims, n_cols=None):
        self.fa = cc.factor_array(dims)
        self.shape = tuple(int(v) for v in np.prod(self.fa, axis=0))
        self.plan = _plan_for(self.shape, 0, factor_arr=self.fa)
        self.n_tail = int(_lib_().ndmps_chain_tail_columns(len(dims), _lib.i64_array(dims)))
        self.n_cols = self.n_tail if n_cols is None else n_cols
        if self.n_cols > 0:
            self.row_off, self.col_off, self.col_perm = self.plan.split_tables(self.n_cols, torch.device(DEV))
        self.dest = cb.flat_destination_factors(self.fa).reshape(-1)


def _scatter(dims, bonds, dev_cores, tab, n_cols=None, ws_bytes=None):
    lib = _lib_()
    need = _ws(dims, bonds, "f32")
    ws = torch.empty(max(need, ws_bytes or 0), dtype=torch.uint8, device=DEV)  # never smaller than claimed
    out = _nan(np.prod(dims, dtype=np.int64), F32)
    rc = lib.ndmps_chain_contract_scatter_f32(
        len(dims), _lib.i64_array(dims), _lib.i64_array(bonds), _ptrs(dev_cores), out.data_ptr(),
        tab.row_off.data_ptr(), tab.col_off.data_ptr(), tab.col_perm.data_ptr(),
        tab.n_cols if n_cols is None else n_cols, ws.data_ptr(), need if ws_bytes is None else ws_bytes,
        _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _permute(tab, dense):
    out = _nan(dense.numel(), dense.dtype)
    _lib.check(_lib_().ndmps_decode_permute(tab.plan.handle, dense.data_ptr(), out.data_ptr(), dense.element_size(),
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


def _within(got, ref, bound, key, label, exact=False):
    """|got - ref| <= bound at every element; no NaN (every element written); records error / bound under `key`."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    bound = np.asarray(bound, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (label, got.shape, ref.shape, bound.shape)
    unwritten = np.isnan(got)
    assert not unwritten.any(), f"{label}: {int(unwritten.sum())} elements never written, first {np.flatnonzero(unwritten)[:8]}"
    err = np.abs(got - ref)
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[decode-reference] {label}: error / bound = {ratio:.3e}")
    bad = err > bound
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} elements outside the bound, worst ratio {ratio:.3e}, "
                           f"first {np.flatnonzero(bad)[:8]}")
    if exact:
        assert np.array_equal(got, ref), f"{label}: integer chain not reproduced bit for bit"


def _exact(name, family, storage):
    return family == "integer" and (storage != "bf16" or int(np.prod(ALL[name][1])) <= 256)


# ------------------------------------------------------------------------------------------------ the chains
@pytest.mark.parametrize("storage", cc.STORAGES)
@pytest.mark.parametrize("name,family", FAMILIES, ids=FAMILY_IDS)
def test_chain_contract_against_fp64_contraction(name, family, storage):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, storage)
    rc, out = _chain(dims, bonds, _device_cores(cores, storage), storage)
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    _within(_host(out), mps_to_dense(cores), cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]), f"chain {storage}",
            f"chain_contract_{storage} {name}/{family}", exact=_exact(name, family, storage))


@pytest.mark.parametrize("name,family", WITH_TAIL, ids=[f"{n}-{f}" for n, f in WITH_TAIL])
def test_fused_scatter_against_reference_through_the_index_map(name, family):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, "f32")
    dev = _device_cores(cores, "f32")
    tab = _Tables(dims)
    assert tab.n_tail == int(np.prod(dims[cc.tail_start(dims):]))
    rc, vol = _scatter(dims, bonds, dev, tab)
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    ref = cb.to_volume(mps_to_dense(cores), tab.dest)
    bound = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["f32"]), tab.dest)
    _within(_host(vol), ref, bound, "fused scatter f32", f"chain_contract_scatter_f32 {name}/{family}",
            exact=family == "integer")
    rc, dense = _chain(dims, bonds, dev, "f32")
    assert rc == _lib.OK
    assert torch.equal(vol, _permute(tab, dense)), "fused decode differs from chain + ndmps_decode_permute"


@pytest.mark.parametrize("name", NO_TAIL)
def test_no_tail_fused_scatter_is_refused_and_writes_nothing(name):
    dims, bonds = cc.CHAINS[name]
    assert int(_lib_().ndmps_chain_tail_columns(len(dims), _lib.i64_array(dims))) == 0
    cores = cc.draw_cores(name, dims, bonds, "uniform", "f32")
    tab = _Tables(dims, n_cols=dims[-1])  # valid tables of this plan; the chain has no tail to use them
    rc, vol = _scatter(dims, bonds, _device_cores(cores, "f32"), tab)
    assert rc == _lib.EINVAL
    assert bool(torch.isnan(vol).all()), "a refused call wrote into its output"


# ------------------------------------------------------------------------------------------------ batched decode
def _batched(dims, bonds_list, dev_list, tab, ws_bytes=None, n_cols=None):
    lib = _lib_()
    batch, L = len(dev_list), len(dims)
    numel = int(np.prod(dims, dtype=np.int64))
    flat_bonds = _lib.i64_array([b for bonds in bonds_list for b in bonds])
    cores = (C.c_void_p * (batch * L))(*[c.data_ptr() for dev in dev_list for c in dev])
    out = torch.full((batch, numel), NAN, dtype=F32, device=DEV)
    outs = (C.c_void_p * batch)(*[out[b].data_ptr() for b in range(batch)])
    need = int(lib.ndmps_chain_batched_workspace_bytes(batch, L, _lib.i64_array(dims), flat_bonds))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, nbytes), dtype=torch.uint8, device=DEV)
    rc = lib.ndmps_chain_contract_scatter_batched_f32(
        batch, L, _lib.i64_array(dims), flat_bonds, cores, outs, tab.row_off.data_ptr(), tab.col_off.data_ptr(),
        tab.col_perm.data_ptr(), tab.n_cols if n_cols is None else n_cols, ws.data_ptr(), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, need


def _check_batch(tag, dims, bonds_list, ws_single=False):
    tab = _Tables(dims)
    host = [cc.draw_cores(tag, dims, bonds, "uniform", "f32", salt=b) for b, bonds in enumerate(bonds_list)]
    dev = [_device_cores(c, "f32") for c in host]
    ws_bytes = None
    if ws_single:
        ws_bytes = -(-_ws(dims, bonds_list[0], "f32") // 256) * 256
    rc, out, need = _batched(dims, bonds_list, dev, tab, ws_bytes=ws_bytes)
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    if ws_single:
        assert ws_bytes < need  # too small for the batched route: the volumes are contracted in turn
    for b, (cores, bonds) in enumerate(zip(host, bonds_list)):
        ref = cb.to_volume(mps_to_dense(cores), tab.dest)
        bound = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["f32"]), tab.dest)
        _within(_host(out[b]), ref, bound, "batched scatter f32", f"batched {tag} volume {b} of {len(host)}")
        rc1, single = _scatter(dims, bonds, dev[b], tab)
        assert rc1 == _lib.OK
        assert torch.equal(out[b], single), f"volume {b}: batched decode differs from the single-volume call"


@pytest.mark.parametrize("batch", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("name", ["L5_ragged", "L4_tail_last"])
def test_batched_decode_same_bonds(name, batch):
    dims, bonds = cc.CHAINS[name]
    _check_batch(f"batched/{name}", dims, [bonds] * batch)


def test_batched_decode_different_bonds_is_contracted_in_turn():
    dims = cc.CHAINS["L4_tail_last"][0]
    _check_batch("batched/mixed", dims, [[1, 3, 13, 13, 1], [1, 1, 1, 1, 1], [1, 3, 27, 64, 1], [1, 2, 5, 33, 1]])


def test_batched_decode_same_bonds_with_a_single_volume_workspace():
    dims, bonds = cc.CHAINS["L4_tail_last"]
    _check_batch("batched/small-ws", dims, [bonds] * 5, ws_single=True)


# ------------------------------------------------------------------------------------------------ indexed GEMM
_SIZES = (1, 5, 33, 130, 1000)


def _indexed_case(m, n, k, a_mode, c_mode, rng):
    """One ndmps_sgemm_indexed call; returns (got C (m, n) on the host, A, B fp64, label)."""
    lib = _lib_()
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    d_b = torch.from_numpy(b).to(DEV)
    if a_mode == "dense":
        d_a, lda, a_row, a_col, vec4 = torch.from_numpy(a).to(DEV), k, None, None, 0
    else:
        vec4 = 1 if a_mode == "vec4" else 0
        stride = -(-(k + 7) // 4) * 4                       # rows 16-byte aligned, with a gap behind each
        row_t = rng.permutation(m).astype(np.int64) * stride
        if vec4:                                            # aligned runs of four consecutive offsets, runs shuffled
            col_t = (rng.permutation(k // 4).astype(np.int64)[:, None] * 4 + np.arange(4)).reshape(-1)
        else:
            col_t = rng.permutation(k).astype(np.int64)
        buf = np.full(m * stride, np.float32(1e30))          # a read outside the tables would wreck the product
        buf[(row_t[:, None] + col_t[None, :]).reshape(-1)] = a.reshape(-1)
        d_a, lda = torch.from_numpy(buf).to(DEV), 0
        a_row, a_col = torch.from_numpy(row_t).to(DEV), torch.from_numpy(col_t).to(DEV)
    if c_mode == "dense":
        d_c, ldc, c_row, c_col = _nan(m * n, F32), n, None, None
        where = np.arange(m * n)
    else:
        col_t = np.cumsum(rng.integers(1, 3, n)).astype(np.int64) - 1   # ascending, with holes
        stride = int(col_t[-1]) + 1 + 3
        row_t = rng.permutation(m).astype(np.int64) * stride + 2
        d_c, ldc = _nan(m * stride + 8, F32), 0
        c_row, c_col = torch.from_numpy(row_t).to(DEV), torch.from_numpy(col_t).to(DEV)
        where = (row_t[:, None] + col_t[None, :]).reshape(-1)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.ndmps_sgemm_indexed(m, n, k, d_a.data_ptr(), lda, p(a_row), p(a_col), vec4, d_b.data_ptr(), n,
                                 d_c.data_ptr(), ldc, p(c_row), p(c_col), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    full = d_c.cpu().numpy()
    rest = np.ones(full.size, dtype=bool)
    rest[where] = False
    assert np.isnan(full[rest]).all(), f"m={m} n={n} k={k} {a_mode}/{c_mode}: wrote outside the scatter tables"
    return full[where].astype(np.float64), a.astype(np.float64), b.astype(np.float64)


@pytest.mark.parametrize("c_mode", ["dense", "scattered"])
@pytest.mark.parametrize("a_mode", ["dense", "gathered", "vec4"])
def test_sgemm_indexed_against_fp64_product(a_mode, c_mode):
    rng = np.random.default_rng(len(a_mode) * 131 + len(c_mode))
    ks = (4, 132, 1000) if a_mode == "vec4" else _SIZES + (4, 132)
    ns = _SIZES + (4, 132)
    for m in _SIZES:
        for n in ns:
            for k in ks:
                got, a, b = _indexed_case(m, n, k, a_mode, c_mode, rng)
                _within(got, a @ b, cb.gemm_bound(a, b, cb.U_F32), f"sgemm_indexed A {a_mode} / C {c_mode}",
                        f"sgemm_indexed m={m} n={n} k={k} A {a_mode} C {c_mode}")


# ------------------------------------------------------------------------------------------------ overlap
def _overlap(dims, bonds_a, cores_a, bonds_b, cores_b, storage, ws_bytes=None):
    lib = _lib_()
    L = len(dims)
    d, ba, bb = _lib.i64_array(dims), _lib.i64_array(bonds_a), _lib.i64_array(bonds_b)
    need = int(lib.ndmps_overlap_workspace_bytes(L, d, ba, bb))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    da, db = _device_cores(cores_a, storage), _device_cores(cores_b, storage)
    out = C.c_double(NAN)
    fn = lib.ndmps_overlap_f64 if storage == "f64" else lib.ndmps_overlap_f32
    rc = fn(L, d, ba, _ptrs(da), bb, _ptrs(db), C.byref(out), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
            _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.value


OVERLAP_PAIRS = {
    "one_site": ([37], [1, 1], [1, 1]),
    "bond1_vs_129": ([16, 16, 16, 16], [1, 16, 129, 16, 1], [1, 1, 1, 1, 1]),
    "ragged_vs_other": ([7, 5, 11, 3, 8], [1, 7, 33, 13, 8, 1], [1, 1, 5, 24, 3, 1]),
    "nonmonotone_vs_max": ([41, 3, 7, 32, 6], [1, 40, 5, 64, 2, 1], [1, 41, 123, 192, 6, 1]),
    "seven_sites": ([2, 3, 2, 3, 2, 65, 64], [1, 2, 5, 5, 7, 13, 33, 1], [1, 1, 3, 7, 13, 65, 64, 1]),
}


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("pair", list(OVERLAP_PAIRS))
def test_overlap_of_two_different_bond_profiles(pair, storage):
    dims, ba, bb = OVERLAP_PAIRS[pair]
    cc.check_chain(dims, ba)
    cc.check_chain(dims, bb)
    a = cc.draw_cores(pair, dims, ba, "uniform", storage, salt=0)
    b = cc.draw_cores(pair, dims, bb, "uniform", storage, salt=1)
    rc, got = _overlap(dims, ba, a, bb, b, storage)
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    _within([got], [mps_overlap(a, b)], [cb.overlap_bound(a, b)], f"overlap {storage}", f"overlap_{storage} {pair}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_overlap_that_cancels_to_nearly_zero(storage):
    """<a | b - t a> with t = <a|b> / <a|a>: the direct-sum chain's overlap with a is zero up to the rounding of
    t a_0 to the storage type, while the sum of magnitudes is of order <|a| | |b|>; the bar is the bound, not a
    relative error (which would be of order one here)."""
    dims, ba, bb = OVERLAP_PAIRS["ragged_vs_other"]
    a = cc.draw_cores("cancel", dims, ba, "uniform", storage, salt=0)
    b = cc.draw_cores("cancel", dims, bb, "uniform", storage, salt=1)
    t = mps_overlap(a, b) / mps_overlap(a, a)
    L = len(dims)
    diff = []
    for i in range(L):
        x, y = b[i], (-t * a[i] if i == 0 else a[i])
        if i == 0:
            core = np.concatenate([x, y], axis=2)
        elif i == L - 1:
            core = np.concatenate([x, y], axis=0)
        else:
            core = np.zeros((x.shape[0] + y.shape[0], dims[i], x.shape[2] + y.shape[2]))
            core[:x.shape[0], :, :x.shape[2]] = x
            core[x.shape[0]:, :, x.shape[2]:] = y
        diff.append(cc.to_storage(core, storage))
    bd = [1] + [c.shape[2] for c in diff]
    ref = mps_overlap(a, diff)
    scale = cb.abs_overlap(a, diff)
    assert abs(ref) < 1e-5 * scale  # the case is what it claims to be
    rc, got = _overlap(dims, ba, a, bd, diff, storage)
    assert rc == _lib.OK, _lib_().ndmps_last_error()
    _within([got], [ref], [cb.overlap_bound(a, diff)], f"overlap {storage}", f"overlap_{storage} cancelling pair")


# ------------------------------------------------------------------------------------------------ argument checks
def _zeros_cores(dims, bonds, storage):
    return [torch.zeros((bonds[i], dims[i], bonds[i + 1]), dtype=TORCH_DT[storage], device=DEV) for i in range(len(dims))]


@pytest.mark.parametrize("storage", cc.STORAGES)
def test_refused_chain_arguments_launch_nothing(storage):
    lib = _lib_()
    dims, bonds = cc.CHAINS["L4_tail_last"]
    dev = _device_cores(cc.draw_cores("args", dims, bonds, "uniform", storage), storage)
    need = _ws(dims, bonds, storage)
    rc, out = _chain(dims, bonds, dev, storage, ws_bytes=need - 1)
    assert rc == _lib.EWORKSPACE and bool(torch.isnan(out).all())
    # a bond above min(left, right): bond 1 = 4 > dims[0] = 3, bond 3 = 65 > dims[3] = 64
    for bad in ([1, 4, 13, 13, 1], [1, 3, 13, 65, 1]):
        rc, out = _chain(dims, bad, _zeros_cores(dims, bad, storage), storage, ws_bytes=1 << 24)
        assert rc == _lib.EINVAL and bool(torch.isnan(out).all()), bad
        assert b"exceeds" in lib.ndmps_last_error()
    for bad in ([2, 3, 13, 13, 1], [1, 3, 13, 13, 2]):
        rc, out = _chain(dims, bad, _zeros_cores(dims, bad, storage), storage, ws_bytes=1 << 24)
        assert rc == _lib.EINVAL and bool(torch.isnan(out).all()), bad


def test_refused_scatter_arguments_launch_nothing():
    dims, bonds = cc.CHAINS["L4_tail_last"]  # its first cumulative product is written into the output buffer
    dev = _device_cores(cc.draw_cores("args", dims, bonds, "uniform", "f32"), "f32")
    good = _Tables(dims)
    other = _Tables(dims, n_cols=dims[-1] * dims[-2])  # tables of the same plan for another split of the sites
    assert other.n_cols != good.n_tail
    rc, out = _scatter(dims, bonds, dev, other)
    assert rc == _lib.EINVAL and bool(torch.isnan(out).all()), "tables for another n_cols"
    rc, out = _scatter(dims, bonds, dev, good, ws_bytes=_ws(dims, bonds, "f32") - 1)
    assert rc == _lib.EWORKSPACE and bool(torch.isnan(out).all())
    for bad in ([1, 4, 13, 13, 1], [2, 3, 13, 13, 1]):
        rc, out = _scatter(dims, bad, _zeros_cores(dims, bad, "f32"), good, ws_bytes=1 << 24)
        assert rc == _lib.EINVAL and bool(torch.isnan(out).all()), bad
    # the batched entry, same-bonds route
    rc, out, _ = _batched(dims, [bonds] * 3, [dev] * 3, other)
    assert rc == _lib.EINVAL and bool(torch.isnan(out).all()), "batched: tables for another n_cols"
    rc, out, _ = _batched(dims, [[1, 4, 13, 13, 1]] * 3, [_zeros_cores(dims, [1, 4, 13, 13, 1], "f32")] * 3, good)
    assert rc == _lib.EINVAL and bool(torch.isnan(out).all())


def test_refused_overlap_workspace():
    dims, ba, bb = OVERLAP_PAIRS["ragged_vs_other"]
    a = cc.draw_cores("args", dims, ba, "uniform", "f32")
    b = cc.draw_cores("args", dims, bb, "uniform", "f32", salt=1)
    need = int(_lib_().ndmps_overlap_workspace_bytes(len(dims), _lib.i64_array(dims), _lib.i64_array(ba), _lib.i64_array(bb)))
    rc, got = _overlap(dims, ba, a, bb, b, "f32", ws_bytes=need - 1)
    assert rc == _lib.EWORKSPACE and np.isnan(got)


# ------------------------------------------------------------------------------------------------ through the class
SHAPES = [(30, 45, 20), (512, 680), (16, 16, 8, 32)]
SHAPE_IDS = ["30x45x20", "512x680", "16x16x8x32"]


def _region_keys(shape):
    """The key list of tests/test_gpu_region.py."""
    rng = np.random.default_rng(len(shape))
    D = len(shape)
    arr = [[int(v) for v in rng.integers(0, n, 7)] + [0, 0] for n in shape]
    return [
        (),
        (Ellipsis,),
        (slice(5, min(37, shape[0])),),
        (slice(None, None, 3),) * D,
        (slice(None, None, -2),) + (1,) * (D - 1),
        tuple(arr),
        tuple(-1 - i for i in range(D)),
        (Ellipsis, np.array(arr[-1])),
        (arr[0], Ellipsis, -3),
        (3, slice(2, None, 5)) + (slice(None, 4),) * (D - 2),
    ]


def _ix(a, key, shape):
    """a[np.ix_(per-axis indices)] with int axes dropped: the outer-indexing meaning of `key`."""
    key = key if isinstance(key, tuple) else (key,)
    if any(k is Ellipsis for k in key):
        i = next(j for j, k in enumerate(key) if k is Ellipsis)
        key = key[:i] + (slice(None),) * (len(shape) - len(key) + 1) + key[i + 1:]
    key = key + (slice(None),) * (len(shape) - len(key))
    idx, out_shape = [], []
    for k, n in zip(key, shape):
        if isinstance(k, (int, np.integer)):
            idx.append(np.array([k % n]))
        elif isinstance(k, slice):
            idx.append(np.arange(*k.indices(n)))
            out_shape.append(idx[-1].size)
        else:
            idx.append(np.asarray(k) % n)
            out_shape.append(idx[-1].size)
    return a[np.ix_(*idx)].reshape(out_shape)


def _block_reduce(vol, blocks, op):
    inter = [v for n, b in zip(vol.shape, blocks) for v in (n // b, b)]
    r = np.asarray(vol, dtype=np.float64).reshape(inter)
    odd = tuple(range(1, 2 * vol.ndim, 2))
    return r.mean(axis=odd) if op == "mean" else r.sum(axis=odd)


def _stored_cores(obj):
    """The object's cores as stored, widened exactly to fp64 on the host."""
    return [c.to(torch.float64).cpu().numpy() for c in obj.mps.cores]


def _randomise(obj, tag):
    """replace_tensordata with random cores of the same shapes (uniform / sqrt(d chi)): not isometric, not smooth."""
    storage = NAME_OF[obj.mps.dtype]
    dims, bonds = obj.mps.dims, obj.mps.bonds
    cores = cc.draw_cores(tag, dims, bonds, "uniform", storage)
    arrays = obj.mps.arrays
    obj.replace_tensordata([c.reshape(tuple(arrays[i].shape)) for i, c in enumerate(cores)])
    for got, want in zip(_stored_cores(obj), cores):
        assert np.array_equal(got, want)
    return obj


def _random_object(shape, storage, sweep_from, seed):
    x = synthetic_mri(shape, seed=seed)
    obj = NDMPS.from_tensor(x, max_bond=12, device=DEV, dtype=F64 if storage == F64 else None, sweep_from=sweep_from)
    obj = _randomise(obj, f"class/{shape}/{sweep_from}/{seed}")
    return obj.astype(BF16) if storage == BF16 else obj


def _lincomb_object(shape, storage, sweep_from):
    dt = F64 if storage == F64 else None
    parts = [NDMPS.from_tensor(synthetic_mri(shape, seed=40 + j), max_bond=mb, device=DEV, dtype=dt, sweep_from=sweep_from)
             for j, mb in enumerate((5, 6, 7))]
    return NDMPS.linear_combination(parts, [0.7, -1.3, 0.45], cutoff=0.0, dtype=BF16 if storage == BF16 else None)


def _check_derived(obj, shape, label):
    storage = NAME_OF[obj.mps.dtype]
    cores = _stored_cores(obj)
    dest = im.flat_destination(shape).reshape(-1)
    ref = cb.to_volume(mps_to_dense(cores), dest).reshape(shape)
    chain_b = cb.to_volume(cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF[storage]), dest).reshape(shape)
    # region and pool widen bf16 cores to fp32 and contract in fp32: u_store is 2**-24 for them, not 2**-8
    wide = cb.CHAIN_ROUNDOFF["f64" if storage == "f64" else "f32"]
    wide_b = cb.to_volume(cb.chain_bound(cores, *wide), dest).reshape(shape)
    _within(obj.to_tensor(), ref, chain_b, f"to_tensor {storage}", f"{label} to_tensor")
    for key in _region_keys(shape):
        want = _ix(ref, key, shape)
        got = obj.decode_region(key)
        assert np.shape(got) == want.shape, (key, np.shape(got), want.shape)
        _within(got, want, _ix(wide_b, key, shape), f"decode_region {storage}", f"{label} decode_region {key!r:.40}")
    rng = np.random.default_rng(5)
    coords = np.stack([rng.integers(-n, n, 500) for n in shape], axis=1)
    _within(obj.values_at(coords), ref[tuple(coords.T)], wide_b[tuple(coords.T)], f"values_at {storage}",
            f"{label} values_at")
    blocks = obj.block_shape(1)
    for op in ("mean", "sum"):
        _within(obj.downsample(1, op=op), _block_reduce(ref, blocks, op), _block_reduce(wide_b, blocks, op),
                f"downsample {storage}", f"{label} downsample(1, {op})")
    nd = len(shape)
    for axis in (None, 0, -1, (0, nd - 1)):
        _within(obj.sum(axis=axis), ref.sum(axis=axis), wide_b.sum(axis=axis), f"sum/mean {storage}",
                f"{label} sum(axis={axis})")
        _within(obj.mean(axis=axis), ref.mean(axis=axis), wide_b.mean(axis=axis), f"sum/mean {storage}",
                f"{label} mean(axis={axis})")
    return cores, ref, chain_b


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("sweep_from", ["right", "left"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_derived_decoders_on_random_cores(shape, sweep_from, storage):
    a = _random_object(shape, storage, sweep_from, seed=17)
    cores_a, ref_a, bound_a = _check_derived(a, shape, f"random {shape} {sweep_from} {NAME_OF[storage]}")
    b = _random_object(shape, storage, sweep_from, seed=18)
    cores_b = _stored_cores(b)
    _within([a.mps @ b.mps], [mps_overlap(cores_a, cores_b)], [cb.overlap_bound(cores_a, cores_b)],
            f"mps @ mps {NAME_OF[storage]}", f"random {shape} a.mps @ b.mps")
    # the grouped decode: three objects over the same sites, each against its own reference
    c = _random_object(shape, storage, sweep_from, seed=19)
    dest = im.flat_destination(shape).reshape(-1)
    recs = NDMPS.to_tensors([a, b, c])
    for obj, rec in zip((a, b, c), recs):
        cs = _stored_cores(obj)
        _within(rec, cb.to_volume(mps_to_dense(cs), dest),
                cb.to_volume(cb.chain_bound(cs, *cb.CHAIN_ROUNDOFF[NAME_OF[storage]]), dest),
                f"to_tensors {NAME_OF[storage]}", f"random {shape} to_tensors")


@pytest.mark.parametrize("storage", [F32, F64, BF16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("sweep_from", ["right", "left"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_derived_decoders_on_a_linear_combination(shape, sweep_from, storage):
    obj = _lincomb_object(shape, storage, sweep_from)
    assert obj.mps.dtype == storage
    cores, _, _ = _check_derived(obj, shape, f"lincomb {shape} {sweep_from} {NAME_OF[storage]}")
    _within([obj.mps @ obj.mps], [mps_overlap(cores, cores)], [cb.overlap_bound(cores, cores)],
            f"mps @ mps {NAME_OF[storage]}", f"lincomb {shape} mps @ mps")
