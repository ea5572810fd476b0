"""The decoders' error bar (oracle/chain_bound.py) checked on the CPU, before any kernel is held to it.

* sound: a NumPy float32 restatement of the chain contraction in the library's stage order (tail right to left,
  then left to right, then the product that joins them; csrc/chain_plan.h) stays within ``chain_bound`` of
  the fp64 contraction on every case of oracle/chain_cases.py, and so does the same chain with its intermediates
  rounded to bf16 against the bf16 bound;
* teeth: three deliberate mistakes in that chain -- the last term of the inner sum of the final product dropped,
  two adjacent output columns of the final product swapped, one core read with its two (equal) bond axes
  transposed -- each put at least one element outside the bound, in every case they apply to;
* the integer cases satisfy the precondition under which their results must be exact.

No tolerance here or in tests/test_gpu_decode_reference.py comes from a kernel's output.
"""
import numpy as np
import pytest

from oracle import chain_bound as cb
from oracle import chain_cases as cc
from oracle import index_map as im
from oracle.mps import mps_overlap, mps_to_dense

ALL = dict(cc.CHAINS, **cc.INTEGER_CHAINS)
FAMILIES = ([(n, "uniform") for n in cc.CHAINS] + [(n, "graded") for n in cc.GRADED]
            + [(n, "integer") for n in cc.INTEGER_CHAINS])
FAMILY_IDS = [f"{n}-{f}" for n, f in FAMILIES]


def _bf16(x):
    torch = pytest.importorskip("torch")
    return torch.tensor(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def staged_chain(cores, dims, bonds, store=None, mutate=None):
    """The chain in float32, staged as chain_plan stages it.  ``store``: rounding applied to every product
    (bf16 intermediates).  ``mutate`` in {None, "drop", "swap"}: a mistake made in the final product."""
    store = store or (lambda x: x)
    c32 = [np.asarray(c, dtype=np.float32) for c in cores]
    L = len(dims)
    if L == 1:
        return c32[0].reshape(-1)
    j0 = cc.tail_start(dims)

    def product(a, b, final):
        assert a.dtype == np.float32 and b.dtype == np.float32
        if final and mutate == "drop":
            out = a[:, :-1] @ b[:-1]      # the last term of every inner sum is missing
        else:
            out = a @ b
        if final and mutate == "swap":
            out[:, [0, 1]] = out[:, [1, 0]]
        return store(out)

    R, n_tail = None, 1
    if j0 < L:
        R, n_tail = c32[L - 1].reshape(bonds[L - 1], dims[L - 1]), dims[L - 1]
        for i in range(L - 2, j0 - 1, -1):
            R = product(c32[i].reshape(bonds[i] * dims[i], bonds[i + 1]), R, False).reshape(bonds[i], dims[i] * n_tail)
            n_tail *= dims[i]
    last_left = j0 - 1 if j0 < L else L - 1
    left, rows = c32[0].reshape(dims[0], bonds[1]), dims[0]
    for i in range(1, last_left + 1):
        final = j0 == L and i == last_left
        left = product(left, c32[i].reshape(bonds[i], dims[i] * bonds[i + 1]), final)
        rows *= dims[i]
        left = left.reshape(rows, -1)
    out = product(left, R, True) if j0 < L else left
    return out.reshape(-1)


def _outside(got, ref, bound):
    return int(np.count_nonzero(np.abs(got.astype(np.float64).reshape(-1) - ref.reshape(-1)) > bound.reshape(-1)))


def test_every_case_obeys_the_library_precondition_and_takes_the_branch_it_is_listed_for():
    for name, (dims, bonds) in ALL.items():
        cc.check_chain(dims, bonds)
    left_products = {}
    for name, (dims, bonds) in cc.CHAINS.items():
        L, j0 = len(dims), cc.tail_start(dims)
        left_products[name] = (j0, (j0 - 1) if j0 < L else L - 1)
    assert all(left_products[n] == (1, 0) for n in cc.CHAINS if "tail_all" in n or n == "L2_maxbond")
    assert [left_products[f"L{L}_tail_last"] for L in (3, 4, 5, 6, 7)] == [(L - 1, L - 2) for L in (3, 4, 5, 6, 7)]
    assert [left_products[f"L{L}_no_tail"] for L in (2, 3, 4)] == [(L, L - 1) for L in (2, 3, 4)]
    assert left_products["L5_mid_tail_129"] == (2, 1) and left_products["L5_mid_tail_65"] == (2, 1)
    assert left_products["L4_large"] == (3, 2)
    assert int(np.prod(cc.CHAINS["L4_tail_4096"][0][1:])) == cc.TAIL_MAX
    sizes = {n: int(np.prod(d, dtype=np.int64)) for n, (d, _) in ALL.items()}
    assert 2 ** 23 < sizes.pop("L4_large") <= 2 ** 24 and max(sizes.values()) <= 2 ** 20


def test_round_bf16_is_torch_round_to_nearest_even():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-6, 6, 4096),
                        np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0, -0.0, 256.0, 257.0], dtype=np.float32)])
    assert np.array_equal(cc.round_bf16(x), _bf16(x))


@pytest.mark.parametrize("shape", [(30, 45, 20), (512, 680), (16, 16, 8, 32), (6, 35)])
def test_explicit_factor_map_equals_the_reference_map(shape):
    fa, _ = im.get_factorlist(shape)
    assert np.array_equal(cb.flat_destination_factors(fa), im.flat_destination(shape))


def test_factor_array_is_a_permutation_with_the_chain_dims():
    for name, (dims, _) in ALL.items():
        fa = cc.factor_array(dims)
        assert list(np.prod(fa, axis=1)) == list(dims)
        dest = cb.flat_destination_factors(fa).reshape(-1)
        assert np.array_equal(np.sort(dest), np.arange(dest.size)), name
    dest = cb.flat_destination_factors(cc.factor_array(cc.CHAINS["L5_ragged"][0])).reshape(-1)
    assert not np.array_equal(dest, np.arange(dest.size))  # a real permutation, not the identity


@pytest.mark.parametrize("name,family", FAMILIES, ids=FAMILY_IDS)
def test_float32_chain_is_within_the_bound(name, family):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, "f32")
    ref = mps_to_dense(cores)
    bound = cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["f32"])
    got = staged_chain(cores, dims, bonds)
    err = np.abs(got.astype(np.float64) - ref.reshape(-1))
    assert _outside(got, ref, bound) == 0, float(np.max(err / np.maximum(bound.reshape(-1), 1e-300)))
    if family == "integer":
        assert np.array_equal(got.astype(np.float64), ref.reshape(-1))


@pytest.mark.parametrize("name,family", FAMILIES, ids=FAMILY_IDS)
def test_bf16_intermediates_are_within_the_bf16_bound(name, family):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, "bf16")
    for c in cores:
        assert np.array_equal(_bf16(c), c.astype(np.float32))  # the reference sees the stored values
    ref = mps_to_dense(cores)
    bound = cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["bf16"])
    got = staged_chain(cores, dims, bonds, store=_bf16)
    assert _outside(got, ref, bound) == 0


def _transposable(bonds):
    return [i for i in range(len(bonds) - 1) if bonds[i] == bonds[i + 1] and bonds[i] > 1]


MUTATION_CASES = [(n, f) for n, f in FAMILIES if len(ALL[n][0]) > 1]  # L = 1 is a copy: no product to get wrong


@pytest.mark.parametrize("mutate", ["drop", "swap"])
@pytest.mark.parametrize("name,family", MUTATION_CASES, ids=[f"{n}-{f}" for n, f in MUTATION_CASES])
def test_a_wrong_final_product_leaves_the_bound(name, family, mutate):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, "f32")
    ref = mps_to_dense(cores)
    bound = cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["f32"])
    assert _outside(staged_chain(cores, dims, bonds, mutate=mutate), ref, bound) >= 1


TRANSPOSE_CASES = [(n, f) for n, f in MUTATION_CASES if _transposable(ALL[n][1])]


def test_enough_cases_have_a_core_with_equal_bonds():
    assert len({n for n, _ in TRANSPOSE_CASES}) >= 6


@pytest.mark.parametrize("name,family", TRANSPOSE_CASES, ids=[f"{n}-{f}" for n, f in TRANSPOSE_CASES])
def test_a_core_read_transposed_leaves_the_bound(name, family):
    dims, bonds = ALL[name]
    cores = cc.draw_cores(name, dims, bonds, family, "f32")
    ref = mps_to_dense(cores)
    bound = cb.chain_bound(cores, *cb.CHAIN_ROUNDOFF["f32"])
    for i in _transposable(bonds):
        wrong = list(cores)
        wrong[i] = np.ascontiguousarray(cores[i].transpose(2, 1, 0))
        assert _outside(staged_chain(wrong, dims, bonds), ref, bound) >= 1, i


@pytest.mark.parametrize("name", list(cc.INTEGER_CHAINS))
def test_integer_cases_are_exactly_representable(name):
    """Every partial product of a {-1, 0, 1} chain is an integer of magnitude at most the product of the bonds
    summed over, so below 2**24 (fp32), 2**53 (fp64) or up to 256 (bf16) no rounding occurs in any association."""
    dims, bonds = cc.INTEGER_CHAINS[name]
    for storage, limit in (("f32", 2 ** 24), ("f64", 2 ** 53), ("bf16", 256)):
        cores = cc.draw_cores(name, dims, bonds, "integer", storage)
        assert all(np.isin(c, (-1.0, 0.0, 1.0)).all() for c in cores)
        m = cb.abs_dense(cores)
        if storage == "bf16":
            if int(np.prod(bonds)) > 256:
                assert name == "int_wide"  # held to the bound only, not bit for bit
                continue
            assert m.max() <= 256
        else:
            assert m.max() < limit and int(np.prod(bonds)) < limit


def test_overlap_bound_is_far_below_a_dropped_site_term():
    dims = [7, 5, 11, 3, 8]
    a = cc.draw_cores("ov", dims, [1, 7, 33, 13, 8, 1], "uniform", "f32")
    b = cc.draw_cores("ov", dims, [1, 1, 5, 24, 3, 1], "uniform", "f32", salt=1)
    ref = mps_overlap(a, b)
    dense = float(np.sum(mps_to_dense(a) * mps_to_dense(b)))  # another order of summation, fp64
    assert abs(dense - ref) <= cb.overlap_bound(a, b) + cb.U_F64 * 9240 * cb.abs_overlap(a, b)
    wrong = [c.copy() for c in b]
    wrong[2][:, -1, :] = 0.0  # the last physical index of one site never enters the sum
    assert abs(mps_overlap(a, wrong) - ref) > 1000 * cb.overlap_bound(a, b)


def test_bound_is_zero_for_one_site_and_where_every_term_vanishes():
    c = cc.draw_cores("L1", [37], [1, 1], "uniform", "f32")
    assert np.all(cb.chain_bound(c, cb.U_F32, cb.U_F32) == 0.0)
    cores = cc.draw_cores("int_tail_all", *cc.INTEGER_CHAINS["int_tail_all"], "integer", "f32")
    cores[0][:, 2, :] = 0.0
    bound = cb.chain_bound(cores, cb.U_F32, cb.U_F32)
    assert np.all(bound[2] == 0.0) and np.all(mps_to_dense(cores)[2] == 0.0) and bound.max() > 0.0
