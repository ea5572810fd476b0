"""Oracle (test infrastructure): the chains the decoders are tested on, and how their cores are drawn.

The (dims, bonds) below are chosen from the branches of the chain contraction (``chain_plan`` in csrc/chain_plan.h,
run by csrc/chain.hip), not from what a sweep produces.  The tail of a chain is the longest run of trailing sites, never
site 0, whose dims multiply to at most TAIL_MAX = 4096; it is contracted right to left first, the sites before it
are contracted cumulatively left to right, and one last product joins the two.  Every bond obeys
``chi_i <= min(prod(dims[:i]), prod(dims[i:]))``, which the library requires (its intermediates live in N elements).

Used by tests/test_decode_bound_host.py (CPU: the bound is sound and has teeth on exactly these cases) and
tests/test_gpu_decode_reference.py (the kernels against the fp64 contraction on the same cases).
"""
from __future__ import annotations

import zlib

import numpy as np

TAIL_MAX = 4096

# name -> (dims, bonds); comments: first tail site j0, number of cumulative left products
CHAINS = {
    # L = 1 (a copy) and L = 2 (one product, no intermediate)
    "L1": ([37], [1, 1]),
    "L2_maxbond": ([33, 65], [1, 33, 1]),                                   # j0 = 1, 0 left
    # the tail is the whole chain but site 0 (j0 = 1): only tail products and the final one
    "L3_tail_all": ([7, 5, 11], [1, 7, 11, 1]),
    "L4_tail_4096": ([16, 16, 16, 16], [1, 16, 129, 16, 1]),               # tail product exactly 4096
    "L5_ragged": ([7, 5, 11, 3, 8], [1, 7, 33, 13, 8, 1]),
    "L6_tail_all": ([4, 6, 4, 6, 4, 6], [1, 3, 7, 13, 5, 2, 1]),
    "L7_tail_all": ([3, 2, 3, 2, 3, 2, 3], [1, 3, 6, 7, 7, 6, 3, 1]),
    "L5_nonmonotone": ([41, 3, 7, 32, 6], [1, 40, 5, 64, 2, 1]),
    "L5_primes_maxbond": ([3, 5, 7, 11, 2], [1, 3, 15, 22, 2, 1]),          # min(left, right) at every bond
    "L5_unit_dims": ([5, 1, 7, 1, 9], [1, 5, 5, 9, 9, 1]),
    "L6_bonds_one": ([4, 6, 4, 6, 4, 6], [1, 1, 1, 1, 1, 1, 1]),
    # the tail is the last site only (64 * 65 and 41 * 100 cross 4096): j0 = L - 1, L - 2 left products
    "L3_tail_last": ([6, 100, 41], [1, 5, 33, 1]),                          # 1 left product
    "L4_tail_last": ([3, 9, 65, 64], [1, 3, 13, 13, 1]),                    # 2
    "L5_tail_last": ([4, 3, 5, 65, 64], [1, 4, 7, 7, 33, 1]),               # 3
    "L6_tail_last": ([2, 3, 2, 3, 65, 64], [1, 2, 3, 3, 9, 63, 1]),         # 4
    "L7_tail_last": ([2, 3, 2, 3, 2, 65, 64], [1, 2, 5, 5, 7, 13, 33, 1]),  # 5
    # a tail of three sites behind one or two cumulative products, odd bonds up to 129
    "L5_mid_tail_129": ([16, 16, 16, 16, 16], [1, 13, 127, 129, 7, 1]),     # j0 = 2, 1 left, 2**20 voxels
    "L5_mid_tail_65": ([9, 10, 11, 12, 13], [1, 3, 65, 33, 13, 1]),         # j0 = 2, 1 left
    # no tail (last dim 8192 > 4096): every product cumulative, the last one lands in the output
    "L2_no_tail": ([4, 8192], [1, 4, 1]),                                   # 1 product
    "L3_no_tail": ([5, 3, 8192], [1, 5, 15, 1]),                            # 2
    "L4_no_tail": ([3, 2, 2, 8192], [1, 3, 5, 7, 1]),                       # 3
    # about 2**24 voxels
    "L4_large": ([60, 66, 64, 65], [1, 33, 127, 65, 1]),                    # j0 = 3, 2 left
}

# integer cores (entries in {-1, 0, 1}): every partial product is an integer of magnitude at most prod(bonds)
INTEGER_CHAINS = {
    "int_tail_all": ([5, 7, 3, 6, 4], [1, 2, 4, 4, 2, 1]),                  # prod(bonds) = 64: exact in bf16 too
    "int_tail_last": ([6, 100, 41], [1, 3, 5, 1]),                          # 15
    "int_no_tail": ([3, 2, 2, 8192], [1, 2, 3, 2, 1]),                      # 12
    "int_wide": ([8, 16, 9, 10], [1, 8, 16, 10, 1]),                        # 1280: exact in fp32 / fp64 only
}

# the graded family is drawn on these chains (one per route through the chain's plan)
GRADED = ["L2_maxbond", "L5_ragged", "L5_tail_last", "L5_mid_tail_65", "L3_no_tail"]

STORAGES = ("f32", "bf16", "f64")


def tail_start(dims):
    """First site of the pre-contracted tail (== len(dims): no tail)."""
    L, j0, right = len(dims), len(dims), 1
    for i in range(L - 1, 0, -1):
        if right * dims[i] > TAIL_MAX:
            break
        right *= dims[i]
        j0 = i
    return j0


def check_chain(dims, bonds):
    """The library's own precondition on a chain; raises AssertionError for a case that breaks it."""
    L = len(dims)
    assert len(bonds) == L + 1 and bonds[0] == 1 and bonds[L] == 1
    numel = int(np.prod(dims, dtype=np.int64))
    left = 1
    for i in range(L):
        left *= dims[i]
        assert 1 <= bonds[i + 1] <= min(left, numel // left), (dims, bonds, i + 1)


def round_bf16(x):
    """Round float32 values to the nearest bf16 (ties to even), returned as float32."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    bits = (bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return bits.view(np.float32)


def to_storage(x, storage):
    """fp64 array holding exactly the values ``x`` has once stored as ``storage``."""
    if storage == "f64":
        return np.asarray(x, dtype=np.float64)
    x32 = np.asarray(x, dtype=np.float32)
    return (round_bf16(x32) if storage == "bf16" else x32).astype(np.float64)


def _seed(name, family, storage, salt):
    return zlib.crc32(f"{name}/{family}/{storage}/{salt}".encode())


def draw_cores(name, dims, bonds, family, storage, salt=0):
    """fp64 cores ``(chi_i, d_i, chi_{i+1})`` whose values are exactly representable in ``storage``.

    uniform : U[-1, 1] / sqrt(d_i chi_i)  (nothing under- or overflows, the voxels are O(1 / sqrt(N)))
    graded  : uniform, then the first and the last core multiplied along their physical index by the pattern
              1e-3, 1, 1e3, 1e-3, ...: voxels differ by up to 1e12 in magnitude and a norm sees only the largest
    integer : entries in {-1, 0, 1}
    """
    rng = np.random.default_rng(_seed(name, family, storage, salt))
    L = len(dims)
    cores = []
    for i in range(L):
        shape = (bonds[i], dims[i], bonds[i + 1])
        if family == "integer":
            cores.append(rng.integers(-1, 2, size=shape).astype(np.float64))
            continue
        c = rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(dims[i] * bonds[i])
        if family == "graded" and i in (0, L - 1):
            c = c * (10.0 ** (3 * (np.arange(dims[i]) % 3 - 1)))[None, :, None]
        elif family not in ("uniform", "graded"):
            raise ValueError(family)
        cores.append(to_storage(c, storage))
    return cores


def factor_array(dims):
    """An (L, 2) factor array with row products ``dims``: a two-axis volume whose site dims these are.  Site i is
    split as (a, d_i / a), a the largest divisor of d_i up to sqrt(d_i), the two swapped on odd sites, so that both
    axes get digits from every composite site and the decode permutation is not the identity."""
    rows = []
    for i, d in enumerate(dims):
        a = max(f for f in range(1, int(np.sqrt(d)) + 1) if d % f == 0)
        rows.append((a, d // a) if i % 2 == 0 else (d // a, a))
    return np.array(rows, dtype=np.int64)
