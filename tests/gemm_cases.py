"""The shapes every dense product (csrc/gemm.hip, csrc/gemm_bf16.hip) is tested on, shared by
tests/test_gemm_cases_host.py (CPU: every case reaches the tile and the fetch path it was chosen for, and the two
assertions have teeth on exactly these cases) and tests/test_gpu_gemm_cases.py (the kernels, through those
assertions).  NumPy only.

Two kinds of data, two assertions:

* ``integer``: operands are integers of magnitude at most ``imax_of(case)``: the largest value with
  ``k imax**2 < 2**24`` (fp32 accumulation: fp32 and bf16 operands; at most 2047, and 255 for bf16 so that the
  operands are exact in 8 significant bits), ``2**19`` for fp64 with ``k <= 2**13`` (``k imax**2 <= 2**51``).  Every
  partial sum of every entry is then an integer the accumulator holds exactly, in any order of summation, and
  ``check_integer`` asks for ``C == op(A) op(B)`` entry for entry; for bf16, for the exact integer rounded once to
  bf16, bit for bit.  A and B are drawn independently, so neither is symmetric and no two of the four transpose
  combinations give the same product.
* ``graded``: Gaussian operands, row ``i`` of op(A) scaled by ``10 ** (-3 i / m)`` and column ``j`` of op(B) by
  ``10 ** (-3 j / n)``, rounded to the storage type.  ``check_graded`` holds every entry to ``bar(case, A, B)``:
  ``oracle.chain_bound.gemm_bound`` = ``1.01 k u |op(A)| |op(B)|`` with ``u = 2**-24`` (fp32) or ``2**-53`` (fp64), and
  ``1.01 (2**-24 k + 2**-8) |op(A)| |op(B)|`` for bf16 (fp32 accumulation, one rounding to bf16: the chain rule of
  oracle.chain_bound for one product stored once).  This is Higham's worst case (Accuracy and Stability, 3.5) for a
  sum of ``k`` products in ANY order; derived, not measured.  Componentwise: an entry of scale 1e-6 weighs as much
  as one of scale 1.  The reference is the fp64 NumPy product for fp32 and bf16 (its own error is 2**-29 of the
  bar) and the extended-precision (``np.longdouble``, 64 significant bits) product for fp64 (2**-11 of the bar).
  With ``k = 0`` the bar is 0: C must be exactly 0.

A case: ``elem`` ("f32", "f64", "bf16"), ``entry`` ("single", "batched"), ``batch``, ``ta``, ``tb``, ``m``, ``n``,
``k``, ``lda`` / ``ldb`` / ``ldc`` (excess over the tight value), ``off_a`` / ``off_b`` / ``off_c`` (elements the base
pointer is moved off its 256-byte boundary), ``odd`` (batched: the member whose A and B are moved one more element
off, or None), ``same_as`` (the case with the same matrices at tight strides and no offsets: the results must agree
bit for bit), ``guarded`` (also run under NDMPS_GEMM_GUARDED=1), ``imax`` (None: ``imax_of``'s rule) and ``facts``: what
``facts_of`` must report.  Operands of a batch cycle over ``DISTINCT`` matrix pairs.  The fold case (``FOLD``) has
integer data only, built row by row (``fold_rows``).
"""
import ctypes
import functools
import zlib

import numpy as np

from oracle import chain_bound as cb
from oracle import chain_cases as cc

ELEMS = {"f32": 0, "bf16": 1, "f64": 2}            # ndmps_gemm_plan_query's elem
ESIZE = {"f32": 4, "bf16": 2, "f64": 8}
PLAN_SLOTS = ("bm", "bn", "vec", "va", "vb", "grid_x", "grid_y", "inner_a", "inner_b", "vec_in", "vec_out", "transposes",
              "launches")                          # include/ndmps_hip.h
SWITCH = "NDMPS_GEMM_GUARDED"
DISTINCT = 3
BK = {"f32": 16, "f64": 16, "bf16": 64}            # k-tile of the kernels
# the tiles and what a thread stages of each operand per k-tile (bm * 16 / 256, bn * 16 / 256 elements): quads only
# where that is a multiple of four
TILES = {"f32": {(128, 32): (1, 0), (64, 64): (1, 1), (128, 128): (1, 1)},
         "f64": {(64, 16): (1, 0), (32, 32): (0, 0), (64, 64): (1, 1)}}
FOLD_ROWS = 65535 * 128                            # rows of one bf16 launch


# ----------------------------------------------------------------------------- data and references
def imax_of(case):
    """The largest operand magnitude of the case's integer data."""
    if case["elem"] == "f64":
        return 2 ** 19
    cap = 255 if case["elem"] == "bf16" else 2047
    k = max(case["k"], 1)
    imax = int(np.sqrt((2 ** 24 - 1) // k))
    while k * imax * imax >= 2 ** 24:
        imax -= 1
    return min(cap, imax) if case.get("imax") is None else case["imax"]


def _rng(kind, case, which, z):
    key = f"{kind}/{case['elem']}/{case['ta']}{case['tb']}/{case['m']}/{case['n']}/{case['k']}/{which}/{z}"
    return np.random.default_rng(zlib.crc32(key.encode()))


def stored(op, trans):
    """How the entry wants op(X) handed in: itself, or its transpose for a set flag."""
    return np.ascontiguousarray(op.T if trans else op)


def draw(case, kind, z):
    """(op(A) (m, k), op(B) (k, n)) of member ``z`` as fp64 arrays holding values exact in the storage type."""
    m, n, k, elem = case["m"], case["n"], case["k"], case["elem"]
    if kind == "integer":
        imax = imax_of(case)
        return (_rng(kind, case, "a", z).integers(-imax, imax + 1, size=(m, k)).astype(np.float64),
                _rng(kind, case, "b", z).integers(-imax, imax + 1, size=(k, n)).astype(np.float64))
    a = _rng(kind, case, "a", z).standard_normal((m, k)) * 10.0 ** (-3.0 * np.arange(m) / m)[:, None]
    b = _rng(kind, case, "b", z).standard_normal((k, n)) * 10.0 ** (-3.0 * np.arange(n) / n)[None, :]
    return cc.to_storage(a, elem), cc.to_storage(b, elem)


def exact_product(a, b, elem):
    """What the entry must return on integer operands, as fp64: the integer product, for bf16 rounded once."""
    c = (a.astype(np.int64) @ b.astype(np.int64))
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b))
    return cc.to_storage(c.astype(np.float64), "bf16") if elem == "bf16" else c.astype(np.float64)


def reference(a, b, elem):
    """The product the graded data is compared with: fp64, from extended precision for fp64 operands."""
    if elem == "f64":
        return (a.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.longdouble)
    return a @ b


def bar(case, a, b):
    if case["elem"] == "bf16":
        return cb.HIGHER_ORDER * (cb.U_F32 * case["k"] + cb.U_BF16) * (np.abs(a) @ np.abs(b))
    return cb.gemm_bound(a, b, cb.U_F64 if case["elem"] == "f64" else cb.U_F32)


def poisoned(a, ld, extra_rows, offset=0):
    """``a`` embedded in a flat buffer of ``offset + (rows + extra_rows) ld`` elements: element (r, c) at
    ``offset + r ld + c``; the leading elements, the pad columns and the trailing rows are NaN (tests/gram_cases.py)."""
    rows, cols = a.shape
    assert ld >= cols
    flat = np.full(offset + (rows + extra_rows) * ld, np.nan)
    flat[offset:].reshape(rows + extra_rows, ld)[:rows, :cols] = a
    return flat


# ----------------------------------------------------------------------------- the two assertions
def check_integer(c, exact):
    """Integer data: C is the exact matrix, entry for entry (bf16: both hold bf16 values, so equal bits)."""
    assert c.shape == exact.shape and c.dtype == np.float64
    bad = np.argwhere(~(c == exact))
    assert bad.size == 0, f"{len(bad)} entries differ, first at {tuple(bad[0])}: {c[tuple(bad[0])]!r} != {exact[tuple(bad[0])]!r}"


def check_graded(c, ref, bound):
    """Graded data: |C - ref| <= bound entrywise; returns the worst |C - ref| / bound (0 where both vanish)."""
    assert c.shape == ref.shape and np.isfinite(c).all()
    err = np.abs(c.astype(ref.dtype) - ref).astype(np.float64)
    excess = err - bound
    if excess.size == 0:
        return 0.0
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[worst] <= 0.0, f"entry {worst}: |{c[worst]!r} - {ref[worst]!r}| = {err[worst]:.3g} > {bound[worst]:.3g}"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max())


# ----------------------------------------------------------------------------- the cases
CASES = {}


def tight(case):
    """The smallest leading dimensions the case's shape allows: (lda, ldb, ldc)."""
    return (case["m"] if case["ta"] else case["k"], case["k"] if case["tb"] else case["n"], case["n"])


def _add(tag, elem, ta, tb, m, n, k, facts, entry="single", batch=1, ld=(0, 0, 0), off=(0, 0, 0), odd=None, same_as=None,
         guarded=False, imax=None, integer_only=False):
    name = f"{tag}-{elem}-{'nt'[ta]}{'nt'[tb]}-{m}x{n}x{k}"
    if entry == "batched":
        name += f"-b{batch}" + (f"odd{odd}" if odd is not None else "")
    if any(ld):
        name += "-ld+" + ".".join(str(v) for v in ld)
    if any(off):
        name += "-off" + ".".join(str(v) for v in off)
    assert name not in CASES, name
    assert same_as is None or same_as in CASES, same_as
    CASES[name] = dict(elem=elem, entry=entry, batch=batch, ta=ta, tb=tb, m=m, n=n, k=k, lda=ld[0], ldb=ld[1], ldc=ld[2],
                       off_a=off[0], off_b=off[1], off_c=off[2], odd=odd, same_as=same_as, guarded=guarded, imax=imax,
                       integer_only=integer_only, facts=facts)
    return name


# per tile: the smallest shapes that reach each fetch path.  n of the vector shape: a multiple of 4 inside the tile's
# range and no multiple of bn; n of the scalar shape: odd, inside the range.
_SHAPES = {("f32", 128, 32): (28, 31), ("f32", 64, 64): (44, 45), ("f32", 128, 128): (132, 131),
           ("f64", 64, 16): (12, 15), ("f64", 32, 32): (28, 31), ("f64", 64, 64): (68, 67)}
VECTOR, SCALAR = {}, {}
for (_elem, _bm, _bn), (_nv, _ns) in _SHAPES.items():
    _va, _vb = TILES[_elem][(_bm, _bn)]
    for _ta in (0, 1):
        for _tb in (0, 1):
            # vector shape: two full row blocks on the straight-line fetch, a ragged one on the guarded quads, two
            # full k-tiles and a partial one
            VECTOR[_elem, _bm, _bn, _ta, _tb] = _add(
                "vector", _elem, _ta, _tb, 2 * _bm + 4, _nv, 36,
                dict(bm=_bm, bn=_bn, vec=1, va=_va, vb=_vb, grid_x=3, grid_y=-(-_nv // _bn), inner_a=2 * _va,
                     inner_b=(_nv // _bn) * _vb, launches=1), guarded=True)
            SCALAR[_elem, _bm, _bn, _ta, _tb] = _add(
                "scalar", _elem, _ta, _tb, _bm + 3, _ns, 35,
                dict(bm=_bm, bn=_bn, vec=0, va=0, vb=0, grid_x=2, grid_y=-(-_ns // _bn), inner_a=0, inner_b=0))
            # no edge at all: one block, one k-tile
            _add("exact", _elem, _ta, _tb, _bm, _bn, 16,
                 dict(bm=_bm, bn=_bn, vec=1, va=_va, vb=_vb, grid_x=1, grid_y=1, inner_a=_va, inner_b=_vb), guarded=True)

# where the tile changes
for _n, _tile in ((32, (128, 32)), (33, (64, 64)), (64, (64, 64)), (65, (128, 128))):
    _add("edge", "f32", 0, 0, 68, _n, 20, dict(bm=_tile[0], bn=_tile[1]))
for _m, _tile in ((64, (64, 64)), (65, (128, 128))):
    _add("edge", "f32", 0, 0, _m, 68, 20, dict(bm=_tile[0], bn=_tile[1]))
for _n, _tile in ((16, (64, 16)), (17, (32, 32)), (32, (32, 32)), (33, (64, 64))):
    _add("edge", "f64", 0, 0, 36, _n, 20, dict(bm=_tile[0], bn=_tile[1]))
for _m, _tile in ((32, (32, 32)), (33, (64, 64))):
    _add("edge", "f64", 0, 0, _m, 36, 20, dict(bm=_tile[0], bn=_tile[1]))

# strides and offsets on the vector shape of every tile: what keeps the quads and what breaks them
for (_elem, _bm, _bn), (_nv, _ns) in _SHAPES.items():
    _va, _vb = TILES[_elem][(_bm, _bn)]
    _on, _offq = dict(vec=1, va=_va, vb=_vb, inner_a=2 * _va), dict(vec=0, va=0, vb=0, inner_a=0, inner_b=0)
    for _ta, _tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        _base = VECTOR[_elem, _bm, _bn, _ta, _tb]
        _shape = (2 * _bm + 4, _nv, 36)
        _add("ld", _elem, _ta, _tb, *_shape, _on, ld=(4, 4, 4), same_as=_base, guarded=True)
        _add("ld", _elem, _ta, _tb, *_shape, _offq, ld=(1, 0, 0), same_as=_base)
        _add("ld", _elem, _ta, _tb, *_shape, _offq, ld=(0, 1, 0), same_as=_base)
        _add("off", _elem, _ta, _tb, *_shape, _on, off=(4, 4, 0), same_as=_base)
        _add("off", _elem, _ta, _tb, *_shape, _offq, off=(1, 0, 0), same_as=_base)
        _add("off", _elem, _ta, _tb, *_shape, _offq, off=(0, 1, 0), same_as=_base)
        if _elem == "f64":   # 16-byte but not 32-byte aligned
            _add("off", _elem, _ta, _tb, *_shape, _offq, off=(2, 0, 0), same_as=_base)
            _add("off", _elem, _ta, _tb, *_shape, _offq, off=(0, 2, 0), same_as=_base)
        _add("padc", _elem, _ta, _tb, *_shape, _on, ld=(0, 0, 3), off=(0, 0, 1), same_as=_base)

# degenerate extents
for _elem, _nn in (("f32", 44), ("f64", 68)):
    for _ta, _tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        # k = 0: nothing is read and C = 0 (leading dimensions above 0, so that every operand has an address)
        _add("k0", _elem, _ta, _tb, 68, _nn, 0, dict(vec=1, launches=1), ld=(4, 4, 0), guarded=True)
        _add("k0", _elem, _ta, _tb, 67, _nn + 1, 0, dict(vec=0, launches=1), ld=(1, 1, 0))
        _add("m1", _elem, _ta, _tb, 1, _nn, 36, dict(vec=1 - _ta, grid_x=1))
        _add("n1", _elem, _ta, _tb, 68, 1, 36, dict(vec=_tb, grid_y=1, bn=32 if _elem == "f32" else 16))
        _add("k1", _elem, _ta, _tb, 68, _nn, 1, dict(vec=0))
        _add("k4", _elem, _ta, _tb, 68, _nn, 4, dict(vec=1, paths_a={"guarded"}, paths_b={"guarded"}), guarded=True)

# batched: the same launch for every triple (grid.z); one unaligned member takes the quads from the whole batch
for _elem in ("f32", "f64"):
    _nv = _SHAPES[_elem, 64, 64][0]
    for _batch in (1, 3, 64):
        _add("batched", _elem, 0, 1, 132, _nv, 36, dict(bm=64, bn=64, vec=1, va=1, vb=1), entry="batched", batch=_batch,
             same_as=VECTOR[_elem, 64, 64, 0, 1], guarded=_batch == 3)
    _add("batched", _elem, 0, 1, 132, _nv, 36, dict(bm=64, bn=64, vec=0, va=0, vb=0), entry="batched", batch=3, odd=1,
         same_as=VECTOR[_elem, 64, 64, 0, 1])
    _add("batched", _elem, 1, 0, 67, _SHAPES[_elem, 64, 64][1], 35, dict(bm=64, bn=64, vec=0), entry="batched", batch=3,
         same_as=SCALAR[_elem, 64, 64, 1, 0])
_add("batched", "f32", 0, 0, 260, 132, 36, dict(bm=128, bn=128, vec=1, va=1, vb=1, inner_a=2, inner_b=1), entry="batched",
     batch=3, same_as=VECTOR["f32", 128, 128, 0, 0])
_add("batched", "f32", 0, 0, 260, 28, 36, dict(bm=128, bn=32, vec=1, va=1, vb=0), entry="batched", batch=3,
     same_as=VECTOR["f32", 128, 32, 0, 0])
_add("batched", "f64", 0, 0, 68, 28, 36, dict(bm=32, bn=32, vec=1, va=0, vb=0), entry="batched", batch=3,
     same_as=VECTOR["f64", 32, 32, 0, 0])

# bf16: k = 8 one chunk, 64 one k-tile, 70 a tail that is no whole chunk, 130 two k-tiles and such a tail; 16-byte
# loads need whole chunks in every row of A and of the (n, k) right operand, 16-byte stores whole chunks in C's rows
BF16_BASE = {}
for _tb in (0, 1):
    for _k in (8, 64, 70, 130):
        for _n in (8, 130):
            for _m in (5, 128, 300):
                BF16_BASE[_tb, _m, _n, _k] = _add(
                    "bf16", "bf16", 0, _tb, _m, _n, _k,
                    dict(bm=128, bn=128, vec_in=int(_k % 8 == 0), vec_out=int(_n % 8 == 0), transposes=1 - _tb,
                         grid_x=-(-_n // 128), grid_y=-(-_m // 128), launches=1))
for _tb in (0, 1):
    _s, _b = (300, 8, 64), BF16_BASE[_tb, 300, 8, 64]
    _add("bf16ld", "bf16", 0, _tb, *_s, dict(vec_in=1, vec_out=1), ld=(8, 8, 8), same_as=_b)
    _add("bf16ld", "bf16", 0, _tb, *_s, dict(vec_in=0, vec_out=1), ld=(1, 0, 0), same_as=_b)
    # a (k, n) right operand is copied into rows of k elements whatever its own leading dimension
    _add("bf16ld", "bf16", 0, _tb, *_s, dict(vec_in=1 - _tb, vec_out=1), ld=(0, 1, 0), same_as=_b)
    _add("bf16ld", "bf16", 0, _tb, *_s, dict(vec_in=1, vec_out=0), ld=(0, 0, 1), same_as=_b)
    _add("bf16off", "bf16", 0, _tb, *_s, dict(vec_in=1, vec_out=0), off=(0, 0, 1), same_as=_b)
    _add("bf16off", "bf16", 0, _tb, *_s, dict(vec_in=0, vec_out=1), off=(1, 0, 0), same_as=_b)
    _add("bf16off", "bf16", 0, _tb, *_s, dict(vec_in=_tb ^ 1, vec_out=1), off=(0, 1, 0), same_as=_b)
# 16-byte loads with a tail: rows of 72 elements, 70 of them the operand (the last chunk is loaded element by element)
_add("bf16tail", "bf16", 0, 1, 300, 130, 70, dict(vec_in=1, vec_out=0), ld=(2, 2, 0), same_as=BF16_BASE[1, 300, 130, 70])
_add("bf16tail", "bf16", 0, 1, 128, 8, 130, dict(vec_in=1, vec_out=1), ld=(6, 6, 0), same_as=BF16_BASE[1, 128, 8, 130])
# the transpose's ld_in
_add("bf16ld", "bf16", 0, 0, 128, 130, 70, dict(vec_in=0, vec_out=0, transposes=1), ld=(0, 3, 0),
     same_as=BF16_BASE[0, 128, 130, 70])
# more than 65535 row tiles: the second launch starts FOLD_ROWS rows into A and C.  Operands up to 5: k imax**2 = 200
# is exact in bf16's 8 bits, so C is the integer matrix itself.
FOLD = _add("bf16fold", "bf16", 0, 1, FOLD_ROWS + 1, 8, 8, dict(vec_in=1, vec_out=1, grid_y=65535, launches=2), imax=5,
            integer_only=True)


def small_cases():
    """Every case whose operands are drawn by ``data`` (all but the fold, which ``fold_rows`` builds row by row)."""
    return [name for name in CASES if name != FOLD]


def guarded_cases():
    return [name for name, case in CASES.items() if case["guarded"]]


def lds(case):
    """(lda, ldb, ldc) in elements."""
    t = tight(case)
    return t[0] + case["lda"], t[1] + case["ldb"], t[2] + case["ldc"]


def misalignment(case):
    """(mis_a, mis_b, mis_c) in bytes, as the entry computes them from buffers on a 256-byte boundary.  The bf16
    kernel reads a (k, n) right operand from the workspace, which the tests keep aligned."""
    e = ESIZE[case["elem"]]
    odd = e if case["odd"] is not None else 0
    mis_b = 0 if case["elem"] == "bf16" and not case["tb"] else (case["off_b"] * e) % 64 | odd
    return (case["off_a"] * e) % 64 | odd, mis_b, (case["off_c"] * e) % 64


def plan_of(lib, case, guarded=False):
    """ndmps_gemm_plan_query's answer for the case, as a dict over PLAN_SLOTS."""
    out = (ctypes.c_int64 * len(PLAN_SLOTS))()
    rc = lib.ndmps_gemm_plan_query(ELEMS[case["elem"]], case["ta"], case["tb"], case["m"], case["n"], case["k"], *lds(case),
                                   *misalignment(case), int(guarded), out)
    assert rc == 0
    return dict(zip(PLAN_SLOTS, list(out)))


def facts_of(case, plan):
    """What a launch of ``case`` does: the plan query's answer and, from it, the fetch paths the blocks of each
    operand take in gemm_body (a restatement of its rule): "inner" straight-line quads, "guarded" quads, "scalar"."""
    f = dict(plan)
    if case["elem"] == "bf16":
        return f
    full_k, part_k = case["k"] >= 16, case["k"] % 16 != 0
    for x, v, inner, blocks in (("a", plan["va"], plan["inner_a"], plan["grid_x"]),
                                ("b", plan["vb"], plan["inner_b"], plan["grid_y"])):
        paths = set()
        if not v:
            paths.add("scalar")
        else:
            if inner > 0 and full_k:
                paths.add("inner")
            if inner < blocks or part_k or not full_k:
                paths.add("guarded")
        f["paths_" + x] = paths
    return f


@functools.lru_cache(maxsize=None)
def data(name, kind):
    """The min(batch, DISTINCT) operand pairs of a case and their references, computed once.  Cases that name the
    same elem, transposes and shape share their matrices (``same_as``).
    kind "integer" -> [(op_a, op_b, exact)], kind "graded" -> [(op_a, op_b, ref, bar)]."""
    case = CASES[name]
    out = []
    for z in range(min(case["batch"], DISTINCT)):
        a, b = draw(case, kind, z)
        if kind == "integer":
            out.append((a, b, exact_product(a, b, case["elem"])))
        else:
            out.append((a, b, reference(a, b, case["elem"]), bar(case, a, b)))
    return out


def fold_rows(rows):
    """Rows ``rows`` (int64 array) of the fold case's A (integers in [-5, 5], int8): a hash of (row, column), so any
    rows can be had without the 67 M elements of the whole."""
    i = np.asarray(rows, dtype=np.uint64)[:, None]
    j = np.arange(8, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + (i >> np.uint64(7)) * np.uint64(97)) >> np.uint64(5)
    return (h % np.uint64(11)).astype(np.int8) - np.int8(5)


def fold_b():
    """The fold case's right operand, stored (n, k) = (8, 8), int8."""
    return np.random.default_rng(8).integers(-5, 6, size=(8, 8)).astype(np.int8)


def fold_checked_rows():
    """The rows compared in full: the first tile, both sides of the fold, the last row."""
    m = CASES[FOLD]["m"]
    assert m - 1 == FOLD_ROWS   # the second launch holds the last row alone
    return np.concatenate([np.arange(128), [FOLD_ROWS - 2, FOLD_ROWS - 1, FOLD_ROWS]]).astype(np.int64)
