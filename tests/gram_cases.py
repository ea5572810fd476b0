"""The shapes every route of the Gram family (csrc/gram.hip) is tested on, shared by tests/test_gram_cases_host.py
(CPU: every case reaches the route and the edge it was chosen for, and the two assertions have teeth on exactly these
cases) and tests/test_gpu_gram_routes.py (the kernels, through those assertions).  NumPy only.

Two kinds of data, two assertions:

* ``integer_matrix``: integers of magnitude at most 2047 (fp32), 255 (bf16), 2**19 (fp64): exactly representable in the
  storage type.  The kernels widen fp32 and bf16 to fp64 in front of ``v_mfma_f64_16x16x4_f64``, a product of two such
  integers is an integer below 2**38, and with ``m <= 2**13`` rows every partial sum of every entry of ``A^T A`` stays
  below 2**51 < 2**53: each add is exact whatever the order, so G IS the integer matrix ``exact_gram`` and
  ``check_integer`` asks for equality.  (Two cases have more rows: 16512 x 64 stays below 2**37 all the same, and
  600000 x 8 draws integers up to 63: below 2**32.  The host test checks ``m imax**2 < 2**53`` case by case.)  The
  diagonal exceeds 2**24 wherever ``m max|a|**2 / 3`` does, so an fp32 accumulator cannot produce it.
* ``graded_matrix``: Gaussian columns scaled by ``10 ** (-6 j / n)`` and rounded to the storage type.  ``check_graded``
  holds every entry to ``bar(m) |A|^T |A|``: ``bar(m) = 2 g``, ``g = m u / (1 - m u)``, ``u = 2**-53`` is the worst case
  of a sum of ``m`` products in ANY order of summation (Higham, Accuracy and Stability, 3.1 -- the rounded product of
  two fp64 elements included), once for the kernel and once for the fp64 NumPy product it is compared with.  Derived,
  not measured.  Componentwise, so an error in the columns of scale 1e-6 weighs as much as one in those of scale 1.

A case: ``elem`` ("f32", "bf16", "f64"), ``entry`` ("single", "batched", "gathered", "gathered_batched"), ``batch``,
``m``, ``n``, ``lda``, ``offset`` (elements the base pointer is moved off its 16-byte boundary), ``imax`` (None: the
element type's limit), ``facts`` (what ``facts_of`` must report under the default switches: the route and the geometry
the case exists for) and ``switches``: ``{"NAME=value": facts under that switch}`` for every switch the case also runs
under.  Operands of a batch cycle over ``DISTINCT`` matrices (they are read-only): matrix ``z`` is matrix ``z % 4``.
"""
import ctypes
import functools
import zlib

import numpy as np

from oracle import chain_cases as cc

ELEMS = {"f32": 0, "bf16": 1, "f64": 2}            # ndmps_gram_plan_query's elem
IMAX = {"f32": 2047, "bf16": 255, "f64": 2 ** 19}
ROUTES = ("None", "Small", "Tiles16", "Tiles64", "Tiles128", "Tiles64Batched", "Stream64")
PLAN_SLOTS = ("route", "small_blocks", "T", "n_tiles", "n_slabs", "rows_per_slab", "tiles_1d", "slabs_off", "slabs_diag",
              "rows_off", "rows_diag", "xcd", "slots", "workspace_bytes")   # include/ndmps_hip.h
SWITCHES = ("NDMPS_GRAM_XCD", "NDMPS_GRAM64_TILES", "NDMPS_GRAM_NO_TURN", "NDMPS_GRAM_GENERAL")
DISTINCT = 4
U = 2.0 ** -53


# ----------------------------------------------------------------------------- data and references
def _rng(kind, elem, m, n, seed):
    return np.random.default_rng(zlib.crc32(f"{kind}/{elem}/{m}/{n}/{seed}".encode()))


def integer_matrix(elem, m, n, seed, imax=None):
    """(m, n) fp64 array of random integers in [-imax, imax] (default: IMAX[elem]): exact in ``elem``."""
    imax = IMAX[elem] if imax is None else imax
    return _rng("int", elem, m, n, seed).integers(-imax, imax + 1, size=(m, n)).astype(np.float64)


def graded_matrix(elem, m, n, seed):
    """(m, n) fp64 array: Gaussian columns scaled by 10 ** (-6 j / n), holding the values as ``elem`` stores them."""
    a = _rng("graded", elem, m, n, seed).standard_normal((m, n)) * 10.0 ** (-6.0 * np.arange(n) / n)
    return cc.to_storage(a, elem)


def exact_gram(a):
    """The int64 A^T A of an integer-valued matrix.  Every partial sum is an integer below 2**53 (asserted), so the
    fp64 product is that integer in whatever order the BLAS adds; tests/test_gram_cases_host.py compares a strip of
    it with int64 arithmetic."""
    assert np.array_equal(np.rint(a), a) and a.shape[0] * float(np.abs(a).max()) ** 2 < 2.0 ** 53
    return (a.T @ a).astype(np.int64)


def abs_gram(a):
    return np.abs(a).T @ np.abs(a)


def bar(m):
    g = m * U / (1.0 - m * U)
    return 2.0 * g


def poisoned(a, lda, extra_rows, offset=0):
    """``a`` embedded in a flat buffer of ``offset + (m + extra_rows) lda`` elements: element (r, c) at
    ``offset + r lda + c``; the leading elements, the pad columns and the trailing rows are NaN."""
    m, n = a.shape
    assert lda >= n
    flat = np.full(offset + (m + extra_rows) * lda, np.nan)
    flat[offset:].reshape(m + extra_rows, lda)[:m, :n] = a
    return flat


def gather_tables(m, n, seed):
    """Offset tables of a gathered operand, as the fused sweep builds them: position ``p`` of the visiting order reads
    ``base[row_off[r] + col_off[p]]`` and is column ``perm[p]`` of the matrix.  ``col_off`` ascends in aligned runs of
    four with a gap of four elements behind each run; rows are ``2 n + 8`` elements apart, in shuffled order; quads of
    columns are permuted.  Returns (row_off, col_off, perm, base_len)."""
    assert n % 4 == 0
    rng = _rng("tables", "f32", m, n, seed)
    pos = np.arange(n)
    col_off = (8 * (pos // 4) + pos % 4).astype(np.int64)
    stride = 2 * n + 8
    row_off = rng.permutation(m).astype(np.int64) * stride
    perm = (4 * rng.permutation(n // 4)[:, None] + np.arange(4)[None, :]).reshape(-1).astype(np.int32)
    return row_off, col_off, perm, m * stride


def gathered_base(a, row_off, col_off, perm, base_len):
    """The flat base ``a`` is gathered from: NaN wherever no (row, column) offset pair points."""
    base = np.full(base_len, np.nan)
    base[row_off[:, None] + col_off[None, :]] = a[:, perm]
    return base


# ----------------------------------------------------------------------------- the two assertions
def check_integer(G, exact):
    """Integer data: G is the integer matrix, entry for entry."""
    assert G.shape == exact.shape and G.dtype == np.float64
    bad = np.argwhere(~(G == exact.astype(np.float64)))
    assert bad.size == 0, f"{len(bad)} entries differ, first at {tuple(bad[0])}: {G[tuple(bad[0])]!r} != {exact[tuple(bad[0])]}"
    assert np.array_equal(G, exact)


def check_graded(G, ref64, absg, m):
    """Graded data: |G - ref64| <= bar(m) |A|^T |A|, entrywise."""
    assert G.shape == ref64.shape and np.isfinite(G).all()
    excess = np.abs(G - ref64) - bar(m) * absg
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[worst] <= 0.0, f"entry {worst}: |{G[worst]!r} - {ref64[worst]!r}| > {bar(m) * absg[worst]:.3g}"


# ----------------------------------------------------------------------------- the cases
CASES = {}


def _add(route, elems, entry, batch, m, n, lda, facts, switches=None, offset=0, imax=None, tag=""):
    for elem in elems.split():
        name = f"{route}-{entry}-{elem}-{batch}x{m}x{n}-ld{lda}" + (f"-off{offset}" if offset else "") + tag
        assert name not in CASES
        CASES[name] = dict(elem=elem, entry=entry, batch=batch, m=m, n=n, lda=lda, offset=offset, imax=imax,
                           facts=dict(route=route, **facts), switches=switches or {})


# Small: one thread per row, 2048 rows per workgroup, 256 workgroups at the most
_add("Small", "f32 bf16", "single", 1, 5000, 7, 9, dict(small_blocks=3, vec_ok=0))
_add("Small", "f32 bf16", "single", 1, 5000, 8, 8, dict(small_blocks=3, vec_ok=1))
_add("Small", "f32", "single", 1, 5000, 8, 12, dict(small_blocks=3, vec_ok=0), offset=1)
_add("Small", "f32", "single", 1, 600000, 8, 8, dict(small_blocks=256, vec_ok=1), imax=63)
# Tiles16: (16 T)^2 tiles, 64-row slabs, groups of 16 slabs in a two-level reduction above 32 slabs
_add("Tiles16", "f32 bf16", "single", 1, 1187, 12, 13, dict(T=1, n_tiles=1, n_slabs=19, last_rows=35, levels=1))
_add("Tiles16", "f32", "single", 1, 4101, 24, 24, dict(T=2, n_tiles=1, n_slabs=65, levels=2, last_group=1, last_rows=5))
_add("Tiles16", "f32 bf16", "single", 1, 2371, 40, 44, dict(T=4, n_tiles=1, n_slabs=38, levels=2, last_group=6, last_rows=3))
_add("Tiles16", "f32", "single", 1, 255, 100, 100, dict(T=4, n_tiles=3, n_slabs=4, levels=1, last_rows=63))
_add("Tiles16", "f64", "single", 1, 2371, 72, 80, dict(T=4, n_tiles=3, n_slabs=38, levels=2, last_group=6, last_rows=3))
_add("Tiles16", "f64", "single", 1, 300, 136, 136, dict(T=4, n_tiles=6, n_slabs=5, levels=1, last_rows=44))
_add("Tiles16", "f64", "single", 1, 50, 200, 208, dict(T=4, n_tiles=10, n_slabs=1, last_rows=50))
# Tiles64: 64 x 64 tiles staged in LDS, 128-row slabs
_add("Tiles64", "f32 bf16", "single", 1, 4229, 100, 104, dict(n_tiles=3, n_slabs=34, levels=2, last_group=2, last_rows=5, vec_ok=1))
_add("Tiles64", "f32", "single", 1, 300, 68, 71, dict(n_tiles=3, n_slabs=3, levels=1, last_rows=44, vec_ok=0))
_add("Tiles64", "f32 bf16", "single", 1, 300, 68, 68, dict(n_tiles=3, n_slabs=3, levels=1, last_rows=44, vec_ok=0), offset=1)
# Tiles128, one matrix: mode 0 the guarded fetch, mode 1 the straight-line one (whole panels, whole 32-row chunks)
_GENERAL = {"NDMPS_GRAM_GENERAL=1": dict(mode=0)}
_add("Tiles128", "f32 bf16", "single", 1, 1000, 132, 136, dict(tiles_1d=2, slabs_off=7, slabs_diag=4, mode=0, vec_ok=1))
_add("Tiles128", "f32", "single", 1, 4128, 256, 256, dict(tiles_1d=2, slabs_off=26, slabs_diag=17, mode=1), switches=_GENERAL)
_add("Tiles128", "f32", "single", 1, 4133, 260, 263, dict(tiles_1d=3, slabs_off=26, slabs_diag=17, mode=0, vec_ok=0))
_add("Tiles128", "f32", "single", 1, 256, 128, 128, dict(tiles_1d=1, slabs_diag=2, slots=2, mode=1))


# Tiles128 batched: every case also under the XCD orders and on the guarded fetch
def _b128(xcd1, xcd2):
    return {"NDMPS_GRAM_XCD=1": xcd1, "NDMPS_GRAM_XCD=2": xcd2, "NDMPS_GRAM_GENERAL=1": dict(mode=0)}


_add("Tiles128", "f32 bf16", "batched", 3, 2600, 256, 256, dict(tiles_1d=2, slabs_off=5, slabs_diag=3, mode=0, launches=1),
     switches=_b128(dict(xcd=1, slabs_off=5, slabs_diag=3), dict(xcd=2, slabs_off=4, slabs_diag=4)))
_add("Tiles128", "f32 bf16", "batched", 2, 2592, 384, 384, dict(tiles_1d=3, slabs_off=5, slabs_diag=3, mode=1, launches=1),
     switches=_b128(dict(xcd=1, slabs_off=5, slabs_diag=3, mode=1), dict(xcd=2, slabs_off=4, slabs_diag=4, mode=1)))
_add("Tiles128", "f32", "batched", 3, 2600, 260, 264, dict(tiles_1d=3, slabs_off=5, slabs_diag=3, mode=0, launches=1),
     switches=_b128(dict(xcd=1, slabs_off=5, slabs_diag=3), dict(xcd=2, slabs_off=4, slabs_diag=4)))
_add("Tiles128", "f32", "batched", 49, 300, 132, 132, dict(tiles_1d=2, slabs_off=1, slabs_diag=1, mode=0, launches=2),
     switches=_b128(dict(xcd=0, launches=2), dict(xcd=0, launches=2)))
_add("Tiles128", "f32", "batched", 50, 2080, 256, 256, dict(tiles_1d=2, slabs_off=4, slabs_diag=3, mode=1, launches=2),
     switches=_b128(dict(xcd=1, slabs_off=4, slabs_diag=2, launches=2), dict(xcd=2, slabs_off=3, slabs_diag=3, launches=2)))
# Tiles64Batched: 64 matrices per launch
_add("Tiles64Batched", "f32 bf16", "batched", 3, 1100, 100, 104, dict(n_tiles=3, n_slabs=9, last_rows=76, launches=1))
_add("Tiles64Batched", "f32", "batched", 66, 260, 68, 68, dict(n_tiles=3, n_slabs=3, last_rows=4, launches=2))
# Stream64: blocks of 128 rows (four unrolled per trip), then the ragged end row by row; also on the tile kernel
_TILES = {"NDMPS_GRAM64_TILES=1": dict(route="Tiles64Batched")}
_add("Stream64", "f32 bf16", "batched", 2, 256, 64, 64, dict(n_slabs=2, full_blocks=1, ragged_rows=0, last_rows=128), switches=_TILES)
_add("Stream64", "f32 bf16", "batched", 3, 4099, 64, 68, dict(n_slabs=33, full_blocks=1, last_rows=3, last_full_blocks=0),
     switches=_TILES)
_add("Stream64", "f32", "batched", 66, 260, 64, 64, dict(n_slabs=3, last_rows=4, launches=2), switches=_TILES)
_add("Stream64", "f32", "batched", 64, 16512, 64, 64, dict(rows_per_slab=704, full_blocks=5, ragged_rows=64, n_slabs=24),
     switches={"NDMPS_GRAM64_TILES=1": dict(route="Tiles64Batched", rows_per_slab=416, n_slabs=40, full_blocks=3, ragged_rows=32)})
# gathered: through the offset tables, stored through the column permutation
_add("Tiles64", "f32", "gathered", 1, 600, 64, 64, dict(n_tiles=1, n_slabs=5))
_add("Tiles128", "f32", "gathered", 1, 1000, 132, 132, dict(mode=0, slabs_off=7, slabs_diag=4))
_add("Tiles128", "f32", "gathered", 1, 4128, 256, 256, dict(mode=2))
_add("Tiles128", "f32", "gathered_batched", 2, 2592, 384, 384, dict(mode=2, slabs_off=5, slabs_diag=3),
     switches={"NDMPS_GRAM_XCD=1": dict(xcd=1, slabs_off=5, mode=2), "NDMPS_GRAM_XCD=2": dict(xcd=2, slabs_off=4, slabs_diag=4, mode=2)})
_add("Stream64", "f32", "gathered_batched", 3, 4099, 64, 64, dict(n_slabs=33, last_rows=3), switches=_TILES)
_add("Tiles128", "f32", "gathered_batched", 49, 300, 132, 132, dict(mode=0, launches=2))


def variants():
    """(case name, switch or None) of every GPU run."""
    return [(name, sw) for name, case in CASES.items() for sw in [None, *case["switches"]]]


def is_gathered(case):
    return case["entry"].startswith("gathered")


def is_batched(case):
    return case["entry"].endswith("batched")


def vec_ok(case):
    """The launchers' own test for 16-byte (bf16: 8-byte) loads: whole fours in every row, on a boundary of four."""
    return int(case["lda"] % 4 == 0 and case["n"] % 4 == 0 and case["offset"] % 4 == 0)


def plan_of(lib, case):
    """ndmps_gram_plan_query's answer for the case, as a dict over PLAN_SLOTS.  ``lib`` is the loaded library; the
    switches are the caller's business (set_switch)."""
    out = (ctypes.c_int64 * len(PLAN_SLOTS))()
    rc = lib.ndmps_gram_plan_query(ELEMS[case["elem"]], case["batch"], case["m"], case["n"], int(is_gathered(case)),
                                   int(is_batched(case)), out)
    assert rc == 0
    return dict(zip(PLAN_SLOTS, list(out)))


def set_switch(monkeypatch, switch):
    """Every switch of the family unset, then ``switch`` ("NAME=value" or None) set."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(*switch.split("="))


def facts_of(case, plan, switch=None):
    """What a launch of ``case`` does, from the plan query's answer (dict over PLAN_SLOTS) and, for what the launchers
    decide behind the plan, a restatement of their rule: ``mode`` of run_tiles128, the launch chunks of 48 and 64
    matrices, the reduction levels of launch_tile_reduce, the 128-row blocks of gram64_stream_kernel."""
    m, n, batch = case["m"], case["n"], case["batch"]
    f = {k: plan[k] for k in PLAN_SLOTS if k != "route"}
    f["route"] = route = ROUTES[plan["route"]]
    f["vec_ok"] = vec_ok(case)
    if route in ("Tiles16", "Tiles64", "Tiles64Batched", "Stream64"):
        rows = plan["rows_per_slab"]
        f["last_rows"] = m - (plan["n_slabs"] - 1) * rows
        f["levels"] = 2 if plan["n_slabs"] > 32 else 1
        if f["levels"] == 2:
            f["last_group"] = plan["n_slabs"] - 16 * ((plan["n_slabs"] + 15) // 16 - 1)
        f["full_blocks"] = min(rows, m) // 128
        f["ragged_rows"] = min(rows, m) % 128
        f["last_full_blocks"] = f["last_rows"] // 128
        f["launches"] = (batch + 63) // 64
    if route == "Tiles128":
        interior = f["vec_ok"] and n % 128 == 0 and m % 32 == 0 and switch != "NDMPS_GRAM_GENERAL=1"
        f["mode"] = (2 if is_gathered(case) else 1) if interior else 0
        f["launches"] = (batch + 47) // 48
    return f


def slab_rows(plan):
    """Rows of one partial sum of the route's first kernel (the off-diagonal slabs of Tiles128; 2048 for Small)."""
    route = ROUTES[plan["route"]]
    return plan["rows_off"] if route == "Tiles128" else (2048 if route == "Small" else plan["rows_per_slab"])


@functools.lru_cache(maxsize=None)
def data(name, kind):
    """The min(batch, DISTINCT) matrices of a case as fp64 arrays and their references, computed once:
    kind "integer" -> [(a, exact_gram)], kind "graded" -> [(a, ref64, abs_gram)]."""
    case = CASES[name]
    out = []
    for z in range(min(case["batch"], DISTINCT)):
        if kind == "integer":
            a = integer_matrix(case["elem"], case["m"], case["n"], z, case["imax"])
            out.append((a, exact_gram(a)))
        else:
            a = graded_matrix(case["elem"], case["m"], case["n"], z)
            out.append((a, a.T @ a, abs_gram(a)))
    return out
