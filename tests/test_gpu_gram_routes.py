"""Every route of the Gram family (csrc/gram.hip) on the MI355X, on the shapes of tests/gram_cases.py.

Bars, and where they come from (tests/gram_cases.py has the derivations, tests/test_gram_cases_host.py shows on the CPU
that both reject an fp32 accumulator, a dropped row, two swapped columns and a pad element on every case used here):

* Integer data: ``G == exact_gram`` entry for entry.  The elements and every partial sum are integers below 2**53, the
  kernels widen to fp64 before the MFMA, so every order of summation gives the same bits.
* Graded data (columns scaled from 1 down to 1e-6): ``|G - ref64| <= bar(m) |A|^T |A|`` entrywise, ``bar(m) = 2 m u /
  (1 - m u)``, ``u = 2**-53``: the worst case of any order of summation, for the kernel and for the fp64 NumPy reference.
* ``NDMPS_GRAM_GENERAL=1`` changes only how the 128-wide kernel fetches (guarded loads instead of straight-line ones):
  same slabs, same order of MFMAs, and G is bit-identical to the default's.  ``NDMPS_GRAM_XCD=1|2`` and
  ``NDMPS_GRAM64_TILES=1`` cut the rows differently: graded data is held to the bar, integer data to equality.

Every launch goes through ``_run``: the operand sits in a buffer whose pad columns, trailing rows and leading elements
are NaN (for a gathered operand: every element no offset pair addresses), every G has 24 doubles of slack behind it
and the workspace 4096 guard bytes; the slack, the guard and everything of G outside n x n must come back untouched,
G finite and exactly symmetric, a second call must give the same bits, and a workspace one byte short must be refused
with G untouched.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import gram_cases as gc  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
SENTINEL, SLACK, GUARD, GUARD_BYTE = -7.0, 24, 4096, 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A launch that faulted leaves the device in an error state: end the session instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


@pytest.fixture
def lib(monkeypatch):
    gc.set_switch(monkeypatch, None)
    return _lib.load()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _size_query(lib, case):
    if gc.is_batched(case):
        return lib.ndmps_gram_batched_workspace_bytes(case["batch"], case["m"], case["n"])
    return (lib.ndmps_gram_f64_workspace_bytes if case["elem"] == "f64" else lib.ndmps_gram_workspace_bytes)(case["m"], case["n"])


def _call(lib, case, ptrs, tables, G, ws, ws_bytes):
    """One call of the case's entry point; returns its return code."""
    batch, m, n, lda = case["batch"], case["m"], case["n"], case["lda"]
    stride_G = G.shape[1]
    sp = _lib.stream_ptr()
    if case["entry"] == "single":
        fn = {"f32": lib.ndmps_gram_f32, "bf16": lib.ndmps_gram_bf16, "f64": lib.ndmps_gram_f64}[case["elem"]]
        return fn(ptrs[0], m, n, lda, G.data_ptr(), ws.data_ptr(), ws_bytes, sp)
    h = (C.c_void_p * batch)(*[ptrs[z % len(ptrs)] for z in range(batch)])
    if case["entry"] == "batched":
        fn = {"f32": lib.ndmps_gram_batched_f32, "bf16": lib.ndmps_gram_batched_bf16}[case["elem"]]
        return fn(batch, h, m, n, lda, G.data_ptr(), stride_G, ws.data_ptr(), ws_bytes, sp)
    t_r, t_c, t_p = (t.data_ptr() for t in tables)
    if case["entry"] == "gathered":
        return lib.ndmps_gram_indexed_f32(ptrs[0], m, n, t_r, t_c, t_p, G.data_ptr(), ws.data_ptr(), ws_bytes, sp)
    return lib.ndmps_gram_batched_indexed_f32(batch, h, m, n, t_r, t_c, t_p, G.data_ptr(), stride_G, ws.data_ptr(), ws_bytes, sp)


def _operands(case, mats):
    """Device buffers of the distinct matrices (kept alive by the caller), the pointers to hand in, the tables."""
    dt = DT[case["elem"]]
    if gc.is_gathered(case):
        row_off, col_off, perm, base_len = gc.gather_tables(case["m"], case["n"], 0)
        bufs = [_dev(gc.gathered_base(a, row_off, col_off, perm, base_len), dt) for a in mats]
        tables = (_dev(row_off), _dev(col_off), _dev(perm))
    else:
        bufs = [_dev(gc.poisoned(a, case["lda"], 3, case["offset"]), dt) for a in mats]
        tables = None
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    return bufs, [b.data_ptr() + case["offset"] * b.element_size() for b in bufs], tables


def _run(lib, case, mats, nbytes=None):
    """G (batch, n, n) of the case on ``mats`` (the distinct matrices, cycled over the batch), with every check of the
    module docstring around the launch.  nbytes: the workspace size to work with (default: the size query's)."""
    batch, n = case["batch"], case["n"]
    bufs, ptrs, tables = _operands(case, mats)
    if nbytes is None:
        nbytes = _size_query(lib, case)
        assert nbytes == gc.plan_of(lib, case)["workspace_bytes"] > 0
    G = torch.full((batch, n * n + SLACK), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)

    def fresh():
        G.fill_(SENTINEL)
        ws[:nbytes] = 0xFF   # doubles of all ones are NaN: a partial tile summed without having been written shows
        ws[nbytes:] = GUARD_BYTE

    fresh()
    with pytest.raises(_lib.NdmpsHipError, match="workspace"):
        _lib.check(_call(lib, case, ptrs, tables, G, ws, nbytes - 1))
    torch.cuda.synchronize()
    assert bool((G == SENTINEL).all()), "a refused call wrote to G"
    out = []
    for _ in range(2):
        fresh()
        _lib.check(_call(lib, case, ptrs, tables, G, ws, nbytes))
        torch.cuda.synchronize()
        assert bool((G[:, n * n:] == SENTINEL).all()), "wrote behind the n x n part of a G"
        assert bool((ws[nbytes:] == GUARD_BYTE).all()), "wrote behind the workspace it asked for"
        out.append(G[:, :n * n].reshape(batch, n, n).cpu().numpy())
    assert np.array_equal(out[0], out[1]), "two calls must give identical bits"
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0], out[0].transpose(0, 2, 1)), "G must be exactly symmetric"
    del bufs
    return out[0]


@pytest.mark.parametrize("name,switch", gc.variants(), ids=lambda v: str(v))
def test_gram_route(lib, monkeypatch, name, switch):
    case = gc.CASES[name]
    m, batch = case["m"], case["batch"]
    gc.set_switch(monkeypatch, switch)
    # a changed constant of the plan must not move the case off the edge it was chosen for, here either
    facts = gc.facts_of(case, gc.plan_of(lib, case), switch)
    want = dict(case["facts"], **(case["switches"][switch] if switch else {}))
    assert {k: facts.get(k) for k in want} == want

    integer, graded = gc.data(name, "integer"), gc.data(name, "graded")
    G_int = _run(lib, case, [a for a, _ in integer])
    for z in range(batch):
        gc.check_integer(G_int[z], integer[z % gc.DISTINCT][1])
    G = _run(lib, case, [a for a, _, _ in graded])
    worst = 0.0
    for z in range(batch):
        _, ref64, absg = graded[z % gc.DISTINCT]
        worst = max(worst, float((np.abs(G[z] - ref64) / (gc.bar(m) * absg)).max()))
        gc.check_graded(G[z], ref64, absg, m)
    print(f"worst |G - ref64| / (bar |A|^T |A|) = {worst:.3g}")
    if switch == "NDMPS_GRAM_GENERAL=1":
        # the guarded fetch feeds the same MFMAs in the same order over the same slabs
        gc.set_switch(monkeypatch, None)
        assert np.array_equal(G, _run(lib, case, [a for a, _, _ in graded])), "GENERAL must not change a bit"


# ----------------------------------------------------------------------------- refusals
def _refused(lib, case, a, exc=ValueError, nbytes=None):
    bufs, ptrs, tables = _operands(case, [a])
    nbytes = max(_size_query(lib, case), 4096) if nbytes is None else nbytes
    G = torch.full((case["batch"], case["n"] ** 2 + SLACK), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(exc):
        _lib.check(_call(lib, case, ptrs, tables, G, ws, nbytes))
    torch.cuda.synchronize()
    assert bool((G == SENTINEL).all()), "a refused call wrote to G"


def _c(entry, batch, m, n, lda, offset=0, elem="f32"):
    return dict(elem=elem, entry=entry, batch=batch, m=m, n=n, lda=lda, offset=offset, imax=None)


@pytest.mark.parametrize("case", [
    _c("batched", 2, 256, 64, 64, offset=1),            # the stream's 16-byte loads: base off by one element
    _c("batched", 2, 256, 64, 64, offset=2, elem="bf16"),
    _c("batched", 2, 256, 64, 65),                      # ... rows that are no whole number of fours
    _c("gathered", 1, 600, 64, 64, offset=1),           # a gathered operand: misaligned base, one matrix ...
    _c("gathered_batched", 2, 600, 64, 64, offset=1),   # ... on the stream ...
    _c("gathered_batched", 2, 600, 96, 96, offset=1),   # ... on the 64-wide tiles ...
    _c("gathered_batched", 2, 600, 132, 132, offset=1),  # ... and on the 128-wide ones
    _c("batched", 3, 300, 48, 48),                      # shapes without a batched route: too narrow,
    _c("batched", 1, 300, 64, 64),                      # a lone 64-column matrix,
    _c("batched", 2, 255, 128, 128),                    # too short
], ids=lambda c: f"{c['entry']}-{c['elem']}-{c['batch']}x{c['m']}x{c['n']}-ld{c['lda']}-off{c['offset']}")
def test_gram_refuses(lib, case):
    if case["entry"] == "batched" and case["n"] >= 64 and case["m"] >= 256 and case["batch"] >= 2:
        assert gc.ROUTES[gc.plan_of(lib, case)["route"]] == "Stream64"
    elif case["entry"] == "batched":
        assert gc.ROUTES[gc.plan_of(lib, case)["route"]] == "None" and _size_query(lib, case) == 0
    _refused(lib, case, gc.integer_matrix(case["elem"], case["m"], case["n"], 0))


def test_gathered_gram_refuses_columns_that_are_no_whole_fours(lib):
    """n % 4 != 0: the offset tables come in aligned runs of four.  The tables are those of n + 2 columns."""
    for entry, batch in (("gathered", 1), ("gathered_batched", 2)):
        wide = _c(entry, batch, 600, 68, 68)
        row_off, col_off, perm, base_len = gc.gather_tables(600, 68, 0)
        base = _dev(gc.gathered_base(gc.integer_matrix("f32", 600, 68, 0), row_off, col_off, perm, base_len), torch.float32)
        tables = (_dev(row_off), _dev(col_off), _dev(perm))
        case = dict(wide, n=66, lda=66)
        nbytes = max(_size_query(lib, wide), _size_query(lib, case))
        G = torch.full((batch, 68 * 68 + SLACK), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError):
            _lib.check(_call(lib, case, [base.data_ptr()], tables, G, ws, nbytes))
        torch.cuda.synchronize()
        assert bool((G == SENTINEL).all())
