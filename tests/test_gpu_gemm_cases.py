"""Every dense product entry (csrc/gemm.hip, csrc/gemm_bf16.hip) on the MI355X, on the shapes of tests/gemm_cases.py.

Bars, and where they come from (tests/gemm_cases.py has the derivations, tests/test_gemm_cases_host.py shows on the CPU
that they reject a dropped k term, a dropped partial k-tile, a wrong transpose flag, a pad element read as data, an
fp16 partial sum and a truncating bf16 store on every case used here):

* Integer data: ``C == op(A) op(B)`` entry for entry (bf16: the exact integer rounded once to bf16, bit for bit).
  Every partial sum is an integer the accumulator holds exactly, so every order of summation gives the same bits.
* Graded data (rows of op(A) and columns of op(B) scaled from 1 down to 1e-3): ``|C - ref| <= 1.01 k u |op(A)||op(B)|``
  entrywise, ``u = 2**-24`` (fp32) or ``2**-53`` (fp64); bf16: ``1.01 (2**-24 k + 2**-8) |op(A)||op(B)|``.
* ``NDMPS_GEMM_GUARDED=1``, a base pointer off its boundary and a leading dimension that is not tight change how the
  operands are fetched and nothing else: the same LDS contents, the same MFMAs in the same order, the same bits.
* A batched launch gives every member the bits of its single call.

Every launch goes through ``_run``: A and B sit in buffers whose leading elements, pad columns and trailing rows are
NaN; C is a sentinel-filled buffer with ``off_c`` leading elements, ``ldc - n`` pad columns, three trailing rows and
slack; everything outside m x n must hold the sentinel afterwards, everything inside must be finite, and a second call
must give the same bits.  The bf16 workspace of a (k, n) right operand has guard bytes that must survive, and a
workspace one byte short must be refused with C untouched.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import gemm_cases as gm  # noqa: E402
from imgcompressionmps_amd import _lib  # noqa: E402

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
SENTINEL, SLACK, GUARD, GUARD_BYTE, TRAIL = -7.0, 24, 4096, 0xA5, 3
WORST = {}   # elem -> the largest |C - ref| / bar seen in this session


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


@pytest.fixture(autouse=True)
def _switch_off(monkeypatch):
    monkeypatch.delenv(gm.SWITCH, raising=False)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _call(lib, case, pa, pb, pc, ws=None, ws_bytes=0, **over):
    """One call of the case's entry on the device addresses pa / pb / pc (lists, one per member); ``over`` replaces
    arguments (m, n, k, lda, ldb, ldc, batch).  Returns the return code."""
    lda, ldb, ldc = gm.lds(case)
    g = dict(m=case["m"], n=case["n"], k=case["k"], lda=lda, ldb=ldb, ldc=ldc, batch=case["batch"])
    g.update(over)
    sp = _lib.stream_ptr()
    ta, tb, elem = case["ta"], case["tb"], case["elem"]
    if elem == "bf16":
        return lib.ndmps_gemm_bf16(tb, g["m"], g["n"], g["k"], pa[0], g["lda"], pb[0], g["ldb"], pc[0], g["ldc"],
                                   ws.data_ptr() if ws is not None else None, ws_bytes, sp)
    if case["entry"] == "single":
        fn = lib.ndmps_sgemm if elem == "f32" else lib.ndmps_dgemm
        return fn(ta, tb, g["m"], g["n"], g["k"], pa[0], g["lda"], pb[0], g["ldb"], pc[0], g["ldc"], sp)
    fn = lib.ndmps_sgemm_batched if elem == "f32" else lib.ndmps_dgemm_batched
    return fn(g["batch"], ta, tb, g["m"], g["n"], g["k"], _ptr_array(pa), g["lda"], _ptr_array(pb), g["ldb"], _ptr_array(pc),
              g["ldc"], sp)


class _Buffers:
    """The device side of a case on ``pairs`` (the distinct (op(A), op(B)), cycled over the batch)."""

    def __init__(self, lib, case, pairs):
        self.case, dt, e = case, DT[case["elem"]], gm.ESIZE[case["elem"]]
        lda, ldb, ldc = gm.lds(case)
        m, n, batch = case["m"], case["n"], case["batch"]
        self.a, self.b, pa, pb = [], [], [], []
        for d, (a, b) in enumerate(pairs):
            odd = 1 if d == case["odd"] else 0
            self.a.append(_dev(gm.poisoned(gm.stored(a, case["ta"]), lda, TRAIL, case["off_a"] + odd), dt))
            self.b.append(_dev(gm.poisoned(gm.stored(b, case["tb"]), ldb, TRAIL, case["off_b"] + odd), dt))
            assert self.a[-1].data_ptr() % 256 == 0 and self.b[-1].data_ptr() % 256 == 0
            pa.append(self.a[-1].data_ptr() + (case["off_a"] + odd) * e)
            pb.append(self.b[-1].data_ptr() + (case["off_b"] + odd) * e)
        self.pa = [pa[z % len(pairs)] for z in range(batch)]
        self.pb = [pb[z % len(pairs)] for z in range(batch)]
        # one C per member, each on a 256-byte boundary
        self.c_len = case["off_c"] + (m + TRAIL) * ldc + SLACK
        self.c = torch.empty((batch, -(-self.c_len // 128) * 128), dtype=dt, device=DEV)
        assert self.c.data_ptr() % 256 == 0
        self.pc = [self.c[z].data_ptr() + case["off_c"] * e for z in range(batch)]
        self.inside = torch.zeros(self.c.shape[1], dtype=torch.bool, device=DEV)
        self.inside[case["off_c"]:case["off_c"] + m * ldc].view(m, ldc)[:, :n] = True
        self.ws_bytes = int(lib.ndmps_gemm_bf16_workspace_bytes(case["tb"], n, case["k"])) if case["elem"] == "bf16" else 0
        self.ws = torch.empty(self.ws_bytes + GUARD, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        self.fresh()

    def fresh(self):
        self.c.fill_(SENTINEL)
        self.ws[:self.ws_bytes] = 0xFF
        self.ws[self.ws_bytes:] = GUARD_BYTE

    def untouched(self):
        return bool((self.c == SENTINEL).all())

    def result(self):
        """C (batch, m, n) as fp64 on the host, after the checks on everything around it."""
        case = self.case
        assert bool((self.c[:, ~self.inside] == SENTINEL).all()), "wrote outside the m x n part of a C"
        assert bool((self.ws[self.ws_bytes:] == GUARD_BYTE).all()), "wrote behind the workspace it asked for"
        got = self.c[:, self.inside].reshape(case["batch"], case["m"], case["n"])
        assert bool(torch.isfinite(got).all()), "a NaN or an infinity inside C: a pad element was read, or C not written"
        return got.to(torch.float64).cpu().numpy()


def _run(lib, case, pairs):
    """C (batch, m, n) of the case on ``pairs`` with every check of the module docstring around the launch."""
    buf = _Buffers(lib, case, pairs)
    if buf.ws_bytes:
        with pytest.raises(_lib.NdmpsHipError, match="workspace"):
            _lib.check(_call(lib, case, buf.pa, buf.pb, buf.pc, buf.ws, buf.ws_bytes - 1))
        torch.cuda.synchronize()
        assert buf.untouched(), "a refused call wrote to C"
    out = []
    for _ in range(2):
        buf.fresh()
        _lib.check(_call(lib, case, buf.pa, buf.pb, buf.pc, buf.ws, buf.ws_bytes))
        torch.cuda.synchronize()
        out.append(buf.result())
    assert np.array_equal(out[0], out[1]), "two calls must give identical bits"
    return out[0]


@functools.lru_cache(maxsize=None)
def _result(name, kind, guarded=False):
    """C of a case of the table on its ``kind`` data, computed once per session (a case is also the base other cases
    are compared with)."""
    case = gm.CASES[name]
    old = os.environ.pop(gm.SWITCH, None)
    if guarded:
        os.environ[gm.SWITCH] = "1"
    try:
        return _run(_lib.load(), case, [(p[0], p[1]) for p in gm.data(name, kind)])
    finally:
        os.environ.pop(gm.SWITCH, None)
        if old is not None:
            os.environ[gm.SWITCH] = old


@pytest.mark.parametrize("name", gm.small_cases())
def test_gemm_case(name):
    lib = _lib.load()
    case = gm.CASES[name]
    # a changed constant of the plan must not move the case off the path it was chosen for, here either
    facts = gm.facts_of(case, gm.plan_of(lib, case))
    assert {k: facts.get(k) for k in case["facts"]} == case["facts"]

    integer, graded = gm.data(name, "integer"), gm.data(name, "graded")
    c_int, c = _result(name, "integer"), _result(name, "graded")
    worst = 0.0
    for z in range(case["batch"]):
        gm.check_integer(c_int[z], integer[z % gm.DISTINCT][2])
        _, _, ref, bound = graded[z % gm.DISTINCT]
        if case["k"] == 0:
            assert not c[z].any() and not c_int[z].any(), "k = 0: C must be all zeros"
        worst = max(worst, gm.check_graded(c[z], ref, bound))
    WORST[case["elem"]] = max(WORST.get(case["elem"], 0.0), worst)
    print(f"worst |C - ref| / bar = {worst:.3g}  (so far: " + ", ".join(f"{e} {v:.3g}" for e, v in sorted(WORST.items())) + ")")

    if case["entry"] == "batched":
        # every member has the bits of its single call (aligned operands, so on the quads where the shape allows)
        single = dict(case, entry="single", batch=1, odd=None)
        for kind, batched in (("integer", c_int), ("graded", c)):
            pairs = gm.data(name, kind)
            alone = [_run(lib, single, [(p[0], p[1])])[0] for p in pairs]
            for z in range(case["batch"]):
                assert np.array_equal(batched[z], alone[z % gm.DISTINCT]), f"member {z} differs from its single call"
    if case["same_as"]:
        # the same matrices at tight strides and on their boundary: only the fetch path differs
        assert np.array_equal(c[0], _result(case["same_as"], "graded")[0])
        assert np.array_equal(c_int[0], _result(case["same_as"], "integer")[0])


@pytest.mark.parametrize("name", gm.guarded_cases())
def test_guarded_fetch_gives_the_same_bits(name):
    for kind in ("integer", "graded"):
        assert np.array_equal(_result(name, kind, guarded=True), _result(name, kind)), f"{gm.SWITCH} changed {kind} bits"


@pytest.mark.parametrize("a_mode,c_mode", [("dense", "dense"), ("vec4", "scattered")])
def test_indexed_entries_under_the_guarded_fetch(monkeypatch, a_mode, c_mode):
    """ndmps_sgemm_indexed reads the same switch: 200 x 132 x 132 runs the 128-wide tile on quads, one row block on
    the straight-line fetch by default."""
    from test_gpu_decode_reference import _indexed_case

    got = {}
    for guarded in (0, 1):
        if guarded:
            monkeypatch.setenv(gm.SWITCH, "1")
        c, a, b = _indexed_case(200, 132, 132, a_mode, c_mode, np.random.default_rng(7))
        got[guarded] = c
        assert np.all(np.abs(c.reshape(200, 132) - a @ b) <= gm.cb.gemm_bound(a, b, gm.cb.U_F32))
    assert np.array_equal(got[0], got[1])


# ----------------------------------------------------------------------------- the fold
def test_bf16_fold_into_two_launches():
    """m = 65535 * 128 + 1: the second launch starts 65535 tiles into A and C.  Integers up to 5, so C is the integer
    matrix itself (k imax**2 = 200 < 2**8).  The first tile, both sides of the fold and the last row are compared in
    full, every row by its sum."""
    lib = _lib.load()
    case = gm.CASES[gm.FOLD]
    m, n, k = case["m"], case["n"], case["k"]
    plan = gm.plan_of(lib, case)
    assert {s: plan[s] for s in case["facts"]} == case["facts"]
    b = gm.fold_b()
    sums = np.empty(m, dtype=np.int64)
    d_a = torch.empty((m, k), dtype=torch.bfloat16, device=DEV)
    step = 1 << 20
    for r0 in range(0, m, step):   # built in int8, a chunk at a time
        rows = gm.fold_rows(np.arange(r0, min(m, r0 + step)))
        sums[r0:r0 + step] = (rows.astype(np.float32) @ b.astype(np.float32).T).sum(axis=1).astype(np.int64)
        d_a[r0:r0 + step] = torch.from_numpy(rows).to(DEV).to(torch.bfloat16)
    d_b = _dev(b, torch.bfloat16)
    d_c = torch.full((m + 1, n), SENTINEL, dtype=torch.bfloat16, device=DEV)
    for _ in range(2):
        _lib.check(lib.ndmps_gemm_bf16(1, m, n, k, d_a.data_ptr(), k, d_b.data_ptr(), k, d_c.data_ptr(), n, None, 0,
                                       _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((d_c[m] == SENTINEL).all()), "wrote behind the last row"
        rows = gm.fold_checked_rows()
        want = gm.fold_rows(rows).astype(np.int64) @ b.astype(np.int64).T
        got = d_c[torch.from_numpy(rows).to(DEV)].to(torch.float64).cpu().numpy()
        gm.check_integer(got, want.astype(np.float64))
        got_sums = torch.cat([d_c[r0:min(m, r0 + step)].to(torch.int32).sum(dim=1) for r0 in range(0, m, step)])
        got_sums = got_sums.cpu().numpy()
        bad = np.flatnonzero(got_sums != sums)
        assert bad.size == 0, f"{bad.size} rows have a wrong sum, first row {bad[0]}"
        d_c[:m] = SENTINEL


# ----------------------------------------------------------------------------- refusals and empty products
def _refusal_case(elem, ta, tb, entry="single", batch=1):
    m, n, k = 20, 12, 16
    return dict(elem=elem, entry=entry, batch=batch, ta=ta, tb=tb, m=m, n=n, k=k, lda=0, ldb=0, ldc=0, off_a=0, off_b=0,
                off_c=0, odd=None)


def _refused(lib, case, exc=ValueError, null=None, **over):
    a, b = gm.draw(case, "integer", 0)
    buf = _Buffers(lib, dict(case, batch=1), [(a, b)])
    batch = over.get("batch", case["batch"])
    pa, pb, pc = ([p[0]] * max(batch, 1) for p in (buf.pa, buf.pb, buf.pc))
    if null == "a":
        pa = [None] * len(pa)
    if null == "b":
        pb = [None] * len(pb)
    if null == "c":
        pc = [None] * len(pc)
    with pytest.raises(exc):
        _lib.check(_call(lib, case, pa, pb, pc, buf.ws, buf.ws_bytes, **over))
    torch.cuda.synchronize()
    assert buf.untouched(), "a refused call wrote to C"


@pytest.mark.parametrize("elem", ["f32", "f64", "bf16"])
def test_gemm_refuses(elem):
    lib = _lib.load()
    for ta in ((0,) if elem == "bf16" else (0, 1)):
        for tb in (0, 1):
            case = _refusal_case(elem, ta, tb)
            lda, ldb, ldc = gm.lds(case)
            # a leading dimension one below the row length, for each of A, B and C
            _refused(lib, case, lda=lda - 1)
            _refused(lib, case, ldb=ldb - 1)
            _refused(lib, case, ldc=ldc - 1)
            for null in "abc":
                _refused(lib, case, null=null)
            for bad in (dict(m=-1), dict(n=-1), dict(k=-1)):
                _refused(lib, case, **bad)
            if elem == "bf16":
                for bad in (dict(k=0), dict(m=0), dict(n=0)):   # the bf16 entry takes no empty extent
                    _refused(lib, case, **bad)
                continue
            batched = _refusal_case(elem, ta, tb, "batched", 2)
            _refused(lib, batched, batch=0)
            _refused(lib, batched, batch=65)
            _refused(lib, batched, null="b")
            _refused(lib, batched, ldc=ldc - 1)
            _refused(lib, batched, m=-1)


@pytest.mark.parametrize("elem", ["f32", "f64"])
def test_empty_products_write_nothing(elem):
    lib = _lib.load()
    for entry, batch in (("single", 1), ("batched", 2)):
        case = _refusal_case(elem, 0, 0, entry, batch)
        a, b = gm.draw(case, "integer", 0)
        buf = _Buffers(lib, case, [(a, b)])
        for over in (dict(m=0), dict(n=0), dict(m=0, n=0, k=0)):
            assert _call(lib, case, buf.pa, buf.pb, buf.pc, **over) == _lib.OK
            torch.cuda.synchronize()
            assert buf.untouched()
