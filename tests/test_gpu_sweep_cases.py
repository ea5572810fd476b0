"""The TT-SVD sweep of csrc/tt.hip on the MI355X, per bond and per core, on the planted-rank cases of
tests/sweep_cases.py and on every route a case names.

Every case runs as its lockstep group through ``NDMPS.from_tensors(volumes, max_bond=cap, cutoff=the case's,
dtype=storage, sweep_from=..., reconstruct=True)``; cores (``mps.cores``), ``sweep_spectra``, the reconstruction,
``boundary_list`` and ``norm_value`` of every member go to ``sweep_cases.check_sweep`` as NumPy arrays -- the comparator
that tests/test_sweep_cases_host.py tests on the CPU, mutations included.

Exact (no tolerance): ``bond_sizes()`` == ``expected_bonds`` on every route; core shapes, dtype, finiteness;
``boundary_list[i]`` == (min, max) of core i as read back; zeros behind the rank in the cap-shaped arena and the cut core
equal to its leading block (two-halves test); the two-halves form bit-identical to the one-call form.  ``norm_value``
equals the Frobenius norm of the norm-carrying core to 4 u.

Bars: quantity q -- the subspace of every bond (sine of the largest principal angle to the fp64 reference's), the
isometry defect of every inner core, the defect of the carrying end against the sweep's OWN basis, the kept singular
values of every bond, the reconstruction against the reference's -- is held to ``MARGIN * Y_q + solver_q``.

* ``Y_q`` = ``sweep_cases.yardstick``: the elementwise maximum, over the model family {SVD route, Gram route} x {carry
  product rounded once, accumulated in the accumulator type in steps of the MFMA's k, the same backwards}, of the
  model's own distance from the reference, floored at u (u s_0 for spectra).  u = 2^-24 (f32), 2^-8 (bf16), 2^-53 (f64).
* ``MARGIN`` = 8 = max(4, 2 R rounded up to a power of two) with R = 3.0: the largest ratio of one quantity between the
  "steps" model summed forwards and backwards, measured on the CPU over all cases (isometry defect of cap32_f64 member 1,
  2 u against 6 u; subspace 2.07 on rank_above_cap; site-0 defect 1.49, spectra 1.80, reconstruction 1.28).  The device's
  tile order is one more realisation of the same rounding process: twice the spread between two realisations is what a
  correct sweep may show.  tests/test_sweep_cases_host.py::test_summation_order_spread_sets_the_margin keeps R below
  MARGIN / 2.  Measured against the model, never against the device.
* ``solver_q`` = ``sweep_cases.solver_terms``, from the eigen-solver's own contract (tests/test_gpu_parity.py::_check_topk:
  residual and orthogonality <= eps(n) = 2e-15 max(n, 50) relative to the largest eigenvalue, n = min(m, n) of the site's
  unfolding): subspace of bond i ``eps / gap2_i`` with gap2_i = (s_k^2 - s_{k+1}^2) / s_0^2 of the reference's spectrum;
  isometry ``eps`` where n <= m (the core is a set of eigenvectors) and ``eps (s_0 / s_k)^2`` where n > m (the core is
  diag(1/s) U^T A); kept value s_j ``eps s_0^2 / s_j``; nothing for the site-0 defect and the reconstruction.  About 1e4 u
  for fp64 storage, below 0.1 u for f32 and bf16.

The route switches change where work is done, not what is computed: the same bars on every route.  DESIGN.md, "Sweep
accuracy per core", holds the measured device / bar ratios.
"""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from imgcompressionmps_amd import NDMPS  # noqa: E402

import sweep_cases as sc  # noqa: E402  (tests/ is on the path: rootdir conftest)

NAMES = list(sc.CASES)
STORE = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
ALL_SWITCHES = sc.SWITCHES + ("NDMPS_EXACT_JACOBI", "NDMPS_NO_FUSED_ENCODE")
SWITCHED = [(n, env) for n in NAMES for env in sc.CASES[n]["routes"]]
FUSED = [n for n in NAMES if "fused encode" in sc.CASES[n]["route"]]
PADDED = [n for n in NAMES if "padded cores" in sc.CASES[n]["route"]]
TWO_HALVES = ["rank_below_cap", "nonuniform_group", "cap32_f32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no HIP device is visible")


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for env in ALL_SWITCHES:
        monkeypatch.delenv(env, raising=False)


def _kwargs(name):
    case = sc.CASES[name]
    return dict(max_bond=case["cap"], cutoff=case["cutoff"], dtype=STORE[case["storage"]], sweep_from=case["sweep_from"])


def _host(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _verify(name, route, member, obj, rec, padded=None):
    """Everything about one member of one run; prints the device / bar ratio of each quantity before it asserts."""
    case = sc.CASES[name]
    x, ref, _ = sc.sweeps(name)[member]
    assert obj.bond_sizes() == sc.expected_bonds(name, member), (name, route, member, obj.bond_sizes())
    cores = obj.mps.cores
    assert all(c.dtype == STORE[case["storage"]] and c.is_cuda for c in cores), (name, route, member)
    assert [tuple(c.shape) for c in cores] == [c.shape for c in ref["cores"]], (name, route, member)
    assert tuple(rec.shape) == case["shape"]
    yard, solver = sc.yardstick(name)[member], sc.solver_terms(name, member)
    args = ([_host(c) for c in cores], obj.sweep_spectra, _host(rec), x, ref, yard, (name, member), sc.MARGIN, solver)
    try:
        got = sc.check_sweep(*args, padded=padded, boundary=obj.boundary_list, norm_value=obj.norm_value)
    except sc.SweepCheckError as err:
        if err.check in ("isometry", "theta", "site0", "spectra", "recon"):
            try:
                got = sc.sweep_quantities(*args[:5], case["sweep_from"])
                print("SWEEP-RATIOS", json.dumps(dict(case=name, route=route, member=member, failed=err.check,
                                                      **sc.worst_ratios(got, yard, sc.MARGIN, solver))))
            except Exception:  # a spectrum too short to compare: the error below says so
                pass
        raise
    print("SWEEP-RATIOS", json.dumps(dict(case=name, route=route, member=member, **sc.worst_ratios(got, yard, sc.MARGIN, solver))))


def _run_group(name, route):
    objs, recs = NDMPS.from_tensors(sc.volumes(name), reconstruct=True, **_kwargs(name))
    assert len(objs) == len(recs) == len(sc.CASES[name]["members"])
    for member, (obj, rec) in enumerate(zip(objs, recs)):
        _verify(name, route, member, obj, rec)
    return objs, recs


@pytest.mark.parametrize("name", NAMES)
def test_sweep_per_core_on_the_default_route(name):
    _run_group(name, "default")


@pytest.mark.parametrize("name,env", SWITCHED, ids=[f"{n}-{e}" for n, e in SWITCHED])
def test_sweep_per_core_under_a_route_switch(name, env, monkeypatch):
    monkeypatch.setenv(env, "1")  # read per call by the library
    _run_group(name, env)


@pytest.mark.parametrize("name", FUSED)
def test_sweep_per_core_without_the_fused_encode(name, monkeypatch):
    monkeypatch.setenv("NDMPS_NO_FUSED_ENCODE", "1")
    _run_group(name, "NDMPS_NO_FUSED_ENCODE")


@pytest.mark.parametrize("name", NAMES)
def test_sweep_per_core_of_a_lone_volume(name):
    """Member 0 through ``from_tensor``: a lone matrix takes other Gram and solver routes than a lockstep group."""
    obj = NDMPS.from_tensor(sc.volumes(name)[0], **_kwargs(name))
    _verify(name, "lone", 0, obj, obj.to_tensor(as_torch=True))


def _two_halves(name):
    """(one-call objects, cap-shaped cores read between the halves [member][site], two-halves objects and
    reconstructions)."""
    want, _ = NDMPS.from_tensors(sc.volumes(name), reconstruct=True, **_kwargs(name))
    pend = NDMPS.from_tensors_begin(sc.volumes(name), reconstruct=True, **_kwargs(name))
    assert pend.asynchronous
    padded = [[_host(c) for c in cores] for cores in pend.arena_cores()]
    objs, recs = pend.result()
    assert pend.arena_cores() is None  # the pending object lets go of the arena with its result
    return want, padded, objs, recs


@pytest.mark.parametrize("name", TWO_HALVES)
def test_two_halves_carry_ranks_below_the_cap(name):
    """``from_tensors_begin(...).result()``: ranks decided on the device travel through the pinned buffers; cores,
    bonds and spectra are bit-identical to ``from_tensors``, and every member meets the bars of the one-call form.
    Between the halves the group's arena holds the cap-shaped cores: the cut core is the leading block, and everything
    behind a member's ranks is exactly zero, as include/ndmps_hip.h documents (the eigenvectors of a Gram matrix with
    zero rows and columns carry rounding noise there; core_from_vectors writes zeros by the right bond's device rank)."""
    case = sc.CASES[name]
    want, padded, objs, recs = _two_halves(name)
    dims = sc.site_dims(case["shape"])
    caps = [1] + [min(case["cap"], int(np.prod(dims[:i])), int(np.prod(dims[i:]))) for i in range(1, len(dims))] + [1]
    assert [p.shape for p in padded[0]] == [(caps[i], dims[i], caps[i + 1]) for i in range(len(dims))]
    if name != "cap32_f32":  # some member stays below a cap, and the ranks on the host say so
        assert any(k < c for o in objs for k, c in zip(o.bond_sizes(), caps[1:-1]))
    for member, (a, b, rec) in enumerate(zip(want, objs, recs)):
        assert a.bond_sizes() == b.bond_sizes() == sc.expected_bonds(name, member)
        assert all(torch.equal(p, q) for p, q in zip(a.mps.cores, b.mps.cores)), (name, member)
        assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a.sweep_spectra, b.sweep_spectra))
        _verify(name, "two halves", member, b, rec, padded=padded[member])


@pytest.mark.parametrize("name", PADDED)
def test_decode_from_the_arena_agrees_with_the_cut_cores(name):
    """``reconstruct=True`` decodes straight from the arena at the cap bonds; ``to_tensors`` decodes the cut cores.  They
    differ by the order of sums with exact zeros only: 4 u relative Frobenius (anything non-zero behind a rank that
    meets a non-zero of its neighbour shows here)."""
    case = sc.CASES[name]
    u = sc.U[case["storage"]]
    objs, recs = NDMPS.from_tensors(sc.volumes(name), reconstruct=True, **_kwargs(name))
    cut = NDMPS.to_tensors(objs, as_torch=True)
    for member, (r, c) in enumerate(zip(recs, cut)):
        r, c = _host(r), _host(c)
        rel = np.linalg.norm(r - c) / np.linalg.norm(c)
        print("ARENA-DECODE", name, member, f"{rel:.3e}", f"bar {4 * u:.3e}")
        assert rel <= 4 * u, (name, member, rel)
