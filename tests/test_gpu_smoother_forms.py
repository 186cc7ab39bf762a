"""The Chebyshev smoother forms, the V-cycle and PCG at every degree p = 1..9 on each schedule of the brick loop, against
the oracle, with the fused transfer forms switched off one by one; the fp32 forms against the oracle's fp32 mode; the
second pipeline of the eight-colour schedule (mgx_macro2.hip) against the first.

The finest level has 8 bricks at every degree (p <= 4: 512 cells, p >= 5: 64 cells), so the fused residual +
restriction (profile form 7) and the prolongation form of the first post-smoothing step (form 9) have bricks to run
on.  Which of them ran on the finest level is read from mgx_profile_read and asserted for every V-cycle:
  * residual + restriction: fused unless no_fused_restrict; on the one-launch schedule only in its scratch form
    (off with no_restrict_scratch);
  * prolongation: fused on the eight-colour schedule and, at p > 4 or with fused_prolong_min_bricks = 0, on the
    two-class one; never on the one-launch schedule, nor without the restriction's block table or with
    no_fused_prolong.
Tolerances (fp64) as tests/test_gpu_parity.py: 1e-10 for a smoother application, 1e-9 for a V-cycle, the PCG history
through assert_same_cg."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle_view import assert_same_cg, oracle_for  # noqa: E402

# the overrides of tests/test_gpu_schedules.py: eight colour launches / two classes / one launch on every level
SCHEDULES = {"eight": {"MGX_FREE_MAX_BRICKS": "0"},
             "two": {"MGX_FREE_MAX_BRICKS": "4000000000", "MGX_FREE_ONE_MAX": "0"},
             "one": {"MGX_FREE_MAX_BRICKS": "4000000000", "MGX_FREE_ONE_MAX": "4000000000"}}
TOGGLES = [{}, {"no_fused_restrict": 1}, {"no_fused_prolong": 1}, {"no_restrict_scratch": 1}, {"fused_prolong_min_bricks": 0}]
FORM_RESTRICT, FORM_PROLONG = 7, 9


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def mesh_of(p):
    return (1, 3) if p <= 4 else (1, 2)


_cubes, _oracles, _refs = {}, {}, {}


def cube_of(p):
    if p not in _cubes:
        _cubes[p] = mg.Cube(p, *mesh_of(p))
    return _cubes[p]


def oracle_of(p, vfloat=False):
    if (p, vfloat) not in _oracles:
        _oracles[(p, vfloat)] = oracle_for(cube_of(p), p, *mesh_of(p), degree=3, n_cycles=1, vfloat=vfloat)
    return _oracles[(p, vfloat)]


def refs_of(p, vfloat=False):
    """inputs and the oracle's smoother / V-cycle results on the finest level (computed once per degree)"""
    if (p, vfloat) not in _refs:
        cube, orc = cube_of(p), oracle_of(p, vfloat)
        l = cube.max_level
        x, b = cube.seeded_vector(l, 21), cube.seeded_vector(l, 22)
        if vfloat:
            x, b = x.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        x1 = orc.cheb_vmult(l, b)
        _refs[(p, vfloat)] = dict(x=x, b=b, vmult=x1, step=orc.cheb_step(l, x1, b), vcycle=orc.vcycle(x))
    return _refs[(p, vfloat)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for o in _oracles.values():
        o.close()
    for c in _cubes.values():
        c.close()
    _oracles.clear()
    _cubes.clear()
    _refs.clear()


def expect_fused(schedule, opts, p):
    restrict = not opts.get("no_fused_restrict") and not (schedule == "one" and opts.get("no_restrict_scratch"))
    prolong = (not opts.get("no_fused_restrict") and not opts.get("no_fused_prolong") and schedule != "one" and
               (schedule == "eight" or p > 4 or opts.get("fused_prolong_min_bricks", 8192) <= 8))
    return restrict, prolong


def smoother_forms(ctx, solver, l, r, vnum, tol, orc=None):
    """smoother.vmult (zero start) and smoother.step of the finest level against the oracle; returns both results"""
    sm = solver.smoother(l)
    if orc is not None:
        gi, oi = sm.info(), orc.cheb_info(l)
        assert gi["degree"] == oi["degree"] and gi["cg_its"] == oi["cg_its"], (gi, oi)
        for k in ("lambda_max", "theta", "delta"):
            assert gi[k] == pytest.approx(oi[k], rel=1e-8 if vnum == mg.F64 else 1e-4), (k, gi, oi)
    bd, xd = ctx.vector(r["b"].size, vnum, r["b"]), ctx.vector(r["b"].size, vnum)
    sm.vmult(xd, bd)
    x1 = xd.download()
    assert rel(x1.astype(np.float64), r["vmult"]) < tol, "smoother.vmult: %g" % rel(x1.astype(np.float64), r["vmult"])
    sm.step(xd, bd)
    x2 = xd.download()
    assert rel(x2.astype(np.float64), r["step"]) < tol, "smoother.step: %g" % rel(x2.astype(np.float64), r["step"])
    return x1, x2


def vcycle_with_profile(ctx, solver, l, r, tol):
    """one V-cycle against the oracle; returns it and the launches of the fused forms on the finest level"""
    A = solver.matrix(l)
    ctx.profile_enable(True)
    A.set_profiled(True)
    ctx.profile_read(FORM_RESTRICT)
    ctx.profile_read(FORM_PROLONG)
    x = r["x"]
    xd, yd = ctx.vector(x.size, data=x), ctx.vector(x.size, data=np.full(x.size, np.nan))
    solver.vmult(yd, xd)
    y = yd.download()
    n7, n9 = ctx.profile_read(FORM_RESTRICT)[0], ctx.profile_read(FORM_PROLONG)[0]
    A.set_profiled(False)
    ctx.profile_enable(False)
    assert rel(y, r["vcycle"]) < tol, "V-cycle: %g" % rel(y, r["vcycle"])
    return y, n7, n9


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("p", range(1, 10))
def test_smoother_vcycle_pcg_on_every_schedule(monkeypatch, p, schedule):
    """Chebyshev parameters, smoother.vmult, smoother.step, one V-cycle and the PCG history against the oracle; then the
    V-cycle again with each fused transfer form switched off (or, fused_prolong_min_bricks = 0, on), against the oracle,
    with the fused forms that ran checked against the ones the case expects"""
    for k, v in SCHEDULES[schedule].items():
        monkeypatch.setenv(k, v)
    cube, orc, r = cube_of(p), oracle_of(p), refs_of(p)
    l = cube.max_level
    for opts in TOGGLES:
        ctx = mg.Context(0, options=opts)
        solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
        try:
            if not opts:
                smoother_forms(ctx, solver, l, r, mg.F64, 1e-10, orc)
            _, n7, n9 = vcycle_with_profile(ctx, solver, l, r, 1e-9)
            restrict, prolong = expect_fused(schedule, opts, p)
            assert (n7 > 0) == restrict, "%s %s: fused residual + restriction launches %d" % (schedule, opts, n7)
            assert (n9 > 0) == prolong, "%s %s: fused prolongation launches %d" % (schedule, opts, n9)
            if not opts:
                assert_same_cg(solver, orc)
        finally:
            solver.close()
            ctx.close()


@pytest.mark.parametrize("p", range(1, 10))
def test_fp32_smoother_forms_and_vcycle(monkeypatch, p):
    """fp32 V-cycle hierarchy (the reference's default) against the oracle in its fp32 mode, on each schedule.
    Chebyshev parameters: both sides estimate them from 15 CG iterations with fp32 operator applications; a relative
    perturbation e of the operator moves a Ritz value by at most e |A| (Weyl), e ~ k u with u = 2^-24 and k ~ 100 terms
    per row of a sweep-factorised application at p <= 9, accumulated over the 15 iterations: 1e-4.  Forms: the fp32
    tolerances of tests/test_gpu_schedules.py -- 5e-5 for a smoother application (two or three fp32 operator
    applications and vector updates), 2e-4 for the V-cycle."""
    cube, orc, r = cube_of(p), oracle_of(p, vfloat=True), refs_of(p, vfloat=True)
    l = cube.max_level
    for schedule, env in SCHEDULES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = mg.Context(0)
        solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F32)
        try:
            smoother_forms(ctx, solver, l, r, mg.F32, 5e-5, orc)
            xd, yd = ctx.vector(r["x"].size, data=r["x"]), ctx.vector(r["x"].size)
            solver.vmult(yd, xd)
            assert rel(yd.download(), r["vcycle"]) < 2e-4, "%s: V-cycle %g" % (schedule, rel(yd.download(), r["vcycle"]))
        finally:
            solver.close()
            ctx.close()


@pytest.mark.parametrize("p", range(1, 10))
def test_second_pipeline_of_the_chebyshev_and_restriction_forms(p):
    """Eight colour launches (free_max_bricks = 0): the second pipeline (mgx_macro2.hip) runs the Chebyshev forms that
    never store the first iterate (kChebInit at p <= 4, kChebOldInit) and the fused residual + restriction (p <= 4),
    the first pipeline (option no_macro_v2) all of them.  smoother.vmult, smoother.step and the V-cycle against the
    oracle with each, and BITWISE against each other: both form the same sweeps (sliced or not: the slices split the
    work, not the sums) and the same update f0 * d * b from the same per-item diagonal table, in the same order."""
    cube, orc, r = cube_of(p), oracle_of(p), refs_of(p)
    l = cube.max_level
    out = []
    for opts in ({"free_max_bricks": 0}, {"free_max_bricks": 0, "no_macro_v2": 1}):
        ctx = mg.Context(0, options=opts)
        solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
        try:
            x1, x2 = smoother_forms(ctx, solver, l, r, mg.F64, 1e-10)
            y, n7, _ = vcycle_with_profile(ctx, solver, l, r, 1e-9)
            assert n7 > 0, "%s: the fused residual + restriction did not run" % opts
            out.append((x1, x2, y))
        finally:
            solver.close()
            ctx.close()
    for name, a, e in zip(("smoother.vmult", "smoother.step", "V-cycle"), out[0], out[1]):
        assert np.array_equal(a, e), "%s: pipelines differ by %g" % (name, rel(a, e))
