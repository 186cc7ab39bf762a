"""Solution-dependent coefficients on quadrilaterals on the GPU (MinimalSurfaceOperator and LaplaceProblem::solve of
minimal_surface/program.cc with dimension = 2; mgx_nonlinear_2d.hip): coefficient evaluation, nonlinear residual, state
interpolation, the refresh of a whole hierarchy and the Newton solve on the square, the sheared square and the annulus
sector with curved cells, against the numpy restatement tests/nonlinear_reference_2d.py (pinned on the CPU by
test_nonlinear_reference_2d.py).

Bounds.  fp64: 1e-12 of the maximum norm, the bound of test_gpu_nonlinear.py.  fp32: ten times the distance of the numpy
law evaluated in float32 on the same inputs from the fp64 one (the rule of DESIGN.md, "Solution-dependent coefficients"),
computed per case and printed next to the device's figure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import nonlinear_reference_2d as nr2  # noqa: E402
from test_nonlinear_reference_2d import NEWTON_CASES_2D, boundary_state, make_square, reference  # noqa: E402

_lib = mg._lib
UNSUPPORTED = -4
DEGREES = [1, 2, 3, 4, 5, 8]
LAWS = [mg.LAW_UNIT, mg.LAW_MINIMAL_SURFACE]
# (coarse cells x, y, n_refine): 6 x 4 cells (an x / y mix-up shows) and 17 x 11 cells (several workgroups, the last one
# partial at every degree)
MESHES = {"6x4": (3, 2, 1), "17x11": (17, 11, 0)}
# how the operator is told its geometry: one metric per level, or JxW_q J^-1 J^-T and JxW_q of every point
PATHS = {"square": ["affine"], "sheared": ["affine", "per_point"], "sector": ["per_point"]}
NUMBERS = ((mg.F64, np.float64), (mg.F32, np.float32))


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def colour_ctx():
    """no ordered assembly: one launch per cell colour"""
    c = mg.Context(0, options=dict(cell_colour_min=1))
    yield c
    c.close()


def rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


def smooth_state(sq, l):
    """not symmetric in x and y"""
    x = sq.dof_coordinates(l)
    return 0.6 * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])) * np.cos(1.3 * x[:, 1]) + 0.2 * x[:, 0] ** 2 + 0.1 * sq.seeded_vector(l, 11)


def general_operator(ctx, sq, l, number, path, coef_q=None):
    op = mg.LaplaceOperator.from_cube(ctx, sq, l, number, coef_q=sq.unit_law_coefficient(l) if coef_q is None else coef_q)
    if path == "affine":
        op.enable_coefficient_update(*sq.affine_metric(l))
    else:
        op.enable_coefficient_update_q(sq.unit_q(l), sq.jxw_q(l))
    return op


def check_against_numpy(what, got, evaluate, u, dt):
    """got: the device's result in dt from the state u (rounded to dt); evaluate(state, dtype): the numpy law"""
    state = u.astype(dt).astype(np.float64)
    want = evaluate(state, np.float64)
    err = rel(got, want)
    if dt == np.float64:
        print("%s f64: %.3e (bound 1e-12)" % (what, err))
        assert err < 1e-12
    else:
        bound = 10 * rel(evaluate(state, np.float32), want)
        print("%s f32: %.3e (numpy float32 x 10: %.3e)" % (what, err, bound))
        assert err <= bound
    return want


@pytest.mark.parametrize("geometry", list(PATHS))
@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("p", DEGREES)
def test_evaluate_coefficient(ctx, p, mesh, geometry):
    """the downloaded coef_q of both laws against numpy; an operator refreshed on the device against one created through
    desc.coef_q from the numpy tensor: vmult, vmult_residual, inverse diagonal"""
    sq = make_square(geometry, p, box=MESHES[mesh])
    l = sq.max_level
    u, x, b = smooth_state(sq, l), sq.seeded_vector(l, 1), sq.seeded_vector(l, 2)
    tensors = {}
    for path in PATHS[geometry]:
        ref = reference(sq, l, affine=path == "affine")
        for number, dt in NUMBERS:
            op = general_operator(ctx, sq, l, number, path)
            state = ctx.vector(u.size, number, u.astype(dt))
            for law in LAWS:
                op.evaluate_coefficient(law, state)
                got = op.get_coefficient().download().reshape(sq.n_cells(l), 3, -1)
                want = check_against_numpy("p=%d %s %s %s law %d: coef_q" % (p, mesh, geometry, path, law), got,
                                           lambda s, t: ref.coefficient(law, s, t), u, dt)
                if number != mg.F64:
                    continue
                tensors[path, law] = got
                made = general_operator(ctx, sq, l, number, path, coef_q=want)
                src, rhs = ctx.vector(x.size, data=x), ctx.vector(x.size, data=b)
                out = []
                for o in (op, made):
                    dst, res = ctx.vector(x.size), ctx.vector(x.size)
                    o.vmult(dst, src)
                    o.vmult_residual(rhs, src, res)
                    o.compute_diagonal()
                    out.append((dst.download(), res.download(), o.get_matrix_diagonal_inverse().download()))
                for g, w in zip(*out):
                    assert rel(g, w) < 1e-12
                assert rel(out[0][0], ref.apply(want, x)) < 1e-12
                made.clear()
            op.clear()
    if geometry == "sheared":  # the per-point path of affine cells is the affine path
        for law in LAWS:
            assert rel(tensors["per_point", law], tensors["affine", law]) < 1e-13
    sq.close()


@pytest.mark.parametrize("geometry", list(PATHS))
@pytest.mark.parametrize("mesh,route", [("6x4", "ordered"), ("17x11", "ordered"), ("17x11", "colour")])
@pytest.mark.parametrize("p", DEGREES)
def test_compute_nonlinear_residual(ctx, colour_ctx, p, mesh, route, geometry):
    """against numpy; two calls bitwise equal; constrained rows exactly zero; the unit law is -A u of the linear operator
    through vmult; the per-point path of the sheared square is the affine one"""
    c = colour_ctx if route == "colour" else ctx
    sq = make_square(geometry, p, box=MESHES[mesh])
    l = sq.max_level
    u = smooth_state(sq, l)
    cons = sq.constrained(l)
    results = {}
    for path in PATHS[geometry]:
        ref = reference(sq, l, affine=path == "affine")
        for number, dt in NUMBERS:
            op = general_operator(c, sq, l, number, path)
            state = c.vector(u.size, number, u.astype(dt))
            for law in LAWS:
                dst, again = c.vector(u.size, number), c.vector(u.size, number)
                again.upload(np.full(u.size, 3.0, dtype=dt))
                op.compute_nonlinear_residual(law, dst, state)
                op.compute_nonlinear_residual(law, again, state)
                got = dst.download()
                assert np.array_equal(got, again.download())               # reproducible assembly
                assert np.array_equal(got[cons], np.zeros(cons.size, dt))  # constrained rows exactly zero
                check_against_numpy("p=%d %s %s %s %s law %d: residual" % (p, mesh, route, geometry, path, law), got,
                                    lambda s, t: ref.residual(law, s, t), u, dt)
                if number == mg.F64:
                    results[path, law] = got
                if law == mg.LAW_UNIT and number == mg.F64:
                    # A u of the linear operator without constraints (its table of constrained entities is the plain one):
                    # the boundary values of u contribute, as they do to the residual
                    d = sq.operator_desc(l)
                    unit = np.ascontiguousarray(sq.unit_law_coefficient(l))
                    d.idx27, d.n_constrained, d.coef_q = d.idx27_plain, 0, unit.ctypes.data_as(_lib.f64p)
                    lin, au = mg.LaplaceOperator(c, d), c.vector(u.size)
                    lin.vmult(au, state)
                    free = np.setdiff1d(np.arange(u.size), cons)
                    assert rel(got[free], -au.download()[free]) < 1e-12
                    lin.clear()
            op.clear()
    if geometry == "sheared":
        for law in LAWS:
            assert rel(results["per_point", law], results["affine", law]) < 1e-13
    sq.close()


@pytest.mark.parametrize("geometry", ["square", "sector"])
@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("p", DEGREES)
def test_interpolate_to_coarse(ctx, p, mesh, geometry):
    """every coarse entry is written (the coarse vector starts as NaN), to 1e-13 of numpy; a polynomial of degree <= p
    in the coordinates of the box is reproduced"""
    sx, sy, _ = MESHES[mesh]
    sq = make_square(geometry, p, box=(sx, sy, 1 if mesh == "17x11" else 2))
    solver = mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, general=True)
    R = nr2.interpolation_matrix_1d(sq.gll())
    box = make_square("square", p, box=(sx, sy, sq.max_level))   # (the box coordinates, for the polynomial)
    f = lambda x: (1 + x[:, 0] - 0.5 * x[:, 0] ** p) * (2 - x[:, 1] ** p + 0.3 * x[:, 1])
    for l in range(1, sq.n_levels):
        for u, want_coarse in ((smooth_state(sq, l), None), (f(box.dof_coordinates(l)), f(box.dof_coordinates(l - 1)))):
            nc = sq.n_dofs(l - 1)
            fine = ctx.vector(u.size, data=u)
            coarse, again = ctx.vector(nc, data=np.full(nc, np.nan)), ctx.vector(nc, data=np.full(nc, np.nan))
            tr = solver.transfer_dp(l)
            tr.interpolate_to_coarse(coarse, fine)
            tr.interpolate_to_coarse(again, fine)
            want = nr2.interpolate_to_coarse(R, sq.children(l), nr2.cell_dofs(sq.idx9_plain(l), p),
                                             nr2.cell_dofs(sq.idx9_plain(l - 1), p), nc, u)
            got = coarse.download()
            assert not np.isnan(got).any()
            assert np.array_equal(got, again.download())
            assert np.abs(got - want).max() < 1e-13
            if want_coarse is not None:
                assert np.abs(got - want_coarse).max() < 1e-12 * max(1.0, np.abs(want_coarse).max())
    solver.close()
    box.close()
    sq.close()


@pytest.mark.parametrize("geometry", ["square", "sector"])
@pytest.mark.parametrize("vnumber", [mg.F64, mg.F32])
@pytest.mark.parametrize("p", [2, 4])
def test_update_coefficient_of_a_hierarchy(ctx, p, vnumber, geometry):
    """after update_coefficient the solver is the solver created from scratch with the numpy tensors of every level; a
    second call with another state matches the from-scratch solver of that state (no stale graph, diagonal, eigenvalues);
    the tensor of an fp32 V-cycle operator is the fp64 tensor of its level, rounded"""
    sq = make_square(geometry, p, 2)  # 3 levels
    lmax = sq.max_level
    R = nr2.interpolation_matrix_1d(sq.gll())
    refs = [reference(sq, l, affine=geometry != "sector") for l in range(sq.n_levels)]
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, vnumber, general=True)
    x = sq.seeded_vector(lmax, 5)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    solver.vmult(dst, src)  # (a V-cycle before the first refresh: the coarse levels' graph exists from here on)
    solver.vmult(dst, src)
    for k, u in enumerate((smooth_state(sq, lmax), 0.5 * sq.seeded_vector(lmax, 3) + boundary_state(sq, lmax, 1.0))):
        states = [None] * sq.n_levels
        states[lmax] = u
        for l in range(lmax, 0, -1):
            states[l - 1] = nr2.interpolate_to_coarse(R, sq.children(l), nr2.cell_dofs(sq.idx9_plain(l), p),
                                                      nr2.cell_dofs(sq.idx9_plain(l - 1), p), sq.n_dofs(l - 1), states[l])
        tensors = [refs[l].coefficient(mg.LAW_MINIMAL_SURFACE, states[l]) for l in range(sq.n_levels)]
        scratch = mg.MultigridSolver(ctx, sq, 3, 3, 1, vnumber, general=True, coef_q=tensors)
        state = ctx.vector(u.size, data=u)
        solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, state)
        want = ctx.vector(x.size)
        for _ in range(3):  # (the third V-cycle replays the captured graph)
            solver.vmult(dst, src)
            scratch.vmult(want, src)
            err = rel(dst.download(), want.download())
            print("p=%d %s vcycle %s state %d: V-cycle %.3e" % (p, geometry, "f64" if vnumber == mg.F64 else "f32", k, err))
            assert err < 1e-9
        for l in range(sq.n_levels):
            a, b = solver.smoother(l).info(), scratch.smoother(l).info()
            assert a["degree"] == b["degree"]
            assert a["lambda_max"] == pytest.approx(b["lambda_max"], rel=1e-8)
            if vnumber == mg.F32:
                t64 = solver.matrix_dp(l).get_coefficient().download()
                assert rel(t64, tensors[l].ravel()) < 1e-12
                assert np.array_equal(solver.matrix(l).get_coefficient().download(), t64.astype(np.float32))
        scratch.close()
    solver.close()
    sq.close()


@pytest.mark.parametrize("vnumber", [mg.F32, mg.F64])
@pytest.mark.parametrize("case", sorted(NEWTON_CASES_2D))
def test_newton_solve(ctx, case, vnumber):
    """MinimalSurfaceProblem on the cases of test_nonlinear_reference_2d.py::test_newton_with_exact_linear_solves: every
    accepted step lowers the residual norm; 1e-6 of the first norm after N6 or N6 + 1 steps, 1e-10 at most 2 steps later;
    the converged state is the numpy Newton state to 1e-8 (maximum norm, relative).  Measured on an MI355X: see the
    Newton table of DESIGN.md (section "Solution-dependent coefficients in two dimensions")."""
    geometry, p, n_refine, amplitude = case
    sq = make_square(geometry, p, n_refine)
    l = sq.max_level
    problem = mg.MinimalSurfaceProblem(ctx, sq, lambda x: amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])), vnumber)
    first = None
    norms = []
    for step in range(12):
        initial, final = problem.solve(step == 0)
        if step == 0:
            first = initial
            norms.append(initial)
        assert final < initial
        norms.append(final)
        if final < 1e-10 * first:
            break
    cg = [h[3] for h in problem.history]
    print("%s p=%d %d^2 cells A=%g vcycle %s: norms %s, CG iterations %s"
          % (geometry, p, 2 ** n_refine, amplitude, "f32" if vnumber == mg.F32 else "f64", " -> ".join("%.2e" % r for r in norms), cg))
    n6, n10 = nr2.steps_to(norms, 1e-6), nr2.steps_to(norms, 1e-10)
    assert n6 in (NEWTON_CASES_2D[case], NEWTON_CASES_2D[case] + 1)
    assert n10 is not None and n10 <= n6 + 2
    u_ref, _, _ = reference(sq, l, affine=geometry != "sector").newton(boundary_state(sq, l, amplitude), max_steps=12,
                                                                       tolerance=1e-10 * first)
    diff = rel(problem.solution.download(), u_ref)
    print("    state against the numpy Newton state: %.3e" % diff)
    assert diff < 1e-8
    problem.close()
    sq.close()


def status_of(call):
    status = call()
    return status, _lib.load().mgx_last_error().decode()


def test_refusals_and_lifetime(ctx):
    """the _2d calls on a 3D operator, the 3D calls on a 2D operator, an operator, transfer or solver that was not
    enabled, an operator without coef_q: MGX_ERR_UNSUPPORTED with a reason; nothing stays allocated after them or
    after a create - refresh - solve - close cycle"""
    lib = _lib.load()
    start = lib.mgx_live_device_allocations()
    f64p = _lib.f64p

    def refused(status_and_reason, word=None):
        status, reason = status_and_reason
        assert status == UNSUPPORTED and reason
        assert word is None or word in reason, reason

    sq, cube = mg.Square(2, 1, 2), mg.Cube(2, 1, 1)
    l = sq.max_level
    three, six = (C.c_double * 3)(1, 1, 0), (C.c_double * 6)(1, 1, 1, 0, 0, 0)
    ones = np.ones(max(sq.n_cells(l) * 6 * 27, cube.n_cells(1) * 6 * 27))
    op3 = mg.LaplaceOperator.from_cube(ctx, cube, 1, coef_q=cube.unit_law_coefficient(1))
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_2d(op3.h, three, 1.0)), "three-dimensional")
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_q_2d(op3.h, ones.ctypes.data_as(f64p),
                                                                              ones.ctypes.data_as(f64p))), "three-dimensional")
    op3.clear()
    op2 = mg.LaplaceOperator.from_cube(ctx, sq, l, coef_q=sq.unit_law_coefficient(l))
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update(op2.h, six, 1.0)), "_2d")
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_q(op2.h, ones.ctypes.data_as(f64p),
                                                                           ones.ctypes.data_as(f64p))), "_2d")
    v, w = ctx.vector(sq.n_dofs(l)), ctx.vector(sq.n_dofs(l))
    refused(status_of(lambda: lib.mgx_evaluate_coefficient(op2.h, 0, v.ptr)), "_2d")
    refused(status_of(lambda: lib.mgx_compute_nonlinear_residual(op2.h, 1, v.ptr, w.ptr)), "_2d")
    # bad geometry: invalid argument, and the operator stays not enabled
    bad = (C.c_double * 3)(1, 1, 2)
    assert lib.mgx_operator_enable_coefficient_update_2d(op2.h, bad, 1.0) == -1
    assert lib.mgx_operator_enable_coefficient_update_2d(op2.h, three, -1.0) == -1
    neg = -np.ones(sq.n_cells(l) * 3 * 9)
    assert lib.mgx_operator_enable_coefficient_update_q_2d(op2.h, neg.ctypes.data_as(f64p), ones.ctypes.data_as(f64p)) == -1
    refused(status_of(lambda: lib.mgx_evaluate_coefficient(op2.h, 0, v.ptr)))
    op2.clear()
    plain = mg.LaplaceOperator.from_cube(ctx, sq, l)   # no coef_q
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_2d(plain.h, three, 1.0)), "coef_q")
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_q_2d(plain.h, ones.ctypes.data_as(f64p),
                                                                              ones.ctypes.data_as(f64p))), "coef_q")
    plain.clear()
    # a per-point hierarchy that was not enabled
    solver = mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, per_point=True)
    coarse = ctx.vector(sq.n_dofs(l - 1))
    refused(status_of(lambda: lib.mgx_interpolate_to_coarse(solver.transfer_dp(l).h, coarse.ptr, v.ptr)))
    refused(status_of(lambda: lib.mgx_solver_update_coefficient(solver.h, 0, v.ptr)))
    x = sq.seeded_vector(l, 1)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    solver.vmult(dst, src)   # still a solver
    assert np.abs(dst.download()).max() > 0
    solver.close()
    # what stays refused in two dimensions on an enabled hierarchy
    general = mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F32, general=True)
    refused(status_of(lambda: lib.mgx_compute_residual(general.matrix_dp(l).h, v.ptr, w.ptr, None)))
    refused(status_of(lambda: lib.mgx_solver_compute_rhs(general.h, l, None)))
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, general=True, comm=object())
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, general=True, agglomerate=False)
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, general=True, device_rhs=True)
    # replace-while-alive: per-point geometry over the affine one and back, results as with the affine one alone
    a = general.matrix_dp(l)
    u = smooth_state(sq, l)
    state, r0, r1 = ctx.vector(u.size, data=u), ctx.vector(u.size), ctx.vector(u.size)
    a.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, r0, state)
    a.enable_coefficient_update_q(sq.unit_q(l), sq.jxw_q(l))
    a.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, r1, state)
    assert rel(r1.download(), r0.download()) < 1e-13
    a.enable_coefficient_update(*sq.affine_metric(l))
    a.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, r1, state)
    assert np.array_equal(r1.download(), r0.download())
    general.update_coefficient(mg.LAW_MINIMAL_SURFACE, state)
    general.vmult(dst, src)
    assert np.isfinite(dst.download()).all()
    general.close()
    for vec in (v, w, coarse, src, dst, state, r0, r1):
        vec.free()
    # a full cycle on curved cells
    sector = mg.Square(2, 1, 2, mapped="annulus_sector")
    with pytest.raises(mg._lib.MgxError) as e:
        mg.MultigridSolver(ctx, sector, 2, 2, 1, mg.F64)   # the Poisson hierarchy
    assert e.value.status == UNSUPPORTED
    problem = mg.MinimalSurfaceProblem(ctx, sector, lambda xy: 0.25 * np.sin(2 * np.pi * (xy[:, 0] + xy[:, 1])), mg.F32)
    assert problem.run(12, 1e-12) <= 12 and problem.history[-1][2] < 1e-10 * problem.history[0][0]
    problem.close()
    for s in (sector, sq, cube):
        s.close()
    assert lib.mgx_live_device_allocations() == start


def test_minimal_surface_harness_runs_in_two_dimensions():
    """tools/minimal_surface.py --dim 2: command line, the program's output lines, convergence"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in ([], ["--geometry", "annulus_sector", "--amplitude", "0.25"]):
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "minimal_surface.py"), "2", "3", "--dim", "2"] + extra,
                             cwd=root, capture_output=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        text = out.stdout.decode()
        lines = [ln for ln in text.splitlines() if ln.startswith("Residual norm:")]
        assert lines and "Computing times: nl iterations:" in text and "Testing FE_Q<2>(2)" in text
        first = float(lines[0].split()[2])
        last = float(lines[-1].split()[-1])
        assert last < 1e-10 * first
