"""Solution-dependent coefficients of the general branch on the GPU (MinimalSurfaceOperator and LaplaceProblem::solve of
minimal_surface/program.cc, in 3D on the affine cube / box): coefficient evaluation, nonlinear residual, state
interpolation, the refresh of a whole hierarchy and the Newton solve, against the numpy restatement
tests/nonlinear_reference.py (pinned on the CPU by test_nonlinear_reference.py).  Tolerances for the operator are those
of test_gpu_shell.py for this branch: 1e-12 (fp64) and 2e-5 (fp32) relative to the largest entry, 1e-9 for a V-cycle."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import nonlinear_reference as nr  # noqa: E402
from test_nonlinear_reference import NEWTON_CASES, boundary_state, reference  # noqa: E402

DEGREES = [1, 2, 3, 4, 5, 8]
# a box with the edge lengths 1.9 x 1.425 x 2.375: the metric is not a multiple of the identity
BOX = np.diag([1.0, 0.75, 1.25])
LAWS = [mg.LAW_UNIT, mg.LAW_MINIMAL_SURFACE]


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def n_refine_for(p):
    return 2 if p <= 5 else 1  # 4^3 cells up to degree 5, 2^3 above


def smooth_state(cube, l, jacobian=None):
    x = cube.dof_coordinates(l, jacobian)
    return 0.6 * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])) * np.cos(1.3 * x[:, 2]) + 0.2 * x[:, 2] ** 2 + 0.1 * cube.seeded_vector(l, 11)


def general_operator(ctx, cube, l, number, jacobian, coef_q=None):
    op = mg.LaplaceOperator.from_cube(ctx, cube, l, number, coef_q=cube.unit_law_coefficient(l, jacobian) if coef_q is None else coef_q)
    op.enable_coefficient_update(*cube.affine_metric(l, jacobian))
    return op


@pytest.mark.parametrize("geometry", ["cube", "box"])
@pytest.mark.parametrize("p", DEGREES)
def test_evaluate_coefficient(ctx, p, geometry):
    """the downloaded coef_q of both laws against numpy; and an operator refreshed on the device against one created
    through desc.coef_q from the numpy tensor: vmult, vmult_residual, inverse diagonal"""
    jac = BOX if geometry == "box" else None
    cube = mg.Cube(p, 1, n_refine_for(p))
    l = cube.max_level
    ref = reference(cube, l, jac)
    u, x, b = smooth_state(cube, l, jac), cube.seeded_vector(l, 1), cube.seeded_vector(l, 2)
    for number, dt, tol in ((mg.F64, np.float64, 1e-12), (mg.F32, np.float32, 2e-5)):
        op = general_operator(ctx, cube, l, number, jac)
        state = ctx.vector(u.size, number, u.astype(dt))
        for law in LAWS:
            op.evaluate_coefficient(law, state)
            got = op.get_coefficient().download().astype(np.float64).reshape(cube.n_cells(l), 6, -1)
            want = ref.coefficient(law, u.astype(dt).astype(np.float64))
            err = rel(got, want)
            print("p=%d %s law %d %s: coef_q %.3e" % (p, geometry, law, dt.__name__, err))
            assert err < tol
            if number == mg.F64:
                made = general_operator(ctx, cube, l, number, jac, coef_q=want)
                src, rhs = ctx.vector(x.size, data=x), ctx.vector(x.size, data=b)
                out = []
                for o in (op, made):
                    dst, res = ctx.vector(x.size), ctx.vector(x.size)
                    o.vmult(dst, src)
                    o.vmult_residual(rhs, src, res)
                    o.compute_diagonal()
                    out.append((dst.download(), res.download(), o.get_matrix_diagonal_inverse().download()))
                for g, w in zip(*out):
                    assert rel(g, w) < 1e-13
                assert rel(out[0][0], ref.apply(want, x)) < 1e-12
                made.clear()
        op.clear()
    cube.close()


def test_refreshed_coefficient_in_the_other_forms_of_the_general_branch(monkeypatch):
    """cell-coloured launches and the brick form at p = 4 read the same refreshed buffer: one level large enough to take
    them (forced as in test_gpu_shell.py), refreshed once from a smooth state; vmult and the nonlinear residual compared
    between the forms with the tolerances of those tests"""
    p, n_refine = 4, 3
    cube = mg.Cube(p, 1, n_refine)
    l = cube.max_level
    monkeypatch.setenv("MGX_CELL_COLOUR_MIN", "1")
    c_colour = mg.Context(0, options={"no_general_bricks": 1})
    monkeypatch.setenv("MGX_CELL_COLOUR_MIN", "4000000000")
    c_brick = mg.Context(0, options={"general_brick_min": 1})
    c_cell = mg.Context(0, options={"no_general_bricks": 1})
    u, x = smooth_state(cube, l), cube.seeded_vector(l, 5)
    vm, rs = [], []
    for c in (c_brick, c_cell, c_colour):
        op = general_operator(c, cube, l, mg.F64, None)
        state, src = c.vector(u.size, data=u), c.vector(x.size, data=x)
        op.evaluate_coefficient(mg.LAW_MINIMAL_SURFACE, state)
        dst, again, res, res2 = (c.vector(x.size) for _ in range(4))
        op.vmult(dst, src)
        op.vmult(again, src)
        assert np.array_equal(dst.download(), again.download())
        op.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, res, state)
        op.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, res2, state)
        assert np.array_equal(res.download(), res2.download())
        vm.append(dst.download())
        rs.append(res.download())
        op.clear()
    assert np.abs(vm[0]).max() > 0
    assert rel(vm[0], vm[1]) < 1e-12   # brick form against the per-cell kernel with ordered assembly
    assert rel(vm[2], vm[1]) < 1e-13   # colour by colour against it
    assert rel(rs[2], rs[1]) < 1e-13
    for c in (c_colour, c_brick, c_cell):
        c.close()
    cube.close()


@pytest.mark.parametrize("geometry", ["cube", "box"])
@pytest.mark.parametrize("p", DEGREES)
def test_compute_nonlinear_residual(ctx, p, geometry):
    jac = BOX if geometry == "box" else None
    cube = mg.Cube(p, 1, n_refine_for(p))
    l = cube.max_level
    ref = reference(cube, l, jac)
    u = smooth_state(cube, l, jac)
    cons = cube.constrained(l)
    for number, dt, tol in ((mg.F64, np.float64, 1e-12), (mg.F32, np.float32, 2e-5)):
        op = general_operator(ctx, cube, l, number, jac)
        state = ctx.vector(u.size, number, u.astype(dt))
        for law in LAWS:
            dst, again = ctx.vector(u.size, number), ctx.vector(u.size, number)
            op.compute_nonlinear_residual(law, dst, state)
            op.compute_nonlinear_residual(law, again, state)
            got = dst.download()
            assert np.array_equal(got, again.download())            # reproducible assembly
            assert np.array_equal(got[cons], np.zeros(cons.size, dt))  # constrained rows exactly zero
            err = rel(got.astype(np.float64), ref.residual(law, u.astype(dt).astype(np.float64)))
            print("p=%d %s law %d %s: residual %.3e" % (p, geometry, law, dt.__name__, err))
            assert err < tol
            if law == mg.LAW_UNIT and number == mg.F64:
                # -(A x) of the linear operator with the boundary values in x (its coefficient is the unit-law tensor)
                lin = ctx.vector(u.size)
                op.compute_residual(lin, state)
                assert rel(got, lin.download()) < 1e-12
        op.clear()
    cube.close()


@pytest.mark.parametrize("p", DEGREES)
def test_interpolate_to_coarse(ctx, p):
    cube = mg.Cube(p, 1, n_refine_for(p))
    solver = mg.MultigridSolver(ctx, cube, 2, 2, 1, mg.F64, general=True)
    R = nr.interpolation_matrix_1d(cube.gll())
    for l in range(1, cube.n_levels):
        u = smooth_state(cube, l)
        fine, coarse, again = ctx.vector(u.size, data=u), ctx.vector(cube.n_dofs(l - 1)), ctx.vector(cube.n_dofs(l - 1))
        tr = solver.transfer_dp(l)
        tr.interpolate_to_coarse(coarse, fine)
        tr.interpolate_to_coarse(again, fine)
        want = nr.interpolate_to_coarse(R, cube.children(l), nr.cell_dofs(cube.idx27_plain(l), p),
                                        nr.cell_dofs(cube.idx27_plain(l - 1), p), cube.n_dofs(l - 1), u)
        assert np.array_equal(coarse.download(), again.download())
        assert np.abs(coarse.download() - want).max() < 1e-13
    solver.close()
    cube.close()


@pytest.mark.parametrize("vnumber", [mg.F64, mg.F32])
@pytest.mark.parametrize("p", [2, 4])
def test_update_coefficient_of_a_hierarchy(ctx, p, vnumber):
    """after update_coefficient the solver is the solver created from scratch with the numpy tensors of every level; a
    second call with another state matches the from-scratch solver of that state (no stale graph, diagonal, eigenvalues)"""
    cube = mg.Cube(p, 1, 2)  # 3 levels
    lmax = cube.max_level
    R = nr.interpolation_matrix_1d(cube.gll())
    refs = [reference(cube, l) for l in range(cube.n_levels)]
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, vnumber, general=True)
    x = cube.seeded_vector(lmax, 5)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    solver.vmult(dst, src)  # (a V-cycle before the first refresh: the coarse levels' graph exists from here on)
    solver.vmult(dst, src)
    for k, u in enumerate((smooth_state(cube, lmax), 0.5 * cube.seeded_vector(lmax, 3) + boundary_state(cube, lmax, 1.0))):
        states = [None] * cube.n_levels
        states[lmax] = u
        for l in range(lmax, 0, -1):
            states[l - 1] = nr.interpolate_to_coarse(R, cube.children(l), nr.cell_dofs(cube.idx27_plain(l), p),
                                                     nr.cell_dofs(cube.idx27_plain(l - 1), p), cube.n_dofs(l - 1), states[l])
        tensors = [refs[l].coefficient(mg.LAW_MINIMAL_SURFACE, states[l]) for l in range(cube.n_levels)]
        scratch = mg.MultigridSolver(ctx, cube, 3, 3, 1, vnumber, general=True, coef_q=tensors)
        state = ctx.vector(u.size, data=u)
        solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, state)
        want = ctx.vector(x.size)
        for _ in range(3):  # (the third V-cycle replays the captured graph)
            solver.vmult(dst, src)
            scratch.vmult(want, src)
            err = rel(dst.download(), want.download())
            print("p=%d vcycle %s state %d: V-cycle %.3e" % (p, "f64" if vnumber == mg.F64 else "f32", k, err))
            assert err < 1e-9
        for l in range(cube.n_levels):
            a, b = solver.smoother(l).info(), scratch.smoother(l).info()
            assert a["degree"] == b["degree"]
            assert a["lambda_max"] == pytest.approx(b["lambda_max"], rel=1e-8)
        scratch.close()
    solver.close()
    cube.close()


@pytest.mark.parametrize("vnumber", [mg.F32, mg.F64])
@pytest.mark.parametrize("case", sorted(NEWTON_CASES))
def test_newton_solve(ctx, case, vnumber):
    """MinimalSurfaceProblem on the cases of test_nonlinear_reference.py::test_newton_with_exact_linear_solves: every
    accepted step lowers the residual norm; 1e-6 of the first norm after N6 or N6 + 1 steps, 1e-10 at most 2 steps later;
    the converged state is the numpy Newton state to 1e-8 (maximum norm, relative).  Measured on an MI355X: see the
    Newton table of DESIGN.md (section "Solution-dependent coefficients")."""
    p, n_refine, amplitude = case
    cube = mg.Cube(p, 1, n_refine)
    l = cube.max_level
    problem = mg.MinimalSurfaceProblem(ctx, cube, lambda x: amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])), vnumber)
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
    print("p=%d %d^3 cells A=%g vcycle %s: norms %s, CG iterations %s"
          % (p, 2 ** n_refine, amplitude, "f32" if vnumber == mg.F32 else "f64", " -> ".join("%.2e" % r for r in norms), cg))
    n6, n10 = nr.steps_to(norms, 1e-6), nr.steps_to(norms, 1e-10)
    assert n6 in (NEWTON_CASES[case], NEWTON_CASES[case] + 1)
    assert n10 is not None and n10 <= n6 + 2
    u_ref, ref_norms, _ = reference(cube, l).newton(boundary_state(cube, l, amplitude), max_steps=12, tolerance=1e-10 * first)
    diff = rel(problem.solution.download(), u_ref)
    print("    state against the numpy Newton state: %.3e" % diff)
    assert diff < 1e-8
    problem.close()
    cube.close()


def test_refusals(ctx):
    """separable-branch operator, communicator present, agglomerated solver: MGX_ERR_UNSUPPORTED with a message, and the
    object stays usable"""
    unsupported = -4
    cube = mg.Cube(2, 1, 2)
    l = cube.max_level
    x = cube.seeded_vector(l, 1)
    # an operator of the separable branch
    op = mg.LaplaceOperator.from_cube(ctx, cube, l)
    with pytest.raises(mg._lib.MgxError) as e:
        op.enable_coefficient_update(*cube.affine_metric(l))
    assert e.value.status == unsupported and "coef_q" in str(e.value)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    op.vmult(dst, src)
    assert rel(dst.download(), reference(cube, l).apply(cube.unit_law_coefficient(l), x)) < 1e-12
    op.clear()
    # a solver of the separable branch (its operators were never enabled): refused as a whole, still a solver
    plain = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
    with pytest.raises(mg._lib.MgxError):
        plain.update_coefficient(mg.LAW_UNIT, src)
    plain.vmult(dst, src)
    plain.close()

    # a context with a communicator (callbacks that are never called on one rank)
    import ctypes as C
    c2 = mg.Context(0)
    general = mg.MultigridSolver(c2, cube, 2, 2, 1, mg.F64, general=True)
    s2, d2, before = c2.vector(x.size, data=x), c2.vector(x.size), c2.vector(x.size)
    general.vmult(before, s2)
    exchange, allreduce = mg._lib.EXCHANGE_FN(lambda *a: 0), mg._lib.ALLREDUCE_FN(lambda *a: 0)
    desc = mg._lib.CommDesc(0, 2, None, exchange, allreduce, mg._lib.ALLOC_FN())
    mg._lib.check(c2.lib.mgx_context_set_comm(c2.h, C.byref(desc)))
    with pytest.raises(mg._lib.MgxError) as e:
        general.update_coefficient(mg.LAW_MINIMAL_SURFACE, s2)
    assert e.value.status == unsupported and "communicator" in str(e.value)
    general.vmult(d2, s2)
    assert rel(d2.download(), before.download()) < 1e-13
    general.close()
    c2.close()
    cube.close()


def test_refusal_on_an_agglomerated_solver():
    """a hierarchy whose coarse levels run on a copy on a context of its own (mgx_solver_set_agglomeration)"""
    import ctypes as C
    c1, c2 = mg.Context(0), mg.Context(0)
    cube, whole = mg.Cube(2, 1, 2), mg.Cube(2, 1, 1)
    solver = mg.MultigridSolver(c1, cube, 2, 2, 1, mg.F64, general=True)
    coarse = mg.MultigridSolver(c2, whole, 2, 2, 1, mg.F64, general=True)
    level = 1
    gg = whole.dof_grid(level)
    order = np.argsort(gg)
    mine = np.ascontiguousarray(order[np.searchsorted(gg[order], cube.dof_grid(level))].astype(np.uint32))
    owned = np.ones(mine.size, dtype=np.uint8)
    mg._lib.check(c1.lib.mgx_solver_set_agglomeration(solver.h, level, coarse.h, mine.ctypes.data_as(mg._lib.u32p),
                                                     owned.ctypes.data_as(C.POINTER(C.c_uint8)), mine.size))
    x = cube.seeded_vector(cube.max_level, 1)
    src, dst, again = c1.vector(x.size, data=x), c1.vector(x.size), c1.vector(x.size)
    # (the V-cycle of an agglomerated solver sums its seam over the ranks: without a communicator the level operators and
    # smoothers show that nothing was touched)
    top = solver.matrix_dp(cube.max_level)
    top.vmult(dst, src)
    before = [solver.smoother(l).info() for l in range(cube.n_levels)]
    with pytest.raises(mg._lib.MgxError) as e:
        solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, src)
    assert e.value.status == -4 and "agglomerated" in str(e.value)
    top.vmult(again, src)
    assert np.abs(dst.download()).max() > 0 and np.array_equal(dst.download(), again.download())
    assert before == [solver.smoother(l).info() for l in range(cube.n_levels)]
    coarse.close()
    c2.close()   # (the coarse context goes before the context of the hierarchy above it)
    solver.close()
    c1.close()
    cube.close()
    whole.close()


def test_minimal_surface_harness_runs():
    """tools/minimal_surface.py (minimal_surface/program.cc): command line, the program's output lines, convergence"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "minimal_surface.py"), "2", "2"], cwd=root,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    text = out.stdout.decode()
    lines = [ln for ln in text.splitlines() if ln.startswith("Residual norm:")]
    assert lines and "Computing times: nl iterations:" in text
    first = float(lines[0].split()[2])
    last = float(lines[-1].split()[-1])
    assert last < 1e-10 * first
