"""Solution-dependent coefficients on curved cells on the GPU (mgx_operator_enable_coefficient_update_q: JxW_q J^-1 J^-T
and JxW_q of every quadrature point): coefficient evaluation, nonlinear residual, state interpolation, the refresh of a
whole hierarchy and the Newton solve on the sheared box, the equiangular shell sector and the whole hyper_shell(6),
against the numpy restatement tests/nonlinear_reference_mapped.py, which computes its geometry from the cell nodes and
is pinned on the CPU by test_nonlinear_reference_mapped.py.  Tolerances are those of test_gpu_nonlinear.py and
test_gpu_shell.py for this branch: 1e-12 (fp64) and 2e-5 (fp32) relative to the largest entry, 1e-9 for a V-cycle, 1e-8
for the converged Newton state.  The fp32 cases print, next to the device's error, the error of the numpy law evaluated
in float32 from the rounded geometry and gradient: what rounding alone costs on these cells."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import nonlinear_reference as nr  # noqa: E402
import nonlinear_reference_mapped as nm  # noqa: E402
from test_nonlinear_reference_mapped import NEWTON_CASES_MAPPED  # noqa: E402

DEGREES = [1, 2, 3, 4, 5, 8]
GEOMETRIES = ["sheared", "shell_sector", "shell6"]
LAWS = [mg.LAW_UNIT, mg.LAW_MINIMAL_SURFACE]
UNSUPPORTED, INVALID_ARGUMENT = -4, -1


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def n_refine_for(p, geometry):
    if geometry == "shell6":  # 6 x 8 cells per refinement
        return 1
    return 2 if p <= 5 else 1


def curved_operator(ctx, cube, l, number, coef_q=None):
    """an operator of the general branch on a mapped cube (its own coef_q is the unit-law tensor), told the per-point
    geometry of the provider"""
    op = mg.LaplaceOperator.from_cube(ctx, cube, l, number, coef_q=coef_q)
    op.enable_coefficient_update_q(cube.coef_q(l), cube.jxw_q(l))
    return op


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("p", DEGREES)
def test_evaluate_coefficient(ctx, p, geometry):
    """the downloaded coef_q of both laws against numpy; and an operator refreshed on the device against one created
    through desc.coef_q from the numpy tensor: vmult, vmult_residual, inverse diagonal"""
    cube = nm.make_cube(mg, geometry, p, n_refine_for(p, geometry))
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    u, x, b = nm.smooth_state(cube, l), cube.seeded_vector(l, 1), cube.seeded_vector(l, 2)
    for number, dt, tol in ((mg.F64, np.float64, 1e-12), (mg.F32, np.float32, 2e-5)):
        op = curved_operator(ctx, cube, l, number)
        state = ctx.vector(u.size, number, u.astype(dt))
        for law in LAWS:
            op.evaluate_coefficient(law, state)
            got = op.get_coefficient().download().astype(np.float64).reshape(cube.n_cells(l), 6, -1)
            want = ref.coefficient(law, u.astype(dt).astype(np.float64))
            err = rel(got, want)
            note = ""
            if number == mg.F32:
                note = " (numpy in float32: %.3e)" % rel(ref.coefficient(law, u, np.float32).astype(np.float64), want)
            print("p=%d %s law %d %s: coef_q %.3e%s" % (p, geometry, law, dt.__name__, err, note))
            assert err < tol
            if number == mg.F64:
                made = curved_operator(ctx, cube, l, number, coef_q=want)
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


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("p", DEGREES)
def test_compute_nonlinear_residual(ctx, p, geometry):
    """against numpy; two calls bitwise equal; constrained rows exactly zero; the unit law is compute_residual of the
    linear operator.  The state is the one of test_gpu_nonlinear.py (smooth + 0.1 seeded_vector: nm.rough_state says why).
    With the smooth state alone the same kernels measured, on an MI355X, up to 1.6e-12 (fp64, p = 8, shell_sector) and
    3.0e-4 (fp32, p = 5, shell_sector) of the largest entry of a residual whose entries are what is left of cancelling
    cell contributions; the tensors of that state sit at 4e-14 / 5e-6;
    test_nonlinear_residual_of_a_smooth_state guards that case in fp32."""
    cube = nm.make_cube(mg, geometry, p, n_refine_for(p, geometry))
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    u = nm.rough_state(cube, l)
    cons = cube.constrained(l)
    for number, dt, tol in ((mg.F64, np.float64, 1e-12), (mg.F32, np.float32, 2e-5)):
        op = curved_operator(ctx, cube, l, number)
        state = ctx.vector(u.size, number, u.astype(dt))
        for law in LAWS:
            dst, again = ctx.vector(u.size, number), ctx.vector(u.size, number)
            op.compute_nonlinear_residual(law, dst, state)
            op.compute_nonlinear_residual(law, again, state)
            got = dst.download()
            assert np.array_equal(got, again.download())            # reproducible assembly
            assert np.array_equal(got[cons], np.zeros(cons.size, dt))  # constrained rows exactly zero
            want = ref.residual(law, u.astype(dt).astype(np.float64))
            err = rel(got.astype(np.float64), want)
            note = ""
            if number == mg.F32:
                note = " (numpy in float32: %.3e)" % rel(ref.residual(law, u, np.float32).astype(np.float64), want)
            print("p=%d %s law %d %s: residual %.3e%s" % (p, geometry, law, dt.__name__, err, note))
            assert err < tol
            if law == mg.LAW_UNIT and number == mg.F64:
                # -(A x) of the linear operator with the boundary values in x (its coefficient is the unit-law tensor)
                lin = ctx.vector(u.size)
                op.compute_residual(lin, state)
                assert rel(got, lin.download()) < 1e-12
        op.clear()
    cube.close()


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("p", DEGREES)
def test_nonlinear_residual_of_a_smooth_state(ctx, p, geometry):
    """the cancelling case of the docstring above, guarded: for the smooth state the fp32 device residual may miss the fp64
    numpy residual by no more than ten times what the numpy residual evaluated in float32 (dense products, geometry and
    state rounded first) misses it by, or by the 2e-5 of the well-conditioned case where that is larger.  Ten: the yardstick
    is one draw of the rounding error of one dense product per direction, the kernel rounds after each of its six
    sum-factorisation sweeps in either direction and adds the cells up in another order; an order of magnitude separates
    that from a wrong term, which shows at the size of the summands (100 to 1000 times the entries of this residual)."""
    cube = nm.make_cube(mg, geometry, p, n_refine_for(p, geometry))
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    u = nm.smooth_state(cube, l)
    op = curved_operator(ctx, cube, l, mg.F32)
    state, dst = ctx.vector(u.size, mg.F32, u.astype(np.float32)), ctx.vector(u.size, mg.F32)
    for law in LAWS:
        op.compute_nonlinear_residual(law, dst, state)
        want = ref.residual(law, u.astype(np.float32).astype(np.float64))
        err = rel(dst.download().astype(np.float64), want)
        yard = rel(ref.residual(law, u, np.float32).astype(np.float64), want)
        print("p=%d %s law %d float32, smooth state: residual %.3e, numpy in float32 %.3e" % (p, geometry, law, err, yard))
        assert err < max(2e-5, 10 * yard)
    op.clear()
    cube.close()


@pytest.mark.parametrize("p", [2, 3, 4])
def test_two_routes_on_the_device(ctx, p):
    """the sheared box through the per-point path against the same box through the affine path (one metric per level);
    and either enable call replaces what the other set"""
    sheared = nm.make_cube(mg, "sheared", p, 2)
    box = mg.Cube(p, n_refine=2, box=(1, 1, 1), origin=-0.9, h0=1.9)
    l = sheared.max_level
    u = nm.smooth_state(sheared, l)
    curved = curved_operator(ctx, sheared, l, mg.F64)
    affine = mg.LaplaceOperator.from_cube(ctx, box, l, mg.F64, coef_q=box.unit_law_coefficient(l, nm.SHEAR))
    affine.enable_coefficient_update(*box.affine_metric(l, nm.SHEAR))
    state = ctx.vector(u.size, data=u)

    def both(op, law):
        r = ctx.vector(u.size)
        op.evaluate_coefficient(law, state)
        op.compute_nonlinear_residual(law, r, state)
        return op.get_coefficient().download(), r.download()

    for law in LAWS:
        (ca, ra), (cc, rc) = both(affine, law), both(curved, law)
        print("p=%d law %d: tensor %.3e, residual %.3e" % (p, law, rel(cc, ca), rel(rc, ra)))
        assert rel(cc, ca) < 1e-12 and rel(rc, ra) < 1e-12
    # the curved operator told the affine geometry is the affine operator; told the per-point one again, itself
    cq, rq = both(curved, mg.LAW_MINIMAL_SURFACE)
    curved.enable_coefficient_update(*box.affine_metric(l, nm.SHEAR))
    c1, r1 = both(curved, mg.LAW_MINIMAL_SURFACE)
    ca, ra = both(affine, mg.LAW_MINIMAL_SURFACE)
    assert np.array_equal(c1, ca) and np.array_equal(r1, ra)
    curved.enable_coefficient_update_q(sheared.coef_q(l), sheared.jxw_q(l))
    c2, r2 = both(curved, mg.LAW_MINIMAL_SURFACE)
    assert np.array_equal(c2, cq) and np.array_equal(r2, rq)
    for o in (curved, affine):
        o.clear()
    sheared.close()
    box.close()


@pytest.mark.parametrize("geometry", ["shell_sector", "shell6"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_interpolate_to_coarse(ctx, p, geometry):
    """the entity mask of the one-writer interpolation on the multi-block shell (and on the sector)"""
    cube = nm.make_cube(mg, geometry, p, 2)
    solver = mg.MultigridSolver(ctx, cube, 2, 2, 1, mg.F64, general=True)
    R = nr.interpolation_matrix_1d(cube.gll())
    for l in range(1, cube.n_levels):
        u = nm.smooth_state(cube, l) + 0.1 * cube.seeded_vector(l, 11)
        nan = np.full(cube.n_dofs(l - 1), np.nan)  # (every coarse DoF has to be written by its one writer)
        fine, coarse, again = ctx.vector(u.size, data=u), ctx.vector(nan.size, data=nan), ctx.vector(nan.size, data=nan)
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
@pytest.mark.parametrize("geometry", ["shell_sector", "shell6"])
def test_update_coefficient_of_a_hierarchy(ctx, geometry, p, vnumber):
    """after update_coefficient the solver is the solver created from scratch with the numpy tensors of every level; a
    second call with another state matches the from-scratch solver of that state (no stale graph, diagonal, eigenvalues)"""
    cube = nm.make_cube(mg, geometry, p, 2)  # 3 levels
    lmax = cube.max_level
    R = nr.interpolation_matrix_1d(cube.gll())
    refs = [nm.mapped_reference(cube, l) for l in range(cube.n_levels)]
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, vnumber, general=True)
    x = cube.seeded_vector(lmax, 5)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    solver.vmult(dst, src)  # (a V-cycle before the first refresh: the coarse levels' graph exists from here on)
    solver.vmult(dst, src)
    for k, u in enumerate((nm.smooth_state(cube, lmax), 0.1 * cube.seeded_vector(lmax, 3) + nm.boundary_state(cube, lmax, 0.25))):
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
            print("%s p=%d vcycle %s state %d: V-cycle %.3e" % (geometry, p, "f64" if vnumber == mg.F64 else "f32", k, err))
            assert err < 1e-9
        for l in range(cube.n_levels):
            a, b = solver.smoother(l).info(), scratch.smoother(l).info()
            assert a["degree"] == b["degree"]
            assert a["lambda_max"] == pytest.approx(b["lambda_max"], rel=1e-8)
        scratch.close()
    solver.close()
    cube.close()


@pytest.mark.parametrize("vnumber", [mg.F32, mg.F64])
@pytest.mark.parametrize("case", sorted(NEWTON_CASES_MAPPED))
def test_newton_solve(ctx, case, vnumber):
    """MinimalSurfaceProblem on the cases of test_nonlinear_reference_mapped.py::test_newton_with_exact_linear_solves:
    every accepted step lowers the residual norm; 1e-6 of the first norm after N6 or N6 + 1 steps, 1e-10 at most 2 steps
    later; the converged state is the numpy Newton state to 1e-8 (maximum norm, relative)."""
    geometry, p, n_refine, amplitude = case
    cube = nm.make_cube(mg, geometry, p, n_refine)
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
    print("%s p=%d %d cells A=%g vcycle %s: norms %s, CG iterations %s"
          % (geometry, p, cube.n_cells(l), amplitude, "f32" if vnumber == mg.F32 else "f64",
             " -> ".join("%.2e" % r for r in norms), cg))
    n6, n10 = nr.steps_to(norms, 1e-6), nr.steps_to(norms, 1e-10)
    assert n6 in (NEWTON_CASES_MAPPED[case], NEWTON_CASES_MAPPED[case] + 1)
    assert n10 is not None and n10 <= n6 + 2
    u_ref, _, _ = nm.mapped_reference(cube, l).newton(nm.boundary_state(cube, l, amplitude), max_steps=12,
                                                      tolerance=1e-10 * first)
    diff = rel(problem.solution.download(), u_ref)
    print("    state against the numpy Newton state: %.3e" % diff)
    assert diff < 1e-8
    problem.close()
    cube.close()


def test_refusals(ctx):
    """a cube whose tensor contains a(x), a jacobian with a mapped cube, non-positive JxW: status and message, and the
    objects stay usable"""
    # MGX_CUBE_PROBLEM_SHELL: the per-point tensor is not the unit law
    shell = mg.Cube(2, n_refine=1, shell=6, problem="shell")
    with pytest.raises(mg._lib.MgxError) as e:
        mg.MultigridSolver(ctx, shell, 2, 2, 1, mg.F64, general=True)
    assert e.value.status == UNSUPPORTED and "PROBLEM_SHELL" in str(e.value)
    plain = mg.MultigridSolver(ctx, shell, 3, 3, 1, mg.F64)  # the cube still makes the hierarchy of poisson_shell
    x = shell.seeded_vector(shell.max_level, 1)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    plain.vmult(dst, src)
    assert np.isfinite(dst.download()).all() and np.abs(dst.download()).max() > 0
    plain.close()
    shell.close()

    # a jacobian on a mapped cube
    cube = nm.make_cube(mg, "shell_sector", 2, 1)
    l = cube.max_level
    with pytest.raises(mg._lib.MgxError) as e:
        mg.MultigridSolver(ctx, cube, 2, 2, 1, mg.F64, general=True, jacobian=nm.SHEAR)
    assert e.value.status == UNSUPPORTED and "jacobian" in str(e.value)
    general = mg.MultigridSolver(ctx, cube, 2, 2, 1, mg.F64, general=True)
    u = nm.smooth_state(cube, l)
    state = ctx.vector(u.size, data=u)
    general.update_coefficient(mg.LAW_MINIMAL_SURFACE, state)
    general.close()

    # non-positive JxW_q / diagonal of the unit tensor: nothing changes, the earlier geometry stays in force
    ref = nm.mapped_reference(cube, l)
    op = curved_operator(ctx, cube, l, mg.F64)
    op.evaluate_coefficient(mg.LAW_MINIMAL_SURFACE, state)
    before = op.get_coefficient().download()
    for which in ("jxw", "unit"):
        U, w = cube.coef_q(l), cube.jxw_q(l)
        if which == "jxw":
            w[3, 5] = 0.0
        else:
            U[2, 1, 4] = -U[2, 1, 4]
        with pytest.raises(mg._lib.MgxError) as e:
            op.enable_coefficient_update_q(U, w)
        assert e.value.status == INVALID_ARGUMENT and "positive" in str(e.value)
    op.evaluate_coefficient(mg.LAW_MINIMAL_SURFACE, state)
    assert np.array_equal(op.get_coefficient().download(), before)
    assert rel(before.reshape(cube.n_cells(l), 6, -1), ref.coefficient(mg.LAW_MINIMAL_SURFACE, u)) < 1e-12
    op.clear()
    # an operator of the separable branch has no tensor to rewrite
    sep = mg.Cube(2, 1, 1)
    op = mg.LaplaceOperator.from_cube(ctx, sep, 1)
    n3 = 27
    with pytest.raises(mg._lib.MgxError) as e:
        mg._lib.check(ctx.lib.mgx_operator_enable_coefficient_update_q(
            op.h, np.ones(sep.n_cells(1) * 6 * n3).ctypes.data_as(mg._lib.f64p),
            np.ones(sep.n_cells(1) * n3).ctypes.data_as(mg._lib.f64p)))
    assert e.value.status == UNSUPPORTED and "coef_q" in str(e.value)
    op.clear()
    sep.close()
    cube.close()


def test_minimal_surface_harness_on_the_shell_sector():
    """tools/minimal_surface.py --geometry shell_sector: the program's output lines, convergence"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "minimal_surface.py"), "2", "2", "--geometry",
                          "shell_sector", "--amplitude", "0.25"], cwd=root, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    text = out.stdout.decode()
    lines = [ln for ln in text.splitlines() if ln.startswith("Residual norm:")]
    assert lines and "Computing times: nl iterations:" in text
    first = float(lines[0].split()[2])
    last = float(lines[-1].split()[-1])
    assert last < 1e-10 * first
