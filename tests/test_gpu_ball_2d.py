"""The unit disc in five blocks on the GPU (Square(mapped="ball"), mgx_square_create_ball; the mesh of
minimal_surface/program.cc): level transfers at the four vertices that three cells share (owner weights in
restrict_2d_kernel), the per-point operator, the nonlinear kernels, the general hierarchy with its refresh, and the Newton
solve, against the dense embedding of tests/ball_reference_2d.py and the numpy laws of tests/nonlinear_reference_2d.py
(both pinned on the CPU by test_ball_reference_2d.py).

Shapes: n_refine 1 (5 -> 20 cells) and 2 (20 -> 80 cells); the three-cell vertices exist on every level.
Bounds, all max|a - b| / max|b|: transfers 1e-13 (fp64) and 2e-5 (fp32) as in test_gpu_feq_2d.py::test_transfers, the
adjoint identity 1e-12; operator 1e-12 / 1e-13 (inverse diagonal) in fp64 and 3e-6 in fp32; nonlinear kernels 1e-12 in
fp64 and ten times the distance of the numpy law in float32 from the fp64 one in fp32 ("Solution-dependent
coefficients"); Newton as test_gpu_nonlinear_2d.py::test_newton_solve."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import ball_reference_2d as br  # noqa: E402
import nonlinear_reference_2d as nr2  # noqa: E402
from test_ball_reference_2d import NEWTON_CASES_BALL  # noqa: E402
from test_gpu_nonlinear_2d import check_against_numpy, general_operator, rel, smooth_state  # noqa: E402
from test_nonlinear_reference_2d import boundary_state, make_square, reference  # noqa: E402

_lib = mg._lib
UNSUPPORTED = -4
NUMBERS = {"f64": (mg.F64, np.float64), "f32": (mg.F32, np.float32)}
LAWS = [mg.LAW_UNIT, mg.LAW_MINIMAL_SURFACE]
_cache = {}


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


@pytest.fixture(scope="module", autouse=True)
def shared():
    """the discs and numpy references the tests share: made once, never changed"""
    yield
    for key, v in _cache.items():
        if key[0] == "ball":
            v.close()
    _cache.clear()


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def ball(p, n_refine=2):
    return once(("ball", p, n_refine), lambda: mg.Square(p, n_refine=n_refine, mapped="ball"))


def numpy_level(p, l, n_refine=2):
    return once(("ref", p, l, n_refine), lambda: reference(ball(p, n_refine), l, affine=False))


def embedding(p, l):
    sq = ball(p)
    return once(("P", p, l), lambda: br.embedding(sq.prolong_1d(), sq.children(l), nr2.cell_dofs(sq.idx9_plain(l - 1), p),
                                                  nr2.cell_dofs(sq.idx9_plain(l), p), sq.n_dofs(l - 1), sq.n_dofs(l)))


def unit_matrix(p, l, n_refine=2):
    ref = numpy_level(p, l, n_refine)
    return once(("A", p, l, n_refine), lambda: ref.matrix(ref.coefficient(nr2.LAW_UNIT, None)))


@pytest.mark.parametrize("l", [1, 2])
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 8])
def test_transfers(ctx, p, number, l):
    """prolongate (overwrite into NaN and add, with and without constraints) and restrict_and_add against the dense P and
    P^T; every call twice, bitwise equal; the adjoint identity.  Before owner weights in two dimensions
    mgx_transfer_create refused these level pairs (MGX_ERR_UNSUPPORTED)."""
    num, dt = NUMBERS[number]
    tol = 2e-5 if number == "f32" else 1e-13
    sq, P = ball(p), embedding(p, l)
    ops = [mg.LaplaceOperator.from_cube(ctx, sq, k, num) for k in (l - 1, l)]
    tr = mg.Transfer(ops[0], ops[1], sq.children(l), sq.prolong_1d())
    xc, xf = sq.seeded_vector(l - 1, 11).astype(dt), sq.seeded_vector(l, 12).astype(dt)
    con = sq.constrained(l - 1)
    dc, df = ctx.vector(xc.size, num, data=xc), ctx.vector(xf.size, num, data=xf)
    out, again = ctx.vector(xf.size, num), ctx.vector(xf.size, num)
    for bc in (False, True):
        cons = con if bc else None
        for o in (out, again):
            o.upload(np.full(xf.size, np.nan, dtype=dt))
            tr.prolongate(o, dc, with_constraints=bc)
        got = out.download()
        assert not np.isnan(got).any()   # every fine entry is written
        assert np.array_equal(got, again.download())
        err = rel(got, br.prolongate(P, xc, cons))
        print("p=%d %s level %d bc=%d: prolongate %.3e" % (p, number, l, bc, err))
        assert err < tol
        for o in (out, again):
            o.upload(xf)
            tr.prolongate_and_add(o, dc, with_constraints=bc)
        assert np.array_equal(out.download(), again.download())
        assert rel(out.download(), br.prolongate(P, xc, cons, fine=xf)) < tol
        outc, againc = ctx.vector(xc.size, num, data=xc), ctx.vector(xc.size, num, data=xc)
        tr.restrict_and_add(outc, df, with_constraints=bc)
        tr.restrict_and_add(againc, df, with_constraints=bc)
        got = outc.download()
        assert np.array_equal(got, againc.download())
        err = rel(got, br.restrict_and_add(P, xc, xf, cons))
        print("p=%d %s level %d bc=%d: restrict_and_add %.3e" % (p, number, l, bc, err))
        assert err < tol
        if bc:
            assert np.array_equal(got[con], xc[con])   # constrained coarse rows are skipped
        outc.free()
        againc.free()
    if number == "f64":   # <P x_c, x_f> = <x_c, R x_f>
        zero = ctx.vector(xc.size, data=np.zeros(xc.size))
        tr.prolongate(out, dc, with_constraints=False)
        tr.restrict_and_add(zero, df, with_constraints=False)
        assert np.vdot(out.download(), xf) == pytest.approx(np.vdot(xc, zero.download()), rel=1e-12)
        zero.free()
    tr.clear()
    for v in (dc, df, out, again):
        v.free()
    for o in ops:
        o.clear()


@pytest.mark.parametrize("route", ["ordered", "colour"])
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_operator(ctx, colour_ctx, p, number, route):
    """vmult and the inverse diagonal of the per-point unit-law operator on the 80 cells of level 2 against numpy"""
    c = colour_ctx if route == "colour" else ctx
    num, dt = NUMBERS[number]
    sq, l = ball(p), 2
    ref, A = numpy_level(p, l), unit_matrix(p, l)
    op = mg.LaplaceOperator.from_cube(c, sq, l, num)
    x = sq.seeded_vector(l, 1).astype(dt)
    src, dst = c.vector(x.size, num, data=x), c.vector(x.size, num)
    op.vmult(dst, src)
    got = dst.download()
    err = rel(got, ref.apply(ref.U, x.astype(np.float64)))
    print("p=%d %s %s: vmult %.3e" % (p, number, route, err))
    assert err < (3e-6 if number == "f32" else 1e-12)
    con = sq.constrained(l)
    assert np.array_equal(got[con], x[con])   # identity rows
    dst.upload(np.full(x.size, 3.0, dtype=dt))
    op.vmult(dst, src)
    assert np.array_equal(dst.download(), got)
    op.compute_diagonal()
    err = rel(op.get_matrix_diagonal_inverse().download(), 1.0 / np.diag(A))
    print("p=%d %s %s: inverse diagonal %.3e" % (p, number, route, err))
    assert err < (3e-6 if number == "f32" else 1e-13)
    for v in (src, dst):
        v.free()
    op.clear()


@pytest.mark.parametrize("p", [1, 2, 3, 4, 8])
def test_nonlinear_kernels(ctx, colour_ctx, p):
    """evaluate_coefficient and compute_nonlinear_residual (ordered and colour route) of both laws in both number types
    against numpy; interpolate_to_coarse fills a NaN-filled coarse vector on both level pairs"""
    sq, l = ball(p), 2
    ref = numpy_level(p, l)
    u = smooth_state(sq, l)
    cons = sq.constrained(l)
    for number, dt in NUMBERS.values():
        for route, c in (("ordered", ctx), ("colour", colour_ctx)):
            op = general_operator(c, sq, l, number, "per_point")
            state = c.vector(u.size, number, u.astype(dt))
            for law in LAWS:
                if route == "ordered":
                    op.evaluate_coefficient(law, state)
                    got = op.get_coefficient().download().reshape(sq.n_cells(l), 3, -1)
                    check_against_numpy("ball p=%d law %d: coef_q" % (p, law), got, lambda s, t: ref.coefficient(law, s, t), u, dt)
                dst, again = c.vector(u.size, number), c.vector(u.size, number)
                again.upload(np.full(u.size, 3.0, dtype=dt))
                op.compute_nonlinear_residual(law, dst, state)
                op.compute_nonlinear_residual(law, again, state)
                got = dst.download()
                assert np.array_equal(got, again.download())
                assert np.array_equal(got[cons], np.zeros(cons.size, dt))
                check_against_numpy("ball p=%d %s law %d: residual" % (p, route, law), got, lambda s, t: ref.residual(law, s, t), u, dt)
                dst.free()
                again.free()
            state.free()
            op.clear()
    solver = mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64, general=True)
    R = nr2.interpolation_matrix_1d(sq.gll())
    for k in (1, 2):
        v = smooth_state(sq, k)
        nc = sq.n_dofs(k - 1)
        fine, coarse = ctx.vector(v.size, data=v), ctx.vector(nc, data=np.full(nc, np.nan))
        solver.transfer_dp(k).interpolate_to_coarse(coarse, fine)
        want = nr2.interpolate_to_coarse(R, sq.children(k), nr2.cell_dofs(sq.idx9_plain(k), p), nr2.cell_dofs(sq.idx9_plain(k - 1), p), nc, v)
        got = coarse.download()
        assert not np.isnan(got).any()
        assert np.abs(got - want).max() < 1e-13
        fine.free()
        coarse.free()
    solver.close()


def asymmetry(ctx, solver, sq):
    """max over four pairs of seeded vectors (zero in the constrained rows) of |<V x, y> - <x, V y>| / (|V x| |y| + |x| |V y|)"""
    l = sq.max_level
    con = sq.constrained(l)
    worst = 0.0
    for k in range(4):
        x, y = sq.seeded_vector(l, 31 + 2 * k), sq.seeded_vector(l, 32 + 2 * k)
        x[con] = y[con] = 0.0
        src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
        solver.vmult(dst, src)
        vx = dst.download()
        src.upload(y)
        solver.vmult(dst, src)
        vy = dst.download()
        worst = max(worst, abs(np.vdot(vx, y) - np.vdot(x, vy)) / (np.linalg.norm(vx) * np.linalg.norm(y) + np.linalg.norm(x) * np.linalg.norm(vy)))
        src.free()
        dst.free()
    return worst


@pytest.mark.parametrize("vnumber", ["f64", "f32"])
@pytest.mark.parametrize("p", [2, 4])
def test_hierarchy(ctx, p, vnumber):
    """MultigridSolver(general=True) on the disc: after solve_cg to a reduction of 1e-9 the true residual b - A x with the
    numpy matrix is at most 1e-8 |b| (the margin of 10 covers the recursive residual of CG); the fp64 V-cycle is as
    symmetric as the one of the annulus sector at the same degree and refinement, within a factor of ten (a restriction
    that is not P^T breaks the symmetry at order one)"""
    sq, l = ball(p), 2
    A = unit_matrix(p, l)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, NUMBERS[vnumber][0], general=True)
    b = sq.seeded_vector(l, 9)
    b[sq.constrained(l)] = 0.0
    solver.get_vector(l, "rhs").upload(b)
    its, red = solver.solve_cg()
    x = solver.get_solution(l, insert_bc=False).download()
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("ball p=%d vcycle %s: %d CG iterations, reduction %.3e, true residual %.3e |b|" % (p, vnumber, its, red, res))
    assert res <= 1e-8
    if vnumber == "f64":
        sector = make_square("sector", p, 2)
        other = mg.MultigridSolver(ctx, sector, 3, 3, 1, mg.F64, general=True)
        measured = asymmetry(ctx, other, sector)
        other.close()
        sector.close()
        got = asymmetry(ctx, solver, sq)
        print("ball p=%d: V-cycle asymmetry %.3e (annulus sector: %.3e)" % (p, got, measured))
        assert got <= 10 * measured
    solver.close()


@pytest.mark.parametrize("vnumber", ["f64", "f32"])
@pytest.mark.parametrize("p", [2, 4])
def test_update_coefficient_of_a_hierarchy(ctx, p, vnumber):
    """after update_coefficient the solver is the solver created from the numpy tensors of every level: one fp64 V-cycle
    agrees to 1e-12; with an fp32 V-cycle the tensor of the V-cycle operator is bitwise the rounded fp64 one"""
    sq, lmax = ball(p), 2
    num = NUMBERS[vnumber][0]
    R = nr2.interpolation_matrix_1d(sq.gll())
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, num, general=True)
    states = [None] * sq.n_levels
    states[lmax] = u = smooth_state(sq, lmax)
    for l in range(lmax, 0, -1):
        states[l - 1] = nr2.interpolate_to_coarse(R, sq.children(l), nr2.cell_dofs(sq.idx9_plain(l), p),
                                                  nr2.cell_dofs(sq.idx9_plain(l - 1), p), sq.n_dofs(l - 1), states[l])
    tensors = [numpy_level(p, l).coefficient(mg.LAW_MINIMAL_SURFACE, states[l]) for l in range(sq.n_levels)]
    state = ctx.vector(u.size, data=u)
    solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, state)
    for l in range(sq.n_levels):
        t64 = solver.matrix_dp(l).get_coefficient().download()
        assert rel(t64, tensors[l].ravel()) < 1e-12
        if vnumber == "f32":
            assert np.array_equal(solver.matrix(l).get_coefficient().download(), t64.astype(np.float32))
    if vnumber == "f64":
        scratch = mg.MultigridSolver(ctx, sq, 3, 3, 1, num, general=True, coef_q=tensors)
        x = sq.seeded_vector(lmax, 5)
        src, dst, want = ctx.vector(x.size, data=x), ctx.vector(x.size), ctx.vector(x.size)
        solver.vmult(dst, src)
        scratch.vmult(want, src)
        err = rel(dst.download(), want.download())
        print("ball p=%d: V-cycle of the refreshed hierarchy against the one created from numpy tensors %.3e" % (p, err))
        assert err < 1e-12
        scratch.close()
        for v in (src, dst, want):
            v.free()
    state.free()
    solver.close()


@pytest.mark.parametrize("vnumber", ["f32", "f64"])
@pytest.mark.parametrize("case", sorted(NEWTON_CASES_BALL))
def test_newton_solve(ctx, case, vnumber):
    """MinimalSurfaceProblem on the cases of test_ball_reference_2d.py::test_newton_with_exact_linear_solves: no step is
    halved; 1e-6 of the first norm after N6 or N6 + 1 steps, 1e-10 at most 2 steps later; the converged state is the
    numpy Newton state to 1e-8 (maximum norm, relative)"""
    _, p, n_refine, amplitude = case
    sq = ball(p, n_refine)
    l = sq.max_level
    problem = mg.MinimalSurfaceProblem(ctx, sq, lambda x: amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])), NUMBERS[vnumber][0])
    first, norms = None, []
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
    print("ball p=%d %d cells A=%g vcycle %s: norms %s, CG iterations %s"
          % (p, sq.n_cells(l), amplitude, vnumber, " -> ".join("%.2e" % r for r in norms), cg))
    assert not any(h[1] for h in problem.history)   # no step halved
    n6, n10 = nr2.steps_to(norms, 1e-6), nr2.steps_to(norms, 1e-10)
    assert n6 in (NEWTON_CASES_BALL[case], NEWTON_CASES_BALL[case] + 1)
    assert n10 is not None and n10 <= n6 + 2
    u_ref, _, _ = numpy_level(p, l, n_refine).newton(boundary_state(sq, l, amplitude), max_steps=12, tolerance=1e-10 * first)
    diff = rel(problem.solution.download(), u_ref)
    print("    state against the numpy Newton state: %.3e" % diff)
    assert diff < 1e-8
    problem.close()


def test_refusals_and_lifetime(ctx):
    """a caller's weight_shift together with irregular counts, a DG solver over the disc and the grid accessors are
    refused with a reason; nothing stays allocated after 20 create - solve - destroy cycles"""
    lib = _lib.load()
    start = lib.mgx_live_device_allocations()
    sq = mg.Square(2, n_refine=1, mapped="ball")
    ops = [mg.LaplaceOperator.from_cube(ctx, sq, k) for k in (0, 1)]
    children, p1 = np.ascontiguousarray(sq.children(1), dtype=np.uint32), np.ascontiguousarray(sq.prolong_1d())
    shifts = np.zeros(9 * sq.n_cells(0), dtype=np.uint8)
    d = _lib.TransferDesc(children.ctypes.data_as(_lib.u32p), p1.ctypes.data_as(_lib.f64p), shifts.ctypes.data_as(C.POINTER(C.c_uint8)))
    h = C.c_void_p()
    assert lib.mgx_transfer_create(ops[0].h, ops[1].h, C.byref(d), C.byref(h)) == UNSUPPORTED
    assert "weight_shift" in lib.mgx_last_error().decode()
    for o in ops:
        o.clear()
    with pytest.raises(ValueError) as e:
        mg.DGMultigridSolver(ctx, sq)
    assert "Cartesian box only" in str(e.value)
    for grid in (sq.cells_per_dim2, sq.cell_coords, sq.dof_grid, sq.weight_shift):
        with pytest.raises(_lib.MgxError) as e:
            grid(1)
        assert e.value.status == UNSUPPORTED and "disc" in str(e.value)
    with pytest.raises(_lib.MgxError) as e:
        mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F64)   # the Poisson hierarchy
    assert e.value.status == UNSUPPORTED
    assert lib.mgx_live_device_allocations() == start
    x = sq.seeded_vector(1, 1)
    for _ in range(20):
        solver = mg.MultigridSolver(ctx, sq, 2, 2, 1, mg.F32, general=True)
        src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
        solver.vmult(dst, src)
        assert np.isfinite(dst.download()).all()
        src.free()
        dst.free()
        solver.close()
        assert lib.mgx_live_device_allocations() == start
    sq.close()


def test_minimal_surface_harness_runs_on_the_disc():
    """tools/minimal_surface.py --dim 2 --geometry ball in a process of its own: exit status, the program's lines"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "minimal_surface.py"), "2", "2", "--dim", "2", "--geometry", "ball"],
                         cwd=root, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    text = out.stdout.decode()
    assert "Testing FE_Q<2>(2)" in text and "(ball, 80 cells, 3 levels)" in text and "CG iterations per Newton step:" in text
    lines = [ln for ln in text.splitlines() if ln.startswith("Residual norm:")]
    converged = [ln for ln in text.splitlines() if ln.startswith("Converged:")]
    assert lines and len(converged) == 1
    assert float(lines[-1].split()[-1]) < 1e-10 * float(lines[0].split()[2])
