"""GPU tests of a linear problem on curved 2D meshes: the residual form of the 2D cell loop (mgx_compute_residual_2d),
the right-hand sides of a hierarchy (mgx_solver_compute_rhs_2d), the L2-error kernel (mgx_compute_l2_error_2d) and the
solver of a SquareProblem (mgx_square_solver_create_problem), against tests/poisson_mapped_reference_2d.py.

Tolerances, all max|a - b| / max|b|: the residual at contrast <= 1 as the transfers of tests/test_gpu_feq_2d.py, 1e-13
(fp64) and 2e-5 (fp32); at contrast 1e6, ten times the spread of the reference itself (see test_residual_high_contrast).
The references of a (mesh, degree) are built once and shared by the cases of both number types."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import poisson_mapped_reference_2d as pm  # noqa: E402
from test_poisson_mapped_reference_2d import CONVERGENCE, make_square  # noqa: E402

_lib = mg._lib
UNSUPPORTED, INVALID_ARGUMENT = -4, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mesh -> (geometry of make_square, level of the disc, the operator's coefficient: None = the descriptor's own form)
RESIDUAL_MESHES = {
    "box_diagonal": ("box", None, None),           # kDiagonalCoefficient
    "sheared_tensor": ("sheared", None, None),     # kTensorPerMesh
    "sheared_per_point": ("sheared", None, 1.0),   # kTensorPerPoint: the shell problem's tensor at contrast 1
    "sector": ("sector", None, 1.0),
    "disc3": ("ball", 3, 1.0),                     # 320 cells: no multiple of floor(256 / (p + 1)) for any p
}


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def colour_ctx():
    c = mg.Context(0, options=dict(cell_colour_min=1))
    yield c
    c.close()


def rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def residual_case(mesh, p):
    """(square, level, reference, coefficient or None, src, rhs_q) of a mesh and degree, left unchanged by its users"""
    geometry, level, contrast = RESIDUAL_MESHES[mesh]
    sq = make_square(geometry, p, n_refine=level)
    l = sq.max_level
    R = pm.PoissonMappedReference2D.from_square(sq, l)
    coef = None if contrast is None else sq.problem_coef_q(l, mg.SquareProblem("shell", contrast))
    rng = np.random.default_rng(100 * p + len(mesh))
    src = sq.seeded_vector(l, 7)
    rhs_q = rng.standard_normal((sq.n_cells(l), (p + 1) ** 2)) * R.jxw_q
    return sq, l, R, coef, src, rhs_q


def run_residual(context, op, number, src, rhs_q):
    """dst of compute_residual, twice: the two calls are bitwise equal"""
    dt = np.float32 if number == mg.F32 else np.float64
    n = op.m()
    dst = context.vector(n, number, data=np.full(n, 3.0, dtype=dt))   # (whatever dst held is gone)
    s = None if src is None else context.vector(n, number, data=src.astype(dt))
    f = None if rhs_q is None else context.vector(rhs_q.size, number, data=rhs_q.ravel().astype(dt))
    op.compute_residual(dst, s, f)
    first = dst.download()
    dst.upload(np.full(n, -5.0, dtype=dt))
    op.compute_residual(dst, s, f)
    assert np.array_equal(dst.download(), first)
    for v in (dst, s, f):
        if v is not None:
            v.free()
    return first


@pytest.mark.parametrize("mesh", list(RESIDUAL_MESHES))
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", range(1, 10))
def test_residual(ctx, colour_ctx, p, number, mesh):
    """all three forms, both assembly routes, the three input combinations; constrained rows exactly zero"""
    num, dt = (mg.F32, np.float32) if number == "f32" else (mg.F64, np.float64)
    tol = 2e-5 if number == "f32" else 1e-13
    sq, l, R, coef, src, rhs_q = residual_case(mesh, p)
    ref_coef = R.ref.U if coef is None else coef
    # (the reference reads what the device reads: the inputs rounded to the number type)
    xs, fs = src.astype(dt).astype(np.float64), rhs_q.astype(dt).astype(np.float64)
    want = {"both": R.residual(ref_coef, xs, fs), "no_src": R.residual(ref_coef, None, fs), "no_rhs_q": R.residual(ref_coef, xs, None)}
    con = sq.constrained(l)
    for route, context in (("ordered", ctx), ("colours", colour_ctx)):
        op = mg.LaplaceOperator.from_cube(context, sq, l, num, coef_q=coef)
        for combo, (s, f) in (("both", (src, rhs_q)), ("no_src", (None, rhs_q)), ("no_rhs_q", (src, None))):
            got = run_residual(context, op, num, s, f)
            err = rel(got, want[combo])
            print("%s p=%d %s %s %s: %.3e" % (mesh, p, number, route, combo, err))
            assert err < tol
            assert np.array_equal(got[con], np.zeros(con.size, dtype=dt))
        op.clear()


@pytest.mark.parametrize("mesh", ["sheared_tensor", "disc3"])
@pytest.mark.parametrize("p", [1, 4, 9])
def test_residual_is_minus_the_unconstrained_operator(ctx, p, mesh):
    """independent of the reference: with rhs_q = NULL the free rows are minus vmult of an operator created from idx9_plain
    without constrained DoFs, applied to u_bc"""
    sq, l, R, coef, src, _ = residual_case(mesh, p)
    u_bc = np.zeros(sq.n_dofs(l))
    u_bc[sq.constrained(l)] = src[sq.constrained(l)]
    op = mg.LaplaceOperator.from_cube(ctx, sq, l, mg.F64, coef_q=coef)
    got = run_residual(ctx, op, mg.F64, u_bc, None)
    d = sq.operator_desc(l, mg.F64)
    d.idx27, d.constrained, d.n_constrained = d.idx27_plain, None, 0
    if coef is not None:
        keep = np.ascontiguousarray(coef)
        d.coef_q = keep.ctypes.data_as(_lib.f64p)
    plain = mg.LaplaceOperator(ctx, d)
    x, y = ctx.vector(u_bc.size, data=u_bc), ctx.vector(u_bc.size)
    plain.vmult(y, x)
    free = R.ref.free
    assert rel(got[free], -y.download()[free]) < 1e-13
    for v in (x, y):
        v.free()
    plain.clear()
    op.clear()


def test_residual_high_contrast(ctx):
    """contrast 1e6, fp64, disc level 3, p = 4: the bound is ten times the spread of the reference's own evaluations --
    cells added forward, reversed, and the whole evaluation in extended precision.  Measured spread: 6.9e-19 between
    the two orders (a DoF has at most five cells), 5.3e-16 against extended precision (the rounding inside a cell, where
    f JxW meets A u_bc, which the order of the cells does not show), so the bound is 5.3e-15; the device is at 2.5e-15."""
    p = 4
    sq, l, R, _, _, _ = residual_case("disc3", p)
    P, Pr = mg.SquareProblem("shell", 1.0e6), pm.Problem("shell", 1.0e6)
    fwd, rev = R.rhs(Pr), R.rhs(Pr, reverse=True)
    ext = R.rhs(Pr, dtype=np.longdouble).astype(np.float64)
    spread = max(rel(rev, fwd), rel(ext, fwd))
    print("spread: orders %.3e, extended %.3e" % (rel(rev, fwd), rel(ext, fwd)))
    op = mg.LaplaceOperator.from_cube(ctx, sq, l, mg.F64, coef_q=sq.problem_coef_q(l, P))
    u_bc = np.zeros(sq.n_dofs(l))
    u_bc[sq.constrained(l)] = sq.problem_bc_value(l, P)
    got = run_residual(ctx, op, mg.F64, u_bc, sq.problem_rhs_quadrature(l, P))
    err = rel(got, fwd)
    print("device against the reference: %.3e, bound %.3e" % (err, 10 * spread))
    assert err <= 10 * spread
    op.clear()


@pytest.mark.parametrize("vcycle", ["f64", "f32"])
@pytest.mark.parametrize("p", [2, 4])
def test_solver_compute_rhs(ctx, p, vcycle):
    """box + the box's own problem: the device right-hand sides are the host's on every level, CG takes the same number
    of iterations and ends at the same solution"""
    vnum = mg.F32 if vcycle == "f32" else mg.F64
    sq = mg.Square(p, 1, 3)
    host = mg.MultigridSolver(ctx, sq, 3, 3, 1, vnum, per_point=True)
    dev = mg.MultigridSolver(ctx, sq, 3, 3, 1, vnum, problem=mg.SquareProblem("cube"))
    for l in range(sq.n_levels):
        err = rel(dev.get_vector(l, "rhs").download(), host.get_vector(l, "rhs").download())
        print("level %d rhs %.3e" % (l, err))
        assert err < 1e-13
    its_h, _ = host.solve_cg()
    its_d, _ = dev.solve_cg()
    assert its_h == its_d
    assert rel(dev.get_solution().download(), host.get_solution().download()) < 1e-9
    assert abs(dev.compute_l2_error() - host.compute_l2_error()) < 1e-9 * host.compute_l2_error()
    dev.close()
    host.close()
    sq.close()


def error_operands(context, sq, l, P, number, vec):
    dt = np.float32 if number == mg.F32 else np.float64
    u_q, jxw = sq.problem_solution_q(l, P).astype(dt), sq.jxw_q(l).astype(dt)
    return (context.vector(vec.size, number, data=vec.astype(dt)), context.vector(u_q.size, number, data=u_q.ravel()),
            context.vector(jxw.size, number, data=jxw.ravel())), u_q.astype(np.float64), jxw.astype(np.float64)


@pytest.mark.parametrize("p", [1, 3, 4, 8, 9])
def test_l2_error_box(ctx, p):
    """box + the box's own problem against Square.l2_error, 1e-12"""
    sq = make_square("box", p)
    l, P = sq.max_level, mg.SquareProblem("cube")
    vec = sq.seeded_vector(l, 11)
    op = mg.LaplaceOperator.from_cube(ctx, sq, l, mg.F64)
    vectors, _, jxw = error_operands(ctx, sq, l, P, mg.F64, vec)
    got = op.compute_l2_error(*vectors)
    want = sq.l2_error(l, vec)
    assert abs(got - want) < 1e-12 * want
    sums = op.compute_l2_error(*vectors, sums=True)
    assert abs(sums[1] - jxw.sum()) < 1e-13 * jxw.sum()
    for v in vectors:
        v.free()
    op.clear()
    sq.close()


@pytest.mark.parametrize("mesh", ["sector", "disc3"])
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", [1, 2, 5, 8, 9])
def test_l2_error_curved(ctx, p, number, mesh):
    """disc and sector against the reference; sums[1] is the area; two calls give the same bits; an fp32 vector with sums
    to 1e-6 (the reference reads the rounded inputs: what differs is the interpolation in fp32)"""
    num, dt = (mg.F32, np.float32) if number == "f32" else (mg.F64, np.float64)
    tol = 1e-6 if number == "f32" else 1e-12
    sq, l, R, coef, src, _ = residual_case(mesh, p)
    P, Pr = mg.SquareProblem("shell", 1.0), pm.Problem("shell", 1.0)
    # a vector near the solution and one far from it
    for vec in (R.boundary_vector(Pr) + 0.0, src):
        vec = vec.astype(dt).astype(np.float64)
        op = mg.LaplaceOperator.from_cube(ctx, sq, l, num, coef_q=coef)
        vectors, u_q, jxw = error_operands(ctx, sq, l, P, num, vec)
        sums = op.compute_l2_error(*vectors, sums=True)
        again = op.compute_l2_error(*vectors, sums=True)
        assert np.array_equal(sums, again)
        uq = vec[R.ref.dofs_plain] @ R.S2.T
        want = np.array([((uq - u_q) ** 2 * jxw).sum(), jxw.sum()])
        print("%s p=%d %s: %.3e %.3e" % (mesh, p, number, abs(sums[0] - want[0]) / want[0], abs(sums[1] - want[1]) / want[1]))
        assert abs(sums[0] - want[0]) < tol * want[0] and abs(sums[1] - want[1]) < tol * want[1]
        if number == "f64":
            e, v = R.error_sums(Pr, vec)
            assert abs(sums[0] - e) < 1e-11 * e and abs(sums[1] - v) < 1e-12 * v
        for x in vectors:
            x.free()
        op.clear()


@functools.lru_cache(maxsize=None)
def dense_solution(p, level, contrast):
    sq = make_square("ball", p, n_refine=level)
    R = pm.PoissonMappedReference2D.from_square(sq, level)
    Pr = pm.Problem("shell", contrast)
    u = R.solve(Pr)
    return sq, u, R.l2_error(Pr, u)


@pytest.mark.parametrize("vcycle", ["f64", "f32"])
@pytest.mark.parametrize("contrast", [0.0, 100.0])
@pytest.mark.parametrize("p", [2, 3])
def test_end_to_end_on_the_disc(ctx, p, contrast, vcycle):
    """n_refine = 2: solve_cg reaches its reduction in fewer than 30 iterations, the solution is the reference's dense solve
    and the device's L2 error the reference's error of that solve"""
    sq, u, error = dense_solution(p, 2, contrast)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F32 if vcycle == "f32" else mg.F64, problem=mg.SquareProblem("shell", contrast))
    its, _ = solver.solve_cg()
    history = solver.cg_history()
    reduction = history[-1] / history[0]   # (solve_cg itself reports the mean rate per iteration)
    got = solver.get_solution().download()
    l2 = solver.compute_l2_error()
    print("p=%d contrast %g %s: %d iterations, reduction %.2e, solution %.3e, error %.6e (reference %.6e)" %
          (p, contrast, vcycle, its, reduction, rel(got, u), l2, error))
    assert its < 30 and len(history) == its + 1 and reduction <= 1e-9
    assert rel(got, u) < 1e-8
    assert abs(l2 - error) < 1e-6 * error
    solver.close()


def test_convergence_on_the_disc(ctx):
    """the error ratio of the level pair of the CPU test, from the device's solves and the device's error kernel"""
    p, levels = CONVERGENCE["p"], CONVERGENCE["levels"]
    errors = []
    for level in levels:
        sq = make_square("ball", p, n_refine=level)
        solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F32, problem=mg.SquareProblem("shell", 0.0))
        solver.solve_cg()
        errors.append(solver.compute_l2_error())
        solver.close()
        sq.close()
    print("disc p = %d, levels %s: errors %.3e %.3e, ratio %.2f" % (p, levels, errors[0], errors[1], errors[0] / errors[1]))
    assert errors[0] / errors[1] >= 0.8 * 2 ** (p + 1)


def status_of(call):
    s = call()
    return s, _lib.load().mgx_last_error().decode()


def test_refusals_and_lifetime(ctx):
    lib = _lib.load()
    start = lib.mgx_live_device_allocations()
    # the _2d calls on a 3D operator
    cube = mg.Cube(2, 1, 1)
    op3 = mg.LaplaceOperator.from_cube(ctx, cube, 1)
    solver3 = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
    v, w = ctx.vector(op3.m()), ctx.vector(op3.m())
    sums = np.zeros(2)
    for call in (lambda: lib.mgx_compute_residual_2d(op3.h, v.ptr, w.ptr, None),
                 lambda: lib.mgx_solver_compute_rhs_2d(solver3.h, 1, None),
                 lambda: lib.mgx_compute_l2_error_2d(op3.h, v.ptr, w.ptr, w.ptr, sums.ctypes.data_as(_lib.f64p))):
        status, reason = status_of(call)
        assert status == UNSUPPORTED and "three-dimensional" in reason
    for x in (v, w):
        x.free()
    solver3.close()
    op3.clear()
    cube.close()
    # arguments
    sq = mg.Square(2, n_refine=2, mapped="ball")
    l = sq.max_level
    op = mg.LaplaceOperator.from_cube(ctx, sq, l)
    v, w = ctx.vector(op.m()), ctx.vector(op.m())
    assert lib.mgx_compute_residual_2d(op.h, v.ptr, v.ptr, None) == INVALID_ARGUMENT       # dst == src
    assert lib.mgx_compute_residual_2d(op.h, None, w.ptr, None) == INVALID_ARGUMENT
    assert lib.mgx_compute_residual_2d(None, v.ptr, w.ptr, None) == INVALID_ARGUMENT
    assert lib.mgx_compute_l2_error_2d(op.h, v.ptr, None, w.ptr, sums.ctypes.data_as(_lib.f64p)) == INVALID_ARGUMENT
    assert lib.mgx_compute_l2_error_2d(op.h, v.ptr, w.ptr, w.ptr, None) == INVALID_ARGUMENT
    d = sq.operator_desc(l)
    d.idx27_plain = None
    bare = mg.LaplaceOperator(ctx, d)
    status, reason = status_of(lambda: lib.mgx_compute_residual_2d(bare.h, v.ptr, w.ptr, None))
    assert status == INVALID_ARGUMENT and "idx27_plain" in reason
    status, reason = status_of(lambda: lib.mgx_compute_l2_error_2d(bare.h, v.ptr, w.ptr, w.ptr, sums.ctypes.data_as(_lib.f64p)))
    assert status == INVALID_ARGUMENT and "idx27_plain" in reason
    bare.clear()
    for x in (v, w):
        x.free()
    op.clear()
    # the problem: none, an unknown kind, and the Python keywords that do not go together
    before = lib.mgx_live_device_allocations()
    s = _lib.CubeSolver()
    assert lib.mgx_square_solver_create_problem(ctx.h, sq.h, mg.F64, 3, 1, None, C.byref(s)) == INVALID_ARGUMENT
    unknown = _lib.SquareProblem(7, 0.0)
    status, reason = status_of(lambda: lib.mgx_square_solver_create_problem(ctx.h, sq.h, mg.F64, 3, 1, C.byref(unknown), C.byref(s)))
    assert status == INVALID_ARGUMENT and "kind" in reason
    with pytest.raises(_lib.MgxError):
        sq.problem_coef_q(l, None)
    with pytest.raises(_lib.MgxError):
        sq.problem_bc_value(l, mg.SquareProblem(7))
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, general=True, problem=mg.SquareProblem("shell", 1.0))
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, device_rhs=True)   # as before
    assert lib.mgx_live_device_allocations() == before   # refused creates leave nothing behind
    # 20 cycles of create, solve, error, close
    for _ in range(20):
        solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F32, problem=mg.SquareProblem("shell", 1.0))
        solver.solve_cg()
        assert solver.compute_l2_error() < 0.1
        solver.close()
    sq.close()
    assert lib.mgx_live_device_allocations() == start


def test_harness():
    """tools/poisson_shell.py 2 3000 --dim 2: exit status 0 and the program's table"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_shell.py"), "2", "3000", "--dim", "2"], check=True,
                         capture_output=True, text=True, timeout=600).stdout.strip().splitlines()
    head = [i for i, ln in enumerate(out) if ln.split() == ["cells", "dofs", "mv_outer", "mv_inner", "reduction", "fmg_L2error",
                                                             "fmg_time", "cg_L2error", "cg_time", "cg_its", "cg_reduction"]]
    assert len(head) == 1 and "Testing FE_Q<2>(2)" in out
    rows = [ln.split() for ln in out[head[0] + 1:]]
    # p = 2: 5 N^2 + 2 N + 1 DoFs with N = 2, 4, 8, 16 (1313 <= 3000 < 5185)
    assert [(int(r[0]), int(r[1])) for r in rows] == [(5, 25), (20, 89), (80, 337), (320, 1313)]
    assert all(np.isfinite(float(v)) for r in rows for v in r[2:])
