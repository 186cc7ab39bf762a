"""GPU tests of the FE_Q Laplace operator and geometric multigrid in two dimensions (mgx_operator_desc::dim == 2,
multigrid_amd.Square) against the numpy reference of tests/feq_reference_2d.py.

Tolerances, all max|a - b| / max|b| (those of tests/test_gpu_parity.py): fp64 vmult and residual 1e-12, inverse
diagonal 1e-13, Chebyshev 1e-10, transfers 1e-13, V-cycle 1e-9, smoother info 1e-8 with exact counts; fp32 vmult 3e-6,
fp32 V-cycle 2e-4.
Bounds the parity tests do not name:
  fp32 residual and inverse diagonal, 3e-6: a residual is the product and one subtraction of numbers of the product's
    size; an entry of the diagonal is a sum of at most four cell terms, far fewer roundings than a product's.
  fp32 transfers, 2e-5: a prolongated value is two sweeps of p + 1 <= 10 multiply-adds, error <= 2 (p + 1) u L^2 max|x|
    with u = 6e-8 and L <= 2.5 the Lebesgue constant of the Gauss-Lobatto nodes, 7.5e-6, relative to max|P x| >= max|x|
    (the embedding is interpolatory); a restricted value is two sweeps of 2p + 1 <= 19 of them, 2 (2p + 1) u = 2.3e-6
    times the squared 1D column sum of |P| (<= 3^2), 2e-5 of max|fine|, and max|R fine| >= max|fine| for the seeded
    vectors (every coarse vertex value is the fine value at that vertex plus its neighbours' shares).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import feq_reference_2d as ref  # noqa: E402

_lib = mg._lib
UNSUPPORTED, INVALID_ARGUMENT = -4, -1
SHEAR = [[1.0, 0.35], [0.15, 0.8]]
STRETCH = [[1.0, 0.0], [0.0, 0.7]]   # diagonal coefficient with xx != yy
MESHES = {"2x2": dict(box=(2, 2), n_refine=0, h0=0.95), "17x11": dict(box=(17, 11), n_refine=0, h0=0.1)}
FORMS = ["diagonal", "tensor", "per_point_sheared", "per_point_varying"]


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


def to_grid(sq, l, v):
    out = np.empty(sq.n_dofs(l))
    out[sq.dof_grid(l)] = v
    return out


def from_grid(sq, l, g):
    return np.ascontiguousarray(np.asarray(g).ravel()[sq.dof_grid(l)])


def make_form(ctx, p, mesh, form, number):
    """(square, operator on level 0 of the mesh, reference level)"""
    sq = mg.Square(p, jacobian=STRETCH if form == "diagonal" else SHEAR, **MESHES[mesh])
    e = ref.arrays_1d(sq)
    coef = ref.Problem(e, A=STRETCH if form == "diagonal" else SHEAR).coef()
    cells, n = sq.cells_per_dim2(0), p + 1
    if form in ("diagonal", "tensor"):
        assert (coef[2] == 0) == (form == "diagonal")
        return sq, mg.LaplaceOperator.from_cube(ctx, sq, 0, number), ref.Level(e, cells, coef)
    cq = sq.coef_q(0)
    if form == "per_point_varying":   # seeded, symmetric positive definite: [1 + a, c; c, 1 + b], |c| <= 1/2
        rng = np.random.default_rng(1000 * p + len(mesh))
        w = np.outer(sq.qweights(), sq.qweights()).ravel()
        cq = np.stack([1 + rng.random((len(cq), n * n)), 1 + rng.random((len(cq), n * n)), rng.random((len(cq), n * n)) - 0.5], axis=1) * w
    cc = sq.cell_coords(0)
    by_coords = np.empty((cells[1], cells[0], 3, n, n))
    by_coords[cc[:, 1], cc[:, 0]] = cq.reshape(-1, 3, n, n)
    return sq, mg.LaplaceOperator.from_cube(ctx, sq, 0, number, coef_q=cq), ref.Level(e, cells, coef_q=by_coords)


def check_operator(ctx, sq, op, L, number, reproducible):
    f32 = number == mg.F32
    dt = np.float32 if f32 else np.float64
    x, b = sq.seeded_vector(0, 1).astype(dt), sq.seeded_vector(0, 2).astype(dt)
    src, rhs, dst = ctx.vector(x.size, number, data=x), ctx.vector(x.size, number, data=b), ctx.vector(x.size, number)
    op.vmult(dst, src)
    got = dst.download()
    want = from_grid(sq, 0, L.vmult(to_grid(sq, 0, x)))
    err = rel(got, want)
    print("vmult %.3e" % err)
    assert err < (3e-6 if f32 else 1e-12)
    con = sq.constrained(0)
    assert np.array_equal(got[con], x[con])   # identity rows
    if reproducible:
        dst.upload(np.full(x.size, 3.0, dtype=dt))
        op.vmult(dst, src)
        assert np.array_equal(dst.download(), got)
    op.vmult_residual(rhs, src, dst)
    err = rel(dst.download(), from_grid(sq, 0, L.vmult_residual(to_grid(sq, 0, b), to_grid(sq, 0, x))))
    print("residual %.3e" % err)
    assert err < (3e-6 if f32 else 1e-12)
    op.compute_diagonal()
    dinv = op.get_matrix_diagonal_inverse().download()
    err = rel(dinv, from_grid(sq, 0, L.inv_diag()))
    print("inverse diagonal %.3e" % err)
    assert err < (3e-6 if f32 else 1e-13)
    assert np.array_equal(dinv[con], np.ones(con.size, dtype=dt))
    for v in (src, rhs, dst):
        v.free()
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", range(1, 10))
def test_operator(ctx, p, number, mesh, form):
    """all three forms through the ordered assembly; two applications on the 187-cell mesh are bitwise equal (187 = 11 x
    17 cells: more than one workgroup at every degree, and no cells-per-workgroup count floor(256 / (p + 1)) = 128, 85,
    64, 51, 42, 36, 32, 28, 25 divides it)"""
    num = mg.F32 if number == "f32" else mg.F64
    sq, op, L = make_form(ctx, p, mesh, form, num)
    check_operator(ctx, sq, op, L, num, reproducible=mesh == "17x11")
    op.clear()
    sq.close()


@pytest.mark.parametrize("form", ["diagonal", "tensor", "per_point_varying"])
@pytest.mark.parametrize("p", range(1, 10))
def test_colour_route(ctx, colour_ctx, p, form):
    """cell_colour_min = 1: no ordered assembly, one launch per colour with plain adds.  Same comparisons; bitwise equal
    between two runs; equal to the ordered route within 1e-13"""
    sq, op, L = make_form(colour_ctx, p, "17x11", form, mg.F64)
    got = check_operator(colour_ctx, sq, op, L, mg.F64, reproducible=True)
    sq2, op2, _ = make_form(ctx, p, "17x11", form, mg.F64)
    x = sq2.seeded_vector(0, 1)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    op2.vmult(dst, src)
    assert rel(got, dst.download()) < 1e-13
    for o in (op, op2):
        o.clear()
    sq.close()
    sq2.close()


@pytest.mark.parametrize("kind", ["first_kind", "fourth_kind"])
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_smoother(ctx, p, kind):
    sq = mg.Square(p, 1, 2)
    s = ref.Solver(ref.arrays_1d(sq), (1, 1), 3, 1.9, fourth_kind=kind == "fourth_kind")
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, polynomial=kind)
    for l in range(sq.n_levels):
        sm = solver.smoother(l)
        gi, oi = sm.info(), s.info[l]
        assert gi["degree"] == oi["degree"] and gi["cg_its"] == oi["cg_its"]
        for k in ("lambda_max", "theta"):
            assert gi[k] == pytest.approx(oi[k], rel=1e-8)
        want_delta = oi["lambda_max"] if (kind == "fourth_kind" and l > 0) else oi["delta"]
        assert gi["delta"] == pytest.approx(want_delta, rel=1e-8, abs=1e-8 * oi["lambda_max"])
        b = sq.seeded_vector(l, 7)
        bd, xd = ctx.vector(b.size, data=b), ctx.vector(b.size)
        sm.vmult(xd, bd)
        x_ref = s.smooth(l, None, to_grid(sq, l, b), False)
        assert rel(xd.download(), from_grid(sq, l, x_ref)) < 1e-10
        sm.step(xd, bd)
        assert rel(xd.download(), from_grid(sq, l, s.smooth(l, x_ref, to_grid(sq, l, b), True))) < 1e-10
    solver.close()
    sq.close()


TRANSFER_MESHES = {"1x1": dict(n_subdiv=1, n_refine=1), "3x2": dict(box=(3, 2), n_refine=1, h0=0.5)}


@pytest.mark.parametrize("mesh", list(TRANSFER_MESHES))
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", range(1, 10))
def test_transfers(ctx, p, number, mesh):
    f32 = number == "f32"
    num, dt, tol = (mg.F32, np.float32, 2e-5) if f32 else (mg.F64, np.float64, 1e-13)
    sq = mg.Square(p, **TRANSFER_MESHES[mesh])
    e = ref.arrays_1d(sq)
    T = ref.Transfer(ref.Level(e, sq.cells_per_dim2(0)), ref.Level(e, sq.cells_per_dim2(1)))
    ops = [mg.LaplaceOperator.from_cube(ctx, sq, l, num) for l in range(2)]
    tr = mg.Transfer(ops[0], ops[1], sq.children(1), sq.prolong_1d())
    xc, xf = sq.seeded_vector(0, 11).astype(dt), sq.seeded_vector(1, 12).astype(dt)
    gc, gf = to_grid(sq, 0, xc), to_grid(sq, 1, xf)
    dc, df = ctx.vector(xc.size, num, data=xc), ctx.vector(xf.size, num, data=xf)
    out = ctx.vector(xf.size, num)
    for bc in (False, True):
        out.upload(np.full(xf.size, 7.0, dtype=dt))
        tr.prolongate(out, dc, with_constraints=bc)   # overwrite: every fine entry is written
        assert rel(out.download(), from_grid(sq, 1, T.prolongate(gc, with_bc=bc))) < tol
        out.upload(xf)
        tr.prolongate_and_add(out, dc, with_constraints=bc)
        assert rel(out.download(), from_grid(sq, 1, T.prolongate(gc, fine=gf, with_bc=bc))) < tol
        outc = ctx.vector(xc.size, num, data=xc)
        tr.restrict_and_add(outc, df, with_constraints=bc)
        assert rel(outc.download(), from_grid(sq, 0, T.restrict_and_add(gc, gf, with_bc=bc))) < tol
        outc.free()
    if not f32:   # <P v, w> = <v, R w>
        zero = ctx.vector(xc.size, data=np.zeros(xc.size))
        tr.prolongate(out, dc, with_constraints=False)
        tr.restrict_and_add(zero, df, with_constraints=False)
        assert np.vdot(out.download(), xf) == pytest.approx(np.vdot(xc, zero.download()), rel=1e-12)
    # a children table that is no permutation, and a 2D / 3D pair
    bad = sq.children(1).copy()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(mg.MgxError) as err:
        mg.Transfer(ops[0], ops[1], bad, sq.prolong_1d())
    assert err.value.status == INVALID_ARGUMENT
    if p == 2 and not f32:
        cube = mg.Cube(p, 1, 1)
        op3 = mg.LaplaceOperator.from_cube(ctx, cube, 1)
        with pytest.raises(mg.MgxError) as err:
            mg.Transfer(ops[0], op3, cube.children(1), sq.prolong_1d())
        assert err.value.status == INVALID_ARGUMENT
        op3.clear()
        cube.close()
    tr.clear()
    for o in ops:
        o.clear()
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 4, 7])
def test_solver(ctx, p):
    """Square(p, 1, 3): levels 0..3, 8^2 cells (p = 1: level 0 has no unknown)"""
    sq = mg.Square(p, 1, 3)
    s = ref.Solver(ref.arrays_1d(sq), (1, 1), 4, 1.9)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64)
    l = sq.max_level
    x = sq.seeded_vector(l, 5)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size, data=np.full(x.size, np.nan))
    solver.vmult(dst, src)
    assert rel(dst.download(), from_grid(sq, l, s.v_cycle(to_grid(sq, l, x)))) < 1e-9
    assert np.array_equal(src.download(), x)
    rate, trace = solver.solve(True)
    otrace = s.solve()
    np.testing.assert_allclose(trace[1:, 0], otrace[1:, 0], rtol=1e-9)   # residual start
    np.testing.assert_allclose(trace[1:, 1], otrace[1:, 1], rtol=1e-6)   # residual end
    assert rel(solver.get_solution().download(), from_grid(sq, l, s.get_solution())) < 1e-9
    its, red = solver.solve_cg()
    oits, ored = s.solve_cg()
    assert its == oits
    np.testing.assert_allclose(solver.cg_history(), s.cg_history, rtol=1e-6)
    assert rel(solver.get_solution().download(), from_grid(sq, l, s.get_solution())) < 1e-8
    err = solver.compute_l2_error()
    res, upd = sq.seeded_vector(l, 21), sq.seeded_vector(l, 22)
    for factor in (0.0, -0.43):
        r, u = ctx.vector(res.size, data=res), ctx.vector(res.size, data=upd)
        out = solver.vmult_with_residual_update(r, u, factor)
        ores, oupd, oout = s.vmult_with_residual_update(to_grid(sq, l, res), to_grid(sq, l, upd), factor)
        np.testing.assert_allclose(out, oout, rtol=1e-9)
        assert rel(r.download(), from_grid(sq, l, ores)) < 1e-14
        assert rel(u.download(), from_grid(sq, l, oupd)) < 1e-9
    fits, fred = solver.solve_cg_fused()
    assert fits == its
    assert fred == pytest.approx(red, rel=1e-6)
    assert solver.compute_l2_error() == pytest.approx(err, rel=1e-6)
    solver.close()
    # fp32 V-cycle inside the fp64 interface
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F32)
    solver.vmult(dst, src)
    assert rel(dst.download(), from_grid(sq, l, s.v_cycle(to_grid(sq, l, x)))) < 2e-4
    assert solver.solve_cg()[0] == oits
    solver.close()
    sq.close()


@pytest.mark.parametrize("p,n_refine", [(2, 4), (4, 3)])
def test_l2_error_of_the_solve(ctx, p, n_refine):
    """after solve_cg within 1e-3 (relative) of the L2 error of the reference's dense solve of the same system: the
    algebraic error left by a 1e-9 residual reduction is orders below that, an indexing or boundary-value mistake
    orders above"""
    sq = mg.Square(p, 1, n_refine)
    e = ref.arrays_1d(sq)
    n = 1 << n_refine
    L, prob = ref.Level(e, (n, n)), ref.Problem(e)
    want = prob.l2_error(L, 1.9 / n, prob.dense_solution(L, 1.9 / n))
    for per_point in (False, True):
        solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, per_point=per_point)
        solver.solve_cg()
        got = solver.compute_l2_error()
        print("p=%d %d^2 cells: L2 error %.6e, dense solve %.6e" % (p, n, got, want))
        assert got == pytest.approx(want, rel=1e-3)
        solver.close()
    sq.close()


def status_of(call):
    s = call()
    return s, _lib.load().mgx_last_error().decode()


def test_refusals_and_lifetime(ctx):
    lib = _lib.load()
    start = lib.mgx_live_device_allocations()
    sq = mg.Square(2, 1, 2)

    def refused(status_and_reason):
        status, reason = status_and_reason
        assert status == UNSUPPORTED and reason

    # an exchange plan; a context with a communicator (operator and solver creation)
    d, h = sq.operator_desc(2), C.c_void_p()
    ex = _lib.ExchangeDesc()
    d.exchange = C.pointer(ex)
    refused(status_of(lambda: lib.mgx_operator_create(ctx.h, C.byref(d), C.byref(h))))
    ctx2 = mg.Context(0)
    keep = (_lib.EXCHANGE_FN(lambda *a: 1), _lib.ALLREDUCE_FN(lambda *a: 1))
    comm = _lib.CommDesc(0, 2, None, keep[0], keep[1], _lib.ALLOC_FN())
    assert lib.mgx_context_set_comm(ctx2.h, C.byref(comm)) == 0
    d = sq.operator_desc(2)
    refused(status_of(lambda: lib.mgx_operator_create(ctx2.h, C.byref(d), C.byref(h))))
    s = _lib.CubeSolver()
    refused(status_of(lambda: lib.mgx_square_solver_create(ctx2.h, sq.h, mg.F64, 3, 1, 0, C.byref(s))))
    ctx2.close()
    assert lib.mgx_live_device_allocations() == start   # refused creates leave nothing behind
    for bad in (1, 4):
        d = sq.operator_desc(2)
        d.dim = bad
        assert lib.mgx_operator_create(ctx.h, C.byref(d), C.byref(h)) == INVALID_ARGUMENT
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, comm=object())
    with pytest.raises(ValueError):
        mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, agglomerate=False)

    # the entry points that exist in three dimensions only
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, per_point=True)
    other = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64)
    op, l = solver.matrix_dp(2), 2
    v, w = ctx.vector(sq.n_dofs(l)), ctx.vector(sq.n_dofs(l))
    coarse = ctx.vector(sq.n_dofs(l - 1))
    six, one = (C.c_double * 6)(1, 1, 1, 0, 0, 0), np.ones(sq.n_cells(l) * 6 * 27)
    ids, owned = np.zeros(sq.n_dofs(1), dtype=np.uint32), np.ones(sq.n_dofs(1), dtype=np.uint8)
    f64p = _lib.f64p
    refused(status_of(lambda: lib.mgx_compute_residual(op.h, v.ptr, w.ptr, None)))
    refused(status_of(lambda: lib.mgx_solver_compute_rhs(solver.h, l, None)))
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update(op.h, six, 1.0)))
    refused(status_of(lambda: lib.mgx_operator_enable_coefficient_update_q(op.h, one.ctypes.data_as(f64p), one.ctypes.data_as(f64p))))
    refused(status_of(lambda: lib.mgx_evaluate_coefficient(op.h, 0, v.ptr)))
    refused(status_of(lambda: lib.mgx_compute_nonlinear_residual(op.h, 0, v.ptr, w.ptr)))
    refused(status_of(lambda: lib.mgx_interpolate_to_coarse(solver.transfer_dp(l).h, coarse.ptr, v.ptr)))
    refused(status_of(lambda: lib.mgx_solver_update_coefficient(solver.h, 0, v.ptr)))
    refused(status_of(lambda: lib.mgx_solver_set_agglomeration(solver.h, 1, other.h, ids.ctypes.data_as(_lib.u32p),
                                                                owned.ctypes.data_as(C.POINTER(C.c_uint8)), ids.size)))
    # a DG level on top of the 2D FE_Q hierarchy
    nb, _ = mg.dg_box_neighbours((2, 2, 2))
    jac = np.eye(3) * 0.5
    dg32, dg64 = (mg.DGLaplaceOperator(ctx, 2, mg.DG_HERMITE, nb, jac, n) for n in (mg.F32, mg.F64))
    gid = np.arange(8, dtype=np.uint32)
    dd = _lib.DGSolverDesc(dg64.h, dg64.h, solver.h, 3, gid.ctypes.data_as(_lib.u32p))
    refused(status_of(lambda: lib.mgx_dg_solver_create(ctx.h, C.byref(dd), C.byref(h))))
    dg32.clear()
    dg64.clear()
    # the per-point coefficient of a 2D operator: [n_cells][3][(p+1)^2]
    ptr, count = C.c_void_p(), C.c_size_t()
    assert lib.mgx_operator_get_coefficient(op.h, C.byref(ptr), C.byref(count)) == 0
    assert count.value == sq.n_cells(l) * 3 * 9
    got = mg.DeviceVector(ctx, count.value, mg.F64, ptr=ptr).download()
    assert rel(got, sq.coef_q(l).ravel()) < 1e-15
    idx, nc, nd, deg = _lib.u32p(), C.c_uint32(), C.c_uint32(), C.c_int()
    assert lib.mgx_operator_device_indices(op.h, C.byref(idx), C.byref(nc), C.byref(nd), C.byref(deg)) == 0
    assert (nc.value, nd.value, deg.value) == (sq.n_cells(l), sq.n_dofs(l), 2)
    # a full cycle: create, solve, timings, close
    solver.enable_timings(True)
    solver.solve(True)
    its, _ = solver.solve_cg()
    assert its > 0 and solver.wall_times().shape == (3, 6)
    solver.do_matvec()
    solver.do_matvec_smoother()
    for x in (v, w, coarse):
        x.free()
    other.close()
    solver.close()
    sq.close()
    assert lib.mgx_live_device_allocations() == start


def test_dim_0_and_3_are_the_same_operator(ctx):
    cube = mg.Cube(3, 1, 1)
    x = cube.seeded_vector(1, 4)
    out = []
    for dim in (0, 3):
        d = cube.operator_desc(1)
        assert d.dim == 3
        d.dim = dim
        op = mg.LaplaceOperator(ctx, d)
        src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
        op.vmult(dst, src)
        out.append(dst.download())
        op.clear()
    assert np.array_equal(out[0], out[1])
    cube.close()


def test_harness(ctx):
    """tools/poisson_cube_2d.py 4 3: the printed L2 errors are the solver's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "poisson_cube_2d.py"), "4", "3"], check=True,
                         capture_output=True, text=True, timeout=600).stdout.strip().splitlines()
    assert out[0].split() == ["cells", "dofs", "reduction", "fmg_L2error", "cg_L2error", "cg_its"]
    row = out[1].split()
    sq = mg.Square(4, 1, 3)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F32)
    assert (int(row[0]), int(row[1])) == (64, 33 * 33)
    solver.solve(True)
    assert float(row[3]) == solver.compute_l2_error()
    its, _ = solver.solve_cg()
    assert float(row[4]) == solver.compute_l2_error() and int(row[5]) == its
    solver.close()
    sq.close()
