"""Ownership of device memory ("Device memory"): every API object keeps its device buffers in one arena and
the temporaries of a call live in an arena of that call, so whatever is created and destroyed again leaves
mgx_live_device_allocations() where it was.  Every case reads the counter, does its work, releases what it created
and compares: exact equality, there is nothing to tolerate.

Balanced lifecycles at the smallest shapes that build each table, then creates that are refused after their first
upload: those must free what they took.  The refused arguments are ordinary ones (an index out of range, an
inconsistent table); nothing here needs more than the suite's environment."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
_lib = mg._lib


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def live():
    return _lib.load().mgx_live_device_allocations()


def test_counter_follows_a_context():
    start = live()
    c = mg.Context(0)
    assert live() == start + 2   # block partials and result of the reductions
    c.close()
    assert live() == start


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("p,ns,nr", [(4, 1, 3), (2, 1, 2)])
def test_solver_lifecycle(ctx, p, ns, nr, number):
    """Cube(4, 1, 3): 1/8/64/512 cells; with the suite's MGX_BRICK_MIN=1 the two finest levels run on a brick
    schedule with its reduced-colour schedule and the fused-transfer tables, the two coarsest on the ordered
    assembly.  Cube(2, 1, 2): the p <= 2 path."""
    start = live()
    cube = mg.Cube(p, ns, nr)
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, number)
    l = cube.max_level
    if p == 4:
        assert cube.n_cells(l) == 512 and cube.n_cells(0) == 1
    created = live()
    assert created > start
    x = cube.seeded_vector(l, 3)
    src, dst = ctx.vector(x.size, data=x), ctx.vector(x.size)
    solver.vmult(dst, src)
    first = dst.download()
    assert np.isfinite(first).all() and np.abs(first).max() > 0
    cycled = live()   # (the smoothers of the brick levels allocate a third iterate buffer at their first step)
    assert cycled >= created
    mg.check(ctx.lib.mgx_solver_reset_smoother(solver.h, l, 20., 3, 15))
    assert cycled - 1 <= live() <= cycled   # the new smoother's two buffers for the old one's two or three
    mg.check(ctx.lib.mgx_solver_set_polynomial_type(solver.h, mg.Chebyshev.POLYNOMIAL["fourth_kind"]))
    assert cycled - 1 <= live() <= cycled
    solver.close()
    cube.close()
    assert live() == start


def test_general_operator_replaces_its_geometry(ctx):
    """per-point coefficient on the smallest sheared box of test_gpu_shell.py; the second
    mgx_operator_enable_coefficient_update_q replaces the geometry of the first"""
    start = live()
    cube = mg.Cube(8, n_refine=1, box=(1, 1, 1), origin=-0.9, h0=1.9, geometry="sheared", problem="cube")
    l = cube.max_level
    for number in (mg.F64, mg.F32):
        op = mg.LaplaceOperator.from_cube(ctx, cube, l, number)
        U, w = cube.coef_q(l), cube.jxw_q(l)
        created = live()
        op.enable_coefficient_update_q(U, w)
        assert live() == created + 2
        op.enable_coefficient_update_q(U, w)
        assert live() == created + 2
        op.enable_coefficient_update([1., 1., 1., 0., 0., 0.], 1.)   # affine geometry instead: the per-point arrays go
        assert live() == created
        op.enable_coefficient_update_q(U, w)
        op.clear()
        assert live() == start
    cube.close()
    assert live() == start


def test_calls_with_temporaries_and_lazy_buffers(ctx):
    """one call each of mgx_interpolate_to_coarse, mgx_compute_residual with src = NULL, mgx_vmult_with_cg_update and
    mgx_compute_diagonal, on a brick level (Cube(2, 1, 2), level 2: 64 cells) and on an ordered-assembly level"""
    start = live()
    cube = mg.Cube(2, 1, 2)
    ops = [mg.LaplaceOperator.from_cube(ctx, cube, l) for l in range(cube.n_levels)]
    tr = mg.Transfer(ops[1], ops[2], cube.children(2), cube.prolong_1d())
    created = live()
    fine = ctx.vector(cube.n_dofs(2), data=cube.seeded_vector(2, 1))
    coarse = ctx.vector(cube.n_dofs(1))
    tr.interpolate_to_coarse(coarse, fine)
    assert live() == created + 2   # 1D matrix and ownership of the coarse cells, built at the first call
    tr.interpolate_to_coarse(coarse, fine)
    assert live() == created + 2
    for l in (1, 2):
        op, n = ops[l], cube.n_dofs(l)
        before = live()
        fq = cube.rhs_quadrature(l)
        dst, f = ctx.vector(n), ctx.vector(fq.size, data=fq.ravel())
        op.compute_residual(dst, None, f)
        assert live() == before   # the zero vector and the cell lists were this call's
        op.compute_diagonal()
        tables = live()
        op.compute_diagonal()   # replaces the per-item diagonal tables of a brick level
        assert live() == tables
        r, q, pp, x = (ctx.vector(n, data=cube.seeded_vector(l, s)) for s in (2, 3, 4, 5))
        sums = op.vmult_with_cg_update(0.3, 0.7, r, q, pp, x)
        assert np.isfinite(sums).all()
        grown = live()
        assert grown >= tables + 2   # partial sums and their result (and the carrier of the brick loop), kept
        op.vmult_with_cg_update(0.3, 0.7, r, q, pp, x)
        assert live() == grown
    tr.clear()
    for op in ops:
        op.clear()
    cube.close()
    assert live() == start


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
def test_dg_operator_and_solver_lifecycle(ctx, number):
    """the smallest mesh of test_gpu_dg_multigrid.py: FE_DGQ(5) on 2^3 cells over its FE_Q hierarchy"""
    start = live()
    cube = mg.Cube(5, 1, 1)
    solver = mg.DGMultigridSolver(ctx, cube, mg.DG_HERMITE, 3, number)
    assert live() > start
    rng = np.random.default_rng(0)
    src = solver.initialize_dof_vector(rng.standard_normal(solver.m()))
    dst = solver.initialize_dof_vector()
    solver.vmult(dst, src)
    assert np.isfinite(dst.download()).all()
    A = solver.matrix_dg
    r, q, pp, x = (A.initialize_dof_vector(rng.standard_normal(A.m())) for _ in range(4))
    before = live()
    A.vmult_with_cg_update(0.3, 0.7, r, q, pp, x)
    assert live() == before + 2   # block sums and their total, allocated at the first use
    A.vmult_with_cg_update(0.3, 0.7, r, q, pp, x)
    assert live() == before + 2
    solver.close()
    cube.close()
    assert live() == start


# ---- failed creates free what they took ----

def test_refusals_of_test_error_paths_leave_nothing(ctx):
    start = live()
    cube = mg.Cube(3, 1, 1)
    d = cube.operator_desc(1)
    bad = cube.idx27(1).copy().ravel()
    bad[5] = cube.n_dofs(1) + 7
    d.idx27 = bad.ctypes.data_as(_lib.u32p)
    with pytest.raises(mg.MgxError):
        mg.LaplaceOperator(ctx, d)
    assert live() == start
    d2 = cube.operator_desc(1)
    d2.coef[3] = 10.0 * d2.coef[0]
    with pytest.raises(mg.MgxError):
        mg.LaplaceOperator(ctx, d2)
    assert live() == start
    op = mg.LaplaceOperator.from_cube(ctx, cube, 1)
    held = live()
    v = op.initialize_dof_vector()
    with pytest.raises(mg.MgxError):
        op.vmult(v, v)
    assert live() == held
    op.clear()
    cube.close()
    assert live() == start


def test_refused_exchange_plan_frees_the_operator(ctx):
    """an exchange plan on a context without a communicator is refused by the last stage of mgx_operator_create, after
    every table of the operator has been uploaded"""
    start = live()
    cube = mg.Cube(2, 1, 2)
    d = cube.operator_desc(2)
    ex = _lib.ExchangeDesc()
    d.exchange = C.pointer(ex)
    with pytest.raises(mg.MgxError, match="no communicator"):
        mg.LaplaceOperator(ctx, d)
    assert live() == start
    cube.close()


def test_transfer_create_with_inconsistent_weight_shift(ctx):
    start = live()
    cube = mg.Cube(2, 1, 2)
    coarse, fine = (mg.LaplaceOperator.from_cube(ctx, cube, l) for l in (1, 2))
    held = live()
    children = np.ascontiguousarray(cube.children(2), dtype=np.uint32)
    p1 = np.ascontiguousarray(cube.prolong_1d(), dtype=np.float64)
    shift = np.zeros(27 * cube.n_cells(1), dtype=np.uint8)
    shift[-1] = 4   # a weight 2^-4: no multiplicity of a uniform mesh
    desc = _lib.TransferDesc(children.ctypes.data_as(_lib.u32p), p1.ctypes.data_as(_lib.f64p),
                             shift.ctypes.data_as(C.POINTER(C.c_uint8)))
    h = C.c_void_p()
    with pytest.raises(mg.MgxError, match="inconsistent weight_shift"):
        mg.check(ctx.lib.mgx_transfer_create(coarse.h, fine.h, C.byref(desc), C.byref(h)))
    assert not h.value
    assert live() == held   # the children table was on the device by then
    tr = mg.Transfer(coarse, fine, children, p1)   # the same levels are valid
    assert live() > held
    tr.clear()
    coarse.clear()
    fine.clear()
    cube.close()
    assert live() == start


def test_solver_create_with_boundary_index_out_of_range(ctx):
    start = live()
    cube = mg.Cube(2, 1, 2)
    nl = cube.n_levels
    ops = [mg.LaplaceOperator.from_cube(ctx, cube, l) for l in range(nl)]
    trs = [None] + [mg.Transfer(ops[l - 1], ops[l], cube.children(l), cube.prolong_1d()) for l in range(1, nl)]
    held = live()
    bcs = [cube.bc(l) for l in range(nl)]
    index = [np.array(b[0], dtype=np.uint32) for b in bcs]   # (copies: one entry is overwritten below)
    value = [np.array(b[1], dtype=np.float64) for b in bcs]
    assert index[nl - 1].size > 0
    index[nl - 1][-1] = cube.n_dofs(nl - 1)   # one past the last DoF of its level
    vp = C.c_void_p
    matrix = (vp * nl)(*[op.h for op in ops])
    transfer = (vp * nl)(*[None if t is None else t.h for t in trs])
    desc = _lib.SolverDesc(nl, 3, 1, matrix, matrix, transfer, transfer, None,
                           (_lib.u32p * nl)(*[a.ctypes.data_as(_lib.u32p) for a in index]),
                           (_lib.f64p * nl)(*[a.ctypes.data_as(_lib.f64p) for a in value]),
                           (C.c_uint32 * nl)(*[a.size for a in index]))
    h = vp()
    with pytest.raises(mg.MgxError, match="boundary index out of range"):
        mg.check(ctx.lib.mgx_solver_create(ctx.h, C.byref(desc), C.byref(h)))
    assert not h.value
    assert live() == held   # the vectors of every level before the refused one were allocated by then
    index[nl - 1][-1] = bcs[nl - 1][0][-1]
    assert index[nl - 1][-1] < cube.n_dofs(nl - 1)
    mg.check(ctx.lib.mgx_solver_create(ctx.h, C.byref(desc), C.byref(h)))   # the same descriptor is valid now
    assert live() > held
    mg.check(ctx.lib.mgx_solver_destroy(h))
    for t in trs[1:]:
        t.clear()
    for op in ops:
        op.clear()
    cube.close()
    assert live() == start
