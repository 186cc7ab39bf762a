"""BASELINE config C2 at full size (FE_Q(4), 128^3 cells, 135 005 697 DoFs, one MI355X): the oracle
cannot run this size in seconds, so the HIP path is checked through size-independent properties of
the operator and of the V-cycle (symmetry, linearity, reproducibility, residual identity, Dirichlet
rows) and through the discretisation error of the full solve, which the reference prints in its
README (README.md:128,159: 4.342e-10 after FMG with 2 cycles, 4.2068e-10 after PCG, 8 iterations)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")


# C2: FE_Q(4) on 128^3 cells; C3: FE_Q(8) on 64^3 cells -- both 513^3 = 135 005 697 DoFs
@pytest.fixture(scope="module", params=[(4, 7), (8, 6)], ids=["C2-p4", "C3-p8"])
def big(request):
    p, nr = request.param
    ctx = mg.Context(0)
    cube = mg.Cube(p, 1, nr)
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
    yield ctx, cube, solver
    solver.close()
    cube.close()
    ctx.close()


def test_c2_operator_properties(big):
    ctx, cube, solver = big
    l = cube.max_level
    n = cube.n_dofs(l)
    assert n == 135005697  # README.md:65
    A = solver.matrix_dp(l)
    x = ctx.vector(n, data=cube.seeded_vector(l, 1))
    y = ctx.vector(n, data=cube.seeded_vector(l, 2))
    Ax, Ay, t = ctx.vector(n), ctx.vector(n), ctx.vector(n)
    A.vmult(Ax, x)
    A.vmult(Ay, y)
    # symmetry  y.(A x) = x.(A y)
    assert ctx.dot(y, Ax) == pytest.approx(ctx.dot(x, Ay), rel=1e-11)
    assert ctx.dot(x, Ax) > 0
    # linearity  A(2x - 3y) = 2 Ax - 3 Ay
    lib = ctx.lib
    mg.check(lib.mgx_copy_cast(ctx.h, t.ptr, mg.F64, x.ptr, mg.F64, n))
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, t.ptr, 2.0, -3.0, y.ptr, n))  # t = 2x - 3y
    At = ctx.vector(n)
    A.vmult(At, t)
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, At.ptr, 1.0, -2.0, Ax.ptr, n))
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, At.ptr, 1.0, 3.0, Ay.ptr, n))
    assert ctx.l2_norm(At) < 1e-12 * ctx.l2_norm(Ax)
    # bitwise reproducible (no atomics on the brick path)
    A.vmult(At, x)
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, At.ptr, 1.0, -1.0, Ax.ptr, n))
    assert ctx.l2_norm(At) == 0.0
    # residual identity  r = b - A x  and Dirichlet rows act as the identity
    A.vmult_residual(y, x, t)
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, t.ptr, 1.0, 1.0, Ax.ptr, n))
    mg.check(lib.mgx_sadd(ctx.h, mg.F64, t.ptr, 1.0, -1.0, y.ptr, n))
    assert ctx.l2_norm(t) < 1e-12 * ctx.l2_norm(Ax)
    nc = cube.n_constrained(l)
    tail_x = np.empty(nc)
    tail_a = np.empty(nc)
    off = (n - nc) * 8
    import ctypes as C
    mg.check(lib.mgx_download(ctx.h, tail_x.ctypes.data_as(C.c_void_p), C.c_void_p(x.ptr.value + off), nc * 8))
    mg.check(lib.mgx_download(ctx.h, tail_a.ctypes.data_as(C.c_void_p), C.c_void_p(Ax.ptr.value + off), nc * 8))
    assert np.array_equal(tail_x, tail_a)  # laplace_operator.h:592-593
    for v in (x, y, Ax, Ay, t, At):
        v.free()


def test_c2_vcycle_is_symmetric_and_linear(big):
    """the V-cycle with equal pre- and post-smoothing polynomials is a symmetric linear operator"""
    ctx, cube, solver = big
    n = cube.n_dofs(cube.max_level)
    x = ctx.vector(n, data=cube.seeded_vector(cube.max_level, 3))
    y = ctx.vector(n, data=cube.seeded_vector(cube.max_level, 4))
    Mx, My = ctx.vector(n), ctx.vector(n)
    solver.vmult(Mx, x)
    solver.vmult(My, y)
    assert ctx.dot(y, Mx) == pytest.approx(ctx.dot(x, My), rel=1e-9)
    mg.check(ctx.lib.mgx_sadd(ctx.h, mg.F64, x.ptr, 0.5, 2.0, y.ptr, n))  # x <- 0.5 x + 2 y
    Mz = ctx.vector(n)
    solver.vmult(Mz, x)
    mg.check(ctx.lib.mgx_sadd(ctx.h, mg.F64, Mz.ptr, 1.0, -0.5, Mx.ptr, n))
    mg.check(ctx.lib.mgx_sadd(ctx.h, mg.F64, Mz.ptr, 1.0, -2.0, My.ptr, n))
    assert ctx.l2_norm(Mz) < 1e-10 * ctx.l2_norm(Mx)
    for v in (x, y, Mx, My, Mz):
        v.free()


def test_c2_full_solve_reaches_the_readme_accuracy(big):
    ctx, cube, solver = big
    rate, trace = solver.solve(True)
    assert 0.05 < rate < 0.25                      # README.md:159: 0.1403 (mixed precision, 2 cycles)
    assert (trace[1:, 1] < trace[1:, 0]).all()     # every level's V-cycle reduces the residual
    its, red = solver.solve_cg()
    if cube.degree == 4:
        assert its == 8                                # README.md:159
        assert red == pytest.approx(6.8e-2, rel=0.1)   # README.md:159: 6.799e-02
        assert solver.compute_l2_error() == pytest.approx(4.2068e-10, rel=0.02)  # README.md:128
    else:
        # C3 (p = 8): no README row.  The discretisation error (h^9) is far below what the PCG
        # tolerance (1e-9 relative residual, multigrid_solver.h:486) leaves: measured 8.8e-11, i.e.
        # more accurate than C2 on the same 513^3 grid
        assert 6 <= its <= 11
        assert solver.compute_l2_error() < 4.2068e-10


FALLBACKS = {"no_fused_restrict": 1, "no_fused_init": 1, "transfer_v1": 1, "restrict_atomic": 1, "no_graph": 1,
             "no_diag_table": 1, "no_fused_prolong": 1, "free_max_bricks": 0}


@pytest.mark.parametrize("p,ns,nr", [(4, 3, 5), (2, 1, 7), (3, 1, 6), (5, 1, 5), (8, 1, 5), (1, 1, 7), (7, 1, 4), (9, 1, 4)])
def test_production_path_equals_plain_path_at_scale(monkeypatch, p, ns, nr):
    """Meshes the oracle cannot run in seconds (4 - 17 M DoFs; production thresholds, i.e. without
    the test overrides of conftest.py): the default V-cycle -- macro-element brick loop on the
    reduced-colour schedules with the inverse diagonal in registers, fused residual + restriction, first
    Chebyshev iterate formed on the fly, pipelined colour-by-colour transfers, graph replay -- against the
    same solver on a context with every one of those switched off (eight colour launches, streamed
    diagonal, first-version transfer kernels, separate residual and restriction, stored first iterate;
    in a cross-check build also the cell-by-cell brick kernel).  The two differ in summation order only."""
    monkeypatch.delenv("MGX_BRICK_MIN", raising=False)
    monkeypatch.delenv("MGX_RESTRICT_COLOUR_MIN", raising=False)
    # every degree runs the fused transfer forms by default (the line products of the embedding in even-odd form);
    # the option force_fused_transfers, once needed to keep those of degree 7 under test here, is a no-op
    ctx = mg.Context(0)
    cube = mg.Cube(p, ns, nr)
    l = cube.max_level
    n = cube.n_dofs(l)
    x = ctx.vector(n, data=cube.seeded_vector(l, 11))
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
    a = ctx.vector(n)
    solver.vmult(a, x)
    solver.vmult(a, x)  # second call: coarse levels replayed from the graph
    options = dict(FALLBACKS)
    if mg._lib.load().mgx_has_cells_form():
        options.update(cells_form=1, brick_wide_max=0)
    ctx2 = mg.Context(0, options=options)
    plain = mg.MultigridSolver(ctx2, cube, 3, 3, 1, mg.F64)
    # a vector belongs to the stream of the context that made it (its zeroing is enqueued there):
    # the second solver works on vectors of its own context, and both streams are drained before
    # one context reads what the other wrote
    ctx.sync()
    b = ctx2.vector(n)
    plain.vmult(b, x)
    ctx2.sync()
    nb = ctx.l2_norm(b)
    mg.check(ctx.lib.mgx_sadd(ctx.h, mg.F64, b.ptr, 1.0, -1.0, a.ptr, n))
    assert ctx.l2_norm(b) < 1e-11 * nb
    # and the full solve converges as it should (rate of the README table: 0.11 - 0.16)
    rate, trace = solver.solve(True)
    assert rate < 0.3 and (trace[1:, 1] < trace[1:, 0]).all()
    for v in (x, a, b):
        v.free()
    plain.close()
    ctx2.close()
    solver.close()
    cube.close()
    ctx.close()
