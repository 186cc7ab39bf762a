"""MultigridSolverDG in two dimensions on the GPU (include/mgx_dg.h: 2D DG operators on top of the FE_Q hierarchy of an
mgx_square) against its restatement tests/dg_multigrid_reference_2d.py (pinned by tests/test_dg_multigrid_reference_2d.py):
tests/test_gpu_dg_multigrid.py test for test.  Transfers DG <-> FE_Q, the merged residual + restriction, eigenvalue
estimate of the block-Jacobi Chebyshev smoother, one DG V-cycle, the V-cycle-preconditioned CG, the refusals and the
harness tools/poisson_dg.py --dim 2.

Meshes: Square(p, 1, n_refine), [-0.9, 1]^2 with 4^n_refine cells in the provider's Morton order.  16 cells is the
smallest mesh whose restriction runs as four launches (cells c, c + 4, ...), 4 cells the smallest on the list route
(colours found by the solver); p = 1 has the entities without DoFs; p = 8, 9 in fp64 take the rolled line products;
every mesh has boundary cells (constrained entries).  Tolerances are those of the 3D file for the same quantity, all
max|a - b| / max|b|."""
import ctypes as C
import os
import re
import ast
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
import dg_multigrid_reference_2d as ref  # noqa: E402
import feq_reference_2d as feq  # noqa: E402
from dg_reference_2d import from_cell_order, to_cell_order  # noqa: E402

_lib = mg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFER_SETS = [(2, 2, 0), (3, 2, 0), (4, 2, 0), (3, 2, 1), (3, 2, 2), (1, 3, 0), (5, 1, 0), (9, 2, 0), (8, 1, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


_references = {}


def reference(sq, p, basis, roots, nr, h0):
    """the CPU reference of a mesh, built once and shared (nothing changes it after its construction)"""
    key = (p, basis, roots, nr, h0)
    if key not in _references:
        _references[key] = ref.make_pair(feq.arrays_1d(sq), p, basis, roots, nr, h0)
    return _references[key]


class Pair:
    def __init__(self, ctx, p, nr, basis, number, box=None, h0=1.9):
        self.ctx = ctx
        self.sq = mg.Square(p, 1, nr) if box is None else mg.Square(p, n_refine=nr, box=box, h0=h0)
        self.solver = mg.DGMultigridSolver(ctx, self.sq, basis, 3, number)
        self.dgo, self.fe, self.orc = reference(self.sq, p, basis, (1, 1) if box is None else tuple(box), nr, h0)
        self.ij = self.solver.cell_ijk
        self.l = self.sq.max_level
        self.grid = self.sq.dof_grid(self.l)   # provider DoF -> position in the lexicographic grid
        self.n_cg = self.sq.n_dofs(self.l)

    def to_oracle(self, v):
        return from_cell_order(np.asarray(v, dtype=float), self.ij, self.dgo.cells, self.dgo.n ** 2)

    def to_product(self, a):
        return to_cell_order(a, self.ij).ravel()

    def cg_to_product(self, g):
        return np.ascontiguousarray(np.asarray(g).ravel()[self.grid])

    def cg_to_grid(self, v):
        out = np.empty(self.n_cg)
        out[self.grid] = v
        return out.reshape(self.orc.G)

    def close(self):
        self.solver.close()
        self.sq.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def check_transfers(ctx, P, number, tol, seed):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal(P.dgo.shape)
    src = ctx.vector(P.solver.m(), number, P.to_product(r))
    cg = ctx.vector(P.n_cg, number, np.full(P.n_cg, 7.0))
    P.solver.restrict_to_cg(cg, src)
    err = rel(cg.download().astype(float), P.cg_to_product(P.orc.restrict_to_cg(r)))
    print("restriction %.3e" % err)
    assert err < tol
    c = rng.standard_normal(P.n_cg)
    d0 = rng.standard_normal(P.dgo.shape)
    dst = ctx.vector(P.solver.m(), number, P.to_product(d0))
    P.solver.prolongate_add_cg_to_dg(dst, ctx.vector(c.size, number, c))
    err = rel(P.to_oracle(dst.download()), d0 + P.orc.prolongate_cg_to_dg(P.cg_to_grid(c)))
    print("prolongation %.3e" % err)
    assert err < tol


@pytest.mark.parametrize("number,tol", [(mg.F64, 1e-11), (mg.F32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("p,nr,basis", TRANSFER_SETS)
def test_transfers_between_dg_and_fe_q(ctx, p, nr, basis, number, tol):
    P = Pair(ctx, p, nr, basis, number)
    check_transfers(ctx, P, number, tol, p + nr)
    P.close()


def check_merged(ctx, P, number, tol, seed):
    rng = np.random.default_rng(seed)
    rhs, lhs = rng.standard_normal(P.dgo.shape), rng.standard_normal(P.dgo.shape)
    b, x = (ctx.vector(P.solver.m(), number, P.to_product(a)) for a in (rhs, lhs))
    cg = ctx.vector(P.n_cg, number, np.full(P.n_cg, 7.0))
    P.solver.vmult_residual_and_restrict_to_cg(cg, b, x)
    got = cg.download()
    err = rel(got.astype(float), P.cg_to_product(P.orc.restrict_to_cg(rhs - P.dgo.vmult(lhs))))
    print("merged against the reference %.3e" % err)
    assert err < tol
    # the unmerged pair of kernels gives the same vector up to rounding
    t = ctx.vector(P.solver.m(), number)
    P.solver.matrix_dg.vmult_residual(t, b, x)
    cg2 = ctx.vector(P.n_cg, number)
    P.solver.restrict_to_cg(cg2, t)
    err = rel(got.astype(float), cg2.download().astype(float))
    print("merged against the pair %.3e" % err)
    assert err < (1e-12 if number == mg.F64 else 1e-5)
    # no atomics on any mesh: a second call gives the same bits
    cg.upload(np.full(P.n_cg, 3.0, dtype=got.dtype))
    P.solver.vmult_residual_and_restrict_to_cg(cg, b, x)
    assert np.array_equal(cg.download(), got)
    got2 = cg2.download()
    P.solver.restrict_to_cg(cg2, t)
    assert np.array_equal(cg2.download(), got2)


@pytest.mark.parametrize("number,tol", [(mg.F64, 1e-10), (mg.F32, 1e-4)], ids=["f64", "f32"])
@pytest.mark.parametrize("p,nr,basis", TRANSFER_SETS + [(3, 3, 0)])
def test_merged_residual_and_restriction(ctx, p, nr, basis, number, tol):
    """vmult_residual_and_restrict_to_cg (laplace_operator_dg.h:852-861, action 1) against the two steps of the
    reference, against the unmerged pair, and bit for bit against itself"""
    P = Pair(ctx, p, nr, basis, number)
    check_merged(ctx, P, number, tol, 3 * p + nr)
    P.close()


def recorded_iterations():
    text = open(os.path.join(ROOT, "tests", "test_dg_multigrid_reference_2d.py")).read()
    return ast.literal_eval(re.search(r"PCG_ITERATIONS_2D = (\{[^}]*\})", text).group(1))


@pytest.mark.parametrize("p,nr,basis", [(2, 2, 0), (3, 2, 0), (4, 2, 0), (3, 3, 0), (3, 2, 2), (2, 2, 1)])
def test_dg_v_cycle_and_pcg_fp64(ctx, p, nr, basis):
    P = Pair(ctx, p, nr, basis, mg.F64)
    info = P.solver.smoother_info()
    assert info["cg_its"] == P.orc.cg_its and info["degree"] == 3
    assert info["lambda_max"] == pytest.approx(P.orc.lambda_max, rel=1e-8)
    assert info["theta"] == pytest.approx(P.orc.theta, rel=1e-8)
    x, rhs = ref.pcg_inputs(P.dgo.shape)
    src, dst = ctx.vector(P.solver.m(), data=P.to_product(x)), ctx.vector(P.solver.m())
    want = P.orc.v_cycle(x)
    for _ in range(3):  # eager, coarse levels captured, replayed
        P.solver.vmult(dst, src)
        assert rel(P.to_oracle(dst.download()), want) < 1e-8
    b, sol = ctx.vector(P.solver.m(), data=P.to_product(rhs)), ctx.vector(P.solver.m())
    its, red = P.solver.solve_cg(b, sol, 1e-9)
    xo, oits, ored = P.orc.solve_cg(rhs, 1e-9)
    print("PCG %d iterations, rate %.6f (reference %d, %.6f)" % (its, red, oits, ored))
    assert its == recorded_iterations()[(p, nr, basis)] and its == oits
    assert red == pytest.approx(ored, rel=1e-5)
    assert rel(P.to_oracle(sol.download()), xo) < 1e-7
    # the solution solves the DG system
    res = ctx.vector(P.solver.m())
    P.solver.matrix_dg_dp.vmult_residual(res, b, sol)
    assert ctx.l2_norm(res) < 2e-9 * ctx.l2_norm(b)
    P.close()


@pytest.mark.parametrize("p,nr,basis", [(3, 2, 0), (4, 2, 0), (2, 3, 0), (3, 2, 2)])
def test_dg_v_cycle_and_pcg_mixed_precision(ctx, p, nr, basis):
    """the reference's default: fp32 V-cycle inside the fp64 CG (poisson_dg/program.cc:72-73)"""
    P = Pair(ctx, p, nr, basis, mg.F32)
    info = P.solver.smoother_info()
    assert info["lambda_max"] == pytest.approx(P.orc.lambda_max, rel=1e-4)
    x, rhs = ref.pcg_inputs(P.dgo.shape)
    src, dst = ctx.vector(P.solver.m(), data=P.to_product(x)), ctx.vector(P.solver.m())
    P.solver.vmult(dst, src)
    assert rel(P.to_oracle(dst.download()), P.orc.v_cycle(x)) < 5e-4
    b, sol = ctx.vector(P.solver.m(), data=P.to_product(rhs)), ctx.vector(P.solver.m())
    its, red = P.solver.solve_cg(b, sol, 1e-9)
    xo, oits, ored = P.orc.solve_cg(rhs, 1e-9)
    assert abs(its - oits) <= 1 and red == pytest.approx(ored, rel=0.05)
    assert rel(P.to_oracle(sol.download()), xo) < 1e-6
    P.close()


def test_unmerged_restrict_option_gives_the_same_v_cycle(ctx):
    """context option dg_unmerged_restrict: residual and restriction as two kernels"""
    out = []
    for c in (ctx, mg.Context(0, options=dict(dg_unmerged_restrict=1))):
        P = Pair(c, 3, 2, 0, mg.F64)
        x, _ = ref.pcg_inputs(P.dgo.shape)
        src, dst = c.vector(P.solver.m(), data=P.to_product(x)), c.vector(P.solver.m())
        P.solver.vmult(dst, src)
        out.append(dst.download())
        P.close()
        if c is not ctx:
            c.close()
    assert rel(out[1], out[0]) < 1e-12


@pytest.mark.parametrize("number,tol,mtol", [(mg.F64, 1e-11, 1e-10), (mg.F32, 2e-5, 1e-4)], ids=["f64", "f32"])
def test_cell_order_without_the_four_classes_takes_the_list_route(ctx, number, tol, mtol):
    """a 3 x 3 box (lexicographic cells, 9 of them) fails the check of cells c, c + 4, ...: accepted, the solver's own
    colours give the reference's restriction, merged and stand-alone"""
    P = Pair(ctx, 3, 0, 0, number, box=(3, 3), h0=0.6)
    assert P.sq.n_cells(P.l) == 9
    check_transfers(ctx, P, number, tol, 5)
    check_merged(ctx, P, number, mtol, 6)
    P.close()


def test_refusals_and_lifetime(ctx):
    lib = _lib.load()
    start = lib.mgx_live_device_allocations()
    sq, cube = mg.Square(2, 1, 1), mg.Cube(2, 1, 1)
    fe2, fe3 = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64), mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F64)
    nb2, _ = mg.dg_box_neighbours((2, 2))
    nb3, _ = mg.dg_box_neighbours((2, 2, 2))
    dg2 = mg.DGLaplaceOperator(ctx, 2, mg.DG_HERMITE, nb2, np.eye(2) * 0.95, mg.F64, dim=2)
    dg3 = mg.DGLaplaceOperator(ctx, 2, mg.DG_HERMITE, nb3, np.eye(3) * 0.95, mg.F64)
    held = lib.mgx_live_device_allocations()
    h = C.c_void_p()
    for dgop, fe, n in ((dg2, fe3, 4), (dg3, fe2, 8)):   # 2D DG over a 3D FE_Q hierarchy, and the converse
        gid = np.arange(n, dtype=np.uint32)
        d = _lib.DGSolverDesc(dgop.h, dgop.h, fe.h, 3, gid.ctypes.data_as(_lib.u32p))
        with pytest.raises(mg.MgxError, match="FE_Q hierarchy is") as e:
            mg.check(lib.mgx_dg_solver_create(ctx.h, C.byref(d), C.byref(h)))
        assert e.value.status == -4   # MGX_ERR_UNSUPPORTED
        assert lib.mgx_live_device_allocations() == held
    for x in (dg2, dg3):
        x.clear()
    fe2.close()
    fe3.close()
    cube.close()
    with pytest.raises(ValueError):
        mg.DGMultigridSolver(ctx, sq, comm=object())
    sq.close()
    for kw in (dict(jacobian=[[1.0, 0.35], [0.15, 0.8]]), dict(mapped="annulus_sector")):
        bad = mg.Square(2, 1, 1, **kw)
        with pytest.raises(ValueError):
            mg.DGMultigridSolver(ctx, bad)
        bad.close()
    assert lib.mgx_live_device_allocations() == start
    P = Pair(ctx, 2, 1, 0, mg.F32)   # a full cycle: create, solve, close
    b, sol = P.solver.initialize_dof_vector(np.ones(P.solver.m())), P.solver.initialize_dof_vector()
    its, _ = P.solver.solve_cg(b, sol)
    assert its > 0
    b.free()
    sol.free()
    P.close()
    assert lib.mgx_live_device_allocations() == start


def run_harness(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_dg.py"), *args, "--dim", "2"], cwd=ROOT,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.decode().strip().splitlines()


def test_poisson_dg_harness_runs_in_2d():
    """tools/poisson_dg.py --dim 2 (poisson_dg/program.cc with dimension = 2): converges in a mesh-independent number of
    iterations and prints the reference's table row"""
    for nr in (3, 4):
        lines = run_harness("3", str(nr))
        assert lines[-2].split() == "cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction".split()
        row = lines[-1].split()
        assert int(row[0]) == 4 ** nr and int(row[1]) == 4 ** nr * 16
        assert 5 <= int(row[6]) <= 10
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_dg.py"), "3", "3", "--dim", "2", "--gpus", "2"],
                         cwd=ROOT, capture_output=True, timeout=600)
    assert out.returncode != 0 and b"--dim 2 runs on one GPU" in out.stderr


def test_poisson_dg_discretisation_error_converges_in_2d():
    """for a solution that vanishes on the boundary the L2 error of FE_DGQHermite(3) falls with h^4"""
    err = [float(run_harness("3", str(nr), "--solution", "vanishing", "--vcycle", "f64")[-1].split()[4]) for nr in (4, 5)]
    assert 11 < err[0] / err[1] < 20, err
