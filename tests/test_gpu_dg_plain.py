"""MultigridSolverDGPlain on the GPU (include/mgx_dg.h: mgx_dg_transfer_*, mgx_dg_plain_solver_*,
common/multigrid_solver_dg_plain.h:55-595) against its numpy restatement tests/dg_plain_reference.py: the DG-to-DG
level transfers, the smoother parameters of every level, the V-cycle, the V-cycle-preconditioned CG and
vmult_with_residual_update, in fp64 and with an fp32 V-cycle; device memory after create / use / destroy and after
refused creates; the harness tools/poisson_dg_plain.py.

The shapes are the smallest that reach every path of the transfer kernel: a non-cubic coarse box (a swapped axis
shows), both cell orderings (the lexicographic one has children[c][k] != 8 c + k), several parents per workgroup with
the last workgroup partly filled, one parent per workgroup, and the largest tile (p = 9).  A transfer does not depend
on the cell Jacobian; the solver cases marked `sheared` use that of dg_cheby_mesh."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_plain_reference as ref  # noqa: E402

_lib = mg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHEARED = dg.cheby_mesh(0)[1]


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def to_oracle(ijk, v, shape):
    out = np.empty(shape)
    out[ijk[:, 2], ijk[:, 1], ijk[:, 0]] = np.asarray(v, dtype=float).reshape(len(ijk), -1)
    return out


def to_product(ijk, a):
    return a[ijk[:, 2], ijk[:, 1], ijk[:, 0]].ravel()


@functools.lru_cache(maxsize=None)
def embedding(p, basis):
    P = ref.embedding_1d(p, basis)
    return P, [dg.kron3(P[k & 1], P[(k >> 1) & 1], P[k >> 2]) for k in range(8)]


def ref_prolongate(P3, coarse):
    nz, ny, nx, n3 = coarse.shape
    fine = np.zeros((2 * nz, 2 * ny, 2 * nx, n3))
    for k in range(8):
        fine[(k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2] = coarse @ P3[k].T
    return fine


def ref_restrict(P3, fine):
    return sum(fine[(k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2] @ P3[k] for k in range(8))


# ---------------------------------------------------------------------------------------- transfers
TRANSFER_F64 = [(p, b, (2, 1, 1)) for p in (1, 2, 3, 4, 5, 7, 9) for b in (0, 1, 2)]
TRANSFER_F64 += [(9, 0, (1, 1, 1))]                                          # the LDS maximum, one parent
TRANSFER_F64 += [(1, 0, (3, 3, 1)), (3, 1, (3, 3, 1)), (4, 0, (3, 2, 1)), (5, 2, (3, 1, 1))]   # last workgroup partly filled
TRANSFER_F32 = [(p, b, (2, 1, 1)) for p in (2, 4, 8) for b in (0, 1, 2)] + [(9, 0, (1, 1, 1)), (4, 0, (3, 2, 1))]


def check_transfer(ctx, p, basis, coarse_cells, ordering, number, tol):
    _, P3 = embedding(p, basis)
    n3 = (p + 1) ** 3
    fine_cells = tuple(2 * c for c in coarse_cells)
    _, cijk = mg.dg_box_neighbours(coarse_cells, ordering)
    _, fijk = mg.dg_box_neighbours(fine_cells, ordering)
    children = mg.dg_box_children(coarse_cells, ordering, ordering)
    if ordering != "z" and len(children) > 1:
        assert not np.array_equal(children.ravel(), np.arange(children.size))
    cshape, fshape = coarse_cells[::-1] + (n3,), fine_cells[::-1] + (n3,)
    rng = np.random.default_rng(100 * p + basis)
    c0, f0 = rng.standard_normal(cshape), rng.standard_normal(fshape)
    T = mg.DGLevelTransfer(ctx, p, basis, children, number)
    coarse = ctx.vector(c0.size, number, to_product(cijk, c0))
    # both operations add: the destination starts from random values
    got = []
    for _ in range(2):
        fine = ctx.vector(f0.size, number, to_product(fijk, f0))
        T.prolongate_and_add(fine, coarse)
        got.append(fine.download())
    print("prolongation p=%d basis=%d %s: %.3e" % (p, basis, ordering, rel(to_oracle(fijk, got[0], fshape), f0 + ref_prolongate(P3, c0))))
    assert rel(to_oracle(fijk, got[0], fshape), f0 + ref_prolongate(P3, c0)) < tol
    assert np.array_equal(got[0], got[1])
    fine = ctx.vector(f0.size, number, to_product(fijk, f0))
    got = []
    for _ in range(2):
        dst = ctx.vector(c0.size, number, to_product(cijk, c0))
        T.restrict_and_add(dst, fine)
        got.append(dst.download())
    print("restriction  p=%d basis=%d %s: %.3e" % (p, basis, ordering, rel(to_oracle(cijk, got[0], cshape), c0 + ref_restrict(P3, f0))))
    assert rel(to_oracle(cijk, got[0], cshape), c0 + ref_restrict(P3, f0)) < tol
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(fine.download().astype(float), to_product(fijk, f0).astype(mg._DT[number]).astype(float))  # source untouched
    T.clear()


@pytest.mark.parametrize("ordering", ["z", "lexicographic"])
@pytest.mark.parametrize("p,basis,coarse_cells", TRANSFER_F64)
def test_transfers_fp64(ctx, p, basis, coarse_cells, ordering):
    check_transfer(ctx, p, basis, coarse_cells, ordering, mg.F64, 1e-11)


@pytest.mark.parametrize("ordering", ["z", "lexicographic"])
@pytest.mark.parametrize("p,basis,coarse_cells", TRANSFER_F32)
def test_transfers_fp32(ctx, p, basis, coarse_cells, ordering):
    check_transfer(ctx, p, basis, coarse_cells, ordering, mg.F32, 2e-5)


@pytest.mark.parametrize("basis", [0, 1, 2])
@pytest.mark.parametrize("p", range(1, 10))
def test_transfer_matrix(ctx, p, basis):
    T = mg.DGLevelTransfer(ctx, p, basis, np.arange(8, dtype=np.uint32).reshape(1, 8), mg.F64)
    assert abs(T.matrix() - embedding(p, basis)[0]).max() < 1e-13
    T.clear()


def test_transfer_refuses_a_child_table_that_is_no_permutation(ctx):
    ch = np.arange(16, dtype=np.uint32).reshape(2, 8)
    for bad in ((3, 16), (3, 4)):      # out of range / a fine cell named twice
        t = ch.copy()
        t.ravel()[bad[0]] = bad[1]
        with pytest.raises(mg.MgxError, match="exactly once"):
            mg.DGLevelTransfer(ctx, 2, 0, t, mg.F64)


# ---------------------------------------------------------------------------------------- solver
#        p, basis, coarse cells, levels, sheared
CASES = [(2, 0, (1, 1, 1), 3, False),
         (3, 0, (2, 1, 1), 3, True),
         (4, 0, (1, 1, 1), 3, False),
         (3, 1, (2, 1, 1), 3, False),
         (3, 2, (1, 2, 1), 3, True),
         (1, 0, (2, 1, 1), 4, False),
         (5, 0, (1, 1, 1), 2, True)]


def case_jacobian(case):
    return SHEARED if case[4] else np.eye(3) * 0.7


@functools.lru_cache(maxsize=None)
def reference(case):
    """the numpy solver of a case with what the tests compare against, computed once and left unchanged"""
    p, basis, cells, levels, _ = case
    o = ref.DGPlainOracle(p, basis, cells, case_jacobian(case), levels)
    shape = o.level[-1].shape
    rng = np.random.default_rng(7)
    x, rhs, upd = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    out = dict(o=o, shape=shape, x=x, rhs=rhs, upd=upd, vcycle=o.v_cycle(x), cg=o.solve_cg(rhs, 1e-9))
    out["update0"] = o.vmult_with_residual_update(rhs, upd, 0.0)
    out["update1"] = o.vmult_with_residual_update(rhs, upd, -0.37)
    return out


def make_solver(ctx, case, number):
    p, basis, cells, levels, _ = case
    return mg.DGPlainMultigridSolver(ctx, p, basis, cells, case_jacobian(case), levels, 3, number)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "p%d-b%d-%dx%dx%d-L%d%s" % (c[0], c[1], *c[2], c[3], "-sheared" if c[4] else ""))
def test_plain_dg_multigrid_fp64(ctx, case):
    R = reference(case)
    o, shape = R["o"], R["shape"]
    S = make_solver(ctx, case, mg.F64)
    ijk = S.cell_ijk[-1]
    for l in range(case[3]):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert info["cg_its"] == want["cg_its"] and info["degree"] == want["degree"]
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-8)
        assert info["theta"] == pytest.approx(want["theta"], rel=1e-8)
    src, dst = ctx.vector(S.m(), data=to_product(ijk, R["x"])), ctx.vector(S.m())
    for _ in range(3):
        S.vmult(dst, src)
        assert rel(to_oracle(ijk, dst.download(), shape), R["vcycle"]) < 1e-8
    b, sol = ctx.vector(S.m(), data=to_product(ijk, R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert its == oits and red == pytest.approx(ored, rel=1e-5)
    assert rel(to_oracle(ijk, sol.download(), shape), xo) < 1e-7
    res = ctx.vector(S.m())
    S.matrix_dg_dp.vmult_residual(res, b, sol)
    assert ctx.l2_norm(res) < 2e-9 * ctx.l2_norm(b)
    # vmult_with_residual_update (multigrid_solver_dg_plain.h:340-427)
    for factor, key in ((0.0, "update0"), (-0.37, "update1")):
        new, mgv, sums = R[key]
        got = []
        for _ in range(2):
            r, u = ctx.vector(S.m(), data=to_product(ijk, R["rhs"])), ctx.vector(S.m(), data=to_product(ijk, R["upd"]))
            got.append((S.vmult_with_residual_update(r, u, factor), r.download(), u.download()))
        s, rr, uu = got[0]
        assert rel(to_oracle(ijk, rr, shape), new) < 1e-8 and rel(to_oracle(ijk, uu, shape), mgv) < 1e-8
        assert s[0] == pytest.approx(sums[0], rel=1e-8) and s[1] == pytest.approx(sums[1], rel=1e-8)
        assert np.array_equal(s, got[1][0]) and np.array_equal(uu, got[1][2])
    S.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4], CASES[6]],
                         ids=lambda c: "p%d-b%d-%dx%dx%d-L%d%s" % (c[0], c[1], *c[2], c[3], "-sheared" if c[4] else ""))
def test_plain_dg_multigrid_fp32_v_cycle(ctx, case):
    """the reference's default: fp32 V-cycle inside the fp64 CG.  Level 0 cannot reach a residual of 1e-10 in fp32:
    its eigenvalue estimate runs on and must stay finite"""
    R = reference(case)
    o, shape = R["o"], R["shape"]
    S = make_solver(ctx, case, mg.F32)
    ijk = S.cell_ijk[-1]
    for l in range(case[3]):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert all(np.isfinite(v) for v in info.values())
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-4)
        if l == 0:
            assert abs(info["degree"] - want["degree"]) <= 1
        else:
            assert info["degree"] == want["degree"]
    src, dst = ctx.vector(S.m(), data=to_product(ijk, R["x"])), ctx.vector(S.m())
    S.vmult(dst, src)
    assert rel(to_oracle(ijk, dst.download(), shape), R["vcycle"]) < 5e-4
    b, sol = ctx.vector(S.m(), data=to_product(ijk, R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert abs(its - oits) <= 1 and red == pytest.approx(ored, rel=0.05)
    assert rel(to_oracle(ijk, sol.download(), shape), xo) < 1e-6
    S.close()


# ---------------------------------------------------------------------------------------- lifetime
def live():
    return _lib.load().mgx_live_device_allocations()


def raw_solver_create(ctx, matrices, matrix_dp, transfers, degree_pre=3):
    d = _lib.DGPlainSolverDesc()
    d.n_levels = len(matrices)
    d.matrix = (_lib.vp * len(matrices))(*[m.h for m in matrices])
    d.matrix_dg_dp = matrix_dp.h
    d.transfer = (_lib.vp * max(1, len(transfers)))(*[t.h for t in transfers])
    d.degree_pre = degree_pre
    h = C.c_void_p()
    mg.check(ctx.lib.mgx_dg_plain_solver_create(ctx.h, C.byref(d), C.byref(h)))
    return h


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
def test_lifecycle_leaves_no_device_memory(ctx, number):
    start = live()
    S = mg.DGPlainMultigridSolver(ctx, 2, mg.DG_HERMITE, (2, 1, 1), SHEARED, 2, 3, number)
    assert live() > start
    rng = np.random.default_rng(0)
    src, dst = S.initialize_dof_vector(rng.standard_normal(S.m())), S.initialize_dof_vector()
    S.vmult(dst, src)
    S.vmult_with_residual_update(src, dst, 0.5)
    assert np.isfinite(dst.download()).all()
    T = mg.DGLevelTransfer(ctx, 3, mg.DG_GAUSS, mg.dg_box_children((1, 1, 1)), number)
    c, f = ctx.vector(64, number, rng.standard_normal(64)), ctx.vector(512, number, rng.standard_normal(512))
    T.prolongate_and_add(f, c)
    T.restrict_and_add(c, f)
    T.clear()
    S.close()
    assert live() == start


def test_refused_creates_leave_no_device_memory(ctx):
    start = live()
    nb1, _ = mg.dg_box_neighbours((1, 1, 1))
    nb2, _ = mg.dg_box_neighbours((2, 2, 2))
    nb3, _ = mg.dg_box_neighbours((2, 2, 1))
    A0 = mg.DGLaplaceOperator(ctx, 2, 0, nb1, np.eye(3), mg.F64)
    A1 = mg.DGLaplaceOperator(ctx, 2, 0, nb2, np.eye(3) / 2, mg.F64)
    A1_p3 = mg.DGLaplaceOperator(ctx, 3, 0, nb2, np.eye(3) / 2, mg.F64)
    A1_four = mg.DGLaplaceOperator(ctx, 2, 0, nb3, np.eye(3) / 2, mg.F64)
    T = mg.DGLevelTransfer(ctx, 2, 0, mg.dg_box_children((1, 1, 1)), mg.F64)
    held = live()
    with pytest.raises(mg.MgxError, match="degree, basis or number type"):      # levels of different degree
        raw_solver_create(ctx, [A0, A1_p3], A1_p3, [T])
    assert live() == held
    with pytest.raises(mg.MgxError, match="8 x coarse = fine"):                  # 8 n(l-1) != n(l)
        raw_solver_create(ctx, [A0, A1_four], A1_four, [T])
    assert live() == held
    h = raw_solver_create(ctx, [A0, A1], A1, [T])                                # the consistent one is accepted
    assert live() > held
    mg.check(ctx.lib.mgx_dg_plain_solver_destroy(h))
    assert live() == held
    for x in (T, A0, A1, A1_p3, A1_four):
        x.clear()
    assert live() == start


def test_operator_with_ghost_cells_is_refused():
    """the plain DG multigrid runs on one rank: an operator that carries ghost cells is refused with
    MGX_ERR_INVALID_ARGUMENT.  A context of its own carries the communicator of rank 0 of 2 that such an operator
    needs; the stand-in never communicates, and need not: creating the operator exchanges nothing and the solver is
    refused before its first reduction."""
    class RankZeroOfTwo:
        def get_rank(self):
            return 0

        def get_world_size(self):
            return 2

        def get_backend(self):
            return "gloo"

    start = live()
    c2 = mg.Context(0)
    mg.Communicator(c2, RankZeroOfTwo(), device_transport=False, native=False)
    # one owned cell whose lower x neighbour is a ghost cell owned by rank 1
    nb = np.array([[1, -1, -1, -1, -1, -1]], dtype=np.int32)
    exchange = [(1, np.array([0], dtype=np.uint32), 1, 1)]
    A = mg.DGLaplaceOperator(c2, 2, mg.DG_GAUSS, nb, np.eye(3), mg.F64, n_ghost=1, exchange=exchange)
    held = live()
    with pytest.raises(mg.MgxError, match="ghost cells") as e:
        raw_solver_create(c2, [A], A, [])
    assert e.value.status == -1  # MGX_ERR_INVALID_ARGUMENT
    assert live() == held
    A.clear()
    c2.close()
    assert live() == start


# ---------------------------------------------------------------------------------------- harness
def run_harness(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_dg_plain.py"), *args], cwd=ROOT,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.decode().strip().splitlines()


def test_poisson_dg_plain_harness_runs():
    """tools/poisson_dg_plain.py: a level-independent number of iterations (the fp64 numpy prototype gives 17 and 16)
    and the reference's table row"""
    rows = []
    for nr in (2, 3):
        lines = run_harness("3", str(nr))
        assert lines[-2].split() == "cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction".split()
        assert sum(l.startswith("level ") for l in lines) == nr + 1
        rows.append(lines[-1].split())
    print(rows)
    assert int(rows[0][0]) == 64 and int(rows[1][0]) == 512 and int(rows[1][1]) == 512 * 64
    assert 13 <= int(rows[0][6]) <= 21 and 13 <= int(rows[1][6]) <= 21


def test_poisson_dg_plain_discretisation_error_converges():
    """for a solution that vanishes on the boundary the L2 error of FE_DGQHermite(3) falls with h^4 -- the criterion of
    test_gpu_dg_multigrid.py::test_poisson_dg_discretisation_error_converges: same space, same problem"""
    err = []
    for nr in (3, 4):
        lines = run_harness("3", str(nr), "--solution", "vanishing", "--vcycle", "f64", "--levels")
        assert any(l.startswith("level  smoother") for l in lines)
        err.append(float(lines[-1].split()[4]))
    print(err)
    assert err[0] < 2e-3 and 11 < err[0] / err[1] < 20, err
