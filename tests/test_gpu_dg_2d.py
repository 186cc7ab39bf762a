"""The DG-SIP operator, its smoother, the DG-to-DG level transfers and MultigridSolverDGPlain in TWO dimensions on the
GPU (include/mgx_dg.h with dim = 2; the dimension poisson_dg_plain/program.cc:65 runs) against the numpy restatement
tests/dg_reference_2d.py, which tests/test_dg_reference_2d.py pins on the CPU.  Tolerances are those of the same
quantities in 3D (tests/test_gpu_dg.py, tests/test_gpu_dg_plain.py), except the fp32 transfers (5e-6).

Cells per 256-thread workgroup of the 2D cell kernel, p = 1 ... 9: 128 85 64 51 42 36 32 28 25.  The boxes:
(1,1), (3,1), (1,3), (3,3) hold each of the 16 combinations of Dirichlet faces exactly where it can occur; (5,3) = 15
cells share one partly filled workgroup at every degree; (17,13) = 221 cells fill 2 (p = 1) ... 9 (p = 9) workgroups,
the last one partly, and at p = 9 more than the 8 of one round of the XCD-aware block order.

Launch forms: the 2D operator runs on one rank and has no FE_Q level above it, so every entry point launches all cells
in order (cell_first = 0, cell_stride = 1, no cell_list); the other two forms are not reachable through the C ABI in
2D and are therefore not run here."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_reference_2d as ref2  # noqa: E402

_lib = mg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
STRETCHED_2D = np.diag([0.7, 1.3])
TOL = {mg.F64: 2e-11, mg.F32: 3e-5}
KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def live():
    return _lib.load().mgx_live_device_allocations()


class Case:
    """oracle and HIP operator on the same box of cells; vectors travel in the oracle's layout"""

    def __init__(self, ctx, p, kind, cells, jac, number, ordering="z"):
        self.ctx, self.number = ctx, number
        self.orc = ref2.DGOracle2D(p, kind, cells, jac)
        nb, self.ij = mg.dg_box_neighbours(cells, ordering)
        self.op = mg.DGLaplaceOperator(ctx, p, kind, nb, jac, number, dim=2)
        assert self.op.m() == int(np.prod(self.orc.shape)) == self.op.vector_size()

    def up(self, x):
        return self.op.initialize_dof_vector(ref2.to_cell_order(x, self.ij).ravel())

    def down(self, v):
        return ref2.from_cell_order(v.download().astype(float), self.ij, self.orc.cells, self.orc.shape[-1])

    def close(self):
        self.op.clear()


# ---------------------------------------------------------------------------------------- operator
#        box, sheared, orderings
BOXES = [((1, 1), True, ("z",)), ((3, 1), False, ("z",)), ((1, 3), True, ("z",)), ((3, 3), True, ("z",)),
         ((5, 3), False, ("z", "lexicographic")), ((17, 13), True, ("z",))]


def check_operator(ctx, p, kind, number):
    rng = np.random.default_rng(100 * p + kind)
    for cells, sheared, orderings in BOXES:
        for ordering in orderings:
            case = Case(ctx, p, kind, cells, SHEARED_2D if sheared else STRETCHED_2D, number, ordering)
            x, rhs = rng.standard_normal(case.orc.shape), rng.standard_normal(case.orc.shape)
            src, b = case.up(x), case.up(rhs)
            got = []
            for _ in range(2):
                dst = case.op.initialize_dof_vector(np.full(x.size, np.nan))     # an unwritten entry shows
                case.op.vmult(dst, src)
                got.append(dst.download())
            err = rel(case.down(dst), case.orc.vmult(x))
            print("vmult p=%d kind=%d %s %s: %.3e" % (p, kind, cells, ordering, err))
            assert err < TOL[number], (cells, ordering)
            assert np.array_equal(got[0], got[1])
            case.op.vmult_residual(dst, b, src)
            assert rel(case.down(dst), rhs - case.orc.vmult(x)) < TOL[number], (cells, ordering)
            case.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", range(1, 10))
def test_operator_equals_face_based_oracle_fp64(ctx, p, kind):
    check_operator(ctx, p, kind, mg.F64)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [2, 3, 4, 8])
def test_operator_equals_face_based_oracle_fp32(ctx, p, kind):
    check_operator(ctx, p, kind, mg.F32)


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [2, 3, 4, 5])
def test_block_jacobi_and_merged_chebyshev_update(ctx, p, kind, number):
    case = Case(ctx, p, kind, (3, 3), SHEARED_2D, number)
    o = case.orc
    info = case.op.info()
    assert np.isclose(info["hermite_derivative_on_face"], dg.hermite_like_basis(p)[0].d(0.0)) or kind != dg.HERMITE
    assert np.allclose(info["eigenvalues_1d"], o.eigenvalues_1d, rtol=1e-9)
    assert info["penalty"].shape == (2,) and np.allclose(info["penalty"], o.penalty)   # laplace_operator_dg.h:789-793
    rng = np.random.default_rng(7 + p)
    rhs, x, xo = (rng.standard_normal(o.shape) for _ in range(3))
    tol = TOL[number] * 5   # (the 3D test's: the preconditioner divides by the diagonal)
    d = case.op.initialize_dof_vector()
    case.op.jacobi_vmult(d, case.up(rhs))
    assert rel(case.down(d), o.jacobi_vmult(rhs)) < tol
    for idx in (0, 1, 2):   # laplace_operator_dg.h:910-955
        got = []
        for _ in range(2):
            sol, old, b = case.up(x), case.up(xo), case.up(rhs)
            case.op.vmult_with_chebyshev_update(b, idx, 0.6, 0.2, sol, old)
            got.append(sol.download())
        new_ref, old_ref = o.vmult_with_chebyshev_update(rhs, idx, 0.6, 0.2, x, xo)
        print("chebyshev p=%d kind=%d index %d: %.3e" % (p, kind, idx, rel(case.down(sol), new_ref)))
        assert rel(case.down(sol), new_ref) < tol, idx
        assert rel(case.down(old), old_ref) < tol, idx
        assert np.array_equal(got[0], got[1])
    # the loop of the harness (matvec_dg_cheby/program.cc:116-121): update, then swap output / input
    out, inp, b = case.up(x), case.up(xo), case.up(rhs)
    ro, ri = x, xo
    for _ in range(3):
        case.op.vmult_with_chebyshev_update(b, 2, 0.6, 0.2, out, inp)
        out, inp = inp, out
        ro, ri = o.vmult_with_chebyshev_update(rhs, 2, 0.6, 0.2, ro, ri)
        ro, ri = ri, ro
    assert rel(case.down(out), ro) < tol * 10 and rel(case.down(inp), ri) < tol * 10
    case.close()


# ---------------------------------------------------------------------------------------- transfers
@functools.lru_cache(maxsize=None)
def embedding(p, basis):
    P = ref2.embedding_1d(p, basis)
    return [ref2.kron2(P[k & 1], P[k >> 1]) for k in range(4)]


def ref_prolongate(P2, coarse):
    ny, nx, n2 = coarse.shape
    fine = np.zeros((2 * ny, 2 * nx, n2))
    for k in range(4):
        fine[(k >> 1)::2, (k & 1)::2] = coarse @ P2[k].T
    return fine


def ref_restrict(P2, fine):
    return sum(fine[(k >> 1)::2, (k & 1)::2] @ P2[k] for k in range(4))


# parents per workgroup of the 2D transfer kernel, p = 1 ... 9: 64 64 64 40 28 20 16 12 10 -- (2,1): one partly filled
# workgroup with several parents; (3,3) = 9 parents: the same; (1,1) at p = 9: the largest tile on its own.  More
# than one workgroup needs more than 64 parents at p <= 3: (13,5) = 65 parents at p = 3, (7,3) = 21 at p = 7.
TRANSFER_F64 = [(p, b, c) for p in (1, 2, 3, 4, 5, 7, 9) for b in (0, 1, 2) for c in ((2, 1), (3, 3))]
TRANSFER_F64 += [(9, 0, (1, 1)), (3, 0, (13, 5)), (7, 1, (7, 3))]
TRANSFER_F32 = [(p, b, c) for p in (2, 4, 8) for b in (0, 1, 2) for c in ((2, 1), (3, 3))]


def check_transfer(ctx, p, basis, coarse_cells, ordering, number, tol):
    P2 = embedding(p, basis)
    n2 = (p + 1) ** 2
    fine_cells = tuple(2 * c for c in coarse_cells)
    _, cij = mg.dg_box_neighbours(coarse_cells, ordering)
    _, fij = mg.dg_box_neighbours(fine_cells, ordering)
    children = mg.dg_box_children(coarse_cells, ordering, ordering)
    assert children.shape == (len(cij), 4)
    if ordering != "z" and len(children) > 1:
        assert not np.array_equal(children.ravel(), np.arange(children.size))   # children[c][k] != 4 c + k: the table is read
    cshape, fshape = coarse_cells[::-1] + (n2,), fine_cells[::-1] + (n2,)
    rng = np.random.default_rng(100 * p + basis)
    c0, f0 = rng.standard_normal(cshape), rng.standard_normal(fshape)
    T = mg.DGLevelTransfer(ctx, p, basis, children, number)
    assert T.dim == 2
    coarse = ctx.vector(c0.size, number, ref2.to_cell_order(c0, cij).ravel())
    # both operations add: the destination starts from random values
    got = []
    for _ in range(2):
        fine = ctx.vector(f0.size, number, ref2.to_cell_order(f0, fij).ravel())
        T.prolongate_and_add(fine, coarse)
        got.append(fine.download())
    err = rel(ref2.from_cell_order(got[0], fij, fine_cells, n2), f0 + ref_prolongate(P2, c0))
    print("prolongation p=%d basis=%d %s %s: %.3e" % (p, basis, coarse_cells, ordering, err))
    assert err < tol
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(coarse.download().astype(float), ref2.to_cell_order(c0, cij).ravel().astype(mg._DT[number]).astype(float))
    fine = ctx.vector(f0.size, number, ref2.to_cell_order(f0, fij).ravel())
    got = []
    for _ in range(2):
        dst = ctx.vector(c0.size, number, ref2.to_cell_order(c0, cij).ravel())
        T.restrict_and_add(dst, fine)
        got.append(dst.download())
    err = rel(ref2.from_cell_order(got[0], cij, coarse_cells, n2), c0 + ref_restrict(P2, f0))
    print("restriction  p=%d basis=%d %s %s: %.3e" % (p, basis, coarse_cells, ordering, err))
    assert err < tol
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(fine.download().astype(float), ref2.to_cell_order(f0, fij).ravel().astype(mg._DT[number]).astype(float))  # source untouched
    T.clear()


@pytest.mark.parametrize("ordering", ["z", "lexicographic"])
@pytest.mark.parametrize("p,basis,coarse_cells", TRANSFER_F64)
def test_transfers_fp64(ctx, p, basis, coarse_cells, ordering):
    check_transfer(ctx, p, basis, coarse_cells, ordering, mg.F64, 1e-11)


@pytest.mark.parametrize("ordering", ["z", "lexicographic"])
@pytest.mark.parametrize("p,basis,coarse_cells", TRANSFER_F32)
def test_transfers_fp32(ctx, p, basis, coarse_cells, ordering):
    check_transfer(ctx, p, basis, coarse_cells, ordering, mg.F32, 5e-6)


def test_transfer_refuses_a_child_table_that_is_no_permutation(ctx):
    start = live()
    ch = np.arange(8, dtype=np.uint32).reshape(2, 4)
    for bad in ((3, 8), (3, 4)):      # out of range / a fine cell named twice
        t = ch.copy()
        t.ravel()[bad[0]] = bad[1]
        with pytest.raises(mg.MgxError, match="exactly once"):
            mg.DGLevelTransfer(ctx, 2, 0, t, mg.F64)
    assert live() == start


# ---------------------------------------------------------------------------------------- solver
#        p, basis, coarse cells, levels, sheared
CASES = [(2, 0, (1, 1), 3, False),
         (3, 0, (2, 1), 3, True),
         (3, 1, (1, 2), 3, False),
         (3, 2, (2, 1), 3, True),
         (1, 0, (3, 2), 3, False),
         (4, 0, (1, 1), 4, True)]
CASE_IDS = ["p%d-b%d-%dx%d-L%d%s" % (c[0], c[1], *c[2], c[3], "-sheared" if c[4] else "") for c in CASES]


def case_jacobian(case):
    return SHEARED_2D if case[4] else np.eye(2) * 0.7


@functools.lru_cache(maxsize=None)
def reference(case):
    """the numpy solver of a case with what the tests compare against, computed once and left unchanged"""
    p, basis, cells, levels, _ = case
    o = ref2.DGPlainOracle2D(p, basis, cells, case_jacobian(case), levels)
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


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_plain_dg_multigrid_fp64(ctx, case):
    R = reference(case)
    o, shape = R["o"], R["shape"]
    S = make_solver(ctx, case, mg.F64)
    ij = S.cell_ijk[-1]
    cells = S.cells[-1]

    def up(a):
        return ref2.to_cell_order(a, ij).ravel()

    def down(v):
        return ref2.from_cell_order(v, ij, cells, shape[-1])

    assert S.dim == 2 and S.m() == int(np.prod(shape))
    for l in range(case[3]):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert info["cg_its"] == want["cg_its"] and info["degree"] == want["degree"]
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-8)
        assert info["theta"] == pytest.approx(want["theta"], rel=1e-8)
    src, dst = ctx.vector(S.m(), data=up(R["x"])), ctx.vector(S.m())
    for _ in range(3):
        S.vmult(dst, src)
        assert rel(down(dst.download()), R["vcycle"]) < 1e-8
    b, sol = ctx.vector(S.m(), data=up(R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert its == oits and red == pytest.approx(ored, rel=1e-5)
    assert rel(down(sol.download()), xo) < 1e-7
    res = ctx.vector(S.m())
    S.matrix_dg_dp.vmult_residual(res, b, sol)
    assert ctx.l2_norm(res) < 2e-9 * ctx.l2_norm(b)
    # vmult_with_residual_update (multigrid_solver_dg_plain.h:340-427)
    for factor, key in ((0.0, "update0"), (-0.37, "update1")):
        new, mgv, sums = R[key]
        got = []
        for _ in range(2):
            r, u = ctx.vector(S.m(), data=up(R["rhs"])), ctx.vector(S.m(), data=up(R["upd"]))
            got.append((S.vmult_with_residual_update(r, u, factor), r.download(), u.download()))
        s, rr, uu = got[0]
        assert rel(down(rr), new) < 1e-8 and rel(down(uu), mgv) < 1e-8
        assert s[0] == pytest.approx(sums[0], rel=1e-8) and s[1] == pytest.approx(sums[1], rel=1e-8)
        assert np.array_equal(s, got[1][0]) and np.array_equal(uu, got[1][2])
    S.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=[CASE_IDS[1], CASE_IDS[3], CASE_IDS[5]])
def test_plain_dg_multigrid_fp32_v_cycle(ctx, case):
    """the reference's default: fp32 V-cycle inside the fp64 CG; the criteria of the 3D test"""
    R = reference(case)
    o, shape = R["o"], R["shape"]
    S = make_solver(ctx, case, mg.F32)
    ij, cells = S.cell_ijk[-1], S.cells[-1]
    for l in range(case[3]):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert all(np.isfinite(v) for v in info.values())
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-4)
        if l == 0:
            assert abs(info["degree"] - want["degree"]) <= 1
        else:
            assert info["degree"] == want["degree"]
    src, dst = ctx.vector(S.m(), data=ref2.to_cell_order(R["x"], ij).ravel()), ctx.vector(S.m())
    S.vmult(dst, src)
    assert rel(ref2.from_cell_order(dst.download(), ij, cells, shape[-1]), R["vcycle"]) < 5e-4
    b, sol = ctx.vector(S.m(), data=ref2.to_cell_order(R["rhs"], ij).ravel()), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert abs(its - oits) <= 1
    assert rel(ref2.from_cell_order(sol.download(), ij, cells, shape[-1]), xo) < 1e-6
    S.close()


# ---------------------------------------------------------------------------------------- refusals and lifetime
def raw_operator(ctx, p, basis, nb, jac9, number, dim_field, width):
    """an operator from a descriptor whose dim field is given as it is (the Python class writes 0 for three dimensions)"""
    nb = np.ascontiguousarray(nb, dtype=np.int32).reshape(-1, width)
    d = _lib.DGOperatorDesc()
    d.degree, d.basis, d.number, d.n_cells = p, basis, number, nb.shape[0]
    d.neighbours = nb.ctypes.data_as(C.POINTER(C.c_int32))
    d.jacobian = (C.c_double * 9)(*np.asarray(jac9, dtype=float).ravel())
    d.dim = dim_field
    h = C.c_void_p()
    mg.check(ctx.lib.mgx_dg_operator_create(ctx.h, C.byref(d), C.byref(h)))
    op = object.__new__(mg.DGLaplaceOperator)
    op.ctx, op.lib, op.degree, op.basis, op.number, op.dim, op.h = ctx, ctx.lib, p, basis, number, 3 if dim_field in (0, 3) else dim_field, h
    return op


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


def test_refused_creates_leave_no_device_memory(ctx):
    start = live()
    nb1, _ = mg.dg_box_neighbours((1, 1))
    for bad in (1, 4, -2):
        with pytest.raises(mg.MgxError, match="dim must be") as e:
            raw_operator(ctx, 2, 0, nb1, np.eye(3), mg.F64, bad, 4)
        assert e.value.status == -1  # MGX_ERR_INVALID_ARGUMENT
        d = _lib.DGTransferDesc(2, 0, mg.F64, 1, np.arange(8, dtype=np.uint32).ctypes.data_as(_lib.u32p), bad)
        h = C.c_void_p()
        with pytest.raises(mg.MgxError, match="dim must be") as e:
            mg.check(ctx.lib.mgx_dg_transfer_create(ctx.h, C.byref(d), C.byref(h)))
        assert e.value.status == -1
    with pytest.raises(mg.MgxError, match="not positive"):                       # a mirrored cell
        mg.DGLaplaceOperator(ctx, 2, 0, nb1, np.array([[0.0, 1.0], [1.0, 0.0]]), mg.F64, dim=2)
    with pytest.raises(mg.MgxError, match="not finite"):
        mg.DGLaplaceOperator(ctx, 2, 0, nb1, np.array([[1.0, np.inf], [0.0, 1.0]]), mg.F64, dim=2)
    assert live() == start
    nb2, _ = mg.dg_box_neighbours((2, 2))
    nb21, _ = mg.dg_box_neighbours((2, 1))
    nb3, _ = mg.dg_box_neighbours((2, 2, 2))
    A0 = mg.DGLaplaceOperator(ctx, 2, 0, nb1, np.eye(2), mg.F64, dim=2)
    A1 = mg.DGLaplaceOperator(ctx, 2, 0, nb2, np.eye(2) / 2, mg.F64, dim=2)
    A1_two = mg.DGLaplaceOperator(ctx, 2, 0, nb21, np.eye(2) / 2, mg.F64, dim=2)
    A1_3d = mg.DGLaplaceOperator(ctx, 2, 0, nb3, np.eye(3) / 2, mg.F64)
    T = mg.DGLevelTransfer(ctx, 2, 0, mg.dg_box_children((1, 1)), mg.F64)
    T_3d = mg.DGLevelTransfer(ctx, 2, 0, mg.dg_box_children((1, 1, 1)), mg.F64)
    held = live()
    with pytest.raises(mg.MgxError, match="has dimension 2, the finest level 3"):   # mixed-dimension levels
        raw_solver_create(ctx, [A0, A1_3d], A1_3d, [T_3d])
    assert live() == held
    with pytest.raises(mg.MgxError, match=r"transfer\[0\] has dimension 3"):        # a 3D transfer between 2D levels
        raw_solver_create(ctx, [A0, A1], A1, [T_3d])
    assert live() == held
    with pytest.raises(mg.MgxError, match="4 x coarse = fine"):                     # 4 n(l-1) != n(l)
        raw_solver_create(ctx, [A0, A1_two], A1_two, [T])
    assert live() == held
    # entry points that are not built in 2D say so
    v = [A1.initialize_dof_vector(np.ones(A1.m())) for _ in range(4)]
    with pytest.raises(mg.MgxError, match="not built for 2D") as e:
        A1.vmult_with_cg_update(0.0, 0.0, *v)
    assert e.value.status == -4  # MGX_ERR_UNSUPPORTED
    with pytest.raises(mg.MgxError, match="one rank only") as e:
        A1.update_ghost_values(v[0])
    assert e.value.status == -4
    sd = _lib.DGSolverDesc()
    sd.matrix_dg, sd.matrix_dg_dp, sd.degree_pre = A1.h, A1.h, 3
    h = C.c_void_p()
    with pytest.raises(mg.MgxError, match="no FE_Q hierarchy in two dimensions") as e:
        mg.check(ctx.lib.mgx_dg_solver_create(ctx.h, C.byref(sd), C.byref(h)))
    assert e.value.status == -4
    for x in v:
        x.free()
    assert live() == held
    h = raw_solver_create(ctx, [A0, A1], A1, [T])                                # the consistent one is accepted
    assert live() > held
    mg.check(ctx.lib.mgx_dg_plain_solver_destroy(h))
    assert live() == held
    for x in (T, T_3d, A0, A1, A1_two, A1_3d):
        x.clear()
    assert live() == start


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
def test_lifecycle_leaves_no_device_memory(ctx, number):
    start = live()
    S = mg.DGPlainMultigridSolver(ctx, 2, mg.DG_HERMITE, (2, 1), SHEARED_2D, 2, 3, number)
    assert live() > start
    rng = np.random.default_rng(0)
    src, dst = S.initialize_dof_vector(rng.standard_normal(S.m())), S.initialize_dof_vector()
    S.vmult(dst, src)
    S.vmult_with_residual_update(src, dst, 0.5)
    assert np.isfinite(dst.download()).all()
    src.free()
    dst.free()
    S.close()
    assert live() == start


# ---------------------------------------------------------------------------------------- 3D untouched
@pytest.mark.parametrize("p", [3, 4])
def test_dim_0_and_dim_3_are_the_same_3d_operator(ctx, p):
    cells, jac = (2, 3, 2), dg.cheby_mesh(4)[1]
    nb, _ = mg.dg_box_neighbours(cells)
    rng = np.random.default_rng(p)
    n = 12 * (p + 1) ** 3
    x, xo, rhs = (rng.standard_normal(n) for _ in range(3))
    out = []
    for dim_field in (0, 3):
        A = raw_operator(ctx, p, dg.HERMITE, nb, jac, mg.F32, dim_field, 6)
        assert A.m() == n
        src, dst = A.initialize_dof_vector(x), A.initialize_dof_vector()
        A.vmult(dst, src)
        sol, old, b = A.initialize_dof_vector(x), A.initialize_dof_vector(xo), A.initialize_dof_vector(rhs)
        A.vmult_with_chebyshev_update(b, 2, 0.6, 0.2, sol, old)
        out.append((dst.download(), sol.download()))
        A.clear()
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------- harness
def recorded_iterations():
    text = open(os.path.join(ROOT, "tests", "test_dg_reference_2d.py")).read()
    m = re.search(r"HARNESS_2D_CG_ITERATIONS = \{2: (\d+), 3: (\d+)\}", text)
    return {2: int(m.group(1)), 3: int(m.group(2))}


def run_harness(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_dg_plain.py"), *args], cwd=ROOT,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.decode().strip().splitlines()


def test_poisson_dg_plain_harness_runs_in_2d():
    """tools/poisson_dg_plain.py --dim 2: the reference's table row and an iteration count in the band the 3D test
    gives its numpy prototype, [count - 3, count + 4] (the default V-cycle is fp32)"""
    want = recorded_iterations()
    rows = []
    for nr in (2, 3):
        lines = run_harness("3", str(nr), "--dim", "2")
        assert lines[-2].split() == "cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction".split()
        assert sum(l.startswith("level ") for l in lines) == nr + 1
        rows.append(lines[-1].split())
    print(rows)
    assert int(rows[0][0]) == 16 and int(rows[1][0]) == 64 and int(rows[1][1]) == 64 * 16
    for row, nr in zip(rows, (2, 3)):
        assert want[nr] - 3 <= int(row[6]) <= want[nr] + 4
    print("plateau of the benchmark's own (non-vanishing) solution in 2D: L2 error", rows[0][4], rows[1][4])


def test_poisson_dg_plain_discretisation_error_converges_in_2d():
    """for a solution that vanishes on the boundary the L2 error of FE_DGQHermite(3) falls with h^4: the 3D test's band"""
    err = []
    for nr in (3, 4):
        lines = run_harness("3", str(nr), "--dim", "2", "--solution", "vanishing", "--vcycle", "f64", "--levels")
        assert any(l.startswith("level  smoother") for l in lines)
        err.append(float(lines[-1].split()[4]))
    print(err)
    assert 11 < err[0] / err[1] < 20, err
