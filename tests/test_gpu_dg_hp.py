"""Degree-to-degree DG transfers and the plain DG multigrid on mixed h/p level hierarchies on the GPU (include/mgx_dg.h:
mgx_dg_degree_transfer_*, mgx_dg_hp_solver_create) against the numpy restatement tests/dg_hp_reference.py: the transfer
kernel for every pair of degrees, in 3D and 2D, fp64 and fp32; the solver on p-only, hp and ph hierarchies as
tests/test_gpu_dg_plain.py checks the h-only one, with its tolerances; an h-only `hierarchy=` against the solver built
without the keyword; refusals, device memory, and the harness tools/poisson_dg_plain.py --hierarchy.

Cell counts of the transfer cases are prime (19 in 3D, 67 in 2D): whatever the cells per workgroup (at most 8 / 64), the
last workgroup is partly filled and there are several."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_hp_reference as hp  # noqa: E402
import dg_reference_2d as ref2  # noqa: E402

_lib = mg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(pf, pc) for pf in range(2, 10) for pc in range(1, pf)]


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def live():
    return _lib.load().mgx_live_device_allocations()


# ---------------------------------------------------------------------------------------- transfers
def check_degree_transfer(ctx, pf, pc, basis, n_cells, dim, number, tol):
    Ek = hp.embedding_nd(hp.degree_embedding_1d(pf, pc, basis), dim)
    rng = np.random.default_rng(1000 * pf + 10 * pc + dim)
    c0, f0 = rng.standard_normal((n_cells, (pc + 1) ** dim)), rng.standard_normal((n_cells, (pf + 1) ** dim))
    dt = mg._DT[number]
    T = mg.DGDegreeTransfer(ctx, pf, pc, basis, n_cells, number, dim)
    coarse = ctx.vector(c0.size, number, c0.ravel())
    got = []
    for _ in range(2):      # both operations add: the destination starts from random values
        fine = ctx.vector(f0.size, number, f0.ravel())
        T.prolongate_and_add(fine, coarse)
        got.append(fine.download())
    want = f0 + c0 @ Ek.T
    print("prolongation %d->%d basis=%d dim=%d n=%d: %.3e" % (pc, pf, basis, dim, n_cells, rel(got[0].reshape(want.shape), want)))
    assert rel(got[0].reshape(want.shape), want) < tol
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(coarse.download(), c0.ravel().astype(dt))          # source untouched
    fine = ctx.vector(f0.size, number, f0.ravel())
    got = []
    for _ in range(2):
        dst = ctx.vector(c0.size, number, c0.ravel())
        T.restrict_and_add(dst, fine)
        got.append(dst.download())
    want = c0 + f0 @ Ek
    print("restriction  %d->%d basis=%d dim=%d n=%d: %.3e" % (pf, pc, basis, dim, n_cells, rel(got[0].reshape(want.shape), want)))
    assert rel(got[0].reshape(want.shape), want) < tol
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(fine.download(), f0.ravel().astype(dt))
    T.clear()


@pytest.mark.parametrize("dim,n_cells", [(3, 1), (3, 19), (2, 1), (2, 67)])
@pytest.mark.parametrize("pf,pc", PAIRS)
def test_degree_transfers_fp64(ctx, pf, pc, dim, n_cells):
    """the bases rotate over the pairs: each basis meets each fine degree >= 4, pf = 2 (one pair) and 3 (two) as far as
    their pairs go"""
    check_degree_transfer(ctx, pf, pc, (pf + pc) % 3, n_cells, dim, mg.F64, 1e-11)


@pytest.mark.parametrize("dim,n_cells", [(3, 19), (2, 67)])
@pytest.mark.parametrize("pf,pc", [(2, 1), (4, 2), (8, 4), (9, 1), (9, 8)])
def test_degree_transfers_fp32(ctx, pf, pc, dim, n_cells):
    check_degree_transfer(ctx, pf, pc, (pf + pc) % 3, n_cells, dim, mg.F32, 5e-6)


@pytest.mark.parametrize("basis", [0, 1, 2])
def test_degree_transfer_matrix_is_the_host_function(ctx, basis):
    for pf, pc in PAIRS:
        T = mg.DGDegreeTransfer(ctx, pf, pc, basis, 1, mg.F64)
        assert np.array_equal(T.matrix(), mg.dg_degree_embedding(pf, pc, basis))
        T.clear()


def test_degree_transfer_refusals(ctx):
    start = live()
    for args, match in (((3, 3, 0, 5), "below the fine degree"), ((2, 4, 0, 5), "below the fine degree"),
                        ((10, 2, 0, 5), "degrees must be in"), ((3, 0, 0, 5), "degrees must be in"),
                        ((3, 1, 3, 5), "basis"), ((3, 1, 0, 0), "n_cells")):
        with pytest.raises(mg.MgxError, match=match):
            mg.DGDegreeTransfer(ctx, *args)
    with pytest.raises(mg.MgxError, match="number"):
        mg.DGDegreeTransfer(ctx, 3, 1, 0, 5, number=7)
    with pytest.raises(mg.MgxError, match="dim"):
        mg.DGDegreeTransfer(ctx, 3, 1, 0, 5, dim=4)
    assert live() == start
    T = mg.DGDegreeTransfer(ctx, 3, 1, 0, 5, mg.F64)
    v = ctx.vector(5 * 64)
    for op in (T.prolongate_and_add, T.restrict_and_add):
        with pytest.raises(mg.MgxError, match="null or aliased"):
            op(v, v)
        with pytest.raises(mg.MgxError, match="null or aliased"):
            op(v, None)
        with pytest.raises(mg.MgxError, match="null or aliased"):
            op(None, v)
    T.clear()
    v.free()
    assert live() == start


# ---------------------------------------------------------------------------------------- solver
def orders(S, dim):
    """(to the reference's array, from it) for the finest level of a solver"""
    ijk, n_loc = S.cell_ijk[-1], (S.degree + 1) ** dim
    if dim == 3:
        shape = tuple(S.cells[-1])[::-1] + (n_loc,)

        def to_oracle(v):
            out = np.empty(shape)
            out[ijk[:, 2], ijk[:, 1], ijk[:, 0]] = np.asarray(v, dtype=float).reshape(len(ijk), -1)
            return out
        return to_oracle, lambda a: a[ijk[:, 2], ijk[:, 1], ijk[:, 0]].ravel()
    return (lambda v: ref2.from_cell_order(np.asarray(v, dtype=float), ijk, S.cells[-1], n_loc),
            lambda a: ref2.to_cell_order(a, ijk).ravel())


def make_solver(ctx, name, number, neumann_sides=()):
    basis, cells, hierarchy, jac = hp.SOLVER_CASES[name]
    return mg.DGPlainMultigridSolver(ctx, hierarchy[-1][0], basis, cells, jac, None, 3, number, neumann_sides=neumann_sides,
                                     hierarchy=hierarchy)


def check_solver_fp64(ctx, name, neumann_sides=()):
    R = hp.solved_case(name, neumann_sides)
    o = R["o"]
    S = make_solver(ctx, name, mg.F64, neumann_sides)
    to_oracle, to_product = orders(S, o.dim)
    assert S.n_levels == o.n_levels
    for l in range(o.n_levels):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert info["cg_its"] == want["cg_its"] and info["degree"] == want["degree"]
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-8)
        assert info["theta"] == pytest.approx(want["theta"], rel=1e-8)
    src, dst = ctx.vector(S.m(), data=to_product(R["x"])), ctx.vector(S.m())
    for _ in range(3):
        S.vmult(dst, src)
        assert rel(to_oracle(dst.download()), R["vcycle"]) < 1e-8
    b, sol = ctx.vector(S.m(), data=to_product(R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert its == oits and red == pytest.approx(ored, rel=1e-5)
    assert rel(to_oracle(sol.download()), xo) < 1e-7
    res = ctx.vector(S.m())
    S.matrix_dg_dp.vmult_residual(res, b, sol)
    assert ctx.l2_norm(res) < 2e-9 * ctx.l2_norm(b)
    for factor, key in ((0.0, "update0"), (-0.37, "update1")):
        new, mgv, sums = R[key]
        got = []
        for _ in range(2):
            r, u = ctx.vector(S.m(), data=to_product(R["rhs"])), ctx.vector(S.m(), data=to_product(R["upd"]))
            got.append((S.vmult_with_residual_update(r, u, factor), r.download(), u.download()))
        s, rr, uu = got[0]
        assert rel(to_oracle(rr), new) < 1e-8 and rel(to_oracle(uu), mgv) < 1e-8
        assert s[0] == pytest.approx(sums[0], rel=1e-8) and s[1] == pytest.approx(sums[1], rel=1e-8)
        assert np.array_equal(s, got[1][0]) and np.array_equal(uu, got[1][2])
    S.close()


@pytest.mark.parametrize("name", sorted(hp.SOLVER_CASES))
def test_hp_dg_multigrid_fp64(ctx, name):
    check_solver_fp64(ctx, name)


def test_hp_dg_multigrid_with_a_neumann_side_fp64(ctx):
    """against DGHPOracle with the side marked on every level as tests/dg_mixed_reference.py marks its operators"""
    check_solver_fp64(ctx, hp.NEUMANN_CASE, hp.NEUMANN_SIDES)


@pytest.mark.parametrize("name", sorted(hp.SOLVER_CASES))
def test_hp_dg_multigrid_fp32_v_cycle(ctx, name):
    R = hp.solved_case(name)
    o = R["o"]
    S = make_solver(ctx, name, mg.F32)
    to_oracle, to_product = orders(S, o.dim)
    for l in range(o.n_levels):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert all(np.isfinite(v) for v in info.values())
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-4)
        if l == 0:
            assert abs(info["degree"] - want["degree"]) <= 1
        else:
            assert info["degree"] == want["degree"]
    src, dst = ctx.vector(S.m(), data=to_product(R["x"])), ctx.vector(S.m())
    S.vmult(dst, src)
    assert rel(to_oracle(dst.download()), R["vcycle"]) < 5e-4
    b, sol = ctx.vector(S.m(), data=to_product(R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert abs(its - oits) <= 1 and red == pytest.approx(ored, rel=0.05)
    assert rel(to_oracle(sol.download()), xo) < 1e-6
    S.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_h_only_hierarchy_is_the_plain_solver(ctx, dim):
    cells, jac = ((2, 1, 1), hp.SHEARED_3D) if dim == 3 else ((2, 1), hp.SHEARED_2D)
    out = []
    for hierarchy in (None, [(3, 0), (3, 1), (3, 2)]):
        S = mg.DGPlainMultigridSolver(ctx, 3, mg.DG_HERMITE, cells, jac, 3, 3, mg.F32, hierarchy=hierarchy)
        rng = np.random.default_rng(5)
        src, dst, sol = S.initialize_dof_vector(rng.standard_normal(S.m())), S.initialize_dof_vector(), S.initialize_dof_vector()
        S.vmult(dst, src)
        its, red = S.solve_cg(src, sol, 1e-9)
        out.append(([S.smoother_info(l) for l in range(3)], dst.download(), sol.download(), its, red))
        S.close()
    a, b = out
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_hierarchy_keyword_is_checked(ctx):
    for hierarchy in ([(1, 1), (2, 1)], [(1, 0), (2, 1)], [(2, 0), (1, 0)], [(1, 0), (1, 2)], [(1, 0), (3, 0)], []):
        with pytest.raises(ValueError, match="hierarchy"):
            mg.DGPlainMultigridSolver(ctx, 2, 0, (1, 1, 1), np.eye(3), None, hierarchy=hierarchy)
    with pytest.raises(ValueError, match="n_levels - 1"):
        mg.DGPlainMultigridSolver(ctx, 2, 0, (1, 1, 1), np.eye(3), 3, hierarchy=[(1, 0), (2, 0)])


# ---------------------------------------------------------------------------------------- refusals and lifetime
def raw_hp_create(ctx, matrices, matrix_dp, transfers, degree_transfers, degree_pre=3):
    n = len(matrices)
    d = _lib.DGHPSolverDesc()
    d.n_levels = n
    d.matrix = (_lib.vp * n)(*[m.h for m in matrices])
    d.matrix_dg_dp = matrix_dp.h
    d.transfer = (_lib.vp * max(1, n - 1))(*[t.h if t is not None else None for t in transfers])
    d.degree_transfer = (_lib.vp * max(1, n - 1))(*[t.h if t is not None else None for t in degree_transfers])
    d.degree_pre = degree_pre
    h = C.c_void_p()
    mg.check(ctx.lib.mgx_dg_hp_solver_create(ctx.h, C.byref(d), C.byref(h)))
    return h


def test_refused_hp_creates_leave_no_device_memory(ctx):
    start = live()
    nb1, _ = mg.dg_box_neighbours((1, 1, 1))
    nb2, _ = mg.dg_box_neighbours((2, 2, 2))
    nbq, _ = mg.dg_box_neighbours((1, 1))
    op = lambda p, nb, basis=0, number=mg.F64, dim=3, h=1.0: mg.DGLaplaceOperator(ctx, p, basis, nb, np.eye(dim) * h, number, dim=dim)
    A1, A2, A3 = op(1, nb1), op(2, nb1), op(3, nb1)
    A2_fine, A2_gl, A2_f32, A2_2d = op(2, nb2, h=0.5), op(2, nb1, basis=1), op(2, nb1, number=mg.F32), op(2, nbq, dim=2)
    H = mg.DGLevelTransfer(ctx, 2, 0, mg.dg_box_children((1, 1, 1)), mg.F64)
    P21 = mg.DGDegreeTransfer(ctx, 2, 1, 0, 1, mg.F64)
    P31 = mg.DGDegreeTransfer(ctx, 3, 1, 0, 1, mg.F64)
    P21_8 = mg.DGDegreeTransfer(ctx, 2, 1, 0, 8, mg.F64)
    held = live()
    cases = [
        (([A1, A2], A2, [H], [P21]), "level 0 to level 1 needs exactly one.*both"),
        (([A1, A2], A2, [None], [None]), "level 0 to level 1 needs exactly one.*neither"),
        (([A1, A2_fine], A2_fine, [None], [P21_8]), "level 0 to level 1 is a degree raise: the levels have 1 and 8 cells"),
        (([A2, A1], A1, [None], [P21]), "level 0 to level 1 is a degree raise: the coarse degree 2 must be below"),
        (([A2, A2], A2, [None], [P21]), "level 0 to level 1 is a degree raise: the coarse degree 2 must be below"),
        (([A1, A2], A2, [None], [P31]), "level 0 to level 1: the degree transfer is between degrees 1 and 3"),
        (([A1, A2, A3], A3, [None, None], [P21, P31]), "level 1 to level 2: the degree transfer is between degrees 1 and 3"),
        (([A1, A2_gl, A3], A3, [None, None], [P21, P31]), "level 1: matrix\\[1\\] differs from the finest level in basis"),
        (([A1, A2_2d, A3], A3, [None, None], [P21, P31]), "level 1: matrix\\[1\\] has dimension 2"),
        (([A1, A2], A2_f32, [None], [P21]), "matrix_dg_dp must be the fp64 twin of the operator of level 1"),
        (([A1, A2], A3, [None], [P21]), "matrix_dg_dp must be the fp64 twin of the operator of level 1"),
        (([A2, A2_fine], A2_fine, [None], [P21_8]), "level 0 to level 1 is a degree raise: the levels have 1 and 8 cells"),
        (([A1, A2_fine], A2_fine, [H], [None]), "level 0 to level 1 is a mesh refinement: the levels have degrees 1 and 2"),
    ]
    for args, match in cases:
        with pytest.raises(mg.MgxError, match=match) as e:
            raw_hp_create(ctx, *args)
        assert e.value.status == -1  # MGX_ERR_INVALID_ARGUMENT
        assert live() == held
    for args in (([A1, A2], A2, [None], [P21]), ([A2, A2_fine], A2_fine, [H], [None])):    # the consistent ones are accepted
        h = raw_hp_create(ctx, *args)
        assert live() > held
        mg.check(ctx.lib.mgx_dg_plain_solver_destroy(h))
        assert live() == held
    for x in (H, P21, P31, P21_8, A1, A2, A3, A2_fine, A2_gl, A2_f32, A2_2d):
        x.clear()
    assert live() == start


@pytest.mark.parametrize("number", [mg.F64, mg.F32], ids=["f64", "f32"])
def test_hp_lifecycle_leaves_no_device_memory(ctx, number):
    start = live()
    rng = np.random.default_rng(0)
    for cells, jac, hierarchy in (((2, 1, 1), hp.SHEARED_3D, [(1, 0), (2, 0)]),               # p
                                  ((2, 1, 1), hp.SHEARED_3D, [(1, 0), (2, 0), (2, 1)]),       # hp
                                  ((2, 1), hp.SHEARED_2D, [(1, 0), (1, 1), (3, 1)])):         # ph
        S = mg.DGPlainMultigridSolver(ctx, hierarchy[-1][0], mg.DG_HERMITE, cells, jac, None, 3, number, hierarchy=hierarchy)
        assert live() > start
        src, dst = S.initialize_dof_vector(rng.standard_normal(S.m())), S.initialize_dof_vector()
        S.vmult(dst, src)
        S.vmult_with_residual_update(src, dst, 0.5)
        assert np.isfinite(dst.download()).all()
        src.free()
        dst.free()
        S.close()
        assert live() == start


# ---------------------------------------------------------------------------------------- harness
@pytest.mark.parametrize("args", [("--hierarchy", "hp"), ("--hierarchy", "ph"), ("--hierarchy", "hp", "--dim", "2")],
                         ids=["hp", "ph", "hp-2d"])
def test_poisson_dg_plain_harness_runs_hp_hierarchies(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poisson_dg_plain.py"), "3", "2", *args], cwd=ROOT,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.decode().strip().splitlines()
    assert lines[-2].split() == "cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction".split()
    row = lines[-1].split()
    print(row)
    assert np.isfinite(float(row[4])) and int(row[6]) < 100
    # degree 3 -> 1 on one mesh, two refinements: four levels, of degrees 1 3 3 3 (hp) or 1 1 1 3 (ph)
    levels = [l for l in lines if l.startswith("level ")]
    assert len(levels) == 4
