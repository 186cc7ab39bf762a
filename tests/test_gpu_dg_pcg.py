"""Lumped-mass PCG on the DG-SIP operator on the GPU (include/mgx_dg.h: mgx_dg_operator_lumped_mass_inverse,
mgx_dg_vmult_with_pcg_sums, mgx_dg_pcg_solver_*; the solver of solver_dg/program.cc) in three and two dimensions,
against the numpy restatement tests/dg_pcg_reference.py, which tests/test_dg_pcg_reference.py pins on the CPU.

Boxes.  3D: (3,1,2) is one partly filled workgroup at every degree; (4,4,2) with the Jacobian of cheby_mesh(5) is several
workgroups with a partly filled last one at p = 2 and p = 4 (14 and 5 cells per workgroup in fp64).  2D: (1,1), (5,3)
and (17,13), the shapes tests/test_gpu_dg_2d.py justifies (one cell; one partly filled workgroup; 2 ... 9 workgroups
with a partly filled last one).

Tolerances.  The operator tolerance is that of tests/test_gpu_dg.py (2e-11 / 3e-5); q is held to 5 x that and the sums
to rtol 20 x that, as test_merged_cg_update holds them.  Solver quantities (x and the history rho_k) are held to 1e-8
(fp64) and 5e-4 (fp32) against the fp64 restatement, in the measure every DG test here uses: the largest difference
over the largest entry of the reference."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_pcg_reference as pcg  # noqa: E402
import dg_reference_2d as ref2  # noqa: E402

_lib = mg._lib
TOL = {mg.F64: 2e-11, mg.F32: 3e-5}
SOLVER_TOL = {mg.F64: 1e-8, mg.F32: 5e-4}
NUMBERS = [mg.F64, mg.F32]
NUMBER_IDS = ["f64", "f32"]
KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
JAC = {2: SHEARED_2D, 3: dg.cheby_mesh(5)[1]}
BOXES_SUMS = [(3, 1, 2), (4, 4, 2), (1, 1), (5, 3), (17, 13)]
BOXES_SOLVER = [(4, 4, 2), (3, 1, 2), (5, 3), (17, 13)]
BOX_IDS = lambda c: "x".join(map(str, c))  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def live():
    return _lib.load().mgx_live_device_allocations()


@functools.lru_cache(maxsize=4)
def oracle(p, kind, cells, jac):
    """the face-based oracle of a box, built once for the cases that follow one another on it (fp64 and fp32; the two
    solves of a test); read only"""
    J = np.array(jac).reshape(len(cells), len(cells))
    return ref2.DGOracle2D(p, kind, cells, J) if len(cells) == 2 else dg.DGOracle(p, kind, cells, J)


class Case:
    """oracle and HIP operator on the same box of cells (two or three dimensions by the length of `cells`); vectors
    travel in the oracle's layout"""

    def __init__(self, ctx, p, kind, cells, number, jac=None):
        self.dim = dim = len(cells)
        self.jac = JAC[dim] if jac is None else jac
        self.orc = oracle(p, kind, tuple(cells), tuple(np.asarray(self.jac).ravel()))
        nb, self.ijk = mg.dg_box_neighbours(cells, "z")
        self.op = mg.DGLaplaceOperator(ctx, p, kind, nb, self.jac, number, dim=dim)
        self.m = pcg.lumped_mass_inverse(p, kind, self.jac)
        assert self.op.m() == int(np.prod(self.orc.shape)) == self.op.vector_size()

    def up(self, x):
        i = self.ijk
        if self.dim == 2:
            return self.op.initialize_dof_vector(ref2.to_cell_order(x, i).ravel())
        return self.op.initialize_dof_vector(x[i[:, 2], i[:, 1], i[:, 0]].ravel())

    def down(self, v):
        a = v.download().astype(float)
        if self.dim == 2:
            return ref2.from_cell_order(a, self.ijk, self.orc.cells, self.orc.shape[-1])
        out, i = np.empty(self.orc.shape), self.ijk
        out[i[:, 2], i[:, 1], i[:, 0]] = a.reshape(len(i), -1)
        return out

    def close(self):
        self.op.clear()


# ---------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lumped_mass_inverse_from_the_c_abi(ctx, kind, number):
    """the fp64 table of the operator (whatever its number type) against numpy, p = 1 ... 9, both dimensions"""
    for dim, cells in ((3, (1, 1, 1)), (2, (1, 1))):
        nb, _ = mg.dg_box_neighbours(cells)
        for p in range(1, 10):
            op = mg.DGLaplaceOperator(ctx, p, kind, nb, JAC[dim], number, dim=dim)
            got, ref = op.lumped_mass_inverse(), pcg.lumped_mass_inverse(p, kind, JAC[dim])
            op.clear()
            assert got.shape == ref.shape == ((p + 1) ** dim,)
            assert (got > 0).all() and np.isfinite(got).all()
            assert abs(got / ref - 1).max() < 1e-13, (dim, p)


# ---------------------------------------------------------------------------------------- kPcgSums
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 6, 8])
def test_vmult_with_pcg_sums(ctx, p, kind, number):
    rng = np.random.default_rng(17 + p)
    tol = TOL[number] * 5
    for cells in BOXES_SUMS:
        case = Case(ctx, p, kind, cells, number)
        o, m = case.orc, case.m
        r, pv = rng.standard_normal(o.shape), rng.standard_normal(o.shape)
        R, Pv = case.up(r), case.up(pv)
        r_bits, p_bits = R.download(), Pv.download()
        got = []
        for _ in range(2):
            Q = case.op.initialize_dof_vector(np.full(r.size, np.nan))      # an unwritten entry shows
            sums = case.op.vmult_with_pcg_sums(R, Q, Pv)
            got.append((Q.download(), sums))
        q_ref = o.vmult(pv)
        ref = np.array([(q_ref * pv).sum(), (r * m * r).sum(), (q_ref * m * r).sum(), (q_ref * m * q_ref).sum()])
        err_q, err_s = rel(case.down(Q), q_ref), abs(sums - ref).max() / abs(ref).max()
        print("pcg sums p=%d kind=%d %s: q %.3e, sums %.3e" % (p, kind, cells, err_q, err_s))
        assert err_q < tol, cells
        assert np.allclose(sums, ref, rtol=tol * 20, atol=tol * 20 * abs(ref).max()), cells
        assert np.array_equal(R.download(), r_bits) and np.array_equal(Pv.download(), p_bits), cells   # r, p not written
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), cells    # same bits
        case.close()


# ---------------------------------------------------------------------------------------- the solver
def solve(case, form, b, n_iterations, tolerance=0.0, check_every=1):
    S = mg.DGConjugateGradient(case.op, form, n_iterations, tolerance, check_every)
    B, X = case.up(b), case.op.initialize_dof_vector(np.full(b.size, np.nan))
    its, rate = S.solve(B, X)
    out = case.down(X), S.history(), its, rate, X.download()
    S.close()
    return out


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [2, 3, 4, 8])
@pytest.mark.parametrize("cells", BOXES_SOLVER, ids=BOX_IDS)
def test_merged_solver_equals_the_restatement(ctx, cells, p, kind, number):
    case = Case(ctx, p, kind, cells, number)
    b = np.random.default_rng(23 + p).random(case.orc.shape)        # rhs in [0, 1), solver_dg/program.cc:157-158
    x_ref, h_ref, stalled = pcg.merged_pcg(case.orc.vmult, case.m, b, 10)
    assert stalled == -1
    x, h, its, rate, bits = solve(case, mg.DG_PCG_MERGED, b, 10)
    err_x, err_h = rel(x, x_ref), rel(h, h_ref)
    print("merged solver p=%d kind=%d %s number=%d: x %.3e, history %.3e" % (p, kind, cells, number, err_x, err_h))
    assert its == 10 and h.shape == (11,)
    assert err_x < SOLVER_TOL[number] and err_h < SOLVER_TOL[number]
    assert np.isclose(rate, np.sqrt(h[10] / h[0]) ** 0.1, rtol=1e-12)
    x2, h2, _, _, bits2 = solve(case, mg.DG_PCG_MERGED, b, 10)
    assert np.array_equal(bits, bits2) and np.array_equal(h, h2)       # two solves, identical bits
    case.close()


def test_many_block_sums_are_added_in_two_stages(ctx):
    """Above 4096 block sums the solver adds them with 256 workgroups first and one workgroup then.  40 x 40 x 36 cells
    at p = 2 in fp64 are 14 cells per workgroup and 4115 block sums, 17 per workgroup of the first stage with the last
    13 workgroups empty and one partly filled; 1.6 M DoFs, three iterations."""
    case = Case(ctx, 2, dg.GAUSS, (40, 40, 36), mg.F64)
    assert -(-case.op.m() // 27 // 14) == 4115
    b = np.random.default_rng(31).random(case.orc.shape)
    x_ref, h_ref, stalled = pcg.merged_pcg(case.orc.vmult, case.m, b, 3)
    x, h, its, _, bits = solve(case, mg.DG_PCG_MERGED, b, 3)
    print("two-stage sums: x %.3e, history %.3e" % (rel(x, x_ref), rel(h, h_ref)))
    assert stalled == -1 and its == 3
    assert rel(x, x_ref) < SOLVER_TOL[mg.F64] and rel(h, h_ref) < SOLVER_TOL[mg.F64]
    _, h2, _, _, bits2 = solve(case, mg.DG_PCG_MERGED, b, 3)
    assert np.array_equal(bits, bits2) and np.array_equal(h, h2)
    case.close()


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("cells", BOXES_SOLVER, ids=BOX_IDS)
def test_separate_form_equals_merged_form(ctx, cells, p, kind, number):
    case = Case(ctx, p, kind, cells, number)
    b = np.random.default_rng(29 + p).random(case.orc.shape)
    x_m, h_m, its_m, rate_m, _ = solve(case, mg.DG_PCG_MERGED, b, 10)
    x_s, h_s, its_s, rate_s, _ = solve(case, mg.DG_PCG_SEPARATE, b, 10)
    err_x, err_h = rel(x_s, x_m), rel(h_s, h_m)
    print("separate vs merged p=%d kind=%d %s number=%d: x %.3e, history %.3e" % (p, kind, cells, number, err_x, err_h))
    assert its_m == its_s == 10 and h_s.shape == h_m.shape == (11,)
    assert err_x < SOLVER_TOL[number] and err_h < SOLVER_TOL[number]
    assert np.isclose(rate_s, rate_m, rtol=SOLVER_TOL[number])
    case.close()


# Cases of the stopping rule, picked on the CPU from the restatement (fp64, tolerance 1e-6, rhs = default_rng(seed).random):
# the iteration k at which sqrt(rho_k / rho_0) first falls below the tolerance, and the factors by which the value one
# iteration earlier lies above it / the value at k below it / the value at k rounded up to a multiple of 4 below it.
# On a 2 x 2 x 2 box at p = 2 the iteration gains a factor of about 1.5 per step around the threshold, so no right-hand
# side there leaves a factor 1.5 on both sides; these boxes are small enough to be in the superlinear phase there.
#               dim-cells   p  kind               seed  k   k4  above  below  below at k4
STOP_CASES = [((2, 1), 3, dg.GAUSS, 1, 30, 32),          # 5.12   5.66   558
              ((1, 1, 1), 2, dg.GAUSS_LOBATTO, 1, 19, 20),  # 2.92   2.06   29.0
              ((1, 1, 1), 2, dg.GAUSS, 2, 15, 16),       # 2.21   2.12   6.58
              ((3, 2), 1, dg.HERMITE, 1, 18, 20),        # 2.37   2.19   116
              ((2, 1), 2, dg.GAUSS_LOBATTO, 2, 16, 16)]  # 4.39   2.69   2.69


@pytest.mark.parametrize("form", [mg.DG_PCG_MERGED, mg.DG_PCG_SEPARATE], ids=["merged", "separate"])
@pytest.mark.parametrize("cells,p,kind,seed,k,k4", STOP_CASES, ids=[BOX_IDS(c[0]) + "-p%d-k%d" % (c[1], c[2]) for c in STOP_CASES])
def test_stopping_rule(ctx, cells, p, kind, seed, k, k4, form):
    jac = SHEARED_2D if len(cells) == 2 else dg.cheby_mesh(3)[1]
    case = Case(ctx, p, kind, cells, mg.F64, jac)
    b = np.random.default_rng(seed).random(case.orc.shape)
    _, h_ref, stalled = pcg.merged_pcg(case.orc.vmult, case.m, b, 60)
    red = np.sqrt(h_ref / h_ref[0])
    assert pcg.stop_iteration(h_ref, 1e-6, 1, stalled) == k and pcg.stop_iteration(h_ref, 1e-6, 4, stalled) == k4
    assert red[k - 1] >= 1.5e-6 and red[k] <= 1e-6 / 1.5 and red[k4] <= 1e-6 / 1.5 and not 0 <= stalled <= k4   # the margins
    for every, expect in ((1, k), (4, k4)):
        x, h, its, rate, _ = solve(case, form, b, 60, 1e-6, every)
        print("stop %s p=%d kind=%d every %d: %d iterations, rate %.4f" % (cells, p, kind, every, its, rate))
        assert its == expect and h.shape == (expect + 1,)
        assert np.sqrt(h[its] / h[0]) <= 1e-6
        assert np.isclose(rate, np.sqrt(h[its] / h[0]) ** (1.0 / its), rtol=1e-12)
    case.close()


# ---------------------------------------------------------------------------------------- guard, refusals, memory
@pytest.mark.parametrize("form", [mg.DG_PCG_MERGED, mg.DG_PCG_SEPARATE], ids=["merged", "separate"])
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
def test_zero_right_hand_side(ctx, number, form):
    for cells in ((5, 3), (3, 1, 2)):
        case = Case(ctx, 3, dg.HERMITE, cells, number)
        for tolerance, every, n in ((0.0, 1, 5), (1e-6, 4, 9), (0.0, 1, 0)):
            x, h, its, rate, bits = solve(case, form, np.zeros(case.orc.shape), n, tolerance, every)
            assert its == 0 and rate == 0.0
            assert not bits.any() and np.isfinite(h).all() and not h.any()
        case.close()


def test_more_iterations_than_unknowns(ctx):
    """1 x 1 cell, p = 1 in 2D: 4 unknowns, 12 iterations in fp64"""
    for kind in KINDS:
        case = Case(ctx, 1, kind, (1, 1), mg.F64)
        b = np.random.default_rng(9).random(case.orc.shape)
        x, h, its, rate, _ = solve(case, mg.DG_PCG_MERGED, b, 12)
        exact = np.linalg.solve(case.orc.dense_matrix(), b.ravel()).reshape(b.shape)
        print("guard kind=%d: %d iterations, error %.3e" % (kind, its, rel(x, exact)))
        assert np.isfinite(x).all() and np.isfinite(h).all() and np.isfinite(rate)
        assert rel(x, exact) < 1e-10
        assert its <= 12 and h.shape == (13,)
        case.close()


def test_refusals(ctx):
    start = live()
    case3, case2 = Case(ctx, 2, dg.HERMITE, (2, 2, 2), mg.F64), Case(ctx, 2, dg.HERMITE, (2, 2), mg.F64)
    held = live()
    for case in (case3, case2):
        v = [case.op.initialize_dof_vector(np.ones(case.op.m())) for _ in range(3)]
        with pytest.raises(mg.MgxError, match="null or aliased"):
            case.op.vmult_with_pcg_sums(v[0], v[1], v[1])                      # q aliases p
        with pytest.raises(mg.MgxError, match="null or aliased"):
            case.op.vmult_with_pcg_sums(v[0], v[0], v[1])                      # q aliases r
        sums = np.empty(4)
        with pytest.raises(mg.MgxError, match="null or aliased"):
            mg.check(ctx.lib.mgx_dg_vmult_with_pcg_sums(case.op.h, v[0].ptr, None, v[1].ptr, sums.ctypes.data_as(_lib.f64p)))
        with pytest.raises(mg.MgxError, match="null argument"):
            mg.check(ctx.lib.mgx_dg_operator_lumped_mass_inverse(case.op.h, None))
        S = mg.DGConjugateGradient(case.op, mg.DG_PCG_MERGED, 3)
        with pytest.raises(mg.MgxError, match="null or aliased"):
            S.solve(v[0], v[0])
        with pytest.raises(mg.MgxError, match="null or aliased"):
            mg.check(ctx.lib.mgx_dg_pcg_solver_solve(S.h, v[0].ptr, None, None, None))
        S.close()
        for form, n, tolerance, every, what in ((7, 3, 0.0, 1, "form must be"), (0, 3, -1.0, 1, "tolerance must be"),
                                                (0, 3, np.nan, 1, "tolerance must be"), (0, 3, 0.0, 0, "check_every must be")):
            with pytest.raises(mg.MgxError, match=what) as e:
                mg.DGConjugateGradient(case.op, form, n, tolerance, every)
            assert e.value.status == -1
        h = C.c_void_p()
        with pytest.raises(mg.MgxError, match="null argument"):
            mg.check(ctx.lib.mgx_dg_pcg_solver_create(ctx.h, None, C.byref(h)))
        for x in v:
            x.free()
        assert live() == held
    # the merged CG iteration without preconditioner stays a 3D entry point
    v = [case2.op.initialize_dof_vector(np.ones(case2.op.m())) for _ in range(4)]
    with pytest.raises(mg.MgxError, match="not built for 2D") as e:
        case2.op.vmult_with_cg_update(0.0, 0.0, *v)
    assert e.value.status == -4
    for x in v:
        x.free()
    # (a decomposed operator -- ghost cells -- needs a communicator on the context, which tests/test_gpu_dg.py builds
    # in worker processes only: its refusal by mgx_dg_pcg_solver_create is not run here)
    case3.close()
    case2.close()
    assert live() == start


@pytest.mark.parametrize("form", [mg.DG_PCG_MERGED, mg.DG_PCG_SEPARATE], ids=["merged", "separate"])
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
def test_lifecycle_leaves_no_device_memory(ctx, number, form):
    start = live()
    case = Case(ctx, 2, dg.GAUSS, (5, 3), number)
    b, x = case.up(np.ones(case.orc.shape)), case.op.initialize_dof_vector()
    before = live()
    S = mg.DGConjugateGradient(case.op, form, 4, 1e-3, 2)
    assert live() > before
    its, _ = S.solve(b, x)
    assert 0 < its <= 4 and np.isfinite(x.download()).all()
    S.close()
    assert live() == before
    b.free()
    x.free()
    case.close()
    assert live() == start
