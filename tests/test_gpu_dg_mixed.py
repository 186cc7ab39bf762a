"""DG-SIP operator with Neumann faces on the GPU (include/mgx_dg.h: MGX_DG_NEUMANN, mgx_dg_box_set_sides,
mgx_dg_compute_rhs_mixed and the solvers' refusals), in three and two dimensions, against the numpy restatement
tests/dg_mixed_reference.py, which tests/test_dg_mixed_reference.py pins on the CPU.

Meshes.  A face is interior (I), Dirichlet (D) or Neumann (N); a cell has a (lower, upper) pair of kinds per direction,
and the kernels, the category of the block-Jacobi diagonal and the right-hand side treat every pair on its own.  A
direction with one cell gives one pair of boundary kinds, so all nine pairs in every direction need four meshes with one
cell in that direction next to the multi-cell ones; MESHES holds the smallest sheared boxes that do it and the module
asserts the coverage (test_meshes_reach_every_pair_of_face_kinds); every degree runs all of them (the boxes of a case
share the dense blocks of one restatement).  LARGE: more cells than one workgroup takes, and no multiple of it
(3D p = 2: 14 cells per workgroup, 30 cells; 2D p = 4: 51 cells per workgroup, 63 cells).

Bounds are those of the Dirichlet tests for the same quantity: the operator 2e-11 (fp64) and 3e-5 (fp32)
(tests/test_gpu_dg.py, test_gpu_dg_2d.py), 5 x that for block Jacobi, the Chebyshev forms and the vectors of the merged
CG forms, 20 x that again (relative) for their sums (test_gpu_dg.py, test_gpu_dg_pcg.py).  At p = 7, 8, 9 (fp64): 1e-9
for the operator, the residual and block Jacobi (test_gpu_dg.py::test_high_degrees); q and the sums of
vmult_with_pcg_sums 5 x 2e-11 and 20 x that, as test_gpu_dg_pcg.py holds them at p = 8; the Chebyshev forms and the
vectors and sums of vmult_with_cg_update have no Dirichlet bound at these degrees and take the same 5 x 2e-11 and 20 x
that, the bounds of the lower degrees.  The right-hand side 2e-11 / 3e-5 (test_gpu_dg_rhs.py); the multigrid
as tests/test_gpu_dg_plain.py and test_gpu_dg_2d.py hold it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_mixed_reference as mx  # noqa: E402
import dg_reference_2d as ref2  # noqa: E402

_lib = mg._lib
TOL = {mg.F64: 2e-11, mg.F32: 3e-5}
NUMBERS = [mg.F64, mg.F32]
NUMBER_IDS = ["f64", "f32"]
KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
JAC = {2: SHEARED_2D, 3: dg.cheby_mesh(5)[1]}
ORIGIN = {2: (-0.9, 0.35), 3: (-0.9, 0.35, 0.2)}

# (cells, Neumann sides 2d+s).  3D: the first two are x (N,D) y (D,N) z (N,N) and x (N,N) y (D,D) z (D,N)
MESHES = {3: [((3, 1, 2), (0, 3, 4, 5)), ((1, 2, 3), (0, 1, 5)), ((2, 3, 1), (1, 2)),
              ((1, 1, 1), (2, 5)), ((1, 1, 1), (1, 2, 3, 4)), ((1, 1, 2), (0, 4)), ((1, 2, 1), (3, 4, 5))],
          2: [((3, 1), (0, 3)), ((1, 3), (0, 1, 3)), ((2, 2), (1, 2)), ((1, 1), (2,)), ((1, 1), (1, 2, 3)), ((1, 1), (0,))]}
LARGE = {3: (2, (5, 3, 2), (1, 2, 5)), 2: (4, (9, 7), (0, 3))}
ALL_PAIRS = {a + b for a in "IDN" for b in "IDN"}


def test_meshes_reach_every_pair_of_face_kinds():
    for dim, meshes in MESHES.items():
        reached = [set() for _ in range(dim)]
        for cells, sides in meshes:
            assert len(sides) < 2 * dim                      # a Dirichlet side is left
            for d, pairs in enumerate(mx.side_kinds(cells, sides)):
                reached[d] |= pairs
        assert all(r == ALL_PAIRS for r in reached), (dim, reached)


@pytest.fixture(scope="module")
def ctx():
    c = mg.Context(0)
    yield c
    c.close()


def rel(a, b):
    return abs(a - b).max() / abs(b).max()


def live():
    return _lib.load().mgx_live_device_allocations()


@functools.lru_cache(maxsize=2)
def base_oracle(dim, p, kind):
    """the all-Dirichlet oracle of one cell whose blocks the boxes of a case share; read only"""
    return dg.DGOracle(p, kind, (1, 1, 1), JAC[3]) if dim == 3 else ref2.DGOracle2D(p, kind, (1, 1), JAC[2])


class Case:
    """restatement and HIP operator on the same box with the same Neumann sides; arrays travel in the oracle's layout"""

    def __init__(self, ctx, p, kind, cells, sides, number, positions=False):
        self.ctx, self.dim, self.number = ctx, len(cells), number
        self.orc = mx.derived_oracle(base_oracle(self.dim, p, kind), cells, sides)
        nb, self.ijk = mg.dg_box_neighbours(cells, "z", neumann_sides=sides)
        assert ((nb == -2).any() == bool(sides)) and (nb >= -2).all()
        self.nb = nb
        self.at = tuple(self.ijk[:, d] for d in reversed(range(self.dim)))
        self.op = mg.DGLaplaceOperator(ctx, p, kind, nb, JAC[self.dim], number, dim=self.dim)
        if positions:
            self.op.set_cell_positions(ORIGIN[self.dim], self.ijk)
        self.vectors = []

    @property
    def ref(self):
        if not hasattr(self, "_ref"):
            self._ref = mx.MixedRhsReference(self.orc, ORIGIN[self.dim])
        return self._ref

    def up(self, x, number=None):
        a = np.ascontiguousarray(np.asarray(x)[self.at]).ravel()
        v = self.ctx.vector(a.size, self.number if number is None else number, data=a)
        self.vectors.append(v)
        return v

    def new(self, fill=np.nan):
        return self.up(np.full(self.orc.shape, fill))

    def down(self, v):
        out = np.empty(self.orc.shape)
        out[self.at] = v.download().astype(float).reshape(len(self.ijk), -1)
        return out

    def close(self):
        for v in self.vectors:
            v.free()
        self.op.clear()


def check_actions(ctx, dim, p, kind, number, meshes, tol_op, tol_pre, tol_jacobi=None):
    """every action of the cell kernel on the boxes of `meshes` against the restatement; prints each figure first.
    tol_op: operator and residual; tol_jacobi (default tol_pre): block Jacobi alone; tol_pre: the Chebyshev forms and the
    vectors of the merged CG forms, 20 x that their sums"""
    tol_jacobi = tol_pre if tol_jacobi is None else tol_jacobi
    rng = np.random.default_rng(1000 * dim + 10 * p + kind)
    worst = {}

    def hold(what, err, tol, where):
        worst[what] = max(worst.get(what, 0.0), err)
        assert err < tol, (what, err, tol, where)

    for cells, sides in meshes:
        case = Case(ctx, p, kind, cells, sides, number)
        o, op, where = case.orc, case.op, (cells, sides)
        x, rhs, xo = (rng.standard_normal(o.shape) for _ in range(3))
        ax = o.vmult(x)
        src, dst = case.up(x), case.new()
        op.vmult(dst, src)
        hold("vmult", rel(case.down(dst), ax), tol_op, where)
        first = dst.download()
        op.vmult(dst, src)
        assert np.array_equal(first, dst.download()), where                  # one writer per entry
        dst = case.new()
        op.vmult_residual(dst, case.up(rhs), src)
        hold("residual", rel(case.down(dst), rhs - ax), tol_op, where)
        dst = case.new()
        op.jacobi_vmult(dst, case.up(rhs))
        hold("jacobi", rel(case.down(dst), o.jacobi_vmult(rhs)), tol_jacobi, where)
        for idx in (0, 1, 2):                                                 # laplace_operator_dg.h:910-955
            sol, old, b = case.up(x), case.up(xo), case.up(rhs)
            op.vmult_with_chebyshev_update(b, idx, 0.6, 0.2, sol, old)
            new_ref, old_ref = o.vmult_with_chebyshev_update(rhs, idx, 0.6, 0.2, x, xo)
            hold("chebyshev %d" % idx, max(rel(case.down(sol), new_ref), rel(case.down(old), old_ref)), tol_pre, where)
        # the merged CG forms: the vectors to tol_pre, the sums to 20 x that relative to the largest
        m = np.tile(op.lumped_mass_inverse(), int(np.prod(cells))).reshape(o.shape)
        r, pv = rng.standard_normal(o.shape), rng.standard_normal(o.shape)
        Q = case.new()
        sums = op.vmult_with_pcg_sums(case.up(r), Q, case.up(pv))
        q_ref = o.vmult(pv)
        want = np.array([(q_ref * pv).sum(), (r * m * r).sum(), (q_ref * m * r).sum(), (q_ref * m * q_ref).sum()])
        hold("pcg q", rel(case.down(Q), q_ref), tol_pre, where)
        hold("pcg sums", abs(sums - want).max() / abs(want).max(), tol_pre * 20, where)
        if dim == 3:
            q0, xv = rng.standard_normal(o.shape), rng.standard_normal(o.shape)
            R, Qv, Pv, X = case.up(r), case.up(q0), case.up(pv), case.up(xv)
            sums = op.vmult_with_cg_update(0.37, 0.81, R, Qv, Pv, X)
            x_ref, p_ref = xv + 0.37 * pv, 0.81 * pv + q0
            q_ref = o.vmult(p_ref)
            want = np.array([(q_ref * p_ref).sum(), (r * r).sum(), (q_ref * r).sum(), (q_ref * q_ref).sum()])
            hold("cg vectors", max(rel(case.down(X), x_ref), rel(case.down(Pv), p_ref), rel(case.down(Qv), q_ref)), tol_pre, where)
            hold("cg sums", abs(sums - want).max() / abs(want).max(), tol_pre * 20, where)
        case.close()
    print("dim %d p=%d kind=%d number=%d:" % (dim, p, kind, number), ", ".join("%s %.2e" % kv for kv in worst.items()))


# ---------------------------------------------------------------------------------------- 1. the actions
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6])
def test_actions_3d(ctx, p, kind, number):
    check_actions(ctx, 3, p, kind, number, MESHES[3], TOL[number], TOL[number] * 5)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [7, 8, 9])
def test_actions_3d_high_degrees(ctx, p, kind):
    check_actions(ctx, 3, p, kind, mg.F64, MESHES[3], 1e-9, TOL[mg.F64] * 5, tol_jacobi=1e-9)


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_actions_2d(ctx, p, kind, number):
    check_actions(ctx, 2, p, kind, number, MESHES[2], TOL[number], TOL[number] * 5)


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("dim", [3, 2])
def test_actions_over_several_workgroups(ctx, dim, number):
    p, cells, sides = LARGE[dim]
    per_group = {3: 128 // (p + 1) ** 2, 2: 256 // (p + 1)}[dim]
    assert np.prod(cells) > per_group and np.prod(cells) % per_group != 0
    check_actions(ctx, dim, p, dg.HERMITE, number, [(cells, sides)], TOL[number], TOL[number] * 5)


# ---------------------------------------------------------------------------------------- 2. all-Neumann boxes, refusals
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("dim", [3, 2])
def test_all_neumann_box_annihilates_the_constants_and_is_refused_by_the_solvers(ctx, dim, number):
    start = live()
    cells = (2, 1, 2) if dim == 3 else (3, 2)
    case = Case(ctx, 2, dg.HERMITE, cells, tuple(range(2 * dim)), number)
    held = live()
    A = case.ref.dense_matrix()
    one = case.ref.interpolate(lambda x: np.ones(x.shape[:-1]))
    dst = case.new()
    case.op.vmult(dst, case.up(one))
    norm = abs(A).sum(axis=1).max()                                  # the operator's maximum norm; |one| is of order 1
    print("all-Neumann box dim %d: |A 1| = %.3e, |A| = %.3e" % (dim, abs(case.down(dst)).max(), norm))
    assert abs(case.down(dst)).max() < TOL[number] * norm * abs(one).max()
    x = np.random.default_rng(3).standard_normal(case.orc.shape)    # ... and it is the restatement's operator
    case.op.vmult(dst, case.up(x))
    assert rel(case.down(dst), case.orc.vmult(x)) < TOL[number]
    for form in (mg.DG_PCG_MERGED, mg.DG_PCG_SEPARATE):
        with pytest.raises(mg.MgxError, match="no Dirichlet face") as e:
            mg.DGConjugateGradient(case.op, form, 5)
        assert e.value.status == -4
    with pytest.raises(mg.MgxError, match="no Dirichlet face") as e:
        mg.DGPlainMultigridSolver(ctx, 2, dg.HERMITE, (2,) + (1,) * (dim - 1), JAC[dim], 2, 3, number,
                                  neumann_sides=tuple(range(2 * dim)))       # (one coarse cell would be refused as an operator)
    assert e.value.status == -4
    assert live() == held
    case.close()
    assert live() == start


@pytest.mark.parametrize("dim", [3, 2])
def test_refused_creates_leave_no_device_memory(ctx, dim):
    start = live()
    # one cell, every face a Neumann face: the cell's block is singular
    nb = np.full((1, 2 * dim), mg.DG_NEUMANN, dtype=np.int32)
    for p in (1, 3):
        with pytest.raises(mg.MgxError, match="transformed cell block is not positive") as e:
            mg.DGLaplaceOperator(ctx, p, dg.HERMITE, nb, JAC[dim], mg.F64, dim=dim)
        assert e.value.status == -4
    # an entry that is none of the three kinds
    bad, _ = mg.dg_box_neighbours((2,) * dim)
    bad[0, 0] = -3
    with pytest.raises(mg.MgxError, match="MGX_DG_BOUNDARY nor MGX_DG_NEUMANN") as e:
        mg.DGLaplaceOperator(ctx, 2, dg.HERMITE, bad, JAC[dim], mg.F64, dim=dim)
    assert e.value.status == -1
    assert live() == start
    if dim == 3:
        # the DG level on the FE_Q hierarchy: refused before the hierarchy is looked at
        nb, _ = mg.dg_box_neighbours((2, 2, 2), neumann_sides=(0,))
        ops = [mg.DGLaplaceOperator(ctx, 2, dg.HERMITE, nb, JAC[3], number) for number in (mg.F32, mg.F64)]
        held = live()
        d = _lib.DGSolverDesc()
        d.matrix_dg, d.matrix_dg_dp, d.cfe, d.degree_pre = ops[0].h, ops[1].h, None, 3
        h = C.c_void_p()
        with pytest.raises(mg.MgxError, match="Neumann faces") as e:
            mg.check(ctx.lib.mgx_dg_solver_create(ctx.h, C.byref(d), C.byref(h)))
        assert e.value.status == -4 and not h.value
        assert live() == held
        for op in ops:
            op.clear()
    assert live() == start


# ---------------------------------------------------------------------------------------- 3. the right-hand side
RHS_CASES = [(p, dg.HERMITE, cells, sides) for cells, sides in (((3, 1, 2), (0, 3, 4, 5)), ((3, 2), (0, 3))) for p in range(1, 10)] + \
            [(p, kind, cells, sides) for cells, sides in (((4, 4, 2), (1, 2, 5)), ((17, 13), (0, 3))) for p in (2, 4) for kind in KINDS]
RHS_IDS = ["p%d-%s-%s" % (p, KIND_IDS[k], "x".join(map(str, c))) for p, k, c, _ in RHS_CASES]
F_SINE = (1.7, (2.1, 3.3, 1.2), (0.3, -0.4, 1.1))
G_SINE = (-0.8, (1.4, 0.9, 2.6), (0.7, 0.2, -0.5))
U_SINE = (0.9, (1.9, 1.3, 2.2), (-0.6, 0.8, 0.1))


def sine(spec, dim):
    amp, wave, phase = spec
    return lambda x: amp * np.prod(np.sin(x * np.array(wave[:dim]) + np.array(phase[:dim])), axis=-1)


def sine_gradient(spec, dim):
    amp, wave, phase = spec
    w, ph = np.array(wave[:dim]), np.array(phase[:dim])

    def grad(x):
        s, c = np.sin(x * w + ph), np.cos(x * w + ph)
        return np.stack([amp * w[k] * c[..., k] * np.prod(np.delete(s, k, axis=-1), axis=-1) for k in range(dim)], axis=-1)
    return grad


def smooth_gradient(x):
    """a field that is no gradient of a sine product, for the sampled kind"""
    return np.stack([np.exp(0.2 * x[..., 0]) + x[..., -1], np.cos(x[..., 0] - x[..., 1]), 0.3 * x[..., 0] * x[..., -1]][:x.shape[-1]],
                    axis=-1)


def fn_sine(spec, dim):
    return mg.DGFunction.sine_product(spec[0], spec[1][:dim], spec[2][:dim])


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("p,kind,cells,sides", RHS_CASES, ids=RHS_IDS)
def test_compute_rhs_mixed(ctx, p, kind, cells, sides, number):
    """the Neumann term alone and with f and g, sampled and as the normal derivative of a potential; compute_rhs on the
    same operator is compute_rhs_mixed with h = NULL, bit for bit; the same bits in two calls"""
    case = Case(ctx, p, kind, cells, sides, number, positions=True)
    r, dim, tol = case.ref, case.dim, TOL[number]
    f, g = sine(F_SINE, dim), sine(G_SINE, dim)
    base = r.load_vector(f) + r.boundary_load(g)
    flux = {"potential": r.neumann_load(sine_gradient(U_SINE, dim)), "sampled": r.neumann_load(smooth_gradient)}
    fn_h = {"potential": fn_sine(U_SINE, dim),
            "sampled": mg.DGFunction.sampled(None, case.up(r.sample_flux(smooth_gradient), mg.F64))}
    fn_f, fn_g = fn_sine(F_SINE, dim), fn_sine(G_SINE, dim)
    for how in ("potential", "sampled"):
        for with_fg in (False, True):
            ref = flux[how] + (base if with_fg else 0)
            got = []
            for _ in range(2):
                dst = case.new()                                              # an unwritten entry shows
                case.op.compute_rhs(dst, fn_f if with_fg else None, fn_g if with_fg else None, fn_h[how])
                got.append(dst.download())
            err = rel(case.down(dst), ref)
            print("mixed rhs p=%d kind=%d %s %s fg=%d: %.3e" % (p, kind, cells, how, with_fg, err))
            assert err < tol, (how, with_fg)
            assert np.array_equal(got[0], got[1]), (how, with_fg)
    # without h: the Neumann faces are Neumann faces with zero flux, not Dirichlet faces
    dst, again = case.new(), case.new()
    case.op.compute_rhs(dst, fn_f, fn_g)
    assert rel(case.down(dst), base) < tol
    mg.check(ctx.lib.mgx_dg_compute_rhs_mixed(case.op.h, C.byref(fn_f.desc), C.byref(fn_g.desc), None, again.ptr))
    assert np.array_equal(dst.download(), again.download())
    # a sampled h without face values is refused, and so is a potential of another dimension
    with pytest.raises(mg.MgxError, match="Neumann faces") as e:
        case.op.compute_rhs(dst, None, None, mg.DGFunction.sampled(None, None))
    assert e.value.status == -1
    with pytest.raises(mg.MgxError, match="dimensions"):
        case.op.compute_rhs(dst, None, None, fn_sine(U_SINE, 5 - dim))
    case.close()


@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("p,kind,cells,sides", RHS_CASES, ids=RHS_IDS)
def test_operator_identity_on_the_device(ctx, p, kind, cells, sides, number):
    """A interpolate(u) = compute_rhs_mixed(f = -Laplace u, g = u, h = d_n u) for a polynomial of total degree p: both
    sides from the device.  5 x the operator tolerance, as tests/test_gpu_dg_rhs.py holds its identity."""
    case = Case(ctx, p, kind, cells, sides, number)
    r, dim = case.ref, case.dim
    a = np.array([0.15, -0.1, 0.2][:dim])
    u = lambda x: (0.6 + x @ a) ** p                                               # noqa: E731
    f = lambda x: -p * (p - 1) * (a @ a) * (0.6 + x @ a) ** max(p - 2, 0)          # noqa: E731
    grad = lambda x: (p * (0.6 + x @ a) ** (p - 1))[..., None] * a                  # noqa: E731
    lhs, rhs = case.new(), case.new()
    case.op.vmult(lhs, case.up(r.interpolate(u)))
    case.op.compute_rhs(rhs, mg.DGFunction.sampled(case.up(r.sample_cells(f), mg.F64)),
                        mg.DGFunction.sampled(None, case.up(r.sample_faces(u), mg.F64)),
                        mg.DGFunction.sampled(None, case.up(r.sample_flux(grad), mg.F64)))
    got, want = case.down(lhs), case.down(rhs)
    err = abs(got - want).max() / abs(want).max()
    print("identity p=%d kind=%d %s: %.3e" % (p, kind, cells, err))
    assert err < 5 * TOL[number]
    case.close()


# ---------------------------------------------------------------------------------------- 4. the plain multigrid
#              dim, p, coarse cells, levels, Neumann sides
PLAIN_CASES = [(2, 3, (1, 1), 4, (0, 3)), (3, 2, (1, 1, 1), 3, (1, 2, 4))]
PLAIN_IDS = ["2d-p3-L4", "3d-p2-L3"]


def plain_jacobian(dim):
    return SHEARED_2D if dim == 2 else dg.cheby_mesh(0)[1]


@functools.lru_cache(maxsize=None)
def plain_reference(case):
    dim, p, cells, levels, sides = case
    cls = mx.MixedPlainOracle2D if dim == 2 else mx.MixedPlainOracle
    o = cls(p, dg.HERMITE, cells, plain_jacobian(dim), levels, sides)
    shape = o.level[-1].shape
    rng = np.random.default_rng(7)
    x, rhs = rng.standard_normal(shape), rng.standard_normal(shape)
    return dict(o=o, shape=shape, x=x, rhs=rhs, vcycle=o.v_cycle(x), cg=o.solve_cg(rhs, 1e-9))


def plain_arrays(S, R, dim):
    ijk = S.cell_ijk[-1]
    at = tuple(ijk[:, d] for d in reversed(range(dim)))

    def down(v):
        out = np.empty(R["shape"])
        out[at] = np.asarray(v, dtype=float).reshape(len(ijk), -1)
        return out
    return (lambda a: np.ascontiguousarray(a[at]).ravel()), down


@pytest.mark.parametrize("case", PLAIN_CASES, ids=PLAIN_IDS)
def test_plain_multigrid_with_neumann_sides_fp64(ctx, case):
    dim, p, cells, levels, sides = case
    R = plain_reference(case)
    o = R["o"]
    S = mg.DGPlainMultigridSolver(ctx, p, dg.HERMITE, cells, plain_jacobian(dim), levels, 3, mg.F64, neumann_sides=sides)
    up, down = plain_arrays(S, R, dim)
    for l in range(levels):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert info["cg_its"] == want["cg_its"] and info["degree"] == want["degree"]
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-8)
        assert info["theta"] == pytest.approx(want["theta"], rel=1e-8)
    src, dst = ctx.vector(S.m(), data=up(R["x"])), ctx.vector(S.m())
    S.vmult(dst, src)
    assert rel(down(dst.download()), R["vcycle"]) < 1e-8
    b, sol = ctx.vector(S.m(), data=up(R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert its == oits and red == pytest.approx(ored, rel=1e-5)
    assert rel(down(sol.download()), xo) < 1e-7
    S.close()


@pytest.mark.parametrize("case", PLAIN_CASES, ids=PLAIN_IDS)
def test_plain_multigrid_with_neumann_sides_fp32_v_cycle(ctx, case):
    dim, p, cells, levels, sides = case
    R = plain_reference(case)
    o = R["o"]
    S = mg.DGPlainMultigridSolver(ctx, p, dg.HERMITE, cells, plain_jacobian(dim), levels, 3, mg.F32, neumann_sides=sides)
    up, down = plain_arrays(S, R, dim)
    for l in range(levels):
        info, want = S.smoother_info(l), o.info[l]
        print("level", l, info, want)
        assert all(np.isfinite(v) for v in info.values())
        assert info["lambda_max"] == pytest.approx(want["lambda_max"], rel=1e-4)
        if l == 0:
            assert abs(info["degree"] - want["degree"]) <= 1
        else:
            assert info["degree"] == want["degree"]
    src, dst = ctx.vector(S.m(), data=up(R["x"])), ctx.vector(S.m())
    S.vmult(dst, src)
    assert rel(down(dst.download()), R["vcycle"]) < 5e-4
    b, sol = ctx.vector(S.m(), data=up(R["rhs"])), ctx.vector(S.m())
    its, red = S.solve_cg(b, sol, 1e-9)
    xo, oits, ored = R["cg"]
    print("iterations", its, oits, "reduction", red, ored)
    assert abs(its - oits) <= 1 and red == pytest.approx(ored, rel=0.05)
    assert rel(down(sol.download()), xo) < 1e-6
    S.close()


def test_convergence_with_two_neumann_sides_through_the_plain_solver_2d(ctx):
    """prod sin(3 pi x_d) on [-0.9, 1]^2 from one coarse cell, Hermite-like basis, p = 3, lower-x and upper-y sides Neumann
    with the exact flux (the potential form of h), fp64 V-cycle, 4^2, 8^2 and 16^2 cells, CG to 1e-12; right-hand side
    and error from the device.  The errors are those of the dense numpy solves (tests/test_dg_mixed_reference.py) to
    1e-3, as tests/test_gpu_dg_rhs.py holds the Dirichlet ones."""
    k, err = 3 * math.pi, []
    u = mg.DGFunction.sine_product(1.0, (k, k), (0.0, 0.0))
    f = mg.DGFunction.sine_product(2 * k * k, (k, k), (0.0, 0.0))
    for n_levels in (3, 4, 5):
        S = mg.DGPlainMultigridSolver(ctx, 3, mg.DG_HERMITE, (1, 1), np.eye(2) * 1.9, n_levels, 3, mg.F64, origin=(-0.9, -0.9),
                                      neumann_sides=mx.DENSE_NEUMANN_SIDES_2D)
        b, x = S.initialize_dof_vector(), S.initialize_dof_vector()
        A = S.matrix_dg_dp
        A.compute_rhs(b, f, u, u)
        its, _ = S.solve_cg(b, x, 1e-12)
        s = A.compute_l2_error(x, u)
        e = math.sqrt(s[0] / s[1])
        print("2D p=3 %d^2 cells, sides 0 and 3 Neumann: L2 error %.6e (dense %.6e), %d iterations"
              % (2 ** (n_levels - 1), e, mx.DENSE_ERRORS_MIXED_2D_P3[n_levels - 3], its))
        err.append(e)
        b.free(); x.free()
        S.close()
    assert np.allclose(err, mx.DENSE_ERRORS_MIXED_2D_P3, rtol=1e-3, atol=0)
    assert err[0] / err[1] >= 8 and err[1] / err[2] >= 8


# ---------------------------------------------------------------------------------------- 5. decomposed
def test_decomposed_operator_with_a_neumann_side_cut_by_the_partition():
    """2 ranks over gloo sharing the GPU (2 x 1 x 1 blocks of the 4 x 4 x 2 harness mesh), Hermite-like basis, p = 3, fp64:
    the lower-y and upper-z sides are Neumann sides on both ranks, the lower-x side on rank 0 only; every action against
    the single-domain restatement, in fresh child processes (tests/dg_mixed_dist_worker.py)"""
    from test_decomposition import launch
    outs = launch(None, 2, None, None, extra=("3", "0", "5", "f64", "0,2,5"), worker="dg_mixed_dist_worker.py")
    assert all("dg mixed ok" in o for o in outs), outs
