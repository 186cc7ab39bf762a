"""DG right-hand side with Dirichlet boundary data and the L2 error sums on the GPU (include/mgx_dg.h:
mgx_dg_operator_set_cell_positions, mgx_dg_compute_rhs, mgx_dg_compute_l2_error) in three and two dimensions, against
the numpy restatement tests/dg_rhs_reference.py, which tests/test_dg_rhs_reference.py pins on the CPU.

Boxes, as the other DG tests justify them.  3D: (3,1,2) is one partly filled workgroup at every degree; (4,4,2) is
several workgroups with a partly filled last one at p = 2 and p = 4 (28 and 10 cells per workgroup here); both with the
Jacobian of cheby_mesh(5).  2D: (1,1), (5,3) and (17,13) with the sheared Jacobian of tests/test_gpu_dg_pcg.py (one
cell; one partly filled workgroup; several workgroups with a partly filled last one).  Cells in z-order.  Every cell
position of a box with an odd number of cells has its own combination of Dirichlet faces next to cells with none.

Tolerances are those of tests/test_gpu_dg.py, 2e-11 (fp64) and 3e-5 (fp32), in the measure every DG test here uses:
the largest difference over the largest entry of the reference."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_reference_2d as ref2  # noqa: E402
import dg_rhs_reference as rr  # noqa: E402

_lib = mg._lib
TOL = {mg.F64: 2e-11, mg.F32: 3e-5}
NUMBERS = [mg.F64, mg.F32]
NUMBER_IDS = ["f64", "f32"]
KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
JAC = {2: SHEARED_2D, 3: dg.cheby_mesh(5)[1]}
ORIGIN = {2: (-0.9, 0.35), 3: (-0.9, 0.35, 0.2)}
# every degree with the Hermite-like basis on the smallest box of each dimension, all bases at p = 2 and 4 on the others
CASES = [(p, dg.HERMITE, cells) for cells in ((3, 1, 2), (1, 1)) for p in range(1, 10)] + \
        [(p, kind, cells) for cells in ((4, 4, 2), (5, 3), (17, 13)) for p in (2, 4) for kind in KINDS]
CASE_IDS = ["p%d-%s-%s" % (p, ["hermite", "gl", "gauss"][k], "x".join(map(str, c))) for p, k, c in CASES]

# a sine product with unequal wave and phase per direction, and functions that are no product, for the sampled kind
F_SINE = (1.7, (2.1, 3.3, 1.2), (0.3, -0.4, 1.1))
G_SINE = (-0.8, (1.4, 0.9, 2.6), (0.7, 0.2, -0.5))


def sine(spec, dim):
    amp, wave, phase = spec
    return lambda x: amp * np.prod(np.sin(x * np.array(wave[:dim]) + np.array(phase[:dim])), axis=-1)


def f_smooth(x):
    return np.exp(0.3 * x.sum(axis=-1)) + np.cos(x[..., 0] * x[..., 1])


def g_smooth(x):
    return 1.0 / (2.0 + np.sin(x[..., 0] - 0.5 * x[..., -1])) - 0.2 * x[..., 0]


def polynomial(dim, p):
    """u = (0.6 + a.x)^p, total degree p, and -Laplace u"""
    a = np.array([0.15, -0.1, 0.2][:dim])
    return (lambda x: (0.6 + x @ a) ** p), (lambda x: -p * (p - 1) * (a @ a) * (0.6 + x @ a) ** max(p - 2, 0))


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
def reference(p, kind, cells):
    """oracle and restatement of a box, built once for the cases that follow one another on it; read only"""
    dim = len(cells)
    o = ref2.DGOracle2D(p, kind, cells, JAC[dim]) if dim == 2 else dg.DGOracle(p, kind, cells, JAC[dim])
    return rr.RhsReference(o, ORIGIN[dim])


class Case:
    """restatement and HIP operator on the same box of cells; arrays travel in the oracle's layout"""

    def __init__(self, ctx, p, kind, cells, number, positions=True):
        self.ctx, self.dim, self.number = ctx, len(cells), number
        self.ref = reference(p, kind, tuple(cells))
        nb, self.ijk = mg.dg_box_neighbours(cells, "z")
        self.at = tuple(self.ijk[:, d] for d in reversed(range(self.dim)))
        self.op = mg.DGLaplaceOperator(ctx, p, kind, nb, JAC[self.dim], number, dim=self.dim)
        if positions:
            self.op.set_cell_positions(ORIGIN[self.dim], self.ijk)
        self.vectors = []

    def up(self, x, number=None):
        """an array over the cells (any trailing shape) as a device vector in the operator's cell order"""
        a = np.ascontiguousarray(x[self.at]).ravel()
        v = self.ctx.vector(a.size, self.number if number is None else number, data=a)
        self.vectors.append(v)
        return v

    def nan_vector(self):
        return self.up(np.full(self.ref.o.shape, np.nan))

    def down(self, v):
        out = np.empty(self.ref.o.shape)
        out[self.at] = v.download().astype(float).reshape(len(self.ijk), -1)
        return out

    def sine(self, spec):
        return mg.DGFunction.sine_product(spec[0], spec[1][:self.dim], spec[2][:self.dim])

    def sampled(self, fn, cells=True, faces=True):
        return mg.DGFunction.sampled(self.up(self.ref.sample_cells(fn), mg.F64) if cells else None,
                                     self.up(self.ref.sample_faces(fn), mg.F64) if faces else None)

    def close(self):
        for v in self.vectors:
            v.free()
        self.op.clear()


# ---------------------------------------------------------------------------------------- compute_rhs
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("p,kind,cells", CASES, ids=CASE_IDS)
def test_compute_rhs(ctx, p, kind, cells, number):
    """f alone, g alone and both, as a sine product and sampled, against the restatement; the same bits in two calls;
    g = None is the host formula of the harnesses, (f w) S"""
    case = Case(ctx, p, kind, cells, number)
    r, dim, tol = case.ref, case.dim, TOL[number]
    fs, gs = sine(F_SINE, dim), sine(G_SINE, dim)
    load = {"sine": r.load_vector(fs), "sampled": r.load_vector(f_smooth)}
    bnd = {"sine": r.boundary_load(gs), "sampled": r.boundary_load(g_smooth)}
    fn_f = {"sine": case.sine(F_SINE), "sampled": case.sampled(f_smooth, faces=False)}
    fn_g = {"sine": case.sine(G_SINE), "sampled": case.sampled(g_smooth, cells=False)}
    scale = abs(load["sine"] + bnd["sine"]).max()
    for how in ("sine", "sampled"):
        for with_f, with_g in ((True, False), (False, True), (True, True)):
            ref = (load[how] if with_f else 0) + (bnd[how] if with_g else 0)
            got = []
            for _ in range(2):
                dst = case.nan_vector()                                       # an unwritten entry shows
                case.op.compute_rhs(dst, fn_f[how] if with_f else None, fn_g[how] if with_g else None)
                got.append(dst.download())
            err = rel(case.down(dst), ref)
            print("rhs p=%d kind=%d %s %s f=%d g=%d: %.3e" % (p, kind, cells, how, with_f, with_g, err))
            assert err < tol, (how, with_f, with_g)
            assert np.array_equal(got[0], got[1]), (how, with_f, with_g)
    # mixed kinds in one call
    dst = case.nan_vector()
    case.op.compute_rhs(dst, fn_f["sampled"], fn_g["sine"])
    assert rel(case.down(dst), load["sampled"] + bnd["sine"]) < tol
    # g = None: the vector the harnesses form on the host today
    S, xq, wq = case.op.basis_1d()
    Sd, wd = rr.kron_all([S] * dim), rr.kron_all([wq] * dim) * abs(np.linalg.det(JAC[dim]))
    host = (r.sample_cells(fs) * wd) @ Sd
    dst = case.nan_vector()
    case.op.compute_rhs(dst, fn_f["sine"])
    assert rel(case.down(dst), host) < tol
    # neither: zeros
    case.op.compute_rhs(dst)
    assert not dst.download().any() and scale > 0
    case.close()


# ---------------------------------------------------------------------------------------- the identity on the device
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("p,kind,cells", CASES, ids=CASE_IDS)
def test_operator_identity(ctx, p, kind, cells, number):
    """A interpolate(u) = compute_rhs(f = -Laplace u, g = u) for a polynomial of total degree p: mgx_dg_vmult against
    the new entry point, both sides from the device and nothing from the restatement (coordinates, samples and the
    interpolation are formed here from the operator's own 1D data).  5 x the operator tolerance, the factor
    tests/test_gpu_dg_pcg.py gives q."""
    dim, J, n = len(cells), JAC[len(cells)], p + 1
    nb, ijk = mg.dg_box_neighbours(cells, "z")
    op = mg.DGLaplaceOperator(ctx, p, kind, nb, J, number, dim=dim)
    S, xq, wq = op.basis_1d()
    u, f = polynomial(dim, p)
    grid = lambda k: np.stack(np.meshgrid(*([xq] * k), indexing="ij"), -1)[..., ::-1].reshape(-1, k)   # noqa: E731
    x = np.array(ORIGIN[dim]) + (ijk[:, None, :] + grid(dim)[None]) @ J.T                      # [cell, q, dim]
    faces = np.empty((len(ijk), 2 * dim, n ** (dim - 1)))
    for d in range(dim):
        for s in (0, 1):
            ref = np.insert(grid(dim - 1), d, float(s), axis=1)
            faces[:, 2 * d + s] = u(np.array(ORIGIN[dim]) + (ijk[:, None, :] + ref[None]) @ J.T)
    P = np.linalg.solve(S.T @ (wq[:, None] * S), S.T * wq)                                   # Gauss values -> coefficients
    Pd = P
    for _ in range(dim - 1):
        Pd = np.kron(P, Pd)
    src = op.initialize_dof_vector((u(x) @ Pd.T).ravel())
    lhs, rhs = op.initialize_dof_vector(), op.initialize_dof_vector()
    fv, uf = ctx.vector(x[..., 0].size, mg.F64, data=f(x).ravel()), ctx.vector(faces.size, mg.F64, data=faces.ravel())
    op.vmult(lhs, src)
    op.compute_rhs(rhs, mg.DGFunction.sampled(fv), mg.DGFunction.sampled(None, uf))
    a, b = lhs.download().astype(float), rhs.download().astype(float)
    err = rel(a, b)
    print("identity p=%d kind=%d %s: %.3e" % (p, kind, cells, err))
    for v in (src, lhs, rhs, fv, uf):
        v.free()
    op.clear()
    assert err < 5 * TOL[number]


# ---------------------------------------------------------------------------------------- compute_l2_error
@pytest.mark.parametrize("number", NUMBERS, ids=NUMBER_IDS)
@pytest.mark.parametrize("p,kind,cells", CASES, ids=CASE_IDS)
def test_compute_l2_error(ctx, p, kind, cells, number):
    case = Case(ctx, p, kind, cells, number)
    r, dim, tol = case.ref, case.dim, TOL[number]
    volume = abs(np.linalg.det(JAC[dim])) * np.prod(cells)
    # a seeded random vector: nothing cancels in the sum of squares
    x = np.random.default_rng(3 + p).standard_normal(r.o.shape)
    X = case.up(x)
    x_dev = case.down(X)                                                      # what the device holds (fp32: rounded)
    for name, fn, call in (("sine", case.sine(G_SINE), sine(G_SINE, dim)), ("sampled", case.sampled(g_smooth, faces=False), g_smooth)):
        got = [case.op.compute_l2_error(X, fn) for _ in range(2)]
        ref = r.l2_sums(x_dev, call)
        print("l2 p=%d kind=%d %s %s: %.3e %.3e" % (p, kind, cells, name, abs(got[0][0] / ref[0] - 1), abs(got[0][1] / ref[1] - 1)))
        assert abs(got[0][0] - ref[0]) < tol * ref[0], name
        assert abs(got[0][1] - volume) < 1e-13 * volume, name
        assert np.array_equal(got[0], got[1]), name                           # same bits
    # an interpolated polynomial against itself
    u, _ = polynomial(dim, p)
    s = case.op.compute_l2_error(case.up(r.interpolate(u)), case.sampled(u, faces=False))
    print("l2 of an interpolant p=%d kind=%d %s: %.3e" % (p, kind, cells, s[0] / s[1]))
    if number == mg.F64:
        assert s[0] <= 1e-24 * s[1]
    else:
        assert s[0] <= (TOL[number] * abs(r.sample_cells(u)).max()) ** 2 * s[1]
    assert abs(s[1] - volume) < 1e-13 * volume
    case.close()


# ---------------------------------------------------------------------------------------- error paths
@pytest.mark.parametrize("cells", [(3, 1, 2), (5, 3)], ids=["3d", "2d"])
def test_error_paths_and_allocations(ctx, cells):
    before = live()
    case = Case(ctx, 2, dg.HERMITE, cells, mg.F64, positions=False)
    dim, dst = case.dim, case.nan_vector()
    INVALID = -1  # MGX_ERR_INVALID_ARGUMENT
    sampled_f = case.sampled(f_smooth, faces=False)

    def refused(call, word):
        with pytest.raises(_lib.MgxError) as e:
            call()
        assert e.value.status == INVALID and word in str(e.value), str(e.value)

    # a sine product without positions (a sampled function needs none)
    refused(lambda: case.op.compute_rhs(dst, case.sine(F_SINE)), "set_cell_positions")
    refused(lambda: case.op.compute_l2_error(dst, case.sine(F_SINE)), "set_cell_positions")
    case.op.compute_rhs(dst, sampled_f)
    assert np.isfinite(dst.download()).all()
    case.op.set_cell_positions(ORIGIN[dim], case.ijk)
    # a sine product of the other dimension
    other = mg.DGFunction.sine_product(1.0, F_SINE[1][:5 - dim], F_SINE[2][:5 - dim])
    refused(lambda: case.op.compute_rhs(dst, other), "dim")
    refused(lambda: case.op.compute_rhs(dst, None, other), "dim")
    refused(lambda: case.op.compute_l2_error(dst, other), "dim")
    # no destination, no vector, no function
    refused(lambda: case.op.compute_rhs(None, case.sine(F_SINE)), "dst")
    refused(lambda: case.op.compute_l2_error(dst, None), "null")
    # a sampled g without face values while the box has Dirichlet faces; an unknown kind
    refused(lambda: case.op.compute_rhs(dst, None, sampled_f), "face_values")
    refused(lambda: case.op.compute_rhs(dst, mg.DGFunction.sampled(None)), "cell_values")
    bad = case.sine(F_SINE)
    bad.desc.kind = 7
    refused(lambda: case.op.compute_rhs(dst, bad), "kind")
    # positions may be set again; the calls that are valid work after the refusals
    case.op.set_cell_positions(ORIGIN[dim], case.ijk)
    case.op.compute_rhs(dst, case.sine(F_SINE), case.sine(G_SINE))
    s = case.op.compute_l2_error(dst, case.sine(G_SINE))
    assert np.isfinite(dst.download()).all() and np.isfinite(s).all()
    case.close()
    assert live() == before


# ---------------------------------------------------------------------------------------- through the solver
def solve_with_boundary_data(ctx, dim, p, n_levels, vnumber, tolerance):
    """prod sin(3 pi x_d) on [-0.9, 1]^dim from one coarse cell: right-hand side and error from the new entry points"""
    S = mg.DGPlainMultigridSolver(ctx, p, mg.DG_HERMITE, (1,) * dim, np.eye(dim) * 1.9, n_levels, 3, vnumber, origin=(-0.9,) * dim)
    k = 3 * math.pi
    u = mg.DGFunction.sine_product(1.0, (k,) * dim, (0.0,) * dim)
    f = mg.DGFunction.sine_product(dim * k * k, (k,) * dim, (0.0,) * dim)
    b, x = S.initialize_dof_vector(), S.initialize_dof_vector()
    A = S.matrix_dg_dp
    A.compute_rhs(b, f, u)
    its, _ = S.solve_cg(b, x, tolerance)
    s = A.compute_l2_error(x, u)
    A.compute_rhs(b, f)                                                       # the reference's vector: the plateau
    S.solve_cg(b, x, tolerance)
    s0 = A.compute_l2_error(x, u)
    b.free(); x.free()
    S.close()
    assert abs(s[1] - 1.9 ** dim) < 1e-12 * 1.9 ** dim
    return math.sqrt(s[0] / s[1]), math.sqrt(s0[0] / s0[1]), its


def test_convergence_through_the_plain_solver_2d(ctx):
    """p = 3, fp64 V-cycle, 4^2, 8^2 and 16^2 cells, CG to 1e-12.  The errors must be those of the dense numpy solves
    (tests/test_dg_rhs_reference.py) to 1e-3: a residual reduction of 1e-12 times a condition number of order 1e4 leaves
    the solution error far below the discretisation error of 2.5e-4.  Ratios >= 8 = 2^p; with the volume term alone
    the ratio is 1.0 (the plateau 0.1383 / 0.1364 / 0.1365)."""
    err, plateau = [], []
    for n_levels in (3, 4, 5):
        e, e0, its = solve_with_boundary_data(ctx, 2, 3, n_levels, mg.F64, 1e-12)
        print("2D p=3 %d^2 cells: L2 error %.6e (dense %.6e, distance %.2e), volume term only %.4f, %d iterations"
              % (2 ** (n_levels - 1), e, rr.DENSE_ERRORS_2D_P3[n_levels - 3], abs(e / rr.DENSE_ERRORS_2D_P3[n_levels - 3] - 1), e0, its))
        err.append(e)
        plateau.append(e0)
    assert np.allclose(err, rr.DENSE_ERRORS_2D_P3, rtol=1e-3, atol=0)
    assert err[0] / err[1] >= 8 and err[1] / err[2] >= 8
    assert np.allclose(plateau, [0.1383, 0.1364, 0.1365], rtol=0, atol=6e-5)


def test_convergence_through_the_plain_solver_3d(ctx):
    """one 3D row: p = 3 on 4^3 and 8^3 cells, ratio >= 8 = 2^p.  The restatement alone meets it on this pair (CG on the
    oracle's operator on the CPU: 2.018914e-02 and 2.345467e-03, ratio 8.61; volume term only 0.1031 and 0.1008), so the
    pair 8^3 / 16^3 is not needed."""
    e4, p4, _ = solve_with_boundary_data(ctx, 3, 3, 3, mg.F64, 1e-12)
    e8, p8, _ = solve_with_boundary_data(ctx, 3, 3, 4, mg.F64, 1e-12)
    print("3D p=3: 4^3 %.6e, 8^3 %.6e, ratio %.2f; volume term only %.4f %.4f" % (e4, e8, e4 / e8, p4, p8))
    assert e4 / e8 >= 8
