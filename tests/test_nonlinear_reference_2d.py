"""The numpy restatement of the solution-dependent coefficient on quadrilaterals (tests/nonlinear_reference_2d.py) and the
host side of the 2D provider (geometry accessors of include/mgx_square.h) pinned on the CPU: the unit law is the
Laplace operator of tests/feq_reference_2d.py, the affine and the per-point laws agree on a sheared box, the
minimal-surface tensor is the derivative of the residual, the isoparametric annulus sector converges to its area at the
rate of its degree, the provider's tables are those the reference computes from the cell nodes, Newton's method with
exact linear solves converges.

NEWTON_CASES_2D records, per case, the number of Newton steps to 1e-6 of the first residual norm with dense exact
solves (no step halved); test_gpu_nonlinear_2d.py uses them as its yardstick."""
import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
import feq_reference_2d as fr  # noqa: E402
import nonlinear_reference_2d as nr2  # noqa: E402
from test_gpu_feq_2d import SHEAR  # noqa: E402

# (geometry, degree, n_refine of one coarse cell, amplitude) -> N6
NEWTON_CASES_2D = {("square", 2, 2, 0.25): 3, ("square", 2, 2, 1.0): 4, ("sector", 3, 1, 1.0): 5, ("sector", 3, 2, 0.25): 4}


def make_square(geometry, p, n_refine=None, box=None):
    """square: [-0.9, 1]^2 (box: cells of size 1.9 / box[0]); sheared: the same under SHEAR; sector: the annulus sector"""
    kw = dict(n_refine=n_refine) if box is None else dict(box=box[:2], n_refine=box[2], h0=1.9 / box[0])
    if geometry == "sector":
        return mg.Square(p, mapped="annulus_sector", **kw)
    return mg.Square(p, jacobian=SHEAR if geometry == "sheared" else None, **kw)


def reference(sq, l, affine):
    return nr2.NonlinearReference2D(sq.degree, sq.shape_values(), sq.colloc_grad(), sq.qweights(), sq.idx9(l), sq.idx9_plain(l),
                                    sq.n_dofs(l), sq.cell_nodes(l), affine)


def boundary_state(sq, l, amplitude):
    """zero in the interior, A sin(2 pi (x + y)) on the Dirichlet DoFs (minimal_surface/program.cc:97-99)"""
    u = np.zeros(sq.n_dofs(l))
    c = sq.constrained(l)
    x = sq.dof_coordinates(l)[c]
    u[c] = amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1]))
    return u


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("geometry", ["square", "sheared", "sector"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_unit_law_is_the_laplace_operator(p, geometry):
    sq = make_square(geometry, p, box=(3, 2, 1))
    e = fr.arrays_1d(sq)
    n = p + 1
    for l in range(sq.n_levels):
        ref = reference(sq, l, affine=geometry != "sector")
        coef = ref.coefficient(nr2.LAW_UNIT, None)
        cc, grid = sq.cell_coords(l), sq.dof_grid(l)
        Nx, Ny = sq.cells_per_dim2(l)
        T = np.empty((Ny, Nx, 3, n, n))
        T[cc[:, 1], cc[:, 0]] = coef.reshape(-1, 3, n, n)
        level = fr.Level(e, (Nx, Ny), coef_q=T)
        x = sq.seeded_vector(l, 3)
        X = np.empty(level.shape).ravel()
        X[grid] = x
        want = level.vmult(X).ravel()[grid]
        assert rel(ref.apply(coef, x), want) < 1e-13
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_affine_and_per_point_laws_agree_on_a_sheared_box(p):
    sq = make_square("sheared", p, box=(3, 2, 1))
    l = sq.max_level
    a, q = reference(sq, l, True), reference(sq, l, False)
    x = sq.dof_coordinates(l)
    u = 0.6 * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])) * np.cos(1.3 * x[:, 1]) + 0.2 * x[:, 0] ** 2 + 0.1 * sq.seeded_vector(l, 11)
    for law in (nr2.LAW_UNIT, nr2.LAW_MINIMAL_SURFACE):
        assert rel(q.coefficient(law, u), a.coefficient(law, u)) < 1e-13
        assert rel(q.residual(law, u), a.residual(law, u)) < 1e-13
    sq.close()


@pytest.mark.parametrize("geometry,p,n_refine", [("square", 2, 2), ("sheared", 3, 1), ("sector", 2, 2), ("sector", 3, 1)])
def test_tensor_is_the_derivative_of_the_residual(geometry, p, n_refine):
    """[R(u - eps d) - R(u + eps d)] / (2 eps) = A(u) d: truncation eps^2 = 1e-10, rounding 1e-16 / eps = 1e-11"""
    sq = make_square(geometry, p, n_refine)
    l = sq.max_level
    ref = reference(sq, l, affine=geometry != "sector")
    rng = np.random.default_rng(7)
    u = rng.uniform(-1, 1, sq.n_dofs(l))  # boundary values included
    d = np.zeros(sq.n_dofs(l))
    d[ref.free] = rng.uniform(-1, 1, ref.free.size)
    eps = 1e-5
    fd = (ref.residual(nr2.LAW_MINIMAL_SURFACE, u - eps * d) - ref.residual(nr2.LAW_MINIMAL_SURFACE, u + eps * d)) / (2 * eps)
    ad = ref.apply(ref.coefficient(nr2.LAW_MINIMAL_SURFACE, u), d)
    ad[ref.constrained] = 0.0
    diff = np.abs(fd - ad).max() / np.abs(ad).max()
    print("%s p=%d: central difference against A(u) d: %.3e" % (geometry, p, diff))
    assert diff < 1e-6
    sq.close()


@pytest.mark.parametrize("p", [2, 3, 4])
def test_annulus_sector_area_converges_at_the_rate_of_the_degree(p):
    """sum of JxW_q against the area 3 pi / 16 of the quarter annulus 0.5 <= r <= 1: per refinement the error of the
    isoparametric degree p falls by 2^(2p) (asserted: at least 0.8 of it between 2^2 and 4^2 cells)"""
    sq = make_square("sector", p, 2)
    err = []
    for l in (1, 2):
        ref = reference(sq, l, affine=False)
        err.append(abs(ref.w.sum() - 3 * np.pi / 16))
        assert abs(sq.jxw_q(l).sum() - ref.w.sum()) < 1e-13
    print("p=%d: area error %.3e (2^2 cells), %.3e (4^2 cells), ratio %.1f" % (p, err[0], err[1], err[0] / err[1]))
    assert err[0] / err[1] >= 0.8 * 2 ** (2 * p)
    sq.close()


@pytest.mark.parametrize("geometry", ["square", "sheared", "sector"])
@pytest.mark.parametrize("p", [1, 2, 3, 5])
def test_provider_geometry(p, geometry):
    """unit_q, jxw_q, affine_metric, unit_law_coefficient and dof_coordinates of the provider against the geometry the
    reference computes from the cell nodes"""
    sq = make_square(geometry, p, box=(3, 2, 1))
    for l in range(sq.n_levels):
        q = reference(sq, l, affine=False)
        assert rel(sq.unit_q(l), q.U) < 1e-13
        assert rel(sq.jxw_q(l), q.w) < 1e-13
        assert rel(sq.unit_law_coefficient(l), q.U) < 1e-13
        if geometry != "sector":
            a = reference(sq, l, affine=True)
            metric, det = sq.affine_metric(l)
            assert rel(metric, np.array([a.M[0, 0], a.M[1, 1], a.M[0, 1]])) < 1e-13
            assert abs(det - a.det) < 1e-13 * a.det
        else:
            with pytest.raises(mg._lib.MgxError) as e:
                sq.affine_metric(l)
            assert e.value.status == -4
        X = sq.dof_coordinates(l)
        assert np.array_equal(X[q.dofs_plain], sq.cell_nodes(l))
        d = sq.operator_desc(l)
        assert d.dim == 2 and bool(d.coef_q) == (geometry == "sector")
    if geometry == "sector":
        # the exact map: r = 0.5 + 0.5 X, theta = (pi / 2) Y on the box normalised to the unit square
        X = sq.dof_coordinates(sq.max_level)
        r, theta = np.hypot(X[:, 0], X[:, 1]), np.arctan2(X[:, 1], X[:, 0])
        assert r.min() == pytest.approx(0.5, abs=1e-15) and r.max() == pytest.approx(1.0, abs=1e-15)
        assert theta.min() > -1e-15 and theta.max() < np.pi / 2 + 1e-15
        c = sq.constrained(sq.max_level)
        on_side = (np.abs(r[c] - 0.5) < 1e-14) | (np.abs(r[c] - 1) < 1e-14) | (np.abs(theta[c]) < 1e-14) | \
            (np.abs(theta[c] - np.pi / 2) < 1e-14)
        assert on_side.all()
        with pytest.raises(ValueError):
            sq.rhs(0)
        with pytest.raises(ValueError):
            sq.bc(0)
        with pytest.raises(mg._lib.MgxError):
            mg.Square(p, jacobian=SHEAR, mapped="annulus_sector")
    sq.close()


@pytest.mark.parametrize("case", sorted(NEWTON_CASES_2D))
def test_newton_with_exact_linear_solves(case):
    geometry, p, n_refine, amplitude = case
    sq = make_square(geometry, p, n_refine)
    l = sq.max_level
    ref = reference(sq, l, affine=geometry != "sector")
    _, norms, halvings = ref.newton(boundary_state(sq, l, amplitude), max_steps=12, tolerance=1e-13)
    print("%s p=%d, %d^2 cells, A=%g: residual norms %s, halvings %s"
          % (geometry, p, 2 ** n_refine, amplitude, " -> ".join("%.2e" % r for r in norms), halvings))
    n6, n10 = nr2.steps_to(norms, 1e-6), nr2.steps_to(norms, 1e-10)
    assert n6 == NEWTON_CASES_2D[case]
    assert n10 is not None and n10 <= n6 + 2
    assert not any(halvings)
    assert all(b < a for a, b in zip(norms, norms[1:]))
    sq.close()


def test_interpolation_to_the_coarser_level():
    """a polynomial of degree <= p per direction on the fine level is reproduced in the coarse nodes"""
    p = 3
    sq = make_square("square", p, box=(3, 2, 2))
    R = nr2.interpolation_matrix_1d(sq.gll())
    f = lambda x: (1 + x[:, 0] - 0.5 * x[:, 0] ** 3) * (2 - x[:, 1] ** 2 + 0.3 * x[:, 1] ** 3)
    for l in range(1, sq.n_levels):
        got = nr2.interpolate_to_coarse(R, sq.children(l), nr2.cell_dofs(sq.idx9_plain(l), p), nr2.cell_dofs(sq.idx9_plain(l - 1), p),
                                        sq.n_dofs(l - 1), f(sq.dof_coordinates(l)))
        assert np.abs(got - f(sq.dof_coordinates(l - 1))).max() < 1e-13
    sq.close()
