"""The numpy restatement of the solution-dependent coefficient (tests/nonlinear_reference.py) pinned on the CPU, so that
the GPU tests do not compare the device against a second copy of the same mistake: the minimal-surface tensor is the
derivative of the minimal-surface residual, the unit law is the Laplace operator of the existing oracle, Newton's method
with exact linear solves converges quadratically, the interpolation matrix reproduces polynomials.

NEWTON_CASES records, per case, the number of Newton steps to 1e-6 of the first residual norm as measured with the
project's own Gauss-Lobatto / Gauss tables (dense exact solves); test_gpu_nonlinear.py uses them as its yardstick."""
import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
import nonlinear_reference as nr  # noqa: E402
from oracle_view import oracle_for  # noqa: E402

# (degree, n_refine, amplitude) -> N6: steps until the residual norm is below 1e-6 of the first one
NEWTON_CASES = {(2, 2, 1.0): 4, (3, 1, 1.0): 4, (2, 2, 0.25): 3, (3, 2, 1.0): 5}


def reference(cube, l, jacobian=None):
    metric, det = cube.affine_metric(l, jacobian)
    return nr.NonlinearReference(cube.degree, cube.shape_values(), cube.colloc_grad(), cube.qweights(), cube.idx27(l),
                                 cube.idx27_plain(l), cube.n_dofs(l), metric, det)


def boundary_state(cube, l, amplitude, jacobian=None):
    """zero in the interior, A sin(2 pi (x + y)) on the Dirichlet DoFs (minimal_surface/program.cc:97-99)"""
    u = np.zeros(cube.n_dofs(l))
    c = cube.constrained(l)
    x = cube.dof_coordinates(l, jacobian)[c]
    u[c] = amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1]))
    return u


@pytest.mark.parametrize("p,n_refine", [(2, 2), (3, 1)])
def test_tensor_is_the_derivative_of_the_residual(p, n_refine):
    cube = mg.Cube(p, 1, n_refine)
    l = cube.max_level
    ref = reference(cube, l)
    rng = np.random.default_rng(7)
    u = rng.uniform(-1, 1, cube.n_dofs(l))  # boundary values included
    v = np.zeros(cube.n_dofs(l))
    v[ref.free] = rng.uniform(-1, 1, ref.free.size)
    eps = 1e-6
    fd = (ref.residual(nr.LAW_MINIMAL_SURFACE, u + eps * v) - ref.residual(nr.LAW_MINIMAL_SURFACE, u - eps * v)) / (2 * eps)
    av = ref.apply(ref.coefficient(nr.LAW_MINIMAL_SURFACE, u), v)
    av[ref.constrained] = 0.0
    diff = np.abs(fd + av).max() / np.abs(av).max()
    print("p=%d: relative difference of the central difference and -A(u) v: %.3e" % (p, diff))
    assert diff < 1e-8
    cube.close()


@pytest.mark.parametrize("p,n_refine", [(2, 2), (3, 1), (4, 1)])
def test_unit_law_is_the_laplace_operator(p, n_refine):
    cube = mg.Cube(p, 1, n_refine)
    orc = oracle_for(cube, p, 1, n_refine)
    for l in range(cube.n_levels):
        ref = reference(cube, l)
        x = cube.seeded_vector(l, 3)
        coef = ref.coefficient(nr.LAW_UNIT, x)
        got, want = ref.apply(coef, x), orc.vmult(l, x)
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-12
        assert np.array_equal(coef, cube.unit_law_coefficient(l))
        # matrix() is the dense form of apply()
        assert np.abs(np.linalg.solve(ref.matrix(coef), got) - x).max() < 1e-10
    cube.close()
    orc.close()


@pytest.mark.parametrize("case", sorted(NEWTON_CASES))
def test_newton_with_exact_linear_solves(case):
    p, n_refine, amplitude = case
    cube = mg.Cube(p, 1, n_refine)
    l = cube.max_level
    ref = reference(cube, l)
    _, norms, halvings = ref.newton(boundary_state(cube, l, amplitude), max_steps=12, tolerance=1e-13)
    print("p=%d, %d^3 cells, A=%g: residual norms %s, halvings %s"
          % (p, 2 ** n_refine, amplitude, " -> ".join("%.2e" % r for r in norms), halvings))
    n6, n10 = nr.steps_to(norms, 1e-6), nr.steps_to(norms, 1e-10)
    assert n6 == NEWTON_CASES[case]
    assert n10 is not None and n10 <= n6 + 2
    assert all(b < a for a, b in zip(norms, norms[1:]))  # the line search's contract
    cube.close()


@pytest.mark.parametrize("p", range(1, 10))
def test_interpolation_matrix(p):
    cube = mg.Cube(p, 1, 0)
    gll = cube.gll()
    R = nr.interpolation_matrix_1d(gll)
    assert np.abs(R.sum(axis=1) - 1).max() < 1e-13
    # fine patch points: the nodes of child 0 on [0, 1/2] and of child 1 on [1/2, 1]
    xf = np.concatenate([gll / 2, 0.5 + gll[1:] / 2])
    rng = np.random.default_rng(p)
    for _ in range(3):
        c = rng.uniform(-1, 1, p + 1)
        assert np.abs(R @ np.polyval(c, xf) - np.polyval(c, gll)).max() < 1e-13
    if p <= 2:  # every coarse node is a fine node: plain injection
        assert set(np.unique(R)) == {0.0, 1.0} and np.array_equal(R @ xf, gll)
    # prolongation followed by interpolation is the identity
    assert np.abs(R @ cube.prolong_1d() - np.eye(p + 1)).max() < 1e-13
    cube.close()


def test_interpolation_to_the_coarser_level():
    """a polynomial of degree <= p per direction on the fine level is reproduced in the coarse nodes"""
    p = 3
    cube = mg.Cube(p, 1, 2)
    R = nr.interpolation_matrix_1d(cube.gll())
    f = lambda x: (1 + x[:, 0] - 0.5 * x[:, 0] ** 3) * (2 - x[:, 1] ** 2) * (0.3 + x[:, 2] ** 3)
    for l in range(1, cube.n_levels):
        fine = f(cube.dof_coordinates(l))
        got = nr.interpolate_to_coarse(R, cube.children(l), nr.cell_dofs(cube.idx27_plain(l), p),
                                       nr.cell_dofs(cube.idx27_plain(l - 1), p), cube.n_dofs(l - 1), fine)
        assert np.abs(got - f(cube.dof_coordinates(l - 1))).max() < 1e-13
    cube.close()
