"""The numpy restatement of the DG right-hand side with Dirichlet boundary data and of the L2 error sums
(tests/dg_rhs_reference.py) on the CPU: the polynomial identity that ties the boundary term to the operator, and the
dense solve that shows the benchmark's plateau turn into convergence.  No GPU."""
import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_reference_2d as ref2
import dg_rhs_reference as rr

KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])


def sheared_box(dim, p, kind):
    if dim == 3:
        return dg.DGOracle(p, kind, (2, 1, 2), dg.cheby_mesh(2)[1])
    return ref2.DGOracle2D(p, kind, (3, 2), SHEARED_2D)


def polynomial(dim, p):
    """u = (1 + a.x)^p, total degree p, and -Laplace u"""
    a = np.array([0.3, -0.2, 0.5][:dim])
    u = lambda x: (1.0 + x @ a) ** p                                               # noqa: E731
    f = lambda x: -p * (p - 1) * (a @ a) * (1.0 + x @ a) ** max(p - 2, 0)          # noqa: E731
    return u, f


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dim", [2, 3])
def test_polynomial_identity(dim, p, kind):
    """A interpolate(u) = load(-Laplace u) + boundary_load(u) for a polynomial of total degree <= p: the quadrature is
    exact for every term, u has no jumps, so only the Dirichlet faces' sigma_F u phi - u d_n phi is left of the faces.
    Rounding alone separates the two sides: 1e-12 of the largest entry leaves three digits to the sums of up to
    (p+1)^3 products of entries of order one."""
    o = sheared_box(dim, p, kind)
    r = rr.RhsReference(o, origin=[-0.9, 0.3, 0.1][:dim])
    u, f = polynomial(dim, p)
    lhs = o.vmult(r.interpolate(u))
    rhs = r.load_vector(f) + r.boundary_load(u)
    assert abs(lhs - rhs).max() < 1e-12 * abs(rhs).max()
    # and the restated sums: the interpolant is u itself, the weights add up to the volume
    s = r.l2_sums(r.interpolate(u), u)
    assert s[0] <= 1e-24 * s[1]
    assert np.isclose(s[1], abs(np.linalg.det(o.J)) * np.prod(o.cells), rtol=1e-13)


@pytest.mark.parametrize("dim", [2, 3])
def test_dense_matrix_from_blocks(dim):
    o = sheared_box(dim, 2, dg.HERMITE)
    A, B = rr.RhsReference(o).dense_matrix(), o.dense_matrix()
    assert abs(A - B).max() <= 1e-14 * abs(B).max()


def test_boundary_term_turns_the_plateau_into_convergence():
    """prod sin(3 pi x_d) on [-0.9, 1]^2, Hermite-like basis, p = 3, dense solves on 4^2, 8^2 and 16^2 cells.  With the
    volume term alone the error is the mismatch of the boundary values, 0.1383 / 0.1364 / 0.1365 at every resolution
    (the 2D plateau of the benchmark); with the boundary term 2.560e-2, 2.811e-3, 2.545e-4, ratios 9.1 and 11.0 >= 2^p."""
    u = lambda x: np.prod(np.sin(3 * np.pi * x), axis=-1)                           # noqa: E731
    f = lambda x: 2 * (3 * np.pi) ** 2 * u(x)                                       # noqa: E731
    plateau, err = [], []
    for n in (4, 8, 16):
        o = ref2.DGOracle2D(3, dg.HERMITE, (n, n), np.eye(2) * 1.9 / n)
        r = rr.RhsReference(o, origin=[-0.9, -0.9])
        A = r.dense_matrix()
        b0 = r.load_vector(f)
        plateau.append(r.l2_error(np.linalg.solve(A, b0.ravel()), u))
        err.append(r.l2_error(np.linalg.solve(A, (b0 + r.boundary_load(u)).ravel()), u))
    print("volume only", plateau, "with the boundary term", err)
    assert np.allclose(plateau, [0.1383, 0.1364, 0.1365], rtol=0, atol=6e-5)        # the printed digits
    assert np.allclose(err, [2.560e-2, 2.811e-3, 2.545e-4], rtol=5e-4)              # ... of four
    # what the GPU test compares with, to 1e-3: the solve's rounding (condition 1e5 x 1e-16) is 1e-7 of the last error
    assert np.allclose(err, rr.DENSE_ERRORS_2D_P3, rtol=1e-6)
    assert err[0] / err[1] >= 8 and err[1] / err[2] >= 8
