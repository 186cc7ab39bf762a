"""CPU checks of the two-dimensional numpy restatement tests/dg_reference_2d.py, so that tests/test_gpu_dg_2d.py does
not measure the HIP kernels against something nobody checked:

  1. extrusion: on a Cartesian mesh the trusted 3D oracle (oracle/dg_oracle.py) applied to u2 (x) v equals
     (A2 u2) (x) (M1 v) + (M2 u2) (x) (A1 v) with the 1D mass and SIP forms of one cell between two Dirichlet ends;
  2. on a sheared mesh the 2D form is symmetric, positive definite and the same operator in the three bases;
  3. it is consistent: A u_h = (f, phi) for a polynomial solution that vanishes on the boundary;
  4. the block-Jacobi preconditioner is the inverse of diag(T2^T A_KK T2) for all 16 combinations of Dirichlet faces;
  5. level transfers: R = P^T, and the prolongation reproduces polynomials of degree p;
  6. the plain V-cycle is symmetric and the preconditioned CG converges.

Recorded results of test_harness_problem_iteration_counts (DGPlainOracle2D, FE_DGQHermite(3) on [-0.9, 1]^2, the
right-hand side of tools/poisson_dg_plain.py --dim 2, tolerance 1e-9); tests/test_gpu_dg_2d.py reads the two counts
from the next line:
HARNESS_2D_CG_ITERATIONS = {2: 16, 3: 16}

One more test covers the mesh helpers mgx_dg_box_neighbours_2d / mgx_dg_box_children_2d through the loaded library
(no device needed)."""
import re

import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_reference_2d as ref2

# sheared and non-symmetric: the entries the issue names, (I + 0.12 (d+1)(e+1)) diag(0.95, 0.89)
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]


def recorded_harness_iterations():
    m = re.search(r"HARNESS_2D_CG_ITERATIONS = \{2: (\d+), 3: (\d+)\}", __doc__)
    return {2: int(m.group(1)), 3: int(m.group(2))}


# ------------------------------------------------------------------------------------------ 1. extrusion
@pytest.mark.parametrize("cells", [(2, 2, 1), (3, 1, 1)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", [1, 2, 3])
def test_extrusion_against_the_3d_oracle(p, kind, cells):
    hx, hy, hz = 0.7, 1.3, 0.45
    n = p + 1
    o3 = dg.DGOracle(p, kind, cells, np.diag([hx, hy, hz]))
    o2 = ref2.DGOracle2D(p, kind, cells[:2], np.diag([hx, hy]))
    # 1D forms of one cell with both ends Dirichlet (sigma_F = 2 sigma, dg_oracle.py:201-203), as :208-212 builds
    # the half-weighted ones
    polys = dg.basis_1d(p, kind)
    S, SD, wq = o3.S, o3.SD, o3.wq
    b = [np.array([[float(f(s)) for f in polys]]) for s in (0.0, 1.0)]
    g = [np.array([[float(f.d(s)) for f in polys]]) for s in (0.0, 1.0)]
    mass = S.T @ (wq[:, None] * S)
    lapl = SD.T @ (wq[:, None] * SD)
    lapl = lapl + 2 * n * n * b[0].T @ b[0] + (g[0].T @ b[0] + b[0].T @ g[0])
    lapl = lapl + 2 * n * n * b[1].T @ b[1] - (g[1].T @ b[1] + b[1].T @ g[1])
    M1, A1 = hz * mass, lapl / hz
    M2 = hx * hy * ref2.kron2(mass, mass)
    rng = np.random.default_rng(10 * p + kind)
    u2, v = rng.standard_normal(o2.shape), rng.standard_normal(n)
    u3 = np.einsum("k,yxl->yxkl", v, u2).reshape(o3.shape)         # local index (k, j, i): k slowest
    want = np.einsum("k,yxl->yxkl", M1 @ v, o2.vmult(u2)) + np.einsum("k,yxl->yxkl", A1 @ v, u2 @ M2.T)
    got = o3.vmult(u3)
    err = abs(got - want.reshape(o3.shape)).max() / abs(got).max()
    print("extrusion p=%d kind=%d cells=%s: %.3e" % (p, kind, cells, err))
    assert err < 1e-11


# ------------------------------------------------------------------------------------------ 2. SPD, basis-independent
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_sheared_form_is_symmetric_definite_and_the_same_in_every_basis(p):
    cells = (3, 2)
    mats = {}
    for kind in KINDS:
        o = ref2.DGOracle2D(p, kind, cells, SHEARED_2D)
        A = o.dense_matrix()
        assert abs(A - A.T).max() < 1e-13 * abs(A).max()
        assert np.linalg.eigvalsh(0.5 * (A + A.T))[0] > 0
        mats[kind] = (o, A)
    Ag = mats[dg.GAUSS][1]
    for kind in (dg.HERMITE, dg.GAUSS_LOBATTO):
        o, A = mats[kind]
        B = np.kron(np.eye(cells[0] * cells[1]), ref2.kron2(o.S, o.S))   # coefficients -> values in the Gauss points
        err = abs(A - B.T @ Ag @ B).max() / abs(A).max()
        print("basis %d against Gauss, p=%d: %.3e" % (kind, p, err))
        assert err < 1e-11


# ------------------------------------------------------------------------------------------ 3. consistency
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", [2, 3, 4])
def test_sheared_form_is_consistent(kind, p):
    o = ref2.DGOracle2D(p, kind, (3, 2), SHEARED_2D)
    N = np.array(o.cells, float)
    inv = np.linalg.inv(o.J)
    G = inv @ inv.T

    def u(x):
        xi = x @ inv.T
        return np.prod(xi * (N - xi), axis=1)

    def f(x):  # -Laplace u
        xi = x @ inv.T
        w, dw = xi * (N - xi), N - 2 * xi
        lap = -2.0 * (G[0, 0] * w[:, 1] + G[1, 1] * w[:, 0]) + 2 * G[0, 1] * dw[:, 0] * dw[:, 1]
        return -lap

    rhs = o.load_vector(f)
    assert abs(o.vmult(o.interpolate(u)) - rhs).max() < 1e-11 * abs(rhs).max()


# ------------------------------------------------------------------------------------------ 4. block Jacobi
@pytest.mark.parametrize("kind", KINDS)
def test_block_jacobi_is_the_inverse_of_the_transformed_diagonal_in_all_16_categories(kind):
    p = 3
    n2 = (p + 1) ** 2
    seen = set()
    rng = np.random.default_rng(4)
    for cells in ((1, 1), (3, 1), (1, 3), (3, 3)):
        o = ref2.DGOracle2D(p, kind, cells, SHEARED_2D)
        mass = o.S.T @ (o.wq[:, None] * o.S)
        assert np.allclose(o.T.T @ mass @ o.T, np.eye(p + 1), atol=1e-12)
        A = o.dense_matrix()
        r = rng.standard_normal(o.shape)
        z = o.jacobi_vmult(r)
        for j in range(cells[1]):
            for i in range(cells[0]):
                c = j * cells[0] + i
                blk = A[c * n2:(c + 1) * n2, c * n2:(c + 1) * n2]
                lower, upper = (i == 0, j == 0), (i == cells[0] - 1, j == cells[1] - 1)
                assert np.allclose(blk, o.own_block(lower, upper), atol=1e-12 * abs(blk).max())
                d = np.diag(o.T2.T @ blk @ o.T2)
                assert np.allclose(z[j, i], o.T2 @ ((o.T2.T @ r[j, i]) / d), rtol=1e-11, atol=1e-13)
                seen.add(lower + upper)
    assert len(seen) == 16
    # the update formulas of laplace_operator_dg.h:1839-1860
    rhs, x, xo = (rng.standard_normal(o.shape) for _ in range(3))
    new, old = o.vmult_with_chebyshev_update(rhs, 2, 0.6, 0.2, x, xo)
    assert np.allclose(old, x) and np.allclose(new, 0.2 * o.jacobi_vmult(rhs - o.vmult(x)) + 1.6 * x - 0.6 * xo)
    new1, _ = o.vmult_with_chebyshev_update(rhs, 1, 0.6, 0.2, x, xo)
    assert np.allclose(new1, 0.2 * o.jacobi_vmult(rhs - o.vmult(x)) + 1.6 * x)
    new0, _ = o.vmult_with_chebyshev_update(rhs, 0, 0.6, 0.2, x, xo)
    assert np.allclose(new0, 0.2 * o.jacobi_vmult(rhs))


# ------------------------------------------------------------------------------------------ 5. level transfers
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", [1, 2, 3, 5])
def test_level_transfers_are_transposes_and_reproduce_polynomials(kind, p):
    o = ref2.DGPlainOracle2D(1, kind, (1, 1), np.eye(2), 1)          # (only to borrow the class's transfer methods)
    o.p, o.P = p, ref2.embedding_1d(p, kind)
    o.P2 = [ref2.kron2(o.P[k & 1], o.P[k >> 1]) for k in range(4)]
    coarse = ref2.DGOracle2D(p, kind, (3, 2), SHEARED_2D)
    fine = ref2.DGOracle2D(p, kind, (6, 4), SHEARED_2D / 2)
    o.level = [coarse, fine]
    rng = np.random.default_rng(5)
    c, f = rng.standard_normal(coarse.shape), rng.standard_normal(fine.shape)
    assert np.vdot(o.prolongate(1, c), f) == pytest.approx(np.vdot(c, o.restrict(1, f)), rel=1e-12)

    inv = np.linalg.inv(SHEARED_2D)

    def poly(x):  # degree p per direction of the (sheared) cells
        xi = x @ inv.T
        return (0.3 + xi[:, 0]) ** p * (1.0 - 0.7 * xi[:, 1]) ** p + xi[:, 0] * xi[:, 1]

    want = fine.interpolate(poly)
    assert abs(o.prolongate(1, coarse.interpolate(poly)) - want).max() < 1e-11 * abs(want).max()


# ------------------------------------------------------------------------------------------ 6. solver
def test_plain_v_cycle_is_symmetric_and_cg_converges():
    o = ref2.DGPlainOracle2D(2, dg.HERMITE, (2, 1), SHEARED_2D, 3)
    A = o.level[-1]
    rng = np.random.default_rng(6)
    x, y = rng.standard_normal(A.shape), rng.standard_normal(A.shape)
    assert np.vdot(o.v_cycle(x), y) == pytest.approx(np.vdot(x, o.v_cycle(y)), rel=1e-9)
    rhs = rng.standard_normal(A.shape)
    sol, its, red = o.solve_cg(rhs, 1e-9)
    print("iterations", its, "reduction", red)
    assert its < 25 and np.linalg.norm(A.vmult(sol) - rhs) < 2e-9 * np.linalg.norm(rhs)
    assert np.allclose(sol, np.linalg.solve(A.dense_matrix(), rhs.ravel()).reshape(A.shape), rtol=0, atol=1e-7 * abs(sol).max())


def harness_rhs_2d(A, n_refine):
    """(f, phi) of tools/poisson_dg_plain.py --dim 2: f = 2 (3 pi)^2 sin(3 pi x) sin(3 pi y) on [-0.9, 1]^2"""
    return A.load_vector(lambda x: 2 * (3 * np.pi) ** 2 * np.prod(np.sin(3 * np.pi * (x - 0.9)), axis=1))


def test_harness_problem_iteration_counts():
    """the CG iteration counts of the harness problem, which the docstring of this module records"""
    got = {}
    for n_refine in (2, 3):
        o = ref2.DGPlainOracle2D(3, dg.HERMITE, (1, 1), np.eye(2) * 1.9, n_refine + 1)
        _, its, red = o.solve_cg(harness_rhs_2d(o.level[-1], n_refine), 1e-9)
        print("n_refine", n_refine, "iterations", its, "reduction", red)
        got[n_refine] = its
    assert got == recorded_harness_iterations()


# ------------------------------------------------------------------------------------------ mesh helpers
@pytest.mark.parametrize("ordering", ["z", "lexicographic"])
@pytest.mark.parametrize("cells", [(3, 2), (4, 4), (1, 5)])
def test_box_helpers_2d(cells, ordering):
    mg = pytest.importorskip("multigrid_amd")
    nb, ij = mg.dg_box_neighbours(cells, ordering)
    n = cells[0] * cells[1]
    assert nb.shape == (n, 4) and ij.shape == (n, 2)
    assert sorted(map(tuple, ij)) == sorted((i, j) for j in range(cells[1]) for i in range(cells[0]))
    if ordering != "z":
        assert np.array_equal(ij[:, 0] + cells[0] * ij[:, 1], np.arange(n))
    at = {tuple(p): c for c, p in enumerate(ij)}
    for c in range(n):
        for d in range(2):
            for s in range(2):
                pos = list(ij[c])
                pos[d] += 2 * s - 1
                inside = 0 <= pos[d] < cells[d]
                assert nb[c, 2 * d + s] == (at[tuple(pos)] if inside else -1)       # boundaries where they should be
                if inside:
                    assert nb[nb[c, 2 * d + s], 2 * d + 1 - s] == c                  # the relation is symmetric
    ch = mg.dg_box_children(cells, ordering, ordering)
    fine = (2 * cells[0], 2 * cells[1])
    _, fij = mg.dg_box_neighbours(fine, ordering)
    assert ch.shape == (n, 4) and sorted(ch.ravel()) == list(range(4 * n))          # a permutation
    for c in range(n):
        for k in range(4):
            assert tuple(fij[ch[c, k]]) == (2 * ij[c, 0] + (k & 1), 2 * ij[c, 1] + (k >> 1))
    if ordering == "z" and cells == (4, 4):
        assert np.array_equal(ch.ravel(), np.arange(4 * n))                          # forest order: the identity table
