"""CPU checks of tests/dg_multigrid_reference_2d.py (DGMultigridOracle2D), so that tests/test_gpu_dg_multigrid_2d.py does
not measure the HIP kernels against something nobody checked.  The DG level (tests/dg_reference_2d.py) and the FE_Q
hierarchy (tests/feq_reference_2d.py) are pinned by their own files; here, what joins them:

  1. the restriction DG -> FE_Q is the transpose of the embedding: (R r, c) = (r, P c);
  2. the embedding of an FE_Q function is exact: the DG function returns the grid values in the cells' Gauss-Lobatto
     nodes, and a polynomial of degree p per direction that vanishes on the boundary comes back in the Gauss points;
  3. P2 = P1 x P1 is the block of the 3D oracle's P3 = P1 x P1 x P1: P3[(k, .), (k', .)] = P1[k, k'] P2;
  4. the V-cycle is symmetric;
  5. the V-cycle-preconditioned CG converges, in the recorded number of iterations.

Recorded results of test_pcg_converges (Square(p, 1, n_refine): [-0.9, 1]^2 refined n_refine times, degree_pre 3, the
right-hand side of dg_multigrid_reference_2d.pcg_inputs, tolerance 1e-9), keys (p, n_refine, basis);
tests/test_gpu_dg_multigrid_2d.py reads the counts from the next line:
PCG_ITERATIONS_2D = {(2, 2, 0): 8, (3, 2, 0): 8, (4, 2, 0): 8, (3, 3, 0): 8, (3, 2, 1): 8, (3, 2, 2): 8, (1, 3, 0): 8, (5, 1, 0): 8, (2, 1, 0): 8, (3, 4, 0): 8, (2, 2, 1): 8, (2, 3, 0): 8}
"""
import ast
import re

import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
from oracle import dg_oracle as dg  # noqa: E402

import dg_multigrid_reference_2d as ref  # noqa: E402
import feq_reference_2d as feq  # noqa: E402
from dg_reference_2d import kron2  # noqa: E402

SETS = [(2, 2, 0), (3, 2, 0), (4, 2, 0), (3, 3, 0), (3, 2, 1), (3, 2, 2), (1, 3, 0), (5, 1, 0), (2, 1, 0), (3, 4, 0), (2, 2, 1),
        (2, 3, 0)]


def recorded_iterations(text=None):
    m = re.search(r"PCG_ITERATIONS_2D = (\{[^}]*\})", __doc__ if text is None else text)
    return ast.literal_eval(m.group(1))


_elements = {}


def element(p):
    """the 1D arrays of FE_Q(p) from the mesh provider (host code)"""
    if p not in _elements:
        sq = mg.Square(p, 1, 0)
        _elements[p] = feq.arrays_1d(sq)
        sq.close()
    return _elements[p]


def pair(p, nr, kind):
    return ref.make_pair(element(p), p, kind, (1, 1), nr, 1.9)


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("p,nr,kind", [(1, 2, 0), (2, 2, 0), (3, 1, 1), (3, 2, 2), (4, 1, 0)])
def test_restriction_is_the_transposed_embedding(p, nr, kind):
    dgo, _, orc = pair(p, nr, kind)
    rng = np.random.default_rng(p + nr)
    r, c = rng.standard_normal(dgo.shape), rng.standard_normal(orc.G)
    lhs, rhs = np.vdot(orc.restrict_to_cg(r), c), np.vdot(r, orc.prolongate_cg_to_dg(c))
    assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(r) * np.linalg.norm(c)
    g = orc.restrict_to_cg(r)
    assert not g[0].any() and not g[-1].any() and not g[:, 0].any() and not g[:, -1].any()


@pytest.mark.parametrize("p,nr,kind", [(1, 2, 0), (2, 2, 0), (3, 1, 1), (3, 2, 2), (4, 1, 0)])
def test_embedding_is_exact(p, nr, kind):
    dgo, fe, orc = pair(p, nr, kind)
    n, (nx, ny) = p + 1, dgo.cells
    rng = np.random.default_rng(5 * p + nr)
    c = rng.standard_normal(orc.G)
    c[0], c[-1], c[:, 0], c[:, -1] = 0, 0, 0, 0
    d = orc.prolongate_cg_to_dg(c)
    polys = dg.basis_1d(p, kind)
    B = np.array([f(dg.gauss_lobatto01(n)) for f in polys]).T      # values in the Gauss-Lobatto nodes
    back = d @ kron2(B, B).T
    for j in range(ny):
        for i in range(nx):
            assert np.abs(back[j, i].reshape(n, n) - c[j * p:j * p + n, i * p:i * p + n]).max() < 1e-12
    if p >= 2:   # u = x (L - x) y (L - y) in units of the cell size: in Q_p of every cell, zero on the boundary
        node = np.append((np.arange(nx)[:, None] + dg.gauss_lobatto01(n)[None, :p]).ravel(), nx)   # the grid, one direction
        u1 = node * (nx - node)
        d = orc.prolongate_cg_to_dg(np.outer(u1, u1))
        q = np.arange(nx)[:, None] + dgo.xq[None, :]                 # Gauss points of every cell, one direction
        uq = q * (nx - q)
        got = d @ kron2(dgo.S, dgo.S).T
        for j in range(ny):
            for i in range(nx):
                assert np.abs(got[j, i].reshape(n, n) - np.outer(uq[j], uq[i])).max() < 1e-11 * nx ** 4


@pytest.mark.parametrize("p,kind", [(1, 0), (2, 1), (3, 0), (3, 2)])
def test_p2_is_the_block_of_the_3d_oracles_p3(p, kind):
    _, _, orc = pair(p, 1, kind)
    n = p + 1
    P3 = dg.kron3(orc.P1, orc.P1, orc.P1).reshape(n, n * n, n, n * n)
    for a in range(n):
        for b in range(n):
            assert np.array_equal(P3[a, :, b, :], orc.P1[a, b] * orc.P2)


@pytest.mark.parametrize("p,nr,kind", [(2, 2, 0), (3, 2, 1), (3, 2, 2), (1, 3, 0)])
def test_v_cycle_is_symmetric(p, nr, kind):
    dgo, _, orc = pair(p, nr, kind)
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal(dgo.shape), rng.standard_normal(dgo.shape)
    a, b = np.vdot(orc.v_cycle(x), y), np.vdot(x, orc.v_cycle(y))
    print("symmetry %.3e" % (abs(a - b) / abs(a)))
    assert abs(a - b) < 1e-11 * abs(a)


@pytest.mark.parametrize("p,nr,kind", SETS)
def test_pcg_converges(p, nr, kind):
    dgo, _, orc = pair(p, nr, kind)
    _, rhs = ref.pcg_inputs(dgo.shape)
    x, its, rate = orc.solve_cg(rhs, 1e-9)
    print("PCG (%d, %d, %d): %d iterations, rate %.4f" % (p, nr, kind, its, rate))
    # (the bound of tests/test_gpu_dg_multigrid.py on the true residual: the iteration stops on the recursive one)
    assert np.linalg.norm(rhs - dgo.vmult(x)) < 2e-9 * np.linalg.norm(rhs)
    assert its == recorded_iterations()[(p, nr, kind)] and rate ** its <= 1e-9
