"""The lattice reference of the cube transfers (tests/transfer_lattice.py) against the CPU oracle, and the check that
the GPU comparison with a non-symmetric embedding is not vacuous (CPU only)."""
import numpy as np
import pytest

from oracle import Oracle
from transfer_lattice import LatticeTransfer, embedding_matrix, lagrange_embedding, skewed_nodes, symmetrised


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def lattice_of(orc, l, P1):
    N = orc.cells_per_dim3(l - 1)
    return LatticeTransfer(P1, N, orc.dof_grid(l - 1), orc.dof_grid(l), orc.constrained(l - 1))


@pytest.mark.parametrize("ns,nr", [(1, 2), (3, 1)])
@pytest.mark.parametrize("p", range(1, 10))
def test_lattice_transfers_equal_the_oracle(p, ns, nr):
    """prolongate, prolongate_and_add, restrict_and_add with and without constraints, and R = P^T, on every level
    pair, to 1e-14 of the max-norm; the oracle's embedding is the Lagrange embedding of its Gauss-Lobatto nodes"""
    orc = Oracle(p, ns, nr)
    P1 = orc.prolong_1d()
    assert np.abs(P1 - lagrange_embedding(orc.gll())).max() < 1e-14
    assert np.abs(symmetrised(P1) - P1).max() < 1e-15  # a symmetric embedding is its own even-odd form
    rng = np.random.default_rng(p + 10 * ns)
    for l in range(1, orc.n_levels):
        lt = lattice_of(orc, l, P1)
        xc, yc = rng.uniform(-1, 1, (2, orc.n_dofs(l - 1)))
        xf, yf = rng.uniform(-1, 1, (2, orc.n_dofs(l)))
        for wc in (False, True):
            assert rel(lt.prolongate(xc, with_constraints=wc), orc.prolongate(l, xc, with_bc=wc)) < 1e-14
            assert rel(lt.prolongate(xc, yf, with_constraints=wc), orc.prolongate(l, xc, fine=yf, with_bc=wc)) < 1e-14
            assert rel(lt.restrict_and_add(yc, xf, with_constraints=wc), orc.restrict_and_add(l, yc, xf, with_bc=wc)) < 1e-14
        # the fourth operation: restriction is the transpose of the prolongation, (R xf, xc) = (xf, P xc)
        Pxc = orc.prolongate(l, xc)
        lhs, rhs = orc.restrict_and_add(l, np.zeros(orc.n_dofs(l - 1)), xf) @ xc, xf @ Pxc
        assert abs(lhs - rhs) < 1e-13 * np.abs(xf).sum() * np.abs(Pxc).max()
        # constrained coarse entries: never written by the restriction with constraints
        cons = orc.constrained(l - 1)
        assert cons.size > 0 and np.array_equal(orc.restrict_and_add(l, yc, xf, with_bc=True)[cons], yc[cons])
    orc.close()


@pytest.mark.parametrize("p", range(2, 10))
def test_a_non_symmetric_embedding_differs_from_its_even_odd_form(p):
    """A Lagrange basis on the nodes (j/p)^1.3: the lattice transfers with this P1 and with the embedding its even-odd
    form stands for (what the pipelined kernels applied before they were restricted to symmetric embeddings) differ
    by more than 1e-3 of the max-norm -- ten orders of magnitude above the fp64 tolerance (1e-13) of the GPU
    comparison and far above its fp32 bound (below 1e-4 at p = 9) -- so that comparison is not vacuous."""
    P1 = lagrange_embedding(skewed_nodes(p))
    assert np.abs(P1[0] - np.eye(p + 1)[0]).max() == 0 and np.abs(P1[2 * p] - np.eye(p + 1)[p]).max() == 0
    Ps = symmetrised(P1)
    orc = Oracle(p, 1, 2)
    l = 2
    lt, ls = lattice_of(orc, l, P1), lattice_of(orc, l, Ps)
    rng = np.random.default_rng(p)
    xc, yc = rng.uniform(-1, 1, (2, orc.n_dofs(l - 1)))
    xf = rng.uniform(-1, 1, orc.n_dofs(l))
    for wc in (False, True):
        assert rel(ls.prolongate(xc, with_constraints=wc), lt.prolongate(xc, with_constraints=wc)) > 1e-3
        assert rel(ls.restrict_and_add(yc, xf, with_constraints=wc), lt.restrict_and_add(yc, xf, with_constraints=wc)) > 1e-3
    # the embedding is consistent (shared fine points agree), a perturbed one is refused
    bad = P1.copy()
    bad[2 * p, 0] = 1e-3
    with pytest.raises(AssertionError):
        embedding_matrix(bad, 2)
    orc.close()
