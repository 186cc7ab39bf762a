"""An independent fp64 reference of the cube transfers, built from the 1D embedding and the DoF lattice alone.

On a structured cube of N^3 cells (per direction N cells of degree p, G = N p + 1 lattice points, lattice id
(gz*Gy+gy)*Gx+gx as mgx_cube_dof_grid / orc_dof_grid report it) the prolongation from level l-1 to level l is the
Kronecker product Pz (x) Py (x) Px of three 1D embeddings.  The 1D factor maps the N p + 1 coarse points to the
2 N p + 1 fine ones: fine cell f (child f % 2 of coarse cell f // 2) takes its rows a' = 0..p from the rows
a' + p (f % 2) of the caller's P1 (prolong_1d[a][j], a in [0, 2p]: coarse basis j at fine patch point a), placed
at the columns (f // 2) p + j.  A fine point shared by two fine cells is built from both and must get the same
row from each: that holds for any embedding that is interpolatory at the parent's vertices, so it checks P1.

The restriction is the transpose.  Constraint semantics follow the oracle (oracle/mg_oracle_num.inc
prolongate / restrict_and_add) and deal.II's MGTransferMatrixFree:
  * with constraints, the coarse Dirichlet entries are read as 0 (prolongation) and never written
    (restriction);
  * fine values are gathered and written plain, constrained or not;
  * prolongate overwrites the fine vector, prolongate_and_add adds to it, restrict_and_add adds to the coarse one.

Nothing here reads the device library, the oracle's transfer code or their even-odd tables: the tests compare
both against this.  Not a conftest.py: tests import it explicitly."""
import numpy as np


def lagrange_embedding(nodes):
    """P1[a, j] = L_j(x_a) of the Lagrange basis on `nodes` (0 = x_0 < ... < x_p = 1) at the 2p+1 points of the
    two children, x_a = (c + nodes[k]) / 2 for a = c p + k (c = 0, 1; child 0's last point is child 1's first)"""
    x = np.asarray(nodes, dtype=np.float64)
    p = x.size - 1
    pts = np.concatenate([x / 2, (1 + x[1:]) / 2])
    P1 = np.ones((2 * p + 1, p + 1))
    for j in range(p + 1):
        for k in range(p + 1):
            if k != j:
                P1[:, j] *= (pts - x[k]) / (x[j] - x[k])
    return P1


def skewed_nodes(p, power=1.3):
    """strictly increasing nodes on [0, 1] that are not mirror-symmetric for p >= 2: x_j = (j / p)^power"""
    return (np.arange(p + 1) / p) ** power


def symmetrised(P1):
    """The embedding that the even-odd form of P1 stands for (Basis1D::P1eo as mgx_transfer_create builds it, applied
    as restrict_half / prolong_half of mgx_brick_device.hpp apply it): column j of the result is what restrict_half
    returns in o[j] for a unit fine value at point a.  Rows a < p are P1's rows, rows 2p - a their mirror images
    (P[2p - a, p - j] = P[a, j]), row p the symmetric half of P1's row p.  Equal to P1 exactly when P1 is symmetric
    under reversal of both indices."""
    P1 = np.asarray(P1, dtype=np.float64)
    p = P1.shape[1] - 1
    nh = (p + 1) // 2
    he = np.array([[0.5 * (P1[a, j] + P1[a, p - j]) for j in range(nh)] for a in range(p + 1)]).reshape(p + 1, nh)
    ho = np.array([[0.5 * (P1[a, j] - P1[a, p - j]) for j in range(nh)] for a in range(p)]).reshape(p, nh)
    R = np.zeros((p + 1, 2 * p + 1))
    for a in range(2 * p + 1):
        r = np.zeros(2 * p + 1)
        r[a] = 1.0
        re = np.array([r[b] + r[2 * p - b] for b in range(p)] + [r[p]])
        ro = np.array([r[b] - r[2 * p - b] for b in range(p)])
        o = np.zeros(p + 1)
        for j in range(nh):
            se, so = he[:, j] @ re, ho[:, j] @ ro
            o[j], o[p - j] = se + so, se - so
        if p % 2 == 0:
            o[p // 2] = P1[:p + 1, p // 2] @ re
        R[:, a] = o
    return R.T


def embedding_matrix(P1, n_coarse, majorant=False):
    """the (2 N p + 1) x (N p + 1) 1D prolongation of N coarse cells; asserts that a fine point shared by two fine
    cells gets the same row from both (majorant=True: P1 is an entrywise bound, not an embedding -- such a point takes
    the larger of the two rows)"""
    P1 = np.asarray(P1, dtype=np.float64)
    p = P1.shape[1] - 1
    assert P1.shape == (2 * p + 1, p + 1)
    M = np.zeros((2 * n_coarse * p + 1, n_coarse * p + 1))
    done = np.zeros(M.shape[0], dtype=bool)
    tol = 1e-14 * max(np.abs(P1).max(), 1.0)
    for f in range(2 * n_coarse):
        for a in range(p + 1):
            row = np.zeros(M.shape[1])
            row[(f // 2) * p:(f // 2) * p + p + 1] = P1[a + p * (f % 2)]
            if done[f * p + a] and majorant:
                M[f * p + a] = np.maximum(M[f * p + a], row)
            elif done[f * p + a]:
                assert np.abs(M[f * p + a] - row).max() <= tol, \
                    "P1 is not a consistent embedding: fine point %d differs between its two cells" % (f * p + a)
            else:
                M[f * p + a], done[f * p + a] = row, True
    assert done.all()
    return M


class LatticeTransfer:
    """Transfers between level l-1 (coarse) and level l (fine) of a structured cube.

    cells_c: coarse cells per direction (x, y, z); gid_c / gid_f: DoF -> lattice id of the two levels (dof_grid);
    constrained_c: the constrained coarse DoFs.  Vectors in and out are in the caller's DoF numbering.  majorant=True:
    P1 is an entrywise bound of an embedding (round-off bounds apply it to absolute values)."""

    def __init__(self, P1, cells_c, gid_c, gid_f, constrained_c, majorant=False):
        self.p = np.asarray(P1).shape[1] - 1
        cells = [int(c) for c in cells_c]
        self.M = [embedding_matrix(P1, n, majorant) for n in cells]   # x, y, z
        self.gc = tuple(n * self.p + 1 for n in cells[::-1])          # lattice shapes (z, y, x)
        self.gf = tuple(2 * n * self.p + 1 for n in cells[::-1])
        self.gid_c = np.asarray(gid_c, dtype=np.int64)
        self.gid_f = np.asarray(gid_f, dtype=np.int64)
        assert np.array_equal(np.sort(self.gid_c), np.arange(int(np.prod(self.gc))))
        assert np.array_equal(np.sort(self.gid_f), np.arange(int(np.prod(self.gf))))
        self.constrained_c = np.asarray(constrained_c, dtype=np.int64)

    @staticmethod
    def _lattice(v, gid, shape):
        out = np.empty(int(np.prod(shape)))
        out[gid] = v
        return out.reshape(shape)

    def _apply(self, u, transpose):
        Mx, My, Mz = (m.T if transpose else m for m in self.M)
        t = np.einsum("xa,cba->cbx", Mx, u)
        t = np.einsum("yb,cbx->cyx", My, t)
        return np.einsum("zc,cyx->zyx", Mz, t)

    def prolongate(self, coarse, fine=None, with_constraints=False):
        """P coarse (fine=None: what prolongate writes) or fine + P coarse (prolongate_and_add)"""
        c = np.array(coarse, dtype=np.float64)
        if with_constraints:
            c[self.constrained_c] = 0.0
        f = self._apply(self._lattice(c, self.gid_c, self.gc), False).ravel()[self.gid_f]
        return f if fine is None else np.asarray(fine, dtype=np.float64) + f

    def restrict_and_add(self, coarse, fine, with_constraints=False):
        """coarse + P^T fine; with constraints the constrained coarse entries keep their old values"""
        r = self._apply(self._lattice(np.asarray(fine, dtype=np.float64), self.gid_f, self.gf), True).ravel()[self.gid_c]
        if with_constraints:
            r[self.constrained_c] = 0.0
        return np.asarray(coarse, dtype=np.float64) + r
