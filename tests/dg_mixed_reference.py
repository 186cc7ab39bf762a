"""CPU restatement (numpy, dense) of the DG-SIP operator with mixed Dirichlet / Neumann boundaries, on top of the
existing oracles: oracle/dg_oracle.py::DGOracle, tests/dg_reference_2d.py::DGOracle2D, the plain multigrid oracles of
tests/dg_plain_reference.py and tests/dg_reference_2d.py, and tests/dg_rhs_reference.py::RhsReference.

TEST INFRASTRUCTURE ONLY.  In the face-based form the oracles restate (oracle/dg_oracle.py:196-204) a boundary face
that contributes nothing to the bilinear form is a Neumann face: fresh oracle instances get the boundary blocks
blocks[d]["bl"] / ["bu"] of the Neumann sides replaced by zero, and everything the oracles derive from the blocks
(vmult, own_block and with it JacobiTransformed, the dense matrix, the multigrid) follows.  The datum h = d_n u of a
Neumann face F enters the right-hand side as int_F h phi_i (neumann_load).

Sides are face numbers 2d + s: direction d, lower (s = 0) or upper (s = 1) side of the box.
"""
import copy
import itertools

import numpy as np

from oracle import dg_oracle as dg

import dg_plain_reference as plain
import dg_reference_2d as ref2
import dg_rhs_reference as rr

INTERIOR, DIRICHLET, NEUMANN = "I", "D", "N"


def mark_neumann(oracle, sides):
    """the Neumann sides of a fresh oracle: their boundary blocks become zero"""
    sides = tuple(sorted(set(int(f) for f in sides)))
    assert all(0 <= f < 2 * len(oracle.cells) for f in sides)
    for f in sides:
        B = oracle.blocks[f // 2]
        key = "bu" if f % 2 else "bl"
        B[key] = np.zeros_like(B[key])
    oracle._diag_cache = {}
    oracle.neumann_sides = sides
    return oracle


def mixed_oracle(degree, kind, cells, jacobian, sides):
    cls = dg.DGOracle if len(cells) == 3 else ref2.DGOracle2D
    return mark_neumann(cls(degree, kind, cells, jacobian), sides)


def derived_oracle(base, cells, sides):
    """a fresh oracle on another box with the same degree, basis and Jacobian as `base` (an unmarked oracle, left
    unchanged): the blocks, the 1D data and the eigenvectors do not depend on the box, so they are shared, not rebuilt"""
    assert not getattr(base, "neumann_sides", ())
    o = copy.copy(base)
    o.cells = tuple(cells)
    o.shape = tuple(cells)[::-1] + (base.shape[-1],)
    o.blocks = {d: dict(B) for d, B in base.blocks.items()}
    return mark_neumann(o, sides)


def side_kinds(cells, sides):
    """the set of (lower kind, upper kind) pairs the cells of a box reach, per direction"""
    out = []
    for d, n in enumerate(cells):
        lo_b = NEUMANN if 2 * d in sides else DIRICHLET
        up_b = NEUMANN if 2 * d + 1 in sides else DIRICHLET
        out.append({(lo_b if i == 0 else INTERIOR) + (up_b if i == n - 1 else INTERIOR) for i in range(n)})
    return out


def neighbour_kinds(cells, sides, positions):
    """numpy marking of a box's neighbour table: [n, 2 dim] of 0 (a cell behind the face), -1 (Dirichlet), -2 (Neumann)"""
    pos = np.asarray(positions)
    out = np.zeros((pos.shape[0], 2 * len(cells)), dtype=np.int32)
    for d, n in enumerate(cells):
        out[pos[:, d] == 0, 2 * d] = -2 if 2 * d in sides else -1
        out[pos[:, d] == n - 1, 2 * d + 1] = -2 if 2 * d + 1 in sides else -1
    return out


def own_block_of_kinds(oracle, kinds):
    """A_KK of a cell of an all-Dirichlet oracle whose face 2d+s is of kind kinds[2d+s]"""
    A = oracle.A_vol.copy()
    for d in range(len(oracle.cells)):
        B = oracle.blocks[d]
        lo, up = kinds[2 * d], kinds[2 * d + 1]
        A += {INTERIOR: B["pp"], DIRICHLET: B["bl"], NEUMANN: 0.0 * B["bl"]}[lo]
        A += {INTERIOR: B["mm"], DIRICHLET: B["bu"], NEUMANN: 0.0 * B["bu"]}[up]
    return A


def transformed_diagonal(oracle, kinds):
    T = oracle.T3 if len(oracle.cells) == 3 else oracle.T2
    return np.einsum("ij,ij->j", T, own_block_of_kinds(oracle, kinds) @ T)


class MixedRhsReference(rr.RhsReference):
    """RhsReference of an oracle made by mixed_oracle: Dirichlet data on the Dirichlet sides only, plus neumann_load"""

    def __init__(self, oracle, origin=None):
        super().__init__(oracle, origin)
        o, dim = oracle, self.dim
        self.sides = tuple(getattr(oracle, "neumann_sides", ()))
        polys = dg.basis_1d(o.p, o.kind)
        b = [np.array([[float(f(s)) for f in polys]]) for s in (0.0, 1.0)]
        inv = np.linalg.inv(o.J)
        self.trace, self.normal = {}, {}
        for d in range(dim):
            for s in (0, 1):
                self.trace[2 * d + s] = rr.kron_all([b[s] if a == d else o.S for a in range(dim)])
                self.normal[2 * d + s] = (1.0 if s else -1.0) * inv[d] / np.linalg.norm(inv[d])   # outward, unit

    def boundary_faces(self, pos):
        return super().dirichlet_faces(pos)

    def dirichlet_faces(self, pos):
        return [f for f in self.boundary_faces(pos) if f not in self.sides]

    def neumann_faces(self, pos):
        return [f for f in self.boundary_faces(pos) if f in self.sides]

    def sample_flux(self, grad):
        """[cells..., 2 dim, (p+1)^(dim-1)]: n . grad u in the Gauss points of every face, n its outward normal"""
        out = np.empty(self.o.shape[:-1] + (2 * self.dim, self.n ** (self.dim - 1)))
        for pos in self.cell_positions():
            for f in range(2 * self.dim):
                out[self._at(pos)][f] = grad(self.points(pos, self.face[f][2])) @ self.normal[f]
        return out

    def neumann_load(self, grad):
        """sum over the Neumann faces of int_F (n . grad u) phi_i; grad: points [..., dim] -> gradients [..., dim]"""
        out = np.zeros(self.o.shape)
        for pos in self.cell_positions():
            for f in self.neumann_faces(pos):
                _, W, ref = self.face[f]
                out[self._at(pos)] += self.trace[f].T @ (W * (grad(self.points(pos, ref)) @ self.normal[f]))
        return out


class MixedPlainOracle(plain.DGPlainOracle):
    """DGPlainOracle whose levels all have the same Neumann sides (marked before the eigenvalue estimates)"""

    def __init__(self, degree, kind, coarse_cells, jacobian0, n_levels, sides, degree_pre=3):
        self.p, self.kind, self.n_levels, self.degree_pre = degree, kind, n_levels, degree_pre
        jac0 = np.asarray(jacobian0, dtype=float).reshape(3, 3)
        self.level = [mixed_oracle(degree, kind, tuple(int(c) << l for c in coarse_cells), jac0 / 2 ** l, sides)
                      for l in range(n_levels)]
        self.P = plain.embedding_1d(degree, kind)
        self.P3 = [dg.kron3(self.P[k & 1], self.P[(k >> 1) & 1], self.P[k >> 2]) for k in range(8)]
        self.info = [self._estimate(l) for l in range(n_levels)]


class MixedPlainOracle2D(ref2.DGPlainOracle2D):
    def __init__(self, degree, kind, coarse_cells, jacobian0, n_levels, sides, degree_pre=3):
        self.p, self.kind, self.n_levels, self.degree_pre = degree, kind, n_levels, degree_pre
        jac0 = np.asarray(jacobian0, dtype=float).reshape(2, 2)
        self.level = [mixed_oracle(degree, kind, tuple(int(c) << l for c in coarse_cells), jac0 / 2 ** l, sides)
                      for l in range(n_levels)]
        self.P = plain.embedding_1d(degree, kind)
        self.P2 = [ref2.kron2(self.P[k & 1], self.P[k >> 1]) for k in range(4)]
        self.info = [self._estimate(l) for l in range(n_levels)]


def all_kind_combinations(dim):
    return itertools.product((INTERIOR, DIRICHLET, NEUMANN), repeat=2 * dim)


# L2 errors of the dense solves of tests/test_dg_mixed_reference.py (prod sin(3 pi x_d) on [-0.9, 1]^2, Hermite-like
# basis, p = 3, lower-x and upper-y sides Neumann with the exact flux) on 4^2, 8^2 and 16^2 cells; that test recomputes
# and pins them
DENSE_NEUMANN_SIDES_2D = (0, 3)
DENSE_ERRORS_MIXED_2D_P3 = (3.008600e-2, 3.040566e-3, 2.607593e-4)
