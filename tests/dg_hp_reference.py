"""CPU restatement (numpy, dense) of the plain DG multigrid on a level sequence that mixes mesh refinements and degree
raises (include/mgx_dg.h: mgx_dg_degree_embedding, mgx_dg_degree_transfer_*, mgx_dg_hp_solver_create), on top of
tests/dg_plain_reference.py and tests/dg_reference_2d.py.

TEST INFRASTRUCTURE ONLY.  A hierarchy is a list of (degree, refinement) pairs from coarsest to finest; level l lives on
coarse_cells * 2^refinement cells with the Jacobian jacobian0 / 2^refinement and is a rediscretisation with its own
degree and penalty.  Only the two transfers know what kind of step lies between two levels; the eigenvalue estimates,
the smoothers, the V-cycle, the outer CG and vmult_with_residual_update are those of DGPlainOracle, inherited untouched.
"""
import numpy as np

from oracle import dg_oracle as dg

import dg_plain_reference as plain
import dg_reference_2d as ref2


def degree_embedding_1d(pf, pc, kind):
    """E[i, j]: coefficient i, in the basis of degree pf, of the function j of the basis of degree pc on the same cell,
    by interpolation in pf + 1 Gauss-Lobatto points (the spaces are nested: any unisolvent set of points gives the same
    matrix)"""
    assert 1 <= pc < pf
    fine, coarse = dg.basis_1d(pf, kind), dg.basis_1d(pc, kind)
    x = dg.gauss_lobatto01(pf + 1)
    B = np.array([f(x) for f in fine]).T        # B[q, i] = phi^f_i(x_q)
    V = np.array([f(x) for f in coarse]).T      # V[q, j] = phi^c_j(x_q)
    return np.linalg.solve(B, V)


def embedding_nd(E, dim):
    """the embedding of a cell: E (x) E (x) E, local index x fastest (dim 2: E (x) E)"""
    return dg.kron3(E, E, E) if dim == 3 else ref2.kron2(E, E)


class DGHPOracle(plain.DGPlainOracle):
    """DGPlainOracle on a hierarchy of (degree, refinement) pairs; a 2-tuple of coarse_cells gives the 2D oracle, an
    instance of DGHPOracle2D (a DGHPOracle and a DGPlainOracle2D)"""

    dim = 3

    def __new__(cls, kind, hierarchy, coarse_cells, *args, **kwargs):
        return object.__new__(DGHPOracle2D if cls is DGHPOracle and len(coarse_cells) == 2 else cls)

    def __init__(self, kind, hierarchy, coarse_cells, jacobian0, degree_pre=3, neumann_sides=()):
        """neumann_sides: sides 2d+s of the box that are Neumann faces on every level, marked as
        tests/dg_mixed_reference.py marks its oracles (before the eigenvalue estimates)"""
        dim = self.dim
        assert len(coarse_cells) == dim
        self.hierarchy = [(int(p), int(r)) for p, r in hierarchy]
        self.kind, self.n_levels, self.degree_pre = kind, len(self.hierarchy), degree_pre
        self.p = self.hierarchy[-1][0]
        assert self.hierarchy[0][1] == 0
        jac0 = np.asarray(jacobian0, dtype=float).reshape(dim, dim)
        level_oracle = dg.DGOracle if dim == 3 else ref2.DGOracle2D
        self.level = [level_oracle(p, kind, tuple(int(c) << r for c in coarse_cells), jac0 / 2 ** r) for p, r in self.hierarchy]
        if neumann_sides:
            from dg_mixed_reference import mark_neumann
            for o in self.level:
                mark_neumann(o, neumann_sides)
        # per step from level l - 1 to level l: ("h", the 2^dim child embeddings of the parent) or ("p", E (x) ... (x) E)
        self.step = [None]
        for (pc, rc), (pf, rf) in zip(self.hierarchy[:-1], self.hierarchy[1:]):
            if pf == pc and rf == rc + 1:
                P = plain.embedding_1d(pf, kind)
                if dim == 3:
                    self.step.append(("h", [dg.kron3(P[k & 1], P[(k >> 1) & 1], P[k >> 2]) for k in range(8)]))
                else:
                    self.step.append(("h", [ref2.kron2(P[k & 1], P[k >> 1]) for k in range(4)]))
            else:
                assert pf > pc and rf == rc, "a step refines the mesh once or raises the degree"
                self.step.append(("p", embedding_nd(degree_embedding_1d(pf, pc, kind), dim)))
        self.info = [self._estimate(l) for l in range(self.n_levels)]

    def _children(self, l):
        """the parent class's transfers read the child embeddings of the step as self.P3 (self.P2 in 2D)"""
        setattr(self, "P3" if self.dim == 3 else "P2", self.step[l][1])

    def prolongate(self, l, coarse):
        kind, M = self.step[l]
        if kind == "h":
            self._children(l)
            return super().prolongate(l, coarse)
        return np.asarray(coarse, dtype=float).reshape(self.level[l - 1].shape) @ M.T

    def restrict(self, l, fine):
        kind, M = self.step[l]
        if kind == "h":
            self._children(l)
            return super().restrict(l, fine)
        return np.asarray(fine, dtype=float).reshape(self.level[l].shape) @ M


class DGHPOracle2D(DGHPOracle, ref2.DGPlainOracle2D):
    dim = 2


# the solver cases of tests/test_gpu_dg_hp.py (tests/test_dg_hp_reference.py checks that the reference converges on
# them): name -> (basis, coarse cells, hierarchy, Jacobian of a coarse cell)
SHEARED_3D = dg.cheby_mesh(0)[1]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
SOLVER_CASES = {
    "3d-p-sheared": (dg.GAUSS_LOBATTO, (2, 2, 1), [(1, 0), (2, 0), (3, 0)], SHEARED_3D),
    "3d-p": (dg.HERMITE, (3, 1, 1), [(1, 0), (2, 0), (4, 0)], np.eye(3) * 0.7),
    "3d-hp": (dg.GAUSS, (3, 2, 1), [(1, 0), (3, 0), (3, 1)], np.eye(3) * 0.7),
    "3d-ph-sheared": (dg.HERMITE, (2, 1, 1), [(1, 0), (1, 1), (2, 1), (5, 1)], SHEARED_3D),
    "2d-hp": (dg.HERMITE, (3, 2), [(1, 0), (2, 0), (4, 0), (4, 1)], np.eye(2) * 0.7),
    "2d-ph-sheared": (dg.GAUSS_LOBATTO, (2, 1), [(1, 0), (1, 1), (3, 1)], SHEARED_2D),
}
NEUMANN_CASE, NEUMANN_SIDES = "3d-hp", (1,)
_solved = {}


def solved_case(name, neumann_sides=()):
    """the numpy solver of a case with what the tests compare against, computed once and left unchanged"""
    key = (name, tuple(neumann_sides))
    if key not in _solved:
        kind, cells, hierarchy, jac = SOLVER_CASES[name]
        o = DGHPOracle(kind, hierarchy, cells, jac, neumann_sides=neumann_sides)
        shape = o.level[-1].shape
        rng = np.random.default_rng(7)
        x, rhs, upd = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
        out = dict(o=o, shape=shape, x=x, rhs=rhs, upd=upd, vcycle=o.v_cycle(x), cg=o.solve_cg(rhs, 1e-9))
        out["update0"] = o.vmult_with_residual_update(rhs, upd, 0.0)
        out["update1"] = o.vmult_with_residual_update(rhs, upd, -0.37)
        _solved[key] = out
    return _solved[key]
