"""CPU restatement (numpy, dense) of the DG right-hand side with Dirichlet boundary data and of the two sums of the L2
error, in two and three dimensions, on top of oracle/dg_oracle.py::DGOracle and tests/dg_reference_2d.py::DGOracle2D.

TEST INFRASTRUCTURE ONLY.  Basis (S, SD, Gauss rule, the 1D polynomials of oracle.dg_oracle.basis_1d) and geometry (the
one Jacobian) are the oracle's.  What is restated:
  * the volume term (f, phi_i) on the (p+1)-point Gauss rule (common/multigrid_solver_dg_plain.h:163-185);
  * the term boundary values g add on a Dirichlet face F.  The face-based form of the operator
    (common/laplace_operator_dg_face.h:146-157) is a_F(u, v) = int_F (sigma_F u v - d_n u v - u d_n v), so
        b_i += int_F g (sigma_F phi_i - d_n phi_i),
    in the notation of oracle/dg_oracle.py:201-203 (sigma the interior penalty, sigma_F = 2 sigma)
        upper face of direction d: (2 sigma V1 - N1)^T (W g),   lower face: (2 sigma V0 + N0)^T (W g);
  * the sums of compute_l2_error (multigrid_solver_dg_plain.h:219-259) before the square root:
        sum_K sum_q (u_h(x_q) - u(x_q))^2 JxW_q   and   sum_K sum_q JxW_q.
Vectors are the oracle's arrays, [nz, ny, nx, (p+1)^3] / [ny, nx, (p+1)^2]; functions are callables on arrays of points
[..., dim].  Real coordinates are x = origin + J (cell position + xi).
"""
import itertools

import numpy as np

from oracle import dg_oracle as dg


def kron_all(ms):
    """tensor product with the first direction fastest"""
    out = ms[0]
    for m in ms[1:]:
        out = np.kron(m, out)
    return out


class RhsReference:
    def __init__(self, oracle, origin=None):
        self.o = o = oracle
        self.dim = dim = len(o.cells)
        self.n = n = o.n
        self.J = o.J
        self.origin = np.zeros(dim) if origin is None else np.asarray(origin, dtype=float)
        self.det = abs(np.linalg.det(o.J))
        polys = dg.basis_1d(o.p, o.kind)
        b = [np.array([[float(f(s)) for f in polys]]) for s in (0.0, 1.0)]
        g = [np.array([[float(f.d(s)) for f in polys]]) for s in (0.0, 1.0)]
        self.Sd = kron_all([o.S] * dim)                      # coefficients -> values in the Gauss points
        self.Wd = kron_all([o.wq] * dim) * self.det          # JxW
        # reference coordinates of the Gauss points of a cell, x fastest
        self.ref = np.array([idx[::-1] for idx in itertools.product(o.xq, repeat=dim)])
        inv = np.linalg.inv(o.J)
        self.face = {}
        for d in range(dim):
            nrm = np.linalg.norm(inv[d])
            c = (inv @ inv.T)[d] / nrm                       # n . grad xi_a, n towards +xi_d
            sigma = dg.PENALTY_FACTOR * n * n * abs(c[d])
            W = kron_all([o.wq] * (dim - 1)) * self.det * nrm
            for s in (0, 1):
                V = kron_all([b[s] if a == d else o.S for a in range(dim)])
                N = sum(c[e] * kron_all([(g[s] if e == d else b[s]) if a == d else (o.SD if a == e else o.S) for a in range(dim)])
                        for e in range(dim))
                T = (2 * sigma * V - N) if s else (2 * sigma * V + N)   # the test side: sigma_F phi - d_n phi
                # reference coordinates of the face's Gauss points, the lower remaining direction fastest
                pts = np.array([idx[::-1] for idx in itertools.product(o.xq, repeat=dim - 1)]).reshape(-1, dim - 1)
                ref = np.insert(pts, d, float(s), axis=1)
                self.face[2 * d + s] = (T, W, ref)

    # ---------------------------------------------------------------- points
    def cell_positions(self):
        """all cell positions (i, j[, k]) in the oracle's order (x fastest)"""
        return [idx[::-1] for idx in itertools.product(*[range(c) for c in self.o.cells[::-1]])]

    def _at(self, pos):
        return tuple(pos[::-1])

    def points(self, pos, ref):
        return self.origin + (np.asarray(pos, dtype=float) + ref) @ self.J.T

    def dirichlet_faces(self, pos):
        return [2 * d + s for d in range(self.dim) for s in (0, 1) if pos[d] == (self.o.cells[d] - 1 if s else 0)]

    # ---------------------------------------------------------------- sampled functions
    def sample_cells(self, fn):
        """[cells..., (p+1)^dim]: values in the Gauss points"""
        out = np.empty(self.o.shape)
        for pos in self.cell_positions():
            out[self._at(pos)] = fn(self.points(pos, self.ref))
        return out

    def sample_faces(self, fn):
        """[cells..., 2 dim, (p+1)^(dim-1)]: values in the Gauss points of every face"""
        out = np.empty(self.o.shape[:-1] + (2 * self.dim, self.n ** (self.dim - 1)))
        for pos in self.cell_positions():
            for f in range(2 * self.dim):
                out[self._at(pos)][f] = fn(self.points(pos, self.face[f][2]))
        return out

    # ---------------------------------------------------------------- the three quantities
    def load_vector(self, fn):
        """(f, phi_i) on the Gauss rule"""
        return (self.sample_cells(fn) * self.Wd) @ self.Sd

    def boundary_load(self, fn):
        """sum over the Dirichlet faces of int_F g (sigma_F phi_i - d_n phi_i)"""
        out = np.zeros(self.o.shape)
        for pos in self.cell_positions():
            for f in self.dirichlet_faces(pos):
                T, W, ref = self.face[f]
                out[self._at(pos)] += T.T @ (W * fn(self.points(pos, ref)))
        return out

    def l2_sums(self, vec, fn):
        uh = np.asarray(vec, dtype=float).reshape(self.o.shape) @ self.Sd.T
        return np.array([float(np.sum(self.Wd * (uh - self.sample_cells(fn)) ** 2)), float(self.Wd.sum() * np.prod(self.o.cells))])

    def dense_matrix(self):
        """the oracle's operator assembled from its blocks (its own dense_matrix applies vmult to every unit vector)"""
        o, dim, m = self.o, self.dim, self.n ** self.dim
        cells = self.cell_positions()
        index = {pos: i for i, pos in enumerate(cells)}
        A = np.zeros((len(cells) * m, len(cells) * m))
        for pos, i in index.items():
            blk = o.A_vol.copy()
            for d in range(dim):
                B = o.blocks[d]
                blk += B["bl"] if pos[d] == 0 else B["pp"]
                blk += B["bu"] if pos[d] == o.cells[d] - 1 else B["mm"]
                if pos[d] + 1 < o.cells[d]:
                    j = index[pos[:d] + (pos[d] + 1,) + pos[d + 1:]]
                    A[i * m:(i + 1) * m, j * m:(j + 1) * m] = B["mp"]
                    A[j * m:(j + 1) * m, i * m:(i + 1) * m] = B["pm"]
            A[i * m:(i + 1) * m, i * m:(i + 1) * m] = blk
        return A

    def l2_error(self, vec, fn):
        s = self.l2_sums(vec, fn)
        return float(np.sqrt(s[0] / s[1]))

    def interpolate(self, fn):
        """coefficients of the L2 projection of fn (exact for polynomials of degree <= p per direction)"""
        o = self.o
        mass = o.S.T @ (o.wq[:, None] * o.S)
        P = np.linalg.solve(mass, o.S.T * o.wq)              # Gauss values -> coefficients, 1D
        return self.sample_cells(fn) @ kron_all([P] * self.dim).T


# L2 errors of the dense solves of tests/test_dg_rhs_reference.py (prod sin(3 pi x_d) on [-0.9, 1]^2, Hermite-like basis,
# p = 3, right-hand side with the boundary term) on 4^2, 8^2 and 16^2 cells; that test recomputes and pins them
DENSE_ERRORS_2D_P3 = (0.02559751456769861, 0.002810859276393028, 0.00025447977405535264)
