"""CPU restatement (numpy, dense) of the symmetric-interior-penalty DG Laplace operator, its block-Jacobi
preconditioner in the eigenvector basis, the merged Chebyshev update and MultigridSolverDGPlain in TWO dimensions:
oracle/dg_oracle.py::DGOracle and tests/dg_plain_reference.py::DGPlainOracle one dimension down.

TEST INFRASTRUCTURE ONLY.  What is restated, and from where: as in oracle/dg_oracle.py (the face-by-face bilinear form
of common/laplace_operator_dg_face.h:66-160, JacobiTransformed laplace_operator_dg.h:2028-2256, the merged Chebyshev
step :910-955) with dim = 2, the dimension poisson_dg_plain/program.cc:65 runs.  The 1D bases are the 3D oracle's
(oracle.dg_oracle.basis_1d).  tests/test_dg_reference_2d.py pins this file against the 3D oracle (extrusion) and
against basis-independent properties.
"""
import numpy as np
import scipy.linalg

from oracle import dg_oracle as dg
from dg_plain_reference import DGPlainOracle, embedding_1d

PENALTY_FACTOR = dg.PENALTY_FACTOR


def kron2(mx, my):
    """local index (j, i), i fastest along x"""
    return np.kron(my, mx)


class DGOracle2D:
    """vectors are arrays [ny, nx, (p+1)^2] over cells in lexicographic order, x fastest, all outer faces Dirichlet
    (homogeneous), one Jacobian for all cells"""

    def __init__(self, degree, kind, cells, jacobian):
        self.p, self.kind = degree, kind
        self.n = n = degree + 1
        self.cells = tuple(cells)
        nx, ny = self.cells
        self.shape = (ny, nx, n ** 2)
        self.J = np.asarray(jacobian, dtype=float).reshape(2, 2)
        polys = dg.basis_1d(degree, kind)
        xq, wq = dg.gauss01(n)
        S = np.array([f(xq) for f in polys]).T             # values at Gauss points [q, i]
        SD = np.array([f.d(xq) for f in polys]).T           # derivatives there
        b = [np.array([[float(f(s)) for f in polys]]) for s in (0.0, 1.0)]
        g = [np.array([[float(f.d(s)) for f in polys]]) for s in (0.0, 1.0)]
        self.S, self.SD, self.xq, self.wq, self.b, self.g = S, SD, xq, wq, b, g
        self.hermite_derivative_on_face = float(polys[0].d(0.0))
        inv = np.linalg.inv(self.J)             # row a = grad xi_a
        det = abs(np.linalg.det(self.J))
        K = det * inv @ inv.T
        W2 = np.kron(wq, wq)
        grads = [kron2(SD, S), kron2(S, SD)]
        self.A_vol = sum(K[a, c] * grads[a].T @ (W2[:, None] * grads[c]) for a in range(2) for c in range(2))

        def trace_ops(d, s):
            """value and the two reference derivatives in the Gauss points of the face s of direction d"""
            def op(normal_derivative, deriv_dir):
                m = []
                for a in range(2):
                    if a == d:
                        m.append(g[s] if normal_derivative else b[s])
                    else:
                        m.append(SD if a == deriv_dir else S)
                return kron2(*m)
            return op(False, -1), [op(a == d, a) for a in range(2)]

        self.blocks, self.penalty = {}, []
        for d in range(2):
            nrm = np.linalg.norm(inv[d])
            c = (inv @ inv.T)[d] / nrm               # n . grad xi_a, n pointing towards +xi_d
            W = (wq * det * nrm)[:, None]
            sigma = PENALTY_FACTOR * n * n * abs(c[d])
            self.penalty.append(sigma)
            V0, G0 = trace_ops(d, 0)
            V1, G1 = trace_ops(d, 1)
            N0 = sum(c[a] * G0[a] for a in range(2))
            N1 = sum(c[a] * G1[a] for a in range(2))
            # interior face between - (its upper face) and + (its lower face), normal from - to +
            mm = V1.T @ (W * (sigma * V1 - 0.5 * N1)) - 0.5 * N1.T @ (W * V1)
            mp = V1.T @ (W * (-sigma * V0 - 0.5 * N0)) + 0.5 * N1.T @ (W * V0)
            pm = -V0.T @ (W * (sigma * V1 - 0.5 * N1)) - 0.5 * N0.T @ (W * V1)
            pp = V0.T @ (W * (sigma * V0 + 0.5 * N0)) + 0.5 * N0.T @ (W * V0)
            # Dirichlet faces: sigma_F = 2 sigma, outward normal +n on the upper and -n on the lower face
            bu = V1.T @ (W * (2 * sigma * V1 - N1)) - N1.T @ (W * V1)
            bl = V0.T @ (W * (2 * sigma * V0 + N0)) + N0.T @ (W * V0)
            self.blocks[d] = dict(mm=mm, mp=mp, pm=pm, pp=pp, bu=bu, bl=bl)

        # JacobiTransformed: 1D generalised eigenvectors (laplace_operator_dg.h:179-215)
        mass = S.T @ (wq[:, None] * S)
        lapl = SD.T @ (wq[:, None] * SD)
        pen = n * n * PENALTY_FACTOR
        lapl = lapl + pen * b[0].T @ b[0] + 0.5 * (g[0].T @ b[0] + b[0].T @ g[0])
        lapl = lapl + pen * b[1].T @ b[1] - 0.5 * (g[1].T @ b[1] + b[1].T @ g[1])
        self.eigenvalues_1d, T = scipy.linalg.eigh(lapl, mass)
        self.T = T
        self.T2 = kron2(T, T)
        self._diag_cache = {}

    # ---------------------------------------------------------------- operator
    def own_block(self, lower, upper):
        """A_KK of a cell whose lower/upper faces in direction d are Dirichlet where flagged"""
        A = self.A_vol.copy()
        for d in range(2):
            B = self.blocks[d]
            A += B["bl"] if lower[d] else B["pp"]
            A += B["bu"] if upper[d] else B["mm"]
        return A

    def _slices(self, d, lo, hi):
        # arrays are [y, x, dof]: axis of direction d is 1 - d
        s = [slice(None)] * 3
        s[1 - d] = slice(lo, hi)
        return tuple(s)

    def vmult(self, x):
        x = np.asarray(x, dtype=float).reshape(self.shape)
        y = x @ self.A_vol.T
        for d in range(2):
            B = self.blocks[d]
            N = self.cells[d]
            first, last = self._slices(d, 0, 1), self._slices(d, N - 1, N)
            lower, upper = self._slices(d, 0, N - 1), self._slices(d, 1, N)
            y[first] += x[first] @ B["bl"].T
            y[last] += x[last] @ B["bu"].T
            if N > 1:
                y[lower] += x[lower] @ B["mm"].T + x[upper] @ B["mp"].T
                y[upper] += x[upper] @ B["pp"].T + x[lower] @ B["pm"].T
        return y

    def dense_matrix(self):
        n = int(np.prod(self.shape))
        A = np.empty((n, n))
        e = np.zeros(n)
        for i in range(n):
            e[i] = 1.0
            A[:, i] = self.vmult(e).ravel()
            e[i] = 0.0
        return A

    # ---------------------------------------------------------------- block Jacobi
    def inverse_diagonal(self, lower, upper):
        key = (tuple(lower), tuple(upper))
        if key not in self._diag_cache:
            A = self.own_block(lower, upper)
            self._diag_cache[key] = 1.0 / np.einsum("ij,ij->j", self.T2, A @ self.T2)
        return self._diag_cache[key]

    def jacobi_vmult(self, r):
        r = np.asarray(r, dtype=float).reshape(self.shape)
        t = r @ self.T2                      # T^T r
        nx, ny = self.cells
        for j in range(ny):
            for i in range(nx):
                idx = (i, j)
                lower = [idx[d] == 0 for d in range(2)]
                upper = [idx[d] == self.cells[d] - 1 for d in range(2)]
                t[j, i] *= self.inverse_diagonal(lower, upper)
        return t @ self.T2.T

    # ---------------------------------------------------------------- merged Chebyshev step
    def vmult_with_chebyshev_update(self, rhs, iteration_index, factor1, factor2, solution, solution_old):
        """returns (solution, solution_old) after the call, including the swap of :931"""
        rhs = np.asarray(rhs, dtype=float).reshape(self.shape)
        if iteration_index == 0:
            return factor2 * self.jacobi_vmult(rhs), solution_old
        solution = np.asarray(solution, dtype=float).reshape(self.shape)
        solution_old = np.asarray(solution_old, dtype=float).reshape(self.shape)
        z = self.jacobi_vmult(rhs - self.vmult(solution))
        new = factor2 * z + (1.0 + factor1) * solution
        if iteration_index > 1:
            new = new - factor1 * solution_old
        return new, solution

    # ---------------------------------------------------------------- helpers for the tests
    def _points(self):
        n = self.n
        return np.array([[self.xq[i], self.xq[j]] for j in range(n) for i in range(n)])

    def interpolate(self, fn):
        """coefficients of the L2 projection of fn (exact for polynomials of degree <= p per direction)"""
        nx, ny = self.cells
        mass = self.S.T @ (self.wq[:, None] * self.S)
        P = np.linalg.solve(mass, self.S.T * self.wq)   # Gauss values -> coefficients, 1D
        P2 = kron2(P, P)
        out = np.empty(self.shape)
        q = self._points()
        for j in range(ny):
            for i in range(nx):
                out[j, i] = P2 @ fn((q + np.array([i, j])) @ self.J.T)
        return out

    def load_vector(self, fn):
        """(f, phi_i) with Gauss quadrature"""
        nx, ny = self.cells
        S2 = kron2(self.S, self.S)
        W2 = np.kron(self.wq, self.wq) * abs(np.linalg.det(self.J))
        q = self._points()
        out = np.empty(self.shape)
        for j in range(ny):
            for i in range(nx):
                out[j, i] = S2.T @ (W2 * fn((q + np.array([i, j])) @ self.J.T))
        return out


class DGPlainOracle2D(DGPlainOracle):
    """tests/dg_plain_reference.py::DGPlainOracle with DGOracle2D levels and four children per cell; the eigenvalue
    estimate, the smoother, the V-cycle, the outer CG and vmult_with_residual_update are inherited: nothing in them
    knows the dimension."""

    def __init__(self, degree, kind, coarse_cells, jacobian0, n_levels, degree_pre=3):
        self.p, self.kind, self.n_levels, self.degree_pre = degree, kind, n_levels, degree_pre
        jac0 = np.asarray(jacobian0, dtype=float).reshape(2, 2)
        self.level = [DGOracle2D(degree, kind, tuple(int(c) << l for c in coarse_cells), jac0 / 2 ** l)
                      for l in range(n_levels)]
        self.P = embedding_1d(degree, kind)
        # child kx + 2 ky
        self.P2 = [kron2(self.P[k & 1], self.P[k >> 1]) for k in range(4)]
        self.info = [self._estimate(l) for l in range(n_levels)]

    def prolongate(self, l, coarse):
        c = np.asarray(coarse, dtype=float).reshape(self.level[l - 1].shape)
        fine = np.zeros(self.level[l].shape)
        for k in range(4):
            fine[(k >> 1)::2, (k & 1)::2] = c @ self.P2[k].T
        return fine

    def restrict(self, l, fine):
        f = np.asarray(fine, dtype=float).reshape(self.level[l].shape)
        return sum(f[(k >> 1)::2, (k & 1)::2] @ self.P2[k] for k in range(4))


def to_cell_order(a, ij):
    """oracle array [ny, nx, dofs] -> [n_cells, dofs] in the cell order whose positions are ij ([n, 2])"""
    return np.ascontiguousarray(a[ij[:, 1], ij[:, 0]])


def from_cell_order(v, ij, cells, n_loc):
    out = np.empty((cells[1], cells[0], n_loc))
    out[ij[:, 1], ij[:, 0]] = np.asarray(v).reshape(-1, n_loc)
    return out
