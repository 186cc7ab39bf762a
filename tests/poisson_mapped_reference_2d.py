"""numpy restatement of a linear problem -div(a grad u) = f with Dirichlet values on a Square, curved ones included
(include/mgx_square.h, mgx_square_problem; include/mgx.h, mgx_compute_residual_2d / mgx_compute_l2_error_2d): quadrature
points, the four provider arrays, the right-hand side with the boundary lifting, the two error sums and a dense solve --
from the index tables, the 1D arrays and the NODES of the cells only.  The geometry and the operator are those of
nonlinear_reference_2d.NonlinearReference2D (apply, matrix); the functions of the two problems are written out here.
test_poisson_mapped_reference_2d.py pins it, test_gpu_poisson_mapped_2d.py compares the device against it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

from nonlinear_reference_2d import NonlinearReference2D

PI = np.pi


class Problem:
    """kind "cube": u = sin(3 pi x) sin(3 pi y), a = 1; "shell": u = sin(2 pi (x + y)), a = 1 + contrast cos^2(2 pi x)
    cos^2(2 pi y + 0.1); f = -(a lap u + grad a . grad u)"""

    def __init__(self, kind, contrast=0.0):
        assert kind in ("cube", "shell")
        self.kind, self.contrast = kind, float(contrast)

    def u(self, x, y):
        if self.kind == "cube":
            return np.sin(3 * PI * x) * np.sin(3 * PI * y)
        return np.sin(2 * PI * (x + y))

    def a(self, x, y):
        if self.kind == "cube":
            return np.ones_like(x)
        return 1.0 + self.contrast * np.cos(2 * PI * x) ** 2 * np.cos(2 * PI * y + 0.1) ** 2

    def f(self, x, y):
        if self.kind == "cube":
            return 2 * (3 * PI) ** 2 * self.u(x, y)
        c0, s0 = np.cos(2 * PI * x), np.sin(2 * PI * x)
        c1, s1 = np.cos(2 * PI * y + 0.1), np.sin(2 * PI * y + 0.1)
        lap = -2 * (2 * PI) ** 2 * np.sin(2 * PI * (x + y))
        du = 2 * PI * np.cos(2 * PI * (x + y))
        ax = self.contrast * (-4 * PI * c0 * s0) * c1 ** 2
        ay = self.contrast * c0 ** 2 * (-4 * PI * c1 * s1)
        return -(lap * self.a(x, y) + (ax + ay) * du)


class PoissonMappedReference2D:
    """one level of a Square: p, the 1D arrays, idx9 / idx9_plain, n_dofs, constrained (the provider's list, whose order
    the boundary values follow) and nodes [n_cells, (p+1)^2, 2]"""

    def __init__(self, p, shape_values, colloc_grad, qweights, idx9, idx9_plain, n_dofs, constrained, nodes):
        n = p + 1
        self.ref = NonlinearReference2D(p, shape_values, colloc_grad, qweights, idx9, idx9_plain, n_dofs, nodes, affine=False)
        r = self.ref
        S = np.asarray(shape_values, dtype=np.float64).reshape(n, n)
        self.S2 = np.kron(S, S)  # rows q = qy n + qx, columns the nodes j n + i
        nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, n * n, 2)
        self.x_q = np.einsum("qi,cia->cqa", self.S2, nodes)
        self.constrained = np.asarray(constrained, dtype=np.int64)
        assert np.array_equal(np.sort(self.constrained), r.constrained)
        self.dof_xy = np.empty((r.n_dofs, 2))
        self.dof_xy[r.dofs_plain] = nodes
        self.jxw_q = r.w

    @classmethod
    def from_square(cls, sq, level):
        return cls(sq.degree, sq.shape_values(), sq.colloc_grad(), sq.qweights(), sq.idx9(level), sq.idx9_plain(level),
                   sq.n_dofs(level), sq.constrained(level), sq.cell_nodes(level))

    # ---- the four provider arrays ----
    def coef_q(self, problem):
        return problem.a(self.x_q[..., 0], self.x_q[..., 1])[:, None, :] * self.ref.U

    def rhs_quadrature(self, problem):
        return problem.f(self.x_q[..., 0], self.x_q[..., 1]) * self.jxw_q

    def solution_q(self, problem):
        return problem.u(self.x_q[..., 0], self.x_q[..., 1])

    def bc_value(self, problem):
        xy = self.dof_xy[self.constrained]
        return problem.u(xy[:, 0], xy[:, 1])

    def boundary_vector(self, problem):
        u = np.zeros(self.ref.n_dofs)
        u[self.constrained] = self.bc_value(problem)
        return u

    # ---- right-hand side and lifting ----
    def residual(self, coef, src=None, rhs_q=None, reverse=False, dtype=np.float64):
        """compute_residual: sum over the cells of S^T rhs_q - G^T (coef G src), src read without, rows scattered with the
        constraints; the cells are added in ascending order, or descending (reverse); dtype: the type of all arithmetic"""
        r = self.ref
        G = r.G.astype(dtype)
        local = np.zeros(r.dofs.shape, dtype=dtype)
        if rhs_q is not None:
            local += np.asarray(rhs_q, dtype=dtype) @ self.S2.astype(dtype)
        if src is not None:
            coef = np.asarray(coef, dtype=dtype)
            g = np.einsum("dqi,ci->cdq", G, np.asarray(src, dtype=dtype)[r.dofs_plain])
            flux = np.stack([coef[:, 0] * g[:, 0] + coef[:, 2] * g[:, 1], coef[:, 2] * g[:, 0] + coef[:, 1] * g[:, 1]], axis=1)
            local -= np.einsum("dqi,cdq->ci", G, flux)
        dofs = r.dofs
        if reverse:
            dofs, local = dofs[::-1], local[::-1]
        ok = dofs >= 0
        dst = np.zeros(r.n_dofs, dtype=dtype)
        np.add.at(dst, dofs[ok], local[ok])
        return dst

    def rhs(self, problem, **kw):
        """sum phi_i f JxW - (A_plain u_bc)_i on the free rows, zero on the constrained ones"""
        return self.residual(self.coef_q(problem), self.boundary_vector(problem), self.rhs_quadrature(problem), **kw)

    # ---- error ----
    def error_sums(self, problem, u_h):
        """(sum (u_h - u)^2 JxW, sum JxW) with the boundary values of u_h in place"""
        uq = np.asarray(u_h, dtype=np.float64)[self.ref.dofs_plain] @ self.S2.T
        d = uq - self.solution_q(problem)
        return float((d * d * self.jxw_q).sum()), float(self.jxw_q.sum())

    def l2_error(self, problem, u_h):
        e, v = self.error_sums(problem, u_h)
        return float(np.sqrt(e / v))

    # ---- dense solve ----
    def solve(self, problem):
        """the discrete solution with its boundary values in place"""
        r = self.ref
        A = r.matrix(self.coef_q(problem))
        u = self.boundary_vector(problem)
        f = r.free
        u[f] = np.linalg.solve(A[np.ix_(f, f)], self.rhs(problem)[f])
        return u
