"""numpy restatement of the solution-dependent coefficient on affine cells (include/mgx.h, "solution-dependent
coefficient of the general branch"; minimal_surface/program.cc:120-197, 414-573): dense per-cell gradient matrices from
the 1D arrays shape_values / colloc_grad / qweights, the compressed index tables idx27 / idx27_plain, nothing else that
the kernels use.  test_nonlinear_reference.py pins it (the tensor is the derivative of the residual, the unit law is
the Laplace operator, Newton converges), test_gpu_nonlinear.py compares the device against it."""
import numpy as np

LAW_UNIT, LAW_MINIMAL_SURFACE = 0, 1
INVALID = 0xFFFFFFFF
# tensor component c of [xx,yy,zz,xy,xz,yz] -> (row, column)
COMPONENTS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def cell_dofs(idx27, p):
    """[n_cells, (p+1)^3] DoF of every node of every cell (x fastest), -1 where the entity is constrained: the
    addressing of read_dof_values_compressed (vector_access_reduced.h:153-229)"""
    n = p + 1
    idx27 = np.asarray(idx27, dtype=np.int64).reshape(-1, 27)
    out = np.empty((idx27.shape[0], n, n, n), dtype=np.int64)
    code = lambda a: 0 if a == 0 else (2 if a == p else 1)
    for k in range(n):
        for j in range(n):
            for i in range(n):
                cx, cy, cz = code(i), code(j), code(k)
                oz, oy = (k - 1 if cz == 1 else 0), (j - 1 if cy == 1 else 0)
                off = (p - 1 if cy == 1 else 1) * oz + oy
                base = idx27[:, 9 * cz + 3 * cy + cx]
                d = base + (off * (p - 1) + i - 1 if cx == 1 else off)
                out[:, k, j, i] = np.where(base == INVALID, -1, d)
    return out.reshape(idx27.shape[0], n ** 3)


def symmetric(metric):
    m = np.zeros((3, 3))
    for c, (a, b) in enumerate(COMPONENTS):
        m[a, b] = m[b, a] = metric[c]
    return m


class NonlinearReference:
    def __init__(self, p, shape_values, colloc_grad, qweights, idx27, idx27_plain, n_dofs, metric, det_jacobian):
        n = p + 1
        S = np.asarray(shape_values, dtype=np.float64).reshape(n, n)
        G1 = np.asarray(colloc_grad, dtype=np.float64).reshape(n, n) @ S  # derivative of the nodal basis at the Gauss points
        w = np.asarray(qweights, dtype=np.float64)
        self.p, self.n_dofs = p, int(n_dofs)
        # rows: quadrature points, columns: nodes, both lexicographic with x fastest
        self.G = np.stack([np.kron(S, np.kron(S, G1)), np.kron(S, np.kron(G1, S)), np.kron(G1, np.kron(S, S))])
        self.M = symmetric(metric)
        self.jxw = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel() * det_jacobian
        self.dofs = cell_dofs(idx27, p)              # constrained table: -1 on Dirichlet entities
        self.dofs_plain = cell_dofs(idx27_plain, p)  # dof-handler slot 1
        assert self.dofs_plain.min() >= 0
        self.constrained = np.setdiff1d(np.arange(self.n_dofs), self.dofs[self.dofs >= 0])
        self.free = np.setdiff1d(np.arange(self.n_dofs), self.constrained)

    def gradients(self, u):
        """[n_cells, 3, n_q] reference-space gradient of the state (boundary values in place) at the quadrature points"""
        return np.einsum("dqi,ci->cdq", self.G, np.asarray(u, dtype=np.float64)[self.dofs_plain])

    def coefficient(self, law, u):
        """[n_cells, 6, n_q]: JxW M (LAW_UNIT) or JxW (M - (M g)(M g)^T / (1 + s)) / sqrt(1 + s), s = g^T M g"""
        g = self.gradients(u)
        v = np.einsum("de,ceq->cdq", self.M, g)
        out = np.empty((g.shape[0], 6, g.shape[2]))
        if law == LAW_UNIT:
            for c, (a, b) in enumerate(COMPONENTS):
                out[:, c, :] = self.jxw[None, :] * self.M[a, b]
            return out
        s1 = 1.0 + np.einsum("cdq,cdq->cq", g, v)
        for c, (a, b) in enumerate(COMPONENTS):
            out[:, c, :] = self.jxw[None, :] * (self.M[a, b] - v[:, a, :] * v[:, b, :] / s1) / np.sqrt(s1)
        return out

    def _scatter(self, local):
        dst = np.zeros(self.n_dofs)
        ok = self.dofs >= 0
        np.add.at(dst, self.dofs[ok], local[ok])
        return dst

    def residual(self, law, u):
        """dst_i = - sum_q grad phi_i(q) . a JxW M g: gathered without, scattered with the constraints"""
        g = self.gradients(u)
        v = np.einsum("de,ceq->cdq", self.M, g)
        a = self.jxw[None, :] * np.ones(g.shape[0])[:, None]
        if law == LAW_MINIMAL_SURFACE:
            a = a / np.sqrt(1.0 + np.einsum("cdq,cdq->cq", g, v))
        return self._scatter(-np.einsum("dqi,cdq->ci", self.G, a[:, None, :] * v))

    def apply(self, coef, x):
        """LaplaceOperator::vmult with the merged coefficient coef [n_cells, 6, n_q]: constrained entries of x read as
        zero, constrained rows the identity"""
        x = np.asarray(x, dtype=np.float64)
        xl = np.where(self.dofs >= 0, x[np.maximum(self.dofs, 0)], 0.0)
        g = np.einsum("dqi,ci->cdq", self.G, xl)
        flux = np.zeros_like(g)
        for c, (a, b) in enumerate(COMPONENTS):
            flux[:, a, :] += coef[:, c, :] * g[:, b, :]
            if a != b:
                flux[:, b, :] += coef[:, c, :] * g[:, a, :]
        dst = self._scatter(np.einsum("dqi,cdq->ci", self.G, flux))
        dst[self.constrained] = x[self.constrained]
        return dst

    def matrix(self, coef):
        """dense matrix of apply()"""
        A = np.zeros((self.n_dofs, self.n_dofs))
        for cell in range(self.dofs.shape[0]):
            K = np.zeros((self.G.shape[2], self.G.shape[2]))
            for c, (a, b) in enumerate(COMPONENTS):
                T = self.G[a].T @ (coef[cell, c, :, None] * self.G[b])
                K += T if a == b else T + T.T
            d = self.dofs[cell]
            ok = d >= 0
            A[np.ix_(d[ok], d[ok])] += K[np.ix_(ok, ok)]
        A[self.constrained, self.constrained] = 1.0
        return A

    def diagonal_inverse(self, coef):
        return 1.0 / np.diag(self.matrix(coef))

    def newton(self, u0, max_steps=20, tolerance=0.0, linear_solve=None):
        """LaplaceProblem::solve(first_time) step by step (minimal_surface/program.cc:414-573) with exact linear solves
        (or linear_solve(A, b)); returns (state, [residual norm before the first step, after step 1, ...], halvings)"""
        u = np.array(u0, dtype=np.float64)
        norms, halvings = [], []
        for step in range(max_steps):
            law = LAW_UNIT if step == 0 else LAW_MINIMAL_SURFACE
            A = self.matrix(self.coefficient(law, u))
            rhs = self.residual(law, u)
            initial = np.linalg.norm(rhs)
            if step == 0:
                norms.append(initial)
            d = np.linalg.solve(A, rhs) if linear_solve is None else linear_solve(A, rhs)
            d[self.constrained] = 0.0
            alpha, n_steps, final, t = 1.0, 0, initial, u
            while n_steps < 100:
                t = u + alpha * d
                final = np.linalg.norm(self.residual(LAW_MINIMAL_SURFACE, t))
                if final < initial:
                    break
                alpha /= 2.0
                n_steps += 1
            u = t
            norms.append(final)
            halvings.append(n_steps)
            if final <= tolerance:
                break
        return u, norms, halvings


def steps_to(norms, factor):
    """number of Newton steps after which the residual norm is below factor * the first one (None: never)"""
    for k, r in enumerate(norms):
        if k > 0 and r < factor * norms[0]:
            return k
    return None


def lagrange(nodes, a, x):
    v = 1.0
    for b in range(len(nodes)):
        if b != a:
            v *= (x - nodes[b]) / (nodes[a] - nodes[b])
    return v


def interpolation_matrix_1d(gll):
    """[(p+1), (2p+1)]: row i = the values at coarse node i of the Lagrange polynomials of the child that contains the
    node (child 0 on [0, 1/2]: fine patch points 0..p, child 1 on [1/2, 1]: p..2p)"""
    gll = np.asarray(gll, dtype=np.float64)
    p = gll.size - 1
    R = np.zeros((p + 1, 2 * p + 1))
    for i in range(p + 1):
        child = 1 if gll[i] > 0.5 else 0
        xi = 2.0 * gll[i] - child
        for a in range(p + 1):
            R[i, child * p + a] = lagrange(gll, a, xi)
    return R


def interpolate_to_coarse(R, children, dofs_fine_plain, dofs_coarse_plain, n_coarse_dofs, fine):
    """the state on the coarser level (minimal_surface/program.cc:425-457): per coarse cell the children patch of
    (2p+1)^3 fine values, R along every direction, written (not added) to the coarse DoFs"""
    n, m = R.shape
    p = n - 1
    fine = np.asarray(fine, dtype=np.float64)
    children = np.asarray(children).reshape(-1, 8)
    out = np.full(n_coarse_dofs, np.nan)
    for pc in range(children.shape[0]):
        patch = np.zeros((m, m, m))
        for ch in range(8):
            ox, oy, oz = (ch & 1) * p, ((ch >> 1) & 1) * p, (ch >> 2) * p
            patch[oz:oz + n, oy:oy + n, ox:ox + n] = fine[dofs_fine_plain[children[pc, ch]]].reshape(n, n, n)
        out[dofs_coarse_plain[pc]] = np.einsum("kc,jb,ia,cba->kji", R, R, R, patch).ravel()
    assert not np.isnan(out).any()
    return out
