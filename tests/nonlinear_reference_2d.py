"""numpy restatement of the solution-dependent coefficient on quadrilaterals (include/mgx.h,
mgx_operator_enable_coefficient_update[_q]_2d; minimal_surface/program.cc:120-197, 414-573 with dimension = 2): dense
per-cell gradient matrices from the 1D arrays shape_values / colloc_grad / qweights, the compressed index tables idx9 /
idx9_plain and the NODES of the cells -- the geometry (metric and det J of affine cells, JxW_q J^-1 J^-T and JxW_q of
curved ones) is computed here from the nodes, not taken from the provider.  test_nonlinear_reference_2d.py pins it,
test_gpu_nonlinear_2d.py compares the device against it.

TEST INFRASTRUCTURE ONLY.  Newton's method, the scatter and the gradients are those of tests/nonlinear_reference.py."""
import numpy as np

import nonlinear_reference as nr
from nonlinear_reference import LAW_MINIMAL_SURFACE, LAW_UNIT, interpolation_matrix_1d, steps_to  # noqa: F401

INVALID = 0xFFFFFFFF
# tensor component c of [xx,yy,xy] -> (row, column)
COMPONENTS = [(0, 0), (1, 1), (0, 1)]


def cell_dofs(idx9, p):
    """[n_cells, (p+1)^2] DoF of every node of every cell (x fastest), -1 where the entity is constrained"""
    n = p + 1
    idx9 = np.asarray(idx9, dtype=np.int64).reshape(-1, 9)
    out = np.empty((idx9.shape[0], n, n), dtype=np.int64)
    code = lambda a: 0 if a == 0 else (2 if a == p else 1)
    for j in range(n):
        for i in range(n):
            cx, cy = code(i), code(j)
            base = idx9[:, 3 * cy + cx]
            d = base + (j - 1 if cy == 1 else 0) * (p - 1 if cx == 1 else 1) + (i - 1 if cx == 1 else 0)
            out[:, j, i] = np.where(base == INVALID, -1, d)
    return out.reshape(idx9.shape[0], n * n)


class NonlinearReference2D(nr.NonlinearReference):
    """affine=True: the laws with one metric M and one det J, taken from the corner nodes of cell 0 (all cells of the
    level are translates of it); affine=False: the laws with U = JxW_q J^-1 J^-T and w = JxW_q of every point, J the
    Jacobian of the degree-p interpolant of the cell's nodes"""

    def __init__(self, p, shape_values, colloc_grad, qweights, idx9, idx9_plain, n_dofs, nodes, affine):
        n = p + 1
        S = np.asarray(shape_values, dtype=np.float64).reshape(n, n)
        G1 = np.asarray(colloc_grad, dtype=np.float64).reshape(n, n) @ S
        w = np.asarray(qweights, dtype=np.float64)
        self.p, self.n_dofs, self.affine = p, int(n_dofs), bool(affine)
        # rows: quadrature points, columns: nodes, both lexicographic with x fastest
        self.G = np.stack([np.kron(S, G1), np.kron(G1, S)])
        self.w1 = w
        self.wq = (w[:, None] * w[None, :]).ravel()
        self.dofs = cell_dofs(idx9, p)
        self.dofs_plain = cell_dofs(idx9_plain, p)
        assert self.dofs_plain.min() >= 0
        self.constrained = np.setdiff1d(np.arange(self.n_dofs), self.dofs[self.dofs >= 0])
        self.free = np.setdiff1d(np.arange(self.n_dofs), self.constrained)
        nodes = np.asarray(nodes, dtype=np.float64).reshape(self.dofs.shape[0], n * n, 2)
        if self.affine:
            x0 = nodes[0, 0]
            J = np.stack([nodes[0, p] - x0, nodes[0, p * n] - x0], axis=1)  # columns: d x / d xi, d x / d eta
            Ji = np.linalg.inv(J)
            self.M = Ji @ Ji.T
            self.det = np.linalg.det(J)
            self.jxw = self.wq * self.det
        else:
            # J[c, q, a, b] = d x_a / d xi_b
            J = np.einsum("bqi,cia->cqab", self.G, nodes)
            det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
            assert det.min() > 0
            Ji = np.linalg.inv(J)
            Mq = np.einsum("cqab,cqdb->cqad", Ji, Ji)
            self.w = self.wq[None, :] * det                                              # [c, q]
            self.U = np.stack([self.w * Mq[..., a, b] for a, b in COMPONENTS], axis=1)   # [c, 3, q]

    def _jxw(self, dtype):
        """JxW_q of affine cells formed in `dtype` from the 1D weights and det J, every product rounded: (w_qx det J) w_qy"""
        w1 = self.w1.astype(dtype)
        return ((w1[None, :] * dtype(self.det)) * w1[:, None]).ravel()

    def unit_tensor(self):
        """[n_cells, 3, n_q] JxW_q J^-1 J^-T"""
        if self.affine:
            t = np.stack([self.jxw * self.M[a, b] for a, b in COMPONENTS])
            return np.ascontiguousarray(np.broadcast_to(t, (self.dofs.shape[0],) + t.shape))
        return self.U

    def _flux_terms(self, u, dtype):
        """g [c, 2, q], v = J^-1 J^-T g [c, 2, q] scaled so that s = g . v / scale, in `dtype` throughout"""
        g = np.einsum("dqi,ci->cdq", self.G.astype(dtype), np.asarray(u, dtype=dtype)[self.dofs_plain])
        T = self.unit_tensor().astype(dtype) if not self.affine else None
        if self.affine:
            M = self.M.astype(dtype)
            v = np.einsum("de,ceq->cdq", M, g)
            return g, v, None
        v = np.stack([T[:, 0] * g[:, 0] + T[:, 2] * g[:, 1], T[:, 2] * g[:, 0] + T[:, 1] * g[:, 1]], axis=1)
        return g, v, self.w.astype(dtype)

    def coefficient(self, law, u, dtype=np.float64):
        """[n_cells, 3, n_q] the tensor of the law, evaluated in `dtype`"""
        one = dtype(1)
        if law == LAW_UNIT and self.affine:  # (JxW_q formed in `dtype` from the weights and det J, then times M)
            jxw, M = self._jxw(dtype), self.M.astype(dtype)
            t = np.stack([jxw * M[a, b] for a, b in COMPONENTS])
            return np.ascontiguousarray(np.broadcast_to(t, (self.dofs.shape[0],) + t.shape))
        if law == LAW_UNIT:
            return self.U.astype(dtype)
        g, v, w = self._flux_terms(u, dtype)
        out = np.empty((g.shape[0], 3, g.shape[2]), dtype=dtype)
        if self.affine:
            jxw, M = self._jxw(dtype), self.M.astype(dtype)
            s1 = one + np.einsum("cdq,cdq->cq", g, v)
            for c, (a, b) in enumerate(COMPONENTS):
                out[:, c] = jxw[None, :] / np.sqrt(s1) * (M[a, b] - v[:, a] * v[:, b] / s1)
            return out
        U = self.U.astype(dtype)
        s1 = one + np.einsum("cdq,cdq->cq", g, v) / w
        for c, (a, b) in enumerate(COMPONENTS):
            out[:, c] = (one / np.sqrt(s1)) * (U[:, c] - v[:, a] * v[:, b] / (w * s1))
        return out

    def residual(self, law, u, dtype=np.float64):
        """dst_i = - sum_q grad phi_i(q) . a JxW_q M g: gathered without, scattered with the constraints"""
        one = dtype(1)
        g, v, w = self._flux_terms(u, dtype)
        if self.affine:
            a = self._jxw(dtype)[None, :] * np.ones((g.shape[0], 1), dtype=dtype)
            if law == LAW_MINIMAL_SURFACE:
                a = a / np.sqrt(one + np.einsum("cdq,cdq->cq", g, v))
        else:
            a = np.ones(w.shape, dtype=dtype)
            if law == LAW_MINIMAL_SURFACE:
                a = a / np.sqrt(one + np.einsum("cdq,cdq->cq", g, v) / w)
        local = -np.einsum("dqi,cdq->ci", self.G.astype(dtype), a[:, None, :] * v)
        dst = np.zeros(self.n_dofs, dtype=dtype)
        ok = self.dofs >= 0
        np.add.at(dst, self.dofs[ok], local[ok])
        return dst

    def apply(self, coef, x):
        """LaplaceOperator::vmult with the tensor coef [n_cells, 3, n_q]: constrained entries of x read as zero,
        constrained rows the identity"""
        x = np.asarray(x, dtype=np.float64)
        xl = np.where(self.dofs >= 0, x[np.maximum(self.dofs, 0)], 0.0)
        g = np.einsum("dqi,ci->cdq", self.G, xl)
        flux = np.stack([coef[:, 0] * g[:, 0] + coef[:, 2] * g[:, 1], coef[:, 2] * g[:, 0] + coef[:, 1] * g[:, 1]], axis=1)
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


def interpolate_to_coarse(R, children, dofs_fine_plain, dofs_coarse_plain, n_coarse_dofs, fine):
    """the state on the coarser level (minimal_surface/program.cc:425-457): per coarse cell the children patch of
    (2p+1)^2 fine values, R along both directions, written (not added) to the coarse DoFs"""
    n, m = R.shape
    p = n - 1
    fine = np.asarray(fine, dtype=np.float64)
    children = np.asarray(children).reshape(-1, 4)
    out = np.full(n_coarse_dofs, np.nan)
    for pc in range(children.shape[0]):
        patch = np.zeros((m, m))
        for ch in range(4):
            ox, oy = (ch & 1) * p, (ch >> 1) * p
            patch[oy:oy + n, ox:ox + n] = fine[dofs_fine_plain[children[pc, ch]]].reshape(n, n)
        out[dofs_coarse_plain[pc]] = np.einsum("jb,ia,ba->ji", R, R, patch).ravel()
    assert not np.isnan(out).any()
    return out
