"""numpy restatement of the solution-dependent coefficient on curved cells (include/mgx.h,
mgx_operator_enable_coefficient_update_q; minimal_surface/program.cc:120-197 with the inverse Jacobian and JxW of every
quadrature point).  The geometry is computed HERE, from the cell nodes alone: the dense gradient matrices of
nonlinear_reference.py applied to the node coordinates give the Jacobian F = dx / dxi of every point, a 3 x 3 inverse and
a determinant give M = F^-1 F^-T and JxW = det F w_q -- not from the provider's coef_q / jxw_q, which
test_nonlinear_reference_mapped.py compares with it.  The laws are written with M and JxW (the form of the affine
reference), not with U = JxW M and w as the kernels have them."""
import numpy as np

from nonlinear_reference import COMPONENTS, LAW_MINIMAL_SURFACE, LAW_UNIT, NonlinearReference


class MappedNonlinearReference(NonlinearReference):
    def __init__(self, p, shape_values, colloc_grad, qweights, idx27, idx27_plain, n_dofs, cell_nodes):
        super().__init__(p, shape_values, colloc_grad, qweights, idx27, idx27_plain, n_dofs, [1, 1, 1, 0, 0, 0], 1.0)
        nodes = np.asarray(cell_nodes, dtype=np.float64).reshape(self.dofs.shape[0], 3, (p + 1) ** 3)
        # F[c, q, a, b] = d x_a / d xi_b
        F = np.einsum("bqi,cai->cqab", self.G, nodes)
        self.det = np.linalg.det(F)
        assert (self.det > 0).all()
        inv = np.linalg.inv(F)  # inv[c, q, b, a] = d xi_b / d x_a
        self.Mq = np.einsum("cqea,cqfa->cqef", inv, inv)  # J^-1 J^-T
        self.jxwq = self.det * self.jxw[None, :]          # (self.jxw of the base class with det J = 1: the weights)
        del self.M

    def unit_tensor(self):
        """[n_cells, 6, n_q] JxW_q J^-1 J^-T"""
        return np.stack([self.jxwq * self.Mq[:, :, a, b] for a, b in COMPONENTS], axis=1)

    def coefficient(self, law, u, dtype=np.float64):
        """[n_cells, 6, n_q]: JxW M (LAW_UNIT) or JxW (M - (M g)(M g)^T / (1 + s)) / sqrt(1 + s), s = g^T M g, per point.
        dtype: the arithmetic of the law (float32: what rounding alone does to it, with the geometry and the gradient
        rounded first)"""
        if law == LAW_UNIT:
            return self.unit_tensor()
        g = self.gradients(u).astype(dtype)
        M, jxw = self.Mq.astype(dtype), self.jxwq.astype(dtype)
        v = np.einsum("cqde,ceq->cdq", M, g)
        s1 = dtype(1.0) + np.einsum("cdq,cdq->cq", g, v)
        out = np.empty((g.shape[0], 6, g.shape[2]), dtype=dtype)
        for c, (a, b) in enumerate(COMPONENTS):
            out[:, c, :] = jxw * (M[:, :, a, b] - v[:, a, :] * v[:, b, :] / s1) / np.sqrt(s1)
        return out

    def residual(self, law, u, dtype=np.float64):
        """dtype: the arithmetic of the gradient, the flux and the sums (float32: what rounding alone does to them)"""
        G, M, jxw = self.G.astype(dtype), self.Mq.astype(dtype), self.jxwq.astype(dtype)
        g = np.einsum("dqi,ci->cdq", G, np.asarray(u, dtype=dtype)[self.dofs_plain])
        v = np.einsum("cqde,ceq->cdq", M, g)
        a = jxw
        if law == LAW_MINIMAL_SURFACE:
            a = a / np.sqrt(dtype(1.0) + np.einsum("cdq,cdq->cq", g, v))
        local = -np.einsum("dqi,cdq->ci", G, a[:, None, :] * v)
        dst = np.zeros(self.n_dofs, dtype=dtype)
        ok = self.dofs >= 0
        np.add.at(dst, self.dofs[ok], local[ok])
        return dst


# the curved meshes of the tests: name -> keyword arguments of multigrid_amd.Cube (degree and n_refine are the caller's)
GEOMETRIES = {
    "sheared": dict(box=(1, 1, 1), origin=-0.9, h0=1.9, geometry="sheared"),
    "shell_sector": dict(box=(1, 1, 1), origin=-0.9, h0=1.9, geometry="shell_sector"),
    "shell6": dict(shell=6, problem="cube"),
}
# the constant Jacobian of the sheared box (mgx_cube.cpp, mgx_cube_s::map)
SHEAR = np.array([[1, 0.1, 0.05], [0.03, 1, 0.1], [0.02, 0.04, 1]])


def make_cube(mg, geometry, p, n_refine):
    return mg.Cube(p, n_refine=n_refine, **GEOMETRIES[geometry])


def mapped_reference(cube, l):
    return MappedNonlinearReference(cube.degree, cube.shape_values(), cube.colloc_grad(), cube.qweights(), cube.idx27(l),
                                    cube.idx27_plain(l), cube.n_dofs(l), cube.cell_nodes(l))


def boundary_state(cube, l, amplitude):
    """zero in the interior, A sin(2 pi (x + y)) at the mapped nodes of the Dirichlet DoFs"""
    u = np.zeros(cube.n_dofs(l))
    c = cube.constrained(l)
    x = cube.dof_coordinates(l)[c]
    u[c] = amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1]))
    return u


def smooth_state(cube, l):
    """a smooth state with gradients of order one, boundary values included"""
    x = cube.dof_coordinates(l)
    return 0.3 * np.sin(2.0 * x[:, 0] + 1.0) * np.cos(1.5 * x[:, 1]) + 0.2 * x[:, 2] ** 2 + 0.1 * x[:, 0] * x[:, 2]


def rough_state(cube, l):
    """the smooth state plus a component that is not: the state of test_gpu_nonlinear.py.  The residual of a smooth
    state is the small remainder of cell contributions that cancel in every interior DoF (the discretisation is
    consistent), so an error "relative to the largest entry" of it measures that cancellation and not the kernel; with
    the rough component the entries of the residual are of the size of their summands."""
    return smooth_state(cube, l) + 0.1 * cube.seeded_vector(l, 11)
