"""CPU restatement (numpy) of multigrid::MultigridSolverDG in TWO dimensions: oracle/dg_oracle.py::DGMultigridOracle one
dimension down, the reference of tests/test_gpu_dg_multigrid_2d.py.

TEST INFRASTRUCTURE ONLY.  It is put together from two files that are pinned on their own:
  tests/dg_reference_2d.py::DGOracle2D   the DG level (operator, JacobiTransformed, merged Chebyshev step)
  tests/feq_reference_2d.py::Solver      the FE_Q(p) hierarchy of the same mesh, vectors as [Gy, Gx] grids
and adds what joins them (common/multigrid_solver_dg.h:55-747): the smoothers of the FE_Q hierarchy re-configured as
:271-291 does (degree_pre - 1 on its finest level; level 0 to 2e-3 with max(3, n) Lanczos steps), the eigenvalue estimate
of the DG level (:293-303), the cell-wise transfers DG <-> FE_Q (laplace_operator_dg.h:1798-1819, :1863-1894) with
P1 = inv(phi_i(g_q)) in the Gauss-Lobatto nodes g_q, and dg_v_cycle (:605-633).  The smoother and the outer CG are the
3D oracle's: nothing in them knows the dimension.  tests/test_dg_multigrid_reference_2d.py pins this file.
"""
import numpy as np

from oracle import dg_oracle as dg
from dg_reference_2d import kron2


class DGMultigridOracle2D(dg.DGMultigridOracle):
    """`dgo`: DGOracle2D; `fe`: feq_reference_2d.Solver on the same cells and degree (its smoother parameters are
    re-configured here); `start`: the start vector of the eigenvalue estimate in the DG oracle's layout (deal.II: (global
    DoF index mod 11) - mean).  FE_Q vectors are [Gy, Gx] grids with zero boundary rows and columns."""

    def __init__(self, dgo, fe, degree_pre, start):
        self.dg, self.fe, self.degree = dgo, fe, degree_pre
        p, n = dgo.p, dgo.n
        self.lmax = lmax = fe.n_levels - 1
        assert (fe.level[lmax].Nx, fe.level[lmax].Ny) == tuple(dgo.cells) and fe.level[lmax].p == p
        # multigrid_solver_dg.h:271-291, by the rule of Solver._estimate
        if lmax > 0:
            keep, fe.degree_pre = fe.degree_pre, max(1, degree_pre - 1)
            fe.info[lmax] = fe._estimate(lmax)
            fe.degree_pre = keep
        fe.info[0] = self._coarse_info(fe._estimate(0), 2e-3)
        polys = dg.basis_1d(p, dgo.kind)
        g = dg.gauss_lobatto01(n)
        B = np.array([f(g) for f in polys]).T            # B[q, i] = phi_i(g_q)
        self.P1 = np.linalg.inv(B)                        # GLL values -> DG coefficients
        self.P2 = kron2(self.P1, self.P1)
        nx, ny = dgo.cells
        self.G = (ny * p + 1, nx * p + 1)
        # eigenvalue estimate: CG preconditioned with JacobiTransformed (multigrid_solver_dg.h:293-303)
        r = np.array(start, dtype=float).reshape(dgo.shape)
        d = None
        diag, off = [], []
        res, rz, alpha, it = np.linalg.norm(r), 0.0, 0.0, 0
        while it < 15 and res > 1e-10:
            it += 1
            rz_old = rz
            z = dgo.jacobi_vmult(r)
            rz = float(np.vdot(r, z))
            beta = rz / rz_old if it > 1 else 0.0
            d = z + beta * d if it > 1 else z
            alpha_old = alpha
            h = dgo.vmult(d)
            alpha = rz / float(np.vdot(d, h))
            r = r - alpha * h
            res = np.linalg.norm(r)
            if it == 1:
                diag.append(1.0 / alpha)
            else:
                off.append(np.sqrt(beta) / alpha_old)
                diag.append(1.0 / alpha + beta / alpha_old)
        ev = np.linalg.eigvalsh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
        self.lambda_max = 1.2 * ev[-1]
        a = self.lambda_max / 20.0
        self.delta, self.theta = 0.5 * (self.lambda_max - a), 0.5 * (self.lambda_max + a)
        self.cg_its = it

    @staticmethod
    def _coarse_info(info, rng):
        """level 0 of the FE_Q hierarchy with smoothing range `rng` < 1 in place of Solver's 1e-3: the Lanczos run (max(3,
        n) steps) and with it the eigenvalues are Solver._estimate's, the interval and Varga's degree are formed anew"""
        lmin, lmax = info["lambda_min"], info["lambda_max"]
        a = min(0.9 * lmax, lmin)
        sigma = (1.0 - np.sqrt(a / lmax)) / (1.0 + np.sqrt(a / lmax))
        degree = 1 + int(np.log(1.0 / rng + np.sqrt(1.0 / rng / rng - 1.0)) / np.log(1.0 / sigma))
        return dict(info, theta=0.5 * (lmax + a), delta=0.5 * (lmax - a), degree=degree)

    # ---- transfers ----
    def _zero_boundary(self, grid):
        grid[0], grid[-1], grid[:, 0], grid[:, -1] = 0, 0, 0, 0
        return grid

    def restrict_to_cg(self, r_dg):
        """P^T r as a [Gy, Gx] grid (constrained rows zero)"""
        p, n = self.dg.p, self.dg.n
        nx, ny = self.dg.cells
        grid = np.zeros(self.G)
        loc = np.asarray(r_dg, dtype=float).reshape(self.dg.shape) @ self.P2      # (P2^T r)_q = sum_i P2[i, q] r_i
        for j in range(ny):
            for i in range(nx):
                grid[j * p:j * p + n, i * p:i * p + n] += loc[j, i].reshape(n, n)
        return self._zero_boundary(grid)

    def prolongate_cg_to_dg(self, u_cg):
        p, n = self.dg.p, self.dg.n
        nx, ny = self.dg.cells
        grid = self._zero_boundary(np.array(u_cg, dtype=float).reshape(self.G))
        out = np.empty(self.dg.shape)
        for j in range(ny):
            for i in range(nx):
                out[j, i] = self.P2 @ grid[j * p:j * p + n, i * p:i * p + n].ravel()
        return out

    def v_cycle(self, defect):
        """dg_v_cycle(1), multigrid_solver_dg.h:605-633"""
        defect = np.asarray(defect, dtype=float).reshape(self.dg.shape)
        x = self.smooth(np.zeros(self.dg.shape), defect, False)
        t = defect - self.dg.vmult(x)
        x = x + self.prolongate_cg_to_dg(self.fe.v_cycle(self.restrict_to_cg(t)))
        return self.smooth(x, defect, True)


def pcg_inputs(shape):
    """(source of a V-cycle, right-hand side of the CG) of the recorded runs: seeded normal vectors in the oracle's layout"""
    rng = np.random.default_rng(7)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def make_pair(e, degree, kind, roots, n_refine, h0, degree_pre=3):
    """(DGOracle2D, feq Solver, DGMultigridOracle2D) on the box of `roots` square cells of size h0 refined n_refine times;
    e: the 1D arrays of the FE_Q element (feq_reference_2d.arrays_1d)"""
    import feq_reference_2d as feq
    from dg_reference_2d import DGOracle2D
    cells = (roots[0] << n_refine, roots[1] << n_refine)
    dgo = DGOracle2D(degree, kind, cells, np.eye(2) * h0 / (1 << n_refine))
    fe = feq.Solver(e, roots, n_refine + 1, h0, degree_pre=degree_pre)
    n = int(np.prod(dgo.shape))
    start = (np.arange(n) % 11).astype(float)
    start -= start.mean()
    return dgo, fe, DGMultigridOracle2D(dgo, fe, degree_pre, start.reshape(dgo.shape))
