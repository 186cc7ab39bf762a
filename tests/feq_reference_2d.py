"""CPU restatement (plain numpy) of the FE_Q Laplace operator, its level transfers and MultigridSolver on a structured
quadrilateral mesh: the reference of tests/test_gpu_feq_2d.py.

TEST INFRASTRUCTURE ONLY.  It shares nothing with the library but the 1D arrays of the element (shape_values,
colloc_grad, qweights, qpoints, gll, prolong_1d, handed in as a dict).  Vectors are [Gy, Gx] arrays in GRID ordering,
G_d = N_d p + 1; the tests map to the provider's numbering through its dof_grid.

Operator on a Cartesian box: the Kronecker form A = cxx (M_y x K_x) + cyy (K_y x M_x) of the global 1D mass and
stiffness matrices.  Full-tensor and per-point forms: cell-by-cell einsum.  Dirichlet DoFs (the boundary of the box)
follow the library's convention (include/mgx.h): identity rows, constrained entries read as zero.
Transfers: Kronecker products of the global 1D embedding; the coarse side is masked with constraints, the fine side
is read and written as it is.
Solver: eigenvalue estimate (the rule of _estimate in tests/dg_plain_reference.py), both Chebyshev kinds, v_cycle, the
full-multigrid solve, solve_cg and vmult_with_residual_update of multigrid_solver.h.
"""
import numpy as np


def arrays_1d(provider):
    """the 1D arrays of a provider object (multigrid_amd.Square or .Cube) as a dict"""
    return dict(S=provider.shape_values(), D=provider.colloc_grad(), w=provider.qweights(), xq=provider.qpoints(),
                gll=provider.gll(), P1=provider.prolong_1d())


def cell_matrices_1d(e):
    """(M, K) of the reference cell: M = S^T W S, K = (D S)^T W (D S)"""
    G = e["D"] @ e["S"]
    return e["S"].T @ (e["w"][:, None] * e["S"]), G.T @ (e["w"][:, None] * G)


def assemble_1d(cell, n_cells):
    p = cell.shape[0] - 1
    A = np.zeros((n_cells * p + 1,) * 2)
    for c in range(n_cells):
        A[c * p:c * p + p + 1, c * p:c * p + p + 1] += cell
    return A


def embedding_1d(P1, n_coarse):
    """global 1D embedding [(2 N p + 1) x (N p + 1)] from prolong_1d [(2p+1) x (p+1)] (coinciding rows are equal)"""
    p = P1.shape[1] - 1
    P = np.zeros((2 * n_coarse * p + 1, n_coarse * p + 1))
    for c in range(n_coarse):
        P[2 * c * p:2 * c * p + 2 * p + 1, c * p:c * p + p + 1] = P1
    return P


class Level:
    """one level: Nx x Ny cells.  coef = [xx, yy, xy] per mesh (weight per point), or coef_q [Ny, Nx, 3, n, n] per cell
    (cy, cx) and point (qy, qx) with the weight folded in."""

    def __init__(self, e, cells, coef=(1.0, 1.0, 0.0), coef_q=None, force_cellwise=False):
        self.e, self.p = e, e["S"].shape[0] - 1
        self.Nx, self.Ny = int(cells[0]), int(cells[1])
        p = self.p
        self.shape = (self.Ny * p + 1, self.Nx * p + 1)
        self.n = self.shape[0] * self.shape[1]
        self.free = np.zeros(self.shape)
        self.free[1:-1, 1:-1] = 1.0
        self.coef, self.coef_q = np.asarray(coef, dtype=float), coef_q
        self.cellwise = force_cellwise or coef_q is not None or self.coef[2] != 0.0
        M, K = cell_matrices_1d(e)
        self.Mx, self.Kx = assemble_1d(M, self.Nx), assemble_1d(K, self.Nx)
        self.My, self.Ky = assemble_1d(M, self.Ny), assemble_1d(K, self.Ny)
        self._diag = None

    # ---- the operator without constraints ----
    def _cells(self, X):
        """[Ny, Nx, n, n] local values (j, i) of every cell"""
        p, n = self.p, self.p + 1
        iy = (np.arange(self.Ny) * p)[:, None] + np.arange(n)[None, :]
        ix = (np.arange(self.Nx) * p)[:, None] + np.arange(n)[None, :]
        return X[iy[:, None, :, None], ix[None, :, None, :]], iy, ix

    def _tensor(self):
        w = self.e["w"]
        if self.coef_q is not None:
            return self.coef_q
        t = self.coef[:, None, None] * (w[:, None] * w[None, :])[None]
        return np.broadcast_to(t, (self.Ny, self.Nx, 3) + t.shape[1:])

    def apply_full(self, X):
        X = np.asarray(X, dtype=float).reshape(self.shape)
        if not self.cellwise:
            return self.coef[0] * (self.My @ X @ self.Kx.T) + self.coef[1] * (self.Ky @ X @ self.Mx.T)
        S, G = self.e["S"], self.e["D"] @ self.e["S"]
        U, iy, ix = self._cells(X)
        gx = np.einsum("qj,ri,cdji->cdqr", S, G, U)   # d/dx at (qy, qx)
        gy = np.einsum("qj,ri,cdji->cdqr", G, S, U)
        T = self._tensor()
        fx = T[:, :, 0] * gx + T[:, :, 2] * gy
        fy = T[:, :, 2] * gx + T[:, :, 1] * gy
        R = np.einsum("qj,ri,cdqr->cdji", S, G, fx) + np.einsum("qj,ri,cdqr->cdji", G, S, fy)
        Y = np.zeros(self.shape)
        np.add.at(Y, (iy[:, None, :, None], ix[None, :, None, :]), R)
        return Y

    def diagonal_full(self):
        if not self.cellwise:
            return self.coef[0] * np.outer(np.diag(self.My), np.diag(self.Kx)) + \
                self.coef[1] * np.outer(np.diag(self.Ky), np.diag(self.Mx))
        S, G = self.e["S"], self.e["D"] @ self.e["S"]
        T = self._tensor()
        dx = np.einsum("qj,ri->qrji", S, G)
        dy = np.einsum("qj,ri->qrji", G, S)
        R = np.einsum("cdqr,qrji->cdji", T[:, :, 0], dx * dx) + np.einsum("cdqr,qrji->cdji", T[:, :, 1], dy * dy) + \
            2 * np.einsum("cdqr,qrji->cdji", T[:, :, 2], dx * dy)
        _, iy, ix = self._cells(np.zeros(self.shape))
        Y = np.zeros(self.shape)
        np.add.at(Y, (iy[:, None, :, None], ix[None, :, None, :]), R)
        return Y

    # ---- with Dirichlet rows (laplace_operator.h:573-634, 745-800) ----
    def vmult(self, x):
        X = np.asarray(x, dtype=float).reshape(self.shape)
        return self.free * self.apply_full(self.free * X) + (1 - self.free) * X

    def vmult_residual(self, rhs, lhs):
        return np.asarray(rhs, dtype=float).reshape(self.shape) - self.vmult(lhs)

    def inv_diag(self):
        if self._diag is None:
            self._diag = 1.0 / (self.free * self.diagonal_full() + (1 - self.free))
        return self._diag

    def dense(self):
        """the matrix with its identity rows (small levels only)"""
        if not self.cellwise:
            A = self.coef[0] * np.kron(self.My, self.Kx) + self.coef[1] * np.kron(self.Ky, self.Mx)
        else:
            A = np.array([self.apply_full(col.reshape(self.shape)).ravel() for col in np.eye(self.n)]).T
        f = self.free.ravel()
        return f[:, None] * A * f[None, :] + np.diag(1 - f)


class Transfer:
    """level pair: coarse (Nx x Ny cells) -> fine (2 Nx x 2 Ny)"""

    def __init__(self, coarse, fine):
        self.c, self.f = coarse, fine
        self.Px, self.Py = embedding_1d(coarse.e["P1"], coarse.Nx), embedding_1d(coarse.e["P1"], coarse.Ny)

    def prolongate(self, xc, fine=None, with_bc=False):
        """fine (None: zero) + P xc"""
        Xc = np.asarray(xc, dtype=float).reshape(self.c.shape)
        out = self.Py @ (Xc * self.c.free if with_bc else Xc) @ self.Px.T
        return out if fine is None else np.asarray(fine, dtype=float).reshape(self.f.shape) + out

    def restrict_and_add(self, xc, xf, with_bc=True):
        R = self.Py.T @ np.asarray(xf, dtype=float).reshape(self.f.shape) @ self.Px
        return np.asarray(xc, dtype=float).reshape(self.c.shape) + (R * self.c.free if with_bc else R)


class Problem:
    """u = sin(3 pi x) sin(3 pi y), f = 2 (3 pi)^2 u on the box of roots cells of size h0 from (origin, origin), mapped
    by the constant matrix A (x = origin + A X): nodal boundary values, rhs = int f phi - int grad u_bc . C grad phi."""

    def __init__(self, e, origin=-0.9, A=None):
        self.e, self.origin = e, origin
        self.A = np.eye(2) if A is None else np.asarray(A, dtype=float).reshape(2, 2)
        self.detA = np.linalg.det(self.A)

    def coef(self):
        C = self.detA * np.linalg.inv(self.A.T @ self.A)
        return np.array([C[0, 0], C[1, 1], C[0, 1]])

    @staticmethod
    def u(x, y):
        return np.sin(3 * np.pi * x) * np.sin(3 * np.pi * y)

    def physical(self, X, Y):
        return self.origin + self.A[0, 0] * X + self.A[0, 1] * Y, self.origin + self.A[1, 0] * X + self.A[1, 1] * Y

    def _coords(self, L, h, ref):
        """reference-box coordinates of the points `ref` of every cell: [N, n] per direction"""
        return h * (np.arange(L.Nx)[:, None] + ref[None, :]), h * (np.arange(L.Ny)[:, None] + ref[None, :])

    def nodal(self, L, h):
        gx, gy = self._coords(L, h, self.e["gll"])
        p = L.p
        X = np.append(gx[:, :p].ravel(), gx[-1, p])
        Y = np.append(gy[:, :p].ravel(), gy[-1, p])
        x, y = self.physical(X[None, :], Y[:, None])
        return self.u(x, y)

    def boundary(self, L, h):
        return (1 - L.free) * self.nodal(L, h)

    def rhs(self, L, h):
        S, w = self.e["S"], self.e["w"]
        qx, qy = self._coords(L, h, self.e["xq"])
        x, y = self.physical(qx[None, :, None, :], qy[:, None, :, None])          # [Ny, Nx, qy, qx]
        fq = 2 * (3 * np.pi) ** 2 * self.u(x, y) * (w[:, None] * w[None, :]) * h * h * self.detA
        R = np.einsum("qj,ri,cdqr->cdji", S, S, fq)
        _, iy, ix = L._cells(np.zeros(L.shape))
        F = np.zeros(L.shape)
        np.add.at(F, (iy[:, None, :, None], ix[None, :, None, :]), R)
        return L.free * (F - L.apply_full(self.boundary(L, h)))

    def l2_error(self, L, h, sol, normalised=True):
        """sqrt(int (u_h - u)^2 / volume) as MultigridSolver::compute_l2_error reports it (multigrid_solver.h:298-343);
        normalised=False: the L2 norm of the error itself"""
        S, w = self.e["S"], self.e["w"]
        U, _, _ = L._cells(np.asarray(sol, dtype=float).reshape(L.shape))
        uq = np.einsum("qj,ri,cdji->cdqr", S, S, U)
        qx, qy = self._coords(L, h, self.e["xq"])
        x, y = self.physical(qx[None, :, None, :], qy[:, None, :, None])
        jxw = (w[:, None] * w[None, :]) * h * h * self.detA
        err2 = ((uq - self.u(x, y)) ** 2 * jxw).sum()
        return float(np.sqrt(err2 / (jxw.sum() * L.Nx * L.Ny) if normalised else err2))

    def dense_solution(self, L, h):
        """the discrete solution by a dense solve, boundary values in place"""
        x = np.linalg.solve(L.dense(), self.rhs(L, h).ravel()).reshape(L.shape)
        return L.free * x + self.boundary(L, h)


def chebyshev_factors(info, fourth_kind):
    """first factor, then a generator of (factor1, factor2) of the recurrence (PreconditionChebyshev; fourth kind:
    multigrid_solver.h:951-952 with delta = lambda_max)"""
    theta, delta = info["theta"], (info["lambda_max"] if fourth_kind else info["delta"])
    first = 4.0 / (3.0 * delta) if fourth_kind else 1.0 / theta

    def rest():
        rhok, k = delta / theta, 0
        while True:
            if fourth_kind:
                yield (2.0 * k + 1.0) / (2.0 * k + 5.0), (8.0 * k + 12.0) / (delta * (2.0 * k + 5.0))
            else:
                rhokp = 1.0 / (2.0 * theta / delta - rhok)
                yield rhokp * rhok, 2.0 * rhokp / delta
                rhok = rhokp
            k += 1
    return first, rest()


class Solver:
    """MultigridSolver (multigrid_solver.h:96-782) on levels 0 .. L of a box of roots cells refined L times"""

    def __init__(self, e, roots, n_levels, h0, degree_pre=3, problem=None, fourth_kind=False, make_level=None):
        self.e, self.n_levels, self.degree_pre, self.fourth_kind = e, n_levels, degree_pre, fourth_kind
        self.problem = problem or Problem(e)
        make_level = make_level or (lambda l, cells: Level(e, cells, self.problem.coef()))
        self.level = [make_level(l, (roots[0] << l, roots[1] << l)) for l in range(n_levels)]
        self.h = [h0 / (1 << l) for l in range(n_levels)]
        self.transfer = [None] + [Transfer(self.level[l - 1], self.level[l]) for l in range(1, n_levels)]
        self.info = [self._estimate(l) for l in range(n_levels)]
        self.rhs = [self.problem.rhs(L, h) for L, h in zip(self.level, self.h)]
        self.bc = [self.problem.boundary(L, h) for L, h in zip(self.level, self.h)]
        self.solution = [np.zeros(L.shape) for L in self.level]
        self.cg_history = []

    # smooth[level].initialize (multigrid_solver.h:269-289) + estimate_eigenvalues: PCG(D^-1) as a Lanczos process on
    # v_i = (grid id mod 11) - mean, stopped at 1e-10
    def _estimate(self, l):
        A = self.level[l]
        if l > 0:
            max_its, rng, degree = 15, 20.0, self.degree_pre
        else:
            max_its, rng, degree = max(3, A.n), 1e-3, None
        r = (np.arange(A.n) % 11).astype(float)
        r = (r - r.mean()).reshape(A.shape)
        d, diag, off = None, [], []
        res, rz, alpha, it = np.linalg.norm(r), 0.0, 0.0, 0
        while it < max_its and res > 1e-10:
            rz_old = rz
            z = A.inv_diag() * r
            rz = float(np.vdot(r, z))
            if not (rz > 0 and np.isfinite(rz)):
                break
            beta = rz / rz_old if it > 0 else 0.0
            d = z if it == 0 else z + beta * d
            h = A.vmult(d)
            dh = float(np.vdot(d, h))
            if not (dh > 0 and np.isfinite(dh)):
                break
            alpha_old, alpha = alpha, rz / dh
            r = r - alpha * h
            res = np.linalg.norm(r)
            it += 1
            if it == 1:
                diag.append(1.0 / alpha)
            else:
                off.append(np.sqrt(beta) / alpha_old)
                diag.append(1.0 / alpha + beta / alpha_old)
        lmin = lmax = 1.0
        if diag:
            ev = np.linalg.eigvalsh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
            lmin, lmax = ev[0], 1.2 * ev[-1]
        a = lmax / rng if rng > 1.0 else min(0.9 * lmax, lmin)
        if degree is None:   # numbers::invalid_unsigned_int: Varga's estimate for eps = smoothing_range
            sigma = (1.0 - np.sqrt(a / lmax)) / (1.0 + np.sqrt(a / lmax))
            degree = 1 + int(np.log(1.0 / rng + np.sqrt(1.0 / rng / rng - 1.0)) / np.log(1.0 / sigma))
        return dict(lambda_min=lmin, lambda_max=lmax, theta=0.5 * (lmax + a), delta=0.5 * (lmax - a), degree=degree,
                    cg_its=it)

    # PreconditionChebyshev::vmult (zero start) / ::step; level 0 keeps the first kind
    def smooth(self, l, x, b, is_step):
        A, I = self.level[l], self.info[l]
        fourth = self.fourth_kind and l > 0
        first, rest = chebyshev_factors(I, fourth)
        b = np.asarray(b, dtype=float).reshape(A.shape)
        dinv = A.inv_diag()
        if is_step:
            x = np.asarray(x, dtype=float).reshape(A.shape)
            old, x = x, x + first * dinv * (b - A.vmult(x))
        else:
            old, x = np.zeros(A.shape), first * dinv * b
        delta = I["lambda_max"] if fourth else I["delta"]
        if I["degree"] < 2 or abs(delta) < 1e-40:
            return x
        for _ in range(I["degree"] - 1):
            f1, f2 = next(rest)
            old, x = x, x + f1 * (x - old) + f2 * dinv * (b - A.vmult(x))
        return x

    def v_cycle(self, defect, l=None):
        l = self.n_levels - 1 if l is None else l
        A = self.level[l]
        defect = np.asarray(defect, dtype=float).reshape(A.shape)
        x = self.smooth(l, None, defect, False)
        if l == 0:
            return x
        t = A.vmult_residual(defect, x)
        T = self.transfer[l]
        xc = self.v_cycle(T.restrict_and_add(np.zeros(T.c.shape), t, with_bc=True), l - 1)
        x = T.prolongate(xc, fine=x, with_bc=True)
        return self.smooth(l, x, defect, True)

    def solve(self):
        """MultigridSolver::solve (:387-476): returns trace [n_levels, 2] = residual norm at the start / end of a level"""
        trace = np.zeros((self.n_levels, 2))
        t = self.smooth(0, None, self.rhs[0], False)
        self.solution[0] = self.smooth(0, t, self.rhs[0], True)
        for l in range(1, self.n_levels):
            A, free = self.level[l], self.level[l].free
            coarse = self.level[l - 1].free * self.solution[l - 1] + self.bc[l - 1]
            self.solution[l - 1] = coarse
            x = free * self.transfer[l].prolongate(coarse, with_bc=False)
            res = A.vmult_residual(self.rhs[l], x)
            trace[l, 0] = np.linalg.norm(res)
            x = free * (x + self.v_cycle(res, l))
            trace[l, 1] = np.linalg.norm(self.rhs[l] - A.vmult(x))
            self.solution[l] = x
        return trace

    def get_solution(self, l=None):
        l = self.n_levels - 1 if l is None else l
        return self.level[l].free * self.solution[l] + self.bc[l]

    def solve_cg(self, max_its=1000, abs_tol=1e-16, reduction=1e-9):
        """SolverCG preconditioned by the V-cycle with ReductionControl(1000, 1e-16, 1e-9) (:483-493)"""
        A = self.level[-1]
        x, r = np.zeros(A.shape), self.rhs[-1].copy()
        res0 = res = np.linalg.norm(r)
        self.cg_history = [res0]
        it, rz, d = 0, 0.0, None
        while res > abs_tol and res > reduction * res0 and it < max_its:
            z = self.v_cycle(r)
            rz_old, rz = rz, float(np.vdot(r, z))
            d = z if it == 0 else z + (rz / rz_old) * d
            h = A.vmult(d)
            alpha = rz / float(np.vdot(d, h))
            x = x + alpha * d
            r = r - alpha * h
            res = np.linalg.norm(r)
            it += 1
            self.cg_history.append(res)
        self.solution[-1] = x
        return it, (res / res0) ** (1.0 / max(it, 1))

    def vmult_with_residual_update(self, residual, update, factor):
        """(:516-619) returns (residual, update, (z.residual, z.(factor update))) after the call; constrained rows:
        identity"""
        A = self.level[-1]
        residual = np.asarray(residual, dtype=float).reshape(A.shape)
        update = np.asarray(update, dtype=float).reshape(A.shape)
        new = residual + factor * update if factor != 0 else residual
        z = self.v_cycle(new)
        z = A.free * z + (1 - A.free) * new
        if factor != 0:
            sums = (float(np.vdot(z, new)), float(np.vdot(z, update) * factor))
        else:
            s = float(np.vdot(z, new))
            sums = (s, s)
        return new, z, sums
