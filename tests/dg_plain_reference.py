"""CPU restatement (numpy, dense) of multigrid::MultigridSolverDGPlain (common/multigrid_solver_dg_plain.h:55-595) on
top of oracle/dg_oracle.py: the DG-SIP operator on every level of a globally refined box, Chebyshev smoothers with the
JacobiTransformed preconditioner, DG-to-DG level transfers, level 0 solved by its Chebyshev iteration.

TEST INFRASTRUCTURE ONLY.  The structure follows oracle.dg_oracle.DGMultigridOracle; vectors are the DG oracle's
[z, y, x, dof] arrays, level l has coarse_cells * 2^l cells and the Jacobian jacobian0 / 2^l.
"""
import numpy as np

from oracle import dg_oracle as dg


def embedding_1d(p, kind):
    """P[c][i, j], c = 0, 1: coefficient i, in the child's basis on [0, 1], of the parent's function phi_j((x + c) / 2).
    Lagrange bases: the value in the child's node i.  Hermite-like basis: interpolation in p + 1 Gauss-Lobatto points
    (the spaces are nested: any unisolvent set of points gives the same matrix)."""
    polys = dg.basis_1d(p, kind)
    n = p + 1
    if kind == dg.GAUSS:
        x, B = dg.gauss01(n)[0], None
    elif kind == dg.GAUSS_LOBATTO:
        x, B = dg.gauss_lobatto01(n), None
    else:
        x = dg.gauss_lobatto01(n)
        B = np.array([f(x) for f in polys]).T          # B[q, i] = phi_i(x_q)
    out = []
    for c in (0, 1):
        V = np.array([f(0.5 * (x + c)) for f in polys]).T   # V[q, j] = phi_j((x_q + c) / 2)
        out.append(V if B is None else np.linalg.solve(B, V))
    return np.array(out)


class DGPlainOracle:
    def __init__(self, degree, kind, coarse_cells, jacobian0, n_levels, degree_pre=3):
        self.p, self.kind, self.n_levels, self.degree_pre = degree, kind, n_levels, degree_pre
        jac0 = np.asarray(jacobian0, dtype=float).reshape(3, 3)
        self.level = [dg.DGOracle(degree, kind, tuple(int(c) << l for c in coarse_cells), jac0 / 2 ** l)
                      for l in range(n_levels)]
        self.P = embedding_1d(degree, kind)
        # child kx + 2 ky + 4 kz
        self.P3 = [dg.kron3(self.P[k & 1], self.P[(k >> 1) & 1], self.P[k >> 2]) for k in range(8)]
        self.info = [self._estimate(l) for l in range(n_levels)]

    # ---- transfers (MGTransferMatrixFree on DG levels: no weights, no constraints) ----
    def prolongate(self, l, coarse):
        """the level-l vector P coarse, coarse on level l - 1"""
        c = np.asarray(coarse, dtype=float).reshape(self.level[l - 1].shape)
        fine = np.zeros(self.level[l].shape)
        for k in range(8):
            fine[(k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2] = c @ self.P3[k].T
        return fine

    def restrict(self, l, fine):
        """the level-(l-1) vector P^T fine, fine on level l"""
        f = np.asarray(fine, dtype=float).reshape(self.level[l].shape)
        return sum(f[(k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2] @ self.P3[k] for k in range(8))

    # ---- smooth[level].initialize (multigrid_solver_dg_plain.h:192-213) ----
    def _estimate(self, l):
        A = self.level[l]
        n = int(np.prod(A.shape))
        L = self.n_levels - 1
        if l > 0:
            max_its, rng, degree = 15, 20.0, (self.degree_pre if l < L else max(1, self.degree_pre - 1))
        else:
            max_its, rng, degree = n, 1e-5, None
        # deal.II: (global DoF index mod 11) - mean; the oracle's layout is the lexicographic one
        r = (np.arange(n) % 11).astype(float)
        r = (r - r.mean()).reshape(A.shape)
        d, diag, off = None, [], []
        res, rz, alpha, it = np.linalg.norm(r), 0.0, 0.0, 0
        while it < max_its and res > 1e-10:
            it += 1
            rz_old = rz
            z = A.jacobi_vmult(r)
            rz = float(np.vdot(r, z))
            if it > 1:
                beta = rz / rz_old
                d = z + beta * d
            else:
                beta, d = 0.0, z
            alpha_old = alpha
            h = A.vmult(d)
            alpha = rz / float(np.vdot(d, h))
            r = r - alpha * h
            res = np.linalg.norm(r)
            if it == 1:
                diag.append(1.0 / alpha)
            else:
                off.append(np.sqrt(beta) / alpha_old)
                diag.append(1.0 / alpha + beta / alpha_old)
        ev = np.linalg.eigvalsh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
        lmin, lmax = ev[0], 1.2 * ev[-1]
        a = lmax / rng if rng > 1.0 else min(0.9 * lmax, lmin)
        if degree is None:   # numbers::invalid_unsigned_int: Varga's estimate for eps = smoothing_range
            sigma = (1.0 - np.sqrt(a / lmax)) / (1.0 + np.sqrt(a / lmax))
            degree = 1 + int(np.log(1.0 / rng + np.sqrt(1.0 / rng / rng - 1.0)) / np.log(1.0 / sigma))
        return dict(lambda_min=lmin, lambda_max=lmax, theta=0.5 * (lmax + a), delta=0.5 * (lmax - a), degree=degree,
                    cg_its=it)

    # ---- PreconditionChebyshev through the merged operation (laplace_operator_dg.h:910-955) ----
    def smooth(self, l, x, b, is_step):
        A, I = self.level[l], self.info[l]
        theta, delta = I["theta"], I["delta"]
        if not is_step:
            x, old = A.vmult_with_chebyshev_update(b, 0, 0.0, 1.0 / theta, x, np.zeros(A.shape))
            index = 1
        else:
            x, old = A.vmult_with_chebyshev_update(b, 1, 0.0, 1.0 / theta, x, np.zeros(A.shape))
            index = 2
        if I["degree"] < 2 or abs(delta) < 1e-40:
            return x
        rhok, sigma = delta / theta, theta / delta
        for _ in range(I["degree"] - 1):
            rhokp = 1.0 / (2.0 * sigma - rhok)
            f1, f2 = rhokp * rhok, 2.0 * rhokp / delta
            rhok = rhokp
            x, old = A.vmult_with_chebyshev_update(b, index, f1, f2, x, old)
            index += 1
        return x

    def v_cycle(self, defect, l=None):
        """v_cycle(level, 1), multigrid_solver_dg_plain.h:456-496"""
        l = self.n_levels - 1 if l is None else l
        A = self.level[l]
        defect = np.asarray(defect, dtype=float).reshape(A.shape)
        x = self.smooth(l, np.zeros(A.shape), defect, False)
        if l == 0:
            return x
        t = defect - A.vmult(x)
        x = x + self.prolongate(l, self.v_cycle(self.restrict(l, t), l - 1))
        return self.smooth(l, x, defect, True)

    def solve_cg(self, rhs, tolerance=1e-9):
        """(solution, iterations, reduction rate), :303-317"""
        A = self.level[-1]
        rhs = np.asarray(rhs, dtype=float).reshape(A.shape)
        x, r = np.zeros(A.shape), rhs.copy()
        res0 = res = np.linalg.norm(r)
        it, rz, d = 0, 0.0, None
        while res > max(1e-16, tolerance * res0) and it < 100:
            it += 1
            z = self.v_cycle(r)
            rz_old, rz = rz, float(np.vdot(r, z))
            d = z if it == 1 else z + (rz / rz_old) * d
            h = A.vmult(d)
            alpha = rz / float(np.vdot(d, h))
            x = x + alpha * d
            r = r - alpha * h
            res = np.linalg.norm(r)
        return x, it, (res / res0) ** (1.0 / max(it, 1))

    def vmult_with_residual_update(self, residual, update, factor):
        """(:340-427) returns (residual, update, sums) after the call"""
        A = self.level[-1]
        residual = np.asarray(residual, dtype=float).reshape(A.shape)
        update = np.asarray(update, dtype=float).reshape(A.shape)
        mg = self.v_cycle(residual + factor * update if factor != 0 else residual)
        if factor != 0:
            new = residual + factor * update
            sums = (float(np.vdot(mg, new)), float(np.vdot(mg, update) * factor))
        else:
            new = residual
            s = float(np.vdot(mg, residual))
            sums = (s, s)
        return new, mg, sums
