"""numpy restatement of the lumped-mass PCG on the DG-SIP operator (include/mgx_dg.h, mgx_dg_pcg_solver_*; the solver
of solver_dg/program.cc): the preconditioner table, textbook PCG and the merged recurrence exactly as the device runs
it, including its breakdown guard.  tests/test_dg_pcg_reference.py pins it on the CPU, tests/test_gpu_dg_pcg.py
compares the GPU with it.

Vectors are arrays whose last axis is the local index of a cell, x fastest (the layout of oracle/dg_oracle.py and
tests/dg_reference_2d.py), so the table of (p+1)^dim numbers broadcasts over them."""
import numpy as np

from oracle import dg_oracle as dg


def lumped_line(p, kind):
    """sum_q w_q phi_i(x_q) on the (p+1)-point Gauss rule, i = 0 .. p"""
    xq, wq = dg.gauss01(p + 1)
    return np.array([np.sum(wq * f(xq)) for f in dg.basis_1d(p, kind)])


def lumped_mass_inverse(p, kind, jacobian):
    """1 / (|det J| prod_d sum_q w_q phi_{i_d}(x_q)), (p+1)^dim entries, x fastest (solver_dg/program.cc:134-148)"""
    J = np.asarray(jacobian, dtype=float)
    line = lumped_line(p, kind)
    t = line
    for _ in range(J.shape[0] - 1):
        t = np.kron(line, t)
    return 1.0 / (abs(np.linalg.det(J)) * t)


def positive_finite(v):
    return bool(v > 0.0 and np.isfinite(v))


def textbook_pcg(A, m, b, n_iterations):
    """PCG as in any textbook (deal.II's SolverCG with a diagonal preconditioner), zero start, fp64.
    Returns x and rho_k = r_k . M^-1 r_k for k = 0 .. n_iterations."""
    x, r = np.zeros_like(b), b.copy()
    z = m * r
    p = z.copy()
    rho = np.sum(r * z)
    hist = [rho]
    for _ in range(n_iterations):
        q = A(p)
        alpha = rho / np.sum(p * q)
        x += alpha * p
        r -= alpha * q
        z = m * r
        rho_next = np.sum(r * z)
        p = z + (rho_next / rho) * p
        rho = rho_next
        hist.append(rho)
    return x, np.array(hist)


def merged_pcg(A, m, b, n_iterations, dtype=np.float64):
    """The merged form: per iteration q = A p with the four sums {q.p, r.(m r), q.(m r), q.(m q)} (products in the
    number type, sums in double), then
        alpha = s1 / s0 ; rho_next = s1 - 2 alpha s2 + alpha^2 s3 ; beta = rho_next / s1 ; rho[k] = s1, rho[k+1] = rho_next
    then x += alpha p ; r -= alpha q ; p = m r + beta p.  The guard: if s0 or s1 is not a positive finite number, rho_next
    not finite, or a breakdown is on record: alpha = beta = 0, rho[k+1] = rho[k] (k = 0: s1 if finite and not negative,
    else 0), and stalled_at = k the first time.  If only rho_next fails, being finite but not positive -- the residual
    has reached rounding level, where the recurrence cancels -- the step is still taken (alpha minimises the error along
    p whatever comes after), beta = 0, rho[k+1] = 0 and stalled_at = k + 1: the number of steps taken, either way.
    Vectors in `dtype`; A maps and returns fp64 arrays.
    Returns x, the history rho[0 .. n_iterations] and stalled_at (-1: none)."""
    T = np.dtype(dtype).type
    mT = m.astype(dtype)
    b = b.astype(dtype)
    x, r = np.zeros_like(b), b.copy()
    p = mT * r
    hist = np.zeros(n_iterations + 1)
    stalled_at = -1
    f8 = np.float64
    for k in range(n_iterations):
        q = A(p.astype(f8)).astype(dtype)
        mr = mT * r
        s0, s1 = np.sum((q * p).astype(f8)), np.sum((r * mr).astype(f8))
        s2, s3 = np.sum((q * mr).astype(f8)), np.sum((q * (mT * q)).astype(f8))
        ok = stalled_at < 0 and positive_finite(s0) and positive_finite(s1)
        alpha = beta = rho_next = 0.0
        if ok:
            alpha = s1 / s0
            rho_next = s1 - 2.0 * alpha * s2 + alpha * alpha * s3
            ok = bool(np.isfinite(rho_next))
        if ok and rho_next > 0.0:
            beta = rho_next / s1
            hist[k], hist[k + 1] = s1, rho_next
        elif ok:
            # the step is taken, the direction is not renewed: the iteration has ended after k + 1 steps
            hist[k], hist[k + 1] = s1, 0.0
            stalled_at = k + 1
        else:
            alpha = 0.0
            if k == 0:
                hist[0] = s1 if (s1 >= 0.0 and np.isfinite(s1)) else 0.0
            hist[k + 1] = hist[k]
            if stalled_at < 0:
                stalled_at = k
        a, bt = T(alpha), T(beta)
        x = x + a * p
        r = r - a * q
        p = mT * r + bt * p
    return x, hist, stalled_at


def stop_iteration(hist, tolerance, check_every, stalled_at=-1):
    """the solver's stopping rule on a history rho[0 .. n]: the first k that is a multiple of check_every (or n) with
    sqrt(rho_k / rho_0) <= tolerance, n if there is none; the iteration of a breakdown if that came first"""
    n = len(hist) - 1
    for k in range(1, n + 1):
        if k % check_every == 0 or k == n:
            if 0 <= stalled_at <= k:
                return stalled_at
            if np.sqrt(hist[k] / hist[0]) <= tolerance:
                return k
    return n
