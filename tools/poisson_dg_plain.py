"""Harness of the plain DG multigrid, mirroring poisson_dg_plain/program.cc in 3D: FE_DGQHermite(p) on the cube
[-0.9, 1]^3 (one cell refined n_refine times, as hyper_cube + refine_global gives), rhs 3 (3 pi)^2 prod sin(3 pi x_d),
CG preconditioned with one V-cycle of MultigridSolverDGPlain -- the DG-SIP operator on every level, DG-to-DG level
transfers, level 0 (the single cell) solved by its Chebyshev iteration; fp32 V-cycle inside the fp64 outer iteration.
The same problem, printed lines and table row as tools/poisson_dg.py, whose solver it is the A/B partner of.

    python tools/poisson_dg_plain.py [degree=3] [n_refine=5] [n_pre_smooth=3] [tolerance=1e-9] [--vcycle f32|f64]
                                     [--basis 0|1|2] [--solution reference|vanishing] [--levels] [--dim 2|3]
                                     [--boundary homogeneous|data] [--neumann 0,3] [--hierarchy h|hp|ph] [--coarse N]

--dim 2: the dimension the reference's driver is compiled for (poisson_dg_plain/program.cc:65): the square [-0.9, 1]^2,
rhs dim (3 pi)^2 prod sin(3 pi x_d) (program.cc:140), the same printed lines and table row.

--hierarchy (default h, the reference's: the mesh alone is coarsened, every level has the full degree): hp refines the
mesh at full degree and bisects the degree (p -> max(1, p // 2) down to 1) on the coarsest mesh; ph bisects the degree
on the finest mesh and refines the mesh at degree 1.  Every level is a rediscretisation with the penalty of its own
degree (mgx_dg_hp_solver_create).  --coarse N (default 1): N cells per direction on the coarsest mesh, which for N = 3
cannot be halved any further -- the case degree coarsening is for.

One line per level gives the degree, the cells and unknowns, the smoother's degree, lambda_max and the CG iterations of its eigenvalue estimate.
--levels: one more solve with the solver's per-level timers on, and the table of the reference's print_wall_times
(multigrid_solver_dg_plain.h:264-287).  The timers synchronise the stream around every part: for diagnosis, the
solve they time is slower than the solves reported above it.

--solution as in tools/poisson_dg.py: the benchmark's own solution does not vanish on the boundary, `vanishing` does
and shows the discretisation error (tests/test_gpu_dg_plain.py).

--boundary data: the right-hand side also carries the boundary values of the chosen solution, b_i += int_F u (sigma_F
phi_i - d_n phi_i) on every Dirichlet face (DGLaplaceOperator.compute_rhs), so the reference solution converges too;
right-hand side and error are then formed on the device (compute_rhs, compute_l2_error) and a line "Time compute rhs"
is printed as the reference prints it (multigrid_solver_dg_plain.h:188).  The default, homogeneous, is the reference's
volume-only vector from the host: nothing it prints changes.

--neumann 0,3 (with --boundary data, either --dim): the listed sides of the box, face numbers 2d+s (direction d, lower
s = 0 / upper s = 1), are Neumann faces on every level; the right-hand side carries the exact flux there, h = n . grad u
of the chosen solution (the potential form of compute_rhs's h), and its boundary values on the other sides.  At least
one side must stay a Dirichlet side.  One more line names the Neumann sides; without the option nothing changes."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402

WAVE = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=3)
    ap.add_argument("n_refine", nargs="?", type=int, default=5)
    ap.add_argument("n_pre_smooth", nargs="?", type=int, default=3)
    ap.add_argument("tolerance", nargs="?", type=float, default=1e-9)
    ap.add_argument("--vcycle", choices=["f32", "f64"], default="f32")
    ap.add_argument("--basis", type=int, default=0)
    ap.add_argument("--solution", choices=["reference", "vanishing"], default="reference")
    ap.add_argument("--levels", action="store_true", help="per-level time table of one more (synchronised) solve")
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3)
    ap.add_argument("--boundary", choices=["homogeneous", "data"], default="homogeneous",
                    help="data: boundary values of the solution in the right-hand side; rhs and error on the device")
    ap.add_argument("--hierarchy", choices=["h", "hp", "ph"], default="h",
                    help="hp: degree bisected on the coarsest mesh; ph: on the finest mesh, the mesh refined at degree 1")
    ap.add_argument("--coarse", type=int, default=1, help="cells per direction of the coarsest mesh")
    ap.add_argument("--neumann", default="", help="sides 2d+s that are Neumann faces, e.g. 0,3 (needs --boundary data)")
    a = ap.parse_args()
    a.neumann = tuple(sorted(set(int(f) for f in a.neumann.split(",") if f.strip() != "")))
    if a.neumann and a.boundary != "data":
        ap.error("--neumann needs --boundary data: the flux enters the right-hand side on the device")
    if any(f < 0 or f >= 2 * a.dim for f in a.neumann) or len(a.neumann) == 2 * a.dim:
        ap.error("--neumann: sides are face numbers 0 .. %d, and one side must stay a Dirichlet side" % (2 * a.dim - 1))
    vnum = mg.F32 if a.vcycle == "f32" else mg.F64
    t0 = time.time()
    ctx = mg.Context(0)
    dim = a.dim
    degrees = [a.degree]
    while degrees[0] > 1:
        degrees.insert(0, max(1, degrees[0] // 2))
    hierarchy = {"h": None,
                 "hp": [(p, 0) for p in degrees] + [(a.degree, r) for r in range(1, a.n_refine + 1)],
                 "ph": [(1, r) for r in range(a.n_refine + 1)] + [(p, a.n_refine) for p in degrees[1:]]}[a.hierarchy]
    solver = mg.DGPlainMultigridSolver(ctx, a.degree, a.basis, (a.coarse,) * dim, np.eye(dim) * 1.9 / a.coarse, a.n_refine + 1,
                                       a.n_pre_smooth, vnum, origin=(-0.9,) * dim, neumann_sides=a.neumann, hierarchy=hierarchy)
    n_levels = solver.n_levels
    n = solver.m()
    nc = n // (a.degree + 1) ** dim
    print("Number of degrees of freedom: %d (%d cells, FE_DGQHermite(%d) on %s %d levels, V-cycle in %s)"
          % (n, nc, a.degree, "every one of" if hierarchy is None else "the finest of", n_levels, a.vcycle))
    if a.neumann:
        print("Neumann sides (2d+s): %s, exact flux in the right-hand side" % ",".join(map(str, a.neumann)))
    for l in range(n_levels):
        i = solver.smoother_info(l)
        print("level %2d  degree %d  cells %9d  dofs %10d  smoother degree %3d  lambda_max %.6f  cg_its %d"
              % (l, solver.hierarchy[l][0], int(np.prod(solver.cells[l])), solver.matrix[l].m(), i["degree"], i["lambda_max"],
                 i["cg_its"]))
    if a.boundary == "data":
        return with_boundary_data(a, ctx, solver, t0)
    S, xq, wq = solver.matrix_dg_dp.basis_1d()
    h = 1.9 / a.coarse / 2 ** a.n_refine
    S3, w3 = S, wq                                           # tensor products over the dim directions, x fastest
    for _ in range(dim - 1):
        S3, w3 = np.kron(S, S3), np.kron(wq, w3)
    w3 = w3 * h ** dim
    ref = np.stack(np.meshgrid(*([xq] * dim), indexing="ij"), axis=-1)[..., ::-1].reshape(-1, dim)  # (k, j, i) order
    x = -0.9 + h * (solver.cell_ijk[-1].astype(float)[:, None, :] + ref[None, :, :])
    if a.solution == "reference":
        u = np.prod(np.sin(np.pi * WAVE * x), axis=-1)
        f = dim * (np.pi * WAVE) ** 2 * u
    else:
        k = np.pi * WAVE / 1.9
        u = np.prod(np.sin(k * (x + 0.9)), axis=-1)
        f = dim * k ** 2 * u
    rhs = (f * w3) @ S3                                      # multigrid_solver_dg_plain.h:163-185
    print("Time setup                    %.3f s   rhs_norm = %.6e" % (time.time() - t0, np.sqrt(float(np.sum(rhs ** 2)))))
    b, sol = solver.initialize_dof_vector(rhs.ravel()), solver.initialize_dof_vector()
    time_cg = 1e10
    for _ in range(4):
        ctx.sync()
        t = time.perf_counter()
        its, red = solver.solve_cg(b, sol, a.tolerance)
        ctx.sync()
        dt = time.perf_counter() - t
        time_cg = min(time_cg, dt)
        print("Time solve CG                 %.6f s   (%d iterations, reduction %.4e)" % (dt, its, red))
    uh = sol.download()[:n].reshape(nc, -1) @ S3.T
    l2 = np.sqrt(float(np.sum(w3 * (uh - u) ** 2)) / (nc * h ** dim))
    report(a, ctx, solver, b, sol, l2, time_cg, its, red)


def with_boundary_data(a, ctx, solver, t0):
    """--boundary data: right-hand side with g = u and the error on the device"""
    dim, A = a.dim, solver.matrix_dg_dp
    if a.solution == "reference":
        k, phase = np.pi * WAVE, 0.0
    else:
        k = np.pi * WAVE / 1.9
        phase = 0.9 * k
    u = mg.DGFunction.sine_product(1.0, (k,) * dim, (phase,) * dim)
    f = mg.DGFunction.sine_product(dim * k ** 2, (k,) * dim, (phase,) * dim)
    b, sol = solver.initialize_dof_vector(), solver.initialize_dof_vector()
    print("Time setup                    %.3f s" % (time.time() - t0))
    ctx.sync()
    t = time.perf_counter()
    A.compute_rhs(b, f, u, u if a.neumann else None)
    ctx.sync()
    dt = time.perf_counter() - t
    print("Time compute rhs              %.6f s   rhs_norm = %.6e" % (dt, ctx.l2_norm(b)))
    time_cg = 1e10
    for _ in range(4):
        ctx.sync()
        t = time.perf_counter()
        its, red = solver.solve_cg(b, sol, a.tolerance)
        ctx.sync()
        dt = time.perf_counter() - t
        time_cg = min(time_cg, dt)
        print("Time solve CG                 %.6f s   (%d iterations, reduction %.4e)" % (dt, its, red))
    sums = A.compute_l2_error(sol, u)                         # one rank: nothing to add up
    report(a, ctx, solver, b, sol, float(np.sqrt(sums[0] / sums[1])), time_cg, its, red)


def report(a, ctx, solver, b, sol, l2, time_cg, its, red):
    n, n_levels = solver.m(), solver.n_levels
    nc = n // (a.degree + 1) ** a.dim
    if a.levels:
        solver.enable_timings(True)
        solver.solve_cg(b, sol, a.tolerance)
        t = solver.wall_times()
        solver.enable_timings(False)
        print("Coarse solver %d times: %.4g tot prec %.4g" % (int(t[0, 1]), t[0, 0], t[0, 0] + t[1:, [0, 1, 2, 5]].sum()))
        print("level  smoother    mg_mv     mg_vec    restrict  prolongate  inhomBC")
        for l in range(1, n_levels):
            print("L%-2d    %-12.4g%-10.4g%-10.4g%-10.4g%-12.4g%-10.4g" % (l, t[l, 5], t[l, 0], t[l, 4], t[l, 1], t[l, 2], t[l, 3]))
    best = {}
    for name, A in (("dp", solver.matrix_dg_dp), ("sp", solver.matrix[-1])):
        v, w = A.initialize_dof_vector(np.ones(n)), A.initialize_dof_vector()
        n_mv = 200 if n < 10000000 else 50
        best[name] = 1e10
        for _ in range(5):
            ctx.sync()
            t = time.perf_counter()
            for _ in range(n_mv):
                A.vmult(w, v)
            ctx.sync()
            dt = (time.perf_counter() - t) / n_mv
            best[name] = min(best[name], dt)
            print("matvec time %s %.6e DoFs/s: %.5e" % (name, dt, n / dt))
        v.free(); w.free()
    print("Best timings for ndof = %d   mv %.6e    mv smooth %.6e   cg-mg %.6e" % (n, best["dp"], best["sp"], time_cg))
    print("L2 error with ndof = %d  %.6e" % (n, l2))
    print("cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction")
    print("%d %d %.4e %.4e %.4e %.4e %d %.4e  | %.3e DoFs/s solved per second of CG"
          % (nc, n, best["dp"], best["sp"], l2, time_cg, its, red, n / time_cg))
    solver.close()
    ctx.close()


if __name__ == "__main__":
    main()
