"""Harness of BASELINE config 5's solver, mirroring poisson_dg/program.cc: FE_DGQHermite(p) on the cube
[-0.9, 1]^3, rhs 3 (3 pi)^2 prod sin(3 pi x_d), V-cycle-preconditioned CG with the DG level on top of the
FE_Q(p) multigrid (fp32 V-cycle inside the fp64 outer iteration, program.cc:72-73).

    python tools/poisson_dg.py [degree=3] [n_refine=5] [n_pre_smooth=3] [tolerance=1e-9] [--vcycle f32|f64] [--gpus N] [--dim 2]

--dim 2: the program with dimension = 2 -- the square [-0.9, 1]^2, rhs 2 (3 pi)^2 prod sin(3 pi x_d), the same lines and
table row; one GPU.

--gpus N: the cube is block-split over N ranks (2x1x1 / 2x2x1 / 2x2x2 coarse cells of the mesh with n_subdiv = 2,
refined n_refine - 1 times: the same cells as on one GPU), one process per GPU, started by this script or by
torch.distributed.run; MGX_BENCH_BACKEND=gloo runs the ranks on one GPU (functional test).

The reference's right-hand side is the volume integral alone (multigrid_solver_dg.h:243-262) while its solution
prod sin(3 pi x_d) does not vanish at x_d = -0.9, and the operator imposes homogeneous Dirichlet values: the
"L2 error" of this benchmark (0.1007 at every resolution, here as there) measures that mismatch, not the
discretisation.  --solution vanishing solves for prod sin(3 pi (x_d + 0.9) / 1.9) instead, which is zero on the
whole boundary: its L2 error falls with h^(p+1) (tests/test_gpu_dg_multigrid.py).

Prints the reference's lines ("Time solve CG", "matvec time dp/sp ... DoFs/s", "L2 error with ndof = ...") and
the row of its convergence table (cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction,
program.cc:318-325).  Right-hand side and error norm are evaluated on the host (numpy), as the reference does
on the CPU; everything timed runs on the GPU.

--boundary data: the right-hand side also carries the boundary values of the chosen solution, b_i += int_F u (sigma_F
phi_i - d_n phi_i) on every Dirichlet face, so the reference solution converges as well.  Right-hand side and error sums
are then formed on the device (DGLaplaceOperator.compute_rhs / compute_l2_error; the sums are added over the ranks
here) and a line "Time compute rhs" is printed as the reference prints it (multigrid_solver_dg.h).  The default,
homogeneous, is the reference's volume-only vector from the host: nothing it prints changes."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402

WAVE = 3.0


def quad_points(cube, ijk, xq, h):
    """[cell, q = (k, j, i), dim] coordinates of the Gauss points; dim = the columns of ijk"""
    dim = ijk.shape[1]
    ref = np.stack(np.meshgrid(*([xq] * dim), indexing="ij"), axis=-1)[..., ::-1].reshape(-1, dim)  # (k, j, i) order
    return -0.9 + h * (ijk[:, None, :] + ref[None, :, :])


def kron_power(a, dim):
    """a x a (x a)"""
    out = a
    for _ in range(dim - 1):
        out = np.kron(a, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=3)
    ap.add_argument("n_refine", nargs="?", type=int, default=5)
    ap.add_argument("n_pre_smooth", nargs="?", type=int, default=3)
    ap.add_argument("tolerance", nargs="?", type=float, default=1e-9)
    ap.add_argument("--vcycle", choices=["f32", "f64"], default="f32")
    ap.add_argument("--basis", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3,
                    help="2: the program with dimension = 2, on the square [-0.9, 1]^2 (one GPU)")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="context option (include/mgx.h mgx_context_set_option), e.g. dg_unmerged_restrict=1")
    ap.add_argument("--solution", choices=["reference", "vanishing"], default="reference",
                    help="reference: prod sin(3 pi x_d) as program.cc:95-100; vanishing: zero on the boundary (convergence check)")
    ap.add_argument("--boundary", choices=["homogeneous", "data"], default="homogeneous",
                    help="data: boundary values of the solution in the right-hand side; rhs and error on the device")
    a = ap.parse_args()
    dim = a.dim
    if dim == 2 and a.gpus > 1:
        raise SystemExit("poisson_dg.py: --dim 2 runs on one GPU (the 2D solver is not decomposed); drop --gpus %d" % a.gpus)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn(a.gpus)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    dist = comm = None
    if world > 1:
        import torch
        import torch.distributed as dist
        if os.environ.get("MGX_BENCH_BACKEND", "nccl") == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            local_rank = 0
            dist.init_process_group(os.environ["MGX_BENCH_BACKEND"])
    say = print if rank == 0 else (lambda *x, **k: None)

    def total(v):
        if dist is None:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t)
        return float(t.item())

    def slowest(v):
        if dist is None:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    vnum = mg.F32 if a.vcycle == "f32" else mg.F64
    t0 = time.time()
    ctx = mg.Context(local_rank, options={k: float(v) for k, v in (o.split("=") for o in a.option)})
    if world > 1:
        comm = mg.Communicator(ctx, dist)
        if comm.native_ready:
            mg.check(ctx.lib.mgx_context_use_rccl(ctx.h, 1))
        cube = mg.Cube(a.degree, n_refine=a.n_refine - 1, box=(2, 2, 2), procs=mg.process_grid(world), rank=rank,
                       origin=-0.9, h0=0.95)
    elif dim == 2:
        cube = mg.Square(a.degree, 1, a.n_refine)
    else:
        cube = mg.Cube(a.degree, 1, a.n_refine)
    solver = mg.DGMultigridSolver(ctx, cube, a.basis, a.n_pre_smooth, vnum, comm=comm)
    n_own = solver.m()
    n = int(round(total(n_own)))
    nc = n // (a.degree + 1) ** dim
    nc_own = n_own // (a.degree + 1) ** dim
    say("Number of degrees of freedom: %d (%d cells, FE_DGQHermite(%d) on FE_Q(%d) multigrid, V-cycle in %s, %d GPU%s)"
        % (n, nc, a.degree, a.degree, a.vcycle, world, "" if world == 1 else "s"))
    on_device = a.boundary == "data"
    if on_device:
        kw = np.pi * WAVE if a.solution == "reference" else np.pi * WAVE / 1.9
        phase = 0.0 if a.solution == "reference" else 0.9 * kw
        u_dev = mg.DGFunction.sine_product(1.0, (kw,) * dim, (phase,) * dim)
        f_dev = mg.DGFunction.sine_product(dim * kw ** 2, (kw,) * dim, (phase,) * dim)
        b, sol = solver.initialize_dof_vector(), solver.initialize_dof_vector()
        say("Time setup                    %.3f s" % (time.time() - t0))
        ctx.sync()
        t = time.perf_counter()
        solver.matrix_dg_dp.compute_rhs(b, f_dev, u_dev)
        ctx.sync()
        dt = slowest(time.perf_counter() - t)
        say("Time compute rhs              %.6f s   rhs_norm = %.6e" % (dt, np.sqrt(total(float(np.sum(b.download()[:n_own] ** 2))))))
    else:
        S, xq, wq = solver.matrix_dg.basis_1d()
        h = cube.cell_size(cube.max_level)
        S3 = kron_power(S, dim)
        w3 = kron_power(wq, dim) * h ** dim
        x = quad_points(cube, solver.cell_ijk.astype(float), xq, h)
        if a.solution == "reference":
            u = np.prod(np.sin(np.pi * WAVE * x), axis=-1)
            f = dim * (np.pi * WAVE) ** 2 * u                    # program.cc:137-141
        else:
            k = np.pi * WAVE / 1.9
            u = np.prod(np.sin(k * (x + 0.9)), axis=-1)
            f = dim * k ** 2 * u
        rhs = (f * w3) @ S3                                      # multigrid_solver_dg.h:243-262
        say("Time setup                    %.3f s   rhs_norm = %.6e" % (time.time() - t0, np.sqrt(total(float(np.sum(rhs ** 2))))))
        b, sol = solver.initialize_dof_vector(rhs.ravel()), solver.initialize_dof_vector()
    time_cg = 1e10
    for _ in range(4):                                          # program.cc:252-258
        ctx.sync()
        t = time.perf_counter()
        its, red = solver.solve_cg(b, sol, a.tolerance)
        ctx.sync()
        dt = slowest(time.perf_counter() - t)
        time_cg = min(time_cg, dt)
        say("Time solve CG                 %.6f s   (%d iterations, reduction %.4e)" % (dt, its, red))
    if on_device:
        sums = solver.matrix_dg_dp.compute_l2_error(sol, u_dev)               # this rank's cells
        l2 = np.sqrt(total(float(sums[0])) / total(float(sums[1])))
    else:
        uh = sol.download()[:n_own].reshape(nc_own, -1) @ S3.T
        l2 = np.sqrt(total(float(np.sum(w3 * (uh - u) ** 2))) / (nc * h ** dim))  # multigrid_solver_dg.h:328-367
    A_dp, A_sp = solver.matrix_dg_dp, solver.matrix_dg
    best = {}
    for name, A, number in (("dp", A_dp, mg.F64), ("sp", A_sp, vnum)):
        v, w = A.initialize_dof_vector(np.ones(n_own)), A.initialize_dof_vector()
        n_mv = 200 if n < 10000000 else 50
        best[name] = 1e10
        for _ in range(5):
            ctx.sync()
            t = time.perf_counter()
            for _ in range(n_mv):
                A.vmult(w, v)
            ctx.sync()
            dt = slowest((time.perf_counter() - t) / n_mv)
            best[name] = min(best[name], dt)
            say("matvec time %s %.6e DoFs/s: %.5e" % (name, dt, n / dt))
        v.free(); w.free()
    say("Best timings for ndof = %d   mv %.6e    mv smooth %.6e   cg-mg %.6e" % (n, best["dp"], best["sp"], time_cg))
    say("L2 error with ndof = %d  %.6e" % (n, l2))
    say("cells dofs mv_outer mv_inner cg_L2error cg_time cg_its cg_reduction")
    say("%d %d %.4e %.4e %.4e %.4e %d %.4e  | %.3e DoFs/s solved per second of CG"
          % (nc, n, best["dp"], best["sp"], l2, time_cg, its, red, n / time_cg))
    solver.close()
    cube.close()
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def spawn(n):
    """start n ranks of this script (the parent never touches the GPU)"""
    codes = mg.spawn_ranks(__file__, sys.argv[1:], n, one_gpu=os.environ.get("MGX_BENCH_BACKEND", "nccl") != "nccl")
    if any(codes):
        raise SystemExit("poisson_dg.py: rank exit codes %s" % codes)


if __name__ == "__main__":
    main()
