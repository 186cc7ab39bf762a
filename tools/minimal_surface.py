#!/usr/bin/env python3
"""minimal_surface/program.cc in 3D on the cube [-0.9, 1]^3: -div(grad u / sqrt(1 + |grad u|^2)) = 0 with the boundary
values A sin(2 pi (x + y)) of the reference's Solution (:97-99; independent of z, so the problem keeps the character of
the 2D one), Newton's method with V-cycle-preconditioned CG at ReductionControl(m, 1e-13, 1e-4) per step and the
step-halving line search (:414-573), at most 100 steps or until the residual norm is below --tolerance (:656-662).
Prints the reference's lines: "Residual norm: ... in ... steps to ...", "Computing times: nl iterations: ...".

--geometry: the same on a mapped mesh with curved cells (per-point geometry): the sheared box, one equiangular sector of
the shell (a box of one coarse cell, n_refine times refined) or the whole hyper_shell(0, 0.5, 1, 6 | 12).

--dim 2: the program as shipped (dimension = 2, :73) on the square [-0.9, 1]^2, the sheared square or the quarter annulus
with curved cells (--geometry square|sheared|annulus_sector), or on the mesh the program itself uses, the unit disc
(--geometry ball: hyper_ball with a SphericalManifold on the boundary, :630-634; "4 3" is its first cycle, 320 cells).

Usage: python tools/minimal_surface.py [degree] [n_refine] [--amplitude A] [--vcycle f32|f64] [--tolerance T]
                                       [--geometry cube|sheared|shell_sector|shell6|shell12]
                                       [--dim 2 [--geometry square|sheared|annulus_sector|ball]]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", type=int, nargs="?", default=2)
    ap.add_argument("n_refine", type=int, nargs="?", default=3)
    ap.add_argument("--amplitude", type=float, default=1.0)
    ap.add_argument("--vcycle", choices=["f32", "f64"], default="f32", help="number type of the V-cycle (level_number)")
    ap.add_argument("--tolerance", type=float, default=1e-12, help="stop when the residual norm is below (:660)")
    ap.add_argument("--max-steps", type=int, default=100, help="n_inner_iterations (:620)")
    ap.add_argument("--geometry", choices=["cube", "sheared", "shell_sector", "shell6", "shell12", "square", "annulus_sector", "ball"],
                    default=None)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3, help="2: the program's own dimension (:73), on a Square")
    args = ap.parse_args()
    if args.geometry is None:
        args.geometry = "cube" if args.dim == 3 else "square"
    allowed = ("square", "sheared", "annulus_sector", "ball") if args.dim == 2 else ("cube", "sheared", "shell_sector", "shell6", "shell12")
    if args.geometry not in allowed:
        ap.error("--dim %d takes --geometry %s" % (args.dim, " | ".join(allowed)))

    ctx = mg.Context(0)
    if args.dim == 2:
        if args.geometry in ("annulus_sector", "ball"):
            cube = mg.Square(args.degree, 1, args.n_refine, mapped=args.geometry)
        else:
            cube = mg.Square(args.degree, 1, args.n_refine, jacobian=[[1.0, 0.35], [0.15, 0.8]] if args.geometry == "sheared" else None)
    elif args.geometry == "cube":
        cube = mg.Cube(args.degree, 1, args.n_refine)
    elif args.geometry in ("sheared", "shell_sector"):
        cube = mg.Cube(args.degree, n_refine=args.n_refine, box=(1, 1, 1), origin=-0.9, h0=1.9, geometry=args.geometry)
    else:
        cube = mg.Cube(args.degree, n_refine=args.n_refine, shell=int(args.geometry[5:]), problem="cube")
    print("Testing FE_Q<%d>(%d)" % (args.dim, args.degree))
    if args.dim == 2 and args.geometry != "ball":
        print("Number of degrees of freedom: %d (%s, %d x %d cells, %d levels)"
              % ((cube.n_dofs(cube.max_level), args.geometry) + cube.cells_per_dim2(cube.max_level) + (cube.n_levels,)), flush=True)
    elif args.geometry == "cube":
        print("Number of degrees of freedom: %d (%d^3 cells, %d levels)"
              % (cube.n_dofs(cube.max_level), cube.cells_per_dim(cube.max_level), cube.n_levels), flush=True)
    else:
        print("Number of degrees of freedom: %d (%s, %d cells, %d levels)"
              % (cube.n_dofs(cube.max_level), args.geometry, cube.n_cells(cube.max_level), cube.n_levels), flush=True)
    t0 = time.perf_counter()
    amplitude = args.amplitude
    problem = mg.MinimalSurfaceProblem(ctx, cube, lambda x: amplitude * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])),
                                       mg.F32 if args.vcycle == "f32" else mg.F64)
    ctx.sync()
    print("Setup time                            %g s" % (time.perf_counter() - t0))
    log = lambda line: print(line, flush=True)
    t0 = time.perf_counter()
    steps = problem.run(args.max_steps, args.tolerance, log)
    ctx.sync()
    total = time.perf_counter() - t0
    print("Computing times: nl iterations: %d residuals %d %g  linear solver %d %g  coefficients %d %g  total %g"
          % (steps, problem.n_residual, problem.time_residual, problem.linear_iterations, problem.time_solve, steps,
             problem.time_coefficient, total))
    print("CG iterations per Newton step: %s" % " ".join(str(h[3]) for h in problem.history))
    first, last = problem.history[0][0], problem.history[-1][2]
    print("%s: residual norm %.6g -> %.6g in %d Newton steps" % ("Converged" if last < 1e-10 * first else "Not converged", first, last, steps))
    problem.close()
    cube.close()
    ctx.close()
    return 0 if last < 1e-10 * first else 1


if __name__ == "__main__":
    sys.exit(main())
