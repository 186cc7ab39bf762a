"""Harness of the FE_Q multigrid in two dimensions, mirroring poisson_cube/program.cc compiled with dimension = 2:
FE_Q(p) on the square [-0.9, 1]^2 (one cell refined n_refine times), u = sin(3 pi x) sin(3 pi y), Dirichlet values on
all four sides; the full multigrid cycle, then CG preconditioned with one V-cycle.

    python tools/poisson_cube_2d.py DEGREE N_REFINE [--number f32|f64]

--number: the number type of the V-cycle (reference default: f32 inside the fp64 outer iteration).

Prints the reference's table columns of the run -- cells, dofs, reduction, fmg_L2error, cg_L2error, cg_its -- as one
header line and one row, errors with 17 digits so that a reader can compare them with the solver's."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def run(degree, n_refine, number):
    ctx = mg.Context(0)
    square = mg.Square(degree, 1, n_refine)
    solver = mg.MultigridSolver(ctx, square, 3, 3, 1, number)
    lmax = square.max_level
    reduction, _ = solver.solve(True)
    fmg_error = solver.compute_l2_error()
    cg_its, _ = solver.solve_cg()
    cg_error = solver.compute_l2_error()
    row = dict(cells=square.n_cells(lmax), dofs=square.n_dofs(lmax), reduction=reduction, fmg_L2error=fmg_error,
               cg_L2error=cg_error, cg_its=cg_its)
    solver.close()
    square.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", type=int)
    ap.add_argument("n_refine", type=int)
    ap.add_argument("--number", choices=["f32", "f64"], default="f32")
    a = ap.parse_args()
    row = run(a.degree, a.n_refine, mg.F32 if a.number == "f32" else mg.F64)
    print("%10s %10s %12s %24s %24s %7s" % ("cells", "dofs", "reduction", "fmg_L2error", "cg_L2error", "cg_its"))
    print("%10d %10d %12.5e %24.17e %24.17e %7d" % (row["cells"], row["dofs"], row["reduction"], row["fmg_L2error"],
                                                   row["cg_L2error"], row["cg_its"]))


if __name__ == "__main__":
    main()
