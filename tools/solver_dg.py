"""Harness mirroring solver_dg/program.cc: conjugate gradients on the DG-SIP operator, preconditioned by the inverse
lumped mass matrix, in the program's two forms -- "cell-based loops" (textbook PCG from separate kernels, scalars on the
host: DG_PCG_SEPARATE) and "interleaved loops" (the whole iteration on the device, three launches: DG_PCG_MERGED).

    python tools/solver_dg.py degree n_cell_steps n_iterations [--dim 2] [--basis 0,1,2] [--number f32|f64] [--outer 3] [--json]

Same positional arguments as the reference program (program.cc:287-300) on the mesh of mgx_dg_cheby_mesh (the
construction of program.cc:89-113; --dim 2: the same formulas with dim = 2), a right-hand side of random numbers in
[0, 1) (:157-158), n_iterations iterations without a tolerance (IterationNumberControl, :177).  Prints the reference's
result lines ("Best MF cell-based ...", :234-239, "Best MF interleaved ...", :256-261; GB/s in the reference's
17-access model, :238) and "Verification of result:", the max-norm difference of the two forms' solutions (:240-241,
262-263), then the time of the plain mgx_dg_vmult of the same operator and the ratio of the two forms.  The merged form
moves 10 vector accesses per DoF and iteration (cell kernel: p, r read, q written; update: x, p, r, q read, x, r, p
written), which is what its roofline fraction is computed from.

Times are wall-clock seconds per iteration around a synchronised solve, the best of --outer solves after one warm-up
solve; with no tolerance a merged solve synchronises once, at its end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402

from matvec_dg_cheby import NAMES, cheby_mesh_2d  # noqa: E402


def ops_approx(n_cells, degree, kind, dim):
    """flop model of solver_dg/program.cc:193-214"""
    p, n1 = degree, degree + 1
    interp = 2 * ((p + 1) // 2) * 2 + p + 1 + 2 * ((p - 1) * (p + 1) // 2)
    per_cell = ((4 if kind < 2 else 2) * dim * interp * n1 ** (dim - 1) + dim * 2 * dim * n1 ** dim
                + (2 * dim * ((5 * (dim - 1) if kind < 2 else 3 * (dim - 1)) * interp * n1 ** (dim - 2)
                              + (4 * dim - 1 + 2 + 2 + 3 + 2 * dim) * n1 ** (dim - 1))
                   + ((dim + 2 if kind == 0 else 2 * dim) * (p + 1 + 2 * (p - 1) + 2) * 2
                      + (((dim - 2) * 4 + 2 * dim * 2) if kind == 0 else 4 * dim * (2 * p + 1))) * n1 ** (dim - 1)))
    return n_cells * per_cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", type=int)
    ap.add_argument("n_cell_steps", type=int)
    ap.add_argument("n_iterations", type=int)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3)
    ap.add_argument("--basis", default="2", help="comma-separated MGX_DG_* (the reference runs 2, program.cc:280-282)")
    ap.add_argument("--number", choices=["f32", "f64"], default="f64")
    ap.add_argument("--outer", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    number = mg.F32 if a.number == "f32" else mg.F64
    nbytes = 4 if number == mg.F32 else 8
    ctx = mg.Context(0)
    cells, jac = mg.dg_cheby_mesh(a.n_cell_steps) if a.dim == 3 else cheby_mesh_2d(a.n_cell_steps)
    nb, _ = mg.dg_box_neighbours(cells)
    n_cells = int(np.prod(cells))
    print("Degree of element:              %d" % a.degree)
    print("Cells:                          %s, number type %s" % (" x ".join(str(c) for c in cells), a.number))
    results = []
    for kind in [int(k) for k in a.basis.split(",")]:
        op = mg.DGLaplaceOperator(ctx, a.degree, kind, nb, jac, number, dim=a.dim)
        n = op.m()
        if kind == int(a.basis.split(",")[0]):
            print("Number of DoFs: %d" % n)
        rhs = op.initialize_dof_vector(np.random.default_rng(0).random(n))   # program.cc:157-158
        x = {form: op.initialize_dof_vector() for form in (mg.DG_PCG_SEPARATE, mg.DG_PCG_MERGED)}
        best, hist = {}, {}
        ops = ops_approx(n_cells, a.degree, kind, a.dim)
        for form, label, word in ((mg.DG_PCG_SEPARATE, "cell-based ", "cell-based"), (mg.DG_PCG_MERGED, "interleaved", "interleaved")):
            S = mg.DGConjugateGradient(op, form, a.n_iterations)
            S.solve(rhs, x[form])                                             # warm-up
            best[form] = 1e10
            for _ in range(a.outer):
                ctx.sync()
                t = time.perf_counter()
                its, _ = S.solve(rhs, x[form])
                ctx.sync()
                per_it = (time.perf_counter() - t) / max(1, a.n_iterations)
                print("Solve with %s loops: %.4e" % (word, per_it))
                best[form] = min(best[form], per_it)
            hist[form] = S.history()
            S.close()
            tb = best[form]
            print("Best MF %s %s n_dof= %-12d%-12.4e   DoFs/s %.5e    GFlop/s %.1f    GB/s %.1f    ops/dof %.1f"
                  % (label, NAMES[kind], n, tb, n / tb, 1e-9 * ops / tb, 1e-9 * n * nbytes * 17 / tb, ops / n)
                  + ("    [10 accesses: %.1f GB/s = %.3f of 8 TB/s]" % (1e-9 * 10 * nbytes * n / tb, 10 * nbytes * n / tb / 8e12)
                     if form == mg.DG_PCG_MERGED else ""))
            if form == mg.DG_PCG_MERGED:
                xs = x[mg.DG_PCG_SEPARATE].download().astype(float)
                diff = np.abs(x[mg.DG_PCG_MERGED].download().astype(float) - xs).max()
                print("Verification of result: %.6e   (max |x| = %.3e)" % (diff, np.abs(xs).max()))
        # the plain operator application of the same operator in the same process
        q = op.initialize_dof_vector()
        op.vmult(q, rhs)
        ctx.sync()
        t = time.perf_counter()
        for _ in range(max(1, a.n_iterations)):
            op.vmult(q, rhs)
        ctx.sync()
        tv = (time.perf_counter() - t) / max(1, a.n_iterations)
        ratio = best[mg.DG_PCG_MERGED] / best[mg.DG_PCG_SEPARATE]
        print("MF vmult             %s n_dof= %-12d%-12.4e   DoFs/s %.5e    [2 accesses: %.3f of 8 TB/s]"
              % (NAMES[kind], n, tv, n / tv, 2 * nbytes * n / tv / 8e12))
        print("interleaved / cell-based time per iteration: %.3f   (byte model: 10 / 17 = 0.59); residual reduction "
              "sqrt(rho_n / rho_0) = %.3e / %.3e\n" % (ratio, np.sqrt(hist[mg.DG_PCG_MERGED][-1] / hist[mg.DG_PCG_MERGED][0]),
                                                      np.sqrt(hist[mg.DG_PCG_SEPARATE][-1] / hist[mg.DG_PCG_SEPARATE][0])))
        results.append(dict(dim=a.dim, basis=NAMES[kind].strip(), degree=a.degree, n_dofs=n, dtype=a.number,
                            iterations=a.n_iterations, seconds_separate=best[mg.DG_PCG_SEPARATE],
                            seconds_merged=best[mg.DG_PCG_MERGED], seconds_vmult=tv, merged_over_separate=ratio,
                            verification=float(diff)))
        for v in (rhs, q, *x.values()):
            v.free()
        op.clear()
    if a.json:
        print(json.dumps(dict(metric="seconds per PCG iteration, DG-SIP operator with lumped-mass preconditioner", results=results)))
    ctx.close()


if __name__ == "__main__":
    main()
