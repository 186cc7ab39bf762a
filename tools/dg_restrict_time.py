"""Time per call of the residual + DG -> FE_Q restriction of MultigridSolverDG in its two routes, in the same process on the
same vectors: the merged action of the cell kernel (mgx_dg_vmult_residual_and_restrict_to_cg, what the V-cycle runs) against
the pair it replaces (mgx_dg_vmult_residual, then mgx_dg_restrict_to_cg; context option dg_unmerged_restrict), and the
embedding FE_Q -> DG next to them.  HIP events around `--repeat` back-to-back calls after a warm-up, five such batches.

    python tools/dg_restrict_time.py [degree=3] [n_refine=9] [--dim 2|3] [--number f32|f64] [--repeat 20]

--dim 2 (default): Square(degree, 1, n_refine), 4^n_refine cells; --dim 3: Cube(degree, 1, n_refine), 8^n_refine cells."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def timed_batches(ctx, fn, repeat, batches=5):
    """best and median time per call in seconds over `batches` batches of `repeat` back-to-back calls"""
    stream = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(3):
        fn()
    out = []
    with torch.cuda.stream(stream):
        for _ in range(batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(repeat):
                fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3 / repeat)
    return min(out), float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=3)
    ap.add_argument("n_refine", nargs="?", type=int, default=9)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=2)
    ap.add_argument("--number", choices=["f32", "f64"], default="f32")
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    number = mg.F32 if a.number == "f32" else mg.F64
    ctx = mg.Context(0)
    mesh = mg.Square(a.degree, 1, a.n_refine) if a.dim == 2 else mg.Cube(a.degree, 1, a.n_refine)
    solver = mg.DGMultigridSolver(ctx, mesh, mg.DG_HERMITE, 3, number)
    n, n_cg = solver.m(), mesh.n_dofs(mesh.max_level)
    rng = np.random.default_rng(0)
    rhs, lhs, t = (ctx.vector(n, number, rng.standard_normal(n)) for _ in range(3))
    cg = ctx.vector(n_cg, number)
    print("FE_DGQHermite(%d) in %dD, %d cells, %d DG DoFs, %d FE_Q DoFs, %s, %d calls per batch"
          % (a.degree, a.dim, mesh.n_cells(mesh.max_level), n, n_cg, a.number, a.repeat))

    def pair():
        solver.matrix_dg.vmult_residual(t, rhs, lhs)
        solver.restrict_to_cg(cg, t)

    rows = [("merged residual + restriction", lambda: solver.vmult_residual_and_restrict_to_cg(cg, rhs, lhs)),
            ("residual, then restriction", pair),
            ("  residual alone", lambda: solver.matrix_dg.vmult_residual(t, rhs, lhs)),
            ("  restriction alone", lambda: solver.restrict_to_cg(cg, t)),
            ("embedding fe_q -> dg", lambda: solver.prolongate_add_cg_to_dg(t, cg))]
    best = {}
    for name, fn in rows:
        best[name], med = timed_batches(ctx, fn, a.repeat)
        print("%-32s best %9.2f us  median %9.2f us  %7.2f ps per DG DoF" % (name, best[name] * 1e6, med * 1e6, best[name] / n * 1e12))
    print("merged / pair: %.3f" % (best[rows[0][0]] / best[rows[1][0]]))
    solver.close()
    mesh.close()
    ctx.close()


if __name__ == "__main__":
    main()
