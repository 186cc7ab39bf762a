"""Time of the DG-to-DG level transfer (mgx_dg_transfer_prolongate_and_add / _restrict_and_add) per call, HIP events,
warm, against the DG <-> FE_Q transfers of MultigridSolverDG (mgx_dg_prolongate_add_cg_to_dg / mgx_dg_restrict_to_cg)
on the same fine cells in the same process, and as a fraction of a streaming ceiling.

    python tools/dg_transfer_time.py [degree=4] [n_refine=6] [--number f32|f64] [--repeat 20] [--ceiling 4.9e12] [--dim 2]
                                     [--degrees PF PC]

--degrees PF PC: the transfer between the degrees PC < PF on one mesh (mgx_dg_degree_transfer_*) next to the h transfer
of the fine degree PF, in the same process on the same 2^(dim n_refine) fine cells (the positional degree is not read):
time, bytes per second and time per fine DoF.  Accesses per fine DoF: prolongation 2 + (nc / nf)^dim, restriction
1 + 2 (nc / nf)^dim, with nf = PF + 1, nc = PC + 1.

--dim 2: the 2D transfers alone, on 4^n_refine fine cells in forest order (there is no FE_Q partner in 2D): 2 1/4
accesses per fine DoF for the prolongation, 1 1/2 for the restriction.

Fine mesh: 2^n_refine cells per direction (the cube provider's finest level, forest order: children[c][k] = 8 c + k).
Bytes per call: prolongation reads and writes the fine vector and reads the coarse one (2 1/8 accesses per fine DoF),
restriction reads the fine vector and reads and writes the coarse one (1 1/4).  --ceiling: bytes per second of the
fp64 copy of tools/microbench.hip."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def timed(ctx, fn, repeat):
    """best and median time per call in seconds, HIP events on the context's stream"""
    stream = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(3):
        fn()
    out = []
    with torch.cuda.stream(stream):
        for _ in range(repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3)
    return min(out), float(np.median(out))


def degree_transfer_rows(a, ctx, number, es):
    """--degrees: the degree transfer and the h transfer of the fine degree on the same fine cells"""
    (pf, pc), dim = a.degrees, a.dim
    n_cells = (1 << dim) ** a.n_refine
    nf, nc = n_cells * (pf + 1) ** dim, n_cells * (pc + 1) ** dim
    nh = nf >> dim                                            # the h transfer's coarse vector
    P = mg.DGDegreeTransfer(ctx, pf, pc, mg.DG_HERMITE, n_cells, number, dim)
    H = mg.DGLevelTransfer(ctx, pf, mg.DG_HERMITE, np.arange(n_cells, dtype=np.uint32).reshape(-1, 1 << dim), number)
    rng = np.random.default_rng(0)
    fine, coarse_p, coarse_h = (ctx.vector(n, number, rng.standard_normal(n)) for n in (nf, nc, nh))
    print("FE_DGQHermite(%d) <-> (%d) in %dD, %d cells, %d fine DoFs, %s" % (pf, pc, dim, n_cells, nf, a.number))
    rows = [("p %d->%d prolongate_and_add" % (pc, pf), lambda: P.prolongate_and_add(fine, coarse_p), es * (2 * nf + nc)),
            ("h p=%d prolongate_and_add" % pf, lambda: H.prolongate_and_add(fine, coarse_h), es * (2 * nf + nh)),
            ("p %d->%d restrict_and_add" % (pf, pc), lambda: P.restrict_and_add(coarse_p, fine), es * (nf + 2 * nc)),
            ("h p=%d restrict_and_add" % pf, lambda: H.restrict_and_add(coarse_h, fine), es * (nf + 2 * nh))]
    best = []
    for name, fn, nbytes in rows:
        b, med = timed(ctx, fn, a.repeat)
        best.append(b)
        print("%-28s best %9.2f us  median %9.2f us  %8.1f GB/s  %5.1f %% of the %.1f TB/s copy ceiling  %.3f ps per fine DoF"
              % (name, b * 1e6, med * 1e6, nbytes / b * 1e-9, 100 * nbytes / b / a.ceiling, a.ceiling * 1e-12, b / nf * 1e12))
    print("time per fine DoF, degree transfer / h transfer: prolongation %.3f   restriction %.3f" % (best[0] / best[1], best[2] / best[3]))
    P.clear()
    H.clear()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=4)
    ap.add_argument("n_refine", nargs="?", type=int, default=6)
    ap.add_argument("--number", choices=["f32", "f64"], default="f64")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--ceiling", type=float, default=4.9e12)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3)
    ap.add_argument("--degrees", type=int, nargs=2, metavar=("PF", "PC"), help="time the degree transfer PC <-> PF too")
    a = ap.parse_args()
    number, es = (mg.F32, 4) if a.number == "f32" else (mg.F64, 8)
    ctx = mg.Context(0)
    if a.degrees:
        return degree_transfer_rows(a, ctx, number, es)
    if a.dim == 2:
        p, n2 = a.degree, (a.degree + 1) ** 2
        n_fine_cells = 4 ** a.n_refine
        n_fine, n_coarse = n_fine_cells * n2, n_fine_cells // 4 * n2
        T = mg.DGLevelTransfer(ctx, p, mg.DG_HERMITE, np.arange(n_fine_cells, dtype=np.uint32).reshape(-1, 4), number)
        rng = np.random.default_rng(0)
        fine = ctx.vector(n_fine, number, rng.standard_normal(n_fine))
        coarse = ctx.vector(n_coarse, number, rng.standard_normal(n_coarse))
        print("FE_DGQHermite(%d) in 2D, %d fine cells, %d fine DoFs, %s" % (p, n_fine_cells, n_fine, a.number))
        for name, fn, nbytes in (("dg->dg prolongate_and_add 2D", lambda: T.prolongate_and_add(fine, coarse), es * (2 * n_fine + n_coarse)),
                                 ("dg->dg restrict_and_add 2D", lambda: T.restrict_and_add(coarse, fine), es * (n_fine + 2 * n_coarse))):
            best, med = timed(ctx, fn, a.repeat)
            print("%-34s best %9.2f us  median %9.2f us  %7.3f TB/s  %5.1f %% of the %.1f TB/s copy ceiling"
                  % (name, best * 1e6, med * 1e6, nbytes / best * 1e-12, 100 * nbytes / best / a.ceiling, a.ceiling * 1e-12))
        T.clear()
        ctx.close()
        return
    p, n3 = a.degree, (a.degree + 1) ** 3
    cube = mg.Cube(p, 1, a.n_refine)
    hybrid = mg.DGMultigridSolver(ctx, cube, mg.DG_HERMITE, 3, number)
    n_fine_cells = cube.n_cells(cube.max_level)
    n_fine, n_coarse = n_fine_cells * n3, n_fine_cells // 8 * n3
    n_cg = cube.n_dofs(cube.max_level)
    # the hybrid solver's cells are in forest order: the child table of the plain transfer on the same cells
    ijk = hybrid.cell_ijk.astype(np.int64)
    parent = ijk[::8] // 2
    assert all((ijk[k::8] == 2 * parent + [k & 1, (k >> 1) & 1, k >> 2]).all() for k in range(8)), "cells not in forest order"
    children = np.arange(n_fine_cells, dtype=np.uint32).reshape(-1, 8)
    T = mg.DGLevelTransfer(ctx, p, mg.DG_HERMITE, children, number)
    rng = np.random.default_rng(0)
    fine = ctx.vector(n_fine, number, rng.standard_normal(n_fine))
    coarse = ctx.vector(n_coarse, number, rng.standard_normal(n_coarse))
    cg = ctx.vector(n_cg, number, rng.standard_normal(n_cg))
    print("FE_DGQHermite(%d), %d fine cells, %d fine DoFs, %s" % (p, n_fine_cells, n_fine, a.number))
    rows = [("dg->dg prolongate_and_add", lambda: T.prolongate_and_add(fine, coarse), es * (2 * n_fine + n_coarse)),
            ("dg->dg restrict_and_add", lambda: T.restrict_and_add(coarse, fine), es * (n_fine + 2 * n_coarse)),
            ("fe_q->dg prolongate_add_cg_to_dg", lambda: hybrid.prolongate_add_cg_to_dg(fine, cg), es * (2 * n_fine + n_cg)),
            ("dg->fe_q restrict_to_cg", lambda: hybrid.restrict_to_cg(cg, fine), es * (n_fine + 2 * n_cg))]
    res = {}
    for name, fn, nbytes in rows:
        best, med = timed(ctx, fn, a.repeat)
        res[name] = best
        print("%-34s best %9.2f us  median %9.2f us  %7.3f TB/s  %5.1f %% of the %.1f TB/s copy ceiling"
              % (name, best * 1e6, med * 1e6, nbytes / best * 1e-12, 100 * nbytes / best / a.ceiling, a.ceiling * 1e-12))
    print("ratio prolongation dg->dg / fe_q->dg: %.3f   restriction dg->dg / dg->fe_q: %.3f"
          % (res[rows[0][0]] / res[rows[2][0]], res[rows[1][0]] / res[rows[3][0]]))
    T.clear()
    hybrid.close()
    cube.close()
    ctx.close()


if __name__ == "__main__":
    main()
