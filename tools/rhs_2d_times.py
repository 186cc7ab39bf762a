"""Times the residual form of the two-dimensional cell loop (mgx_compute_residual_2d) against vmult of the same operator
in the same process, on both assembly routes, and the set-up of all right-hand sides of a hierarchy through the device
path against the host assembly.

    python tools/rhs_2d_times.py [--degree 4] [--refine 10] [--ball 9] [--repeat 20] [--groups 7] [--no-setup]

--refine R: the square [-0.9, 1]^2 with 2^R cells per direction (10: 1024^2 cells, 16.8 M unknowns at p = 4, the box of
profiles/feq_2d_times.txt).  --ball L: the disc refined L times on top (5 4^L cells; -1: none).

Kernel times: HIP events on the context's stream around `repeat` applications, `groups` times, the forms alternated
(vmult, residual, vmult, ...) after a warm-up of every form; best and median per application.  Bytes from shapes: the
residual form reads one more stream than vmult, rhs_q with (p+1)^2 values per cell, which is (p+1)^2 / p^2 values per
unknown -- printed next to the measured ratio.
Set-up: host clock around work that ends in a synchronisation -- (a) Square.problem_rhs_quadrature of every level (host
evaluation of f JxW), upload and mgx_solver_compute_rhs_2d, against (b) the host assembly of mgx_square_rhs of every
level on a fresh Square.  Nothing here is a pass criterion."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402
from multigrid_amd import _lib  # noqa: E402


def kernel_times(ctx, forms, repeat, groups):
    device = torch.device("cuda", ctx.device)
    stream = torch.cuda.ExternalStream(ctx.stream, device=device) if ctx.stream else torch.cuda.default_stream(device)
    times = {name: [] for name in forms}
    for fn in forms.values():
        for _ in range(3):
            fn()
    ctx.sync()
    with torch.cuda.stream(stream):
        for _ in range(groups):
            for name, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(repeat):
                    fn()
                t1.record(stream)
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / repeat)
    return times


def operator_times(a, sq, label):
    p, l = sq.degree, sq.max_level
    n_cells, n_dofs = sq.n_cells(l), sq.n_dofs(l)
    P = mg.SquareProblem("shell", 1.0)
    coef = sq.problem_coef_q(l, P)
    rhs_q = sq.problem_rhs_quadrature(l, P)
    x = sq.seeded_vector(l, 3)
    print("%s: p = %d, %d cells, %d unknowns, fp64, per-point tensor" % (label, p, n_cells, n_dofs))
    for route, options in (("ordered assembly", None), ("colour by colour", dict(cell_colour_min=1))):
        ctx = mg.Context(0, options=options)
        op = mg.LaplaceOperator.from_cube(ctx, sq, l, mg.F64, coef_q=coef)
        src, dst, f = ctx.vector(n_dofs, data=x), ctx.vector(n_dofs), ctx.vector(rhs_q.size, data=rhs_q.ravel())
        forms = {"vmult": lambda: op.vmult(dst, src), "residual": lambda: op.compute_residual(dst, src, f),
                 "residual, rhs_q = NULL": lambda: op.compute_residual(dst, src, None)}
        t = kernel_times(ctx, forms, a.repeat, a.groups)
        for name, v in t.items():
            print("  %-18s %-24s best %9.2f us  median %9.2f us  (%s)" % (route, name, min(v), float(np.median(v)),
                                                                         " ".join("%.1f" % u for u in v)))
        print("  %-18s residual / vmult: %.3f measured (medians); one more stream of 8 B per quadrature point = %.2f B per "
              "unknown" % (route, np.median(t["residual"]) / np.median(t["vmult"]), 8.0 * n_cells * (p + 1) ** 2 / n_dofs))
        for v in (src, dst, f):
            v.free()
        op.clear()
        ctx.close()


def setup_times(a):
    ctx = mg.Context(0)
    sq = mg.Square(a.degree, 1, a.refine)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64, problem=mg.SquareProblem("cube"))   # (its own rhs: warm-up)
    lib, P = ctx.lib, mg.SquareProblem("cube")
    ctx.sync()
    t = time.perf_counter()
    t_eval = 0.0
    for l in range(sq.n_levels):
        t1 = time.perf_counter()
        fq = sq.problem_rhs_quadrature(l, P)
        t_eval += time.perf_counter() - t1
        dev = ctx.vector(fq.size, data=fq.ravel())
        _lib.check(lib.mgx_solver_compute_rhs_2d(solver.h, l, dev.ptr))
        ctx.sync()
        dev.free()
    t_dev = time.perf_counter() - t
    solver.close()
    sq.close()
    sq = mg.Square(a.degree, 1, a.refine)   # (mgx_square_rhs keeps what it assembled: a fresh square)
    t = time.perf_counter()
    for l in range(sq.n_levels):
        sq.lib.mgx_square_rhs(sq.h, l)
    t_host = time.perf_counter() - t
    print("set-up of all %d right-hand sides, p = %d, %d unknowns on the finest level:" % (sq.n_levels, a.degree, sq.n_dofs(sq.max_level)))
    print("  device path (f JxW on the host %.3f s, upload, kernel)  %.3f s" % (t_eval, t_dev))
    print("  host assembly (mgx_square_rhs)                           %.3f s" % t_host)
    sq.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--refine", type=int, default=10)
    ap.add_argument("--ball", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--no-setup", action="store_true")
    a = ap.parse_args()
    sq = mg.Square(a.degree, 1, a.refine)
    operator_times(a, sq, "box")
    sq.close()
    if a.ball >= 0:
        sq = mg.Square(a.degree, n_refine=a.ball, mapped="ball")
        operator_times(a, sq, "disc level %d" % a.ball)
        sq.close()
    if not a.no_setup:
        setup_times(a)


if __name__ == "__main__":
    main()
