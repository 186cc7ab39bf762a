"""Times the two-dimensional FE_Q path on one GPU: vmult, one Chebyshev step (PreconditionChebyshev::step with the
level's smoother) and one V-cycle on the square [-0.9, 1]^2, next to the three-dimensional per-cell path (context
option "no_bricks": the same design one dimension up) at a comparable number of unknowns.

    python tools/feq_2d_times.py [--degree 4] [--refine 10] [--refine3d 6] [--number f64|f32] [--reps 20]
                                 [--colour] [--no-vcycle]

--refine R: 2^R cells per direction (10: 1024^2 cells, 16.8 M unknowns at p = 4; 11: 2048^2, whose (p+1)^2 local values
per cell exceed the 2^26 of the ordered assembly at p = 4, so that level runs colour by colour).
--colour: context option cell_colour_min = 1, every level colour by colour.
--no-vcycle: operator only (no hierarchy: the large sizes fit that way).

Per form: time per application (host clock around `reps` applications between two synchronisations, after a warm-up),
unknowns per second, the bytes per unknown the form moves by its own design (counted from the shapes, the scratch round
trip of the ordered assembly and the index tables included; listed with the result) and the share of 8 TB/s those
bytes per second are.  Nothing here is a pass criterion."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402

PEAK = 8.0e12


def timed(ctx, reps, f):
    for _ in range(3):
        f()
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    ctx.sync()
    return (time.perf_counter() - t) / reps


def bytes_per_dof(dim, p, size, n_cells, n_dofs, ordered, form):
    """what one application moves by design.  Ordered assembly: the source, (p+1)^dim local values per cell written and
    read back (with a 4-byte position each), a 4-byte start per unknown, the result; colour route: the source, the
    result read and written (the zeroing before it: one more write).  Index table: 4 bytes per entity and cell.
    Chebyshev step: b, the inverse diagonal and x_old (read and written) on top, x written instead of dst."""
    local = n_cells * (p + 1) ** dim / n_dofs
    index = 4 * 3 ** dim * n_cells / n_dofs
    if ordered:
        b = size + local * size + local * (size + 4) + 4 + size
    else:
        b = size + 3 * size
    if form == "chebyshev":
        b += 4 * size if ordered else 6 * size   # unfused on the colour route: t written and read, then the update
    return b + index


def report(name, t, n_dofs, bpd):
    print("  %-22s %9.3f ms  %8.3f GDoF/s  %6.1f B/DoF  %5.1f %% of 8 TB/s" %
          (name, t * 1e3, n_dofs / t * 1e-9, bpd, 100 * n_dofs * bpd / t / PEAK))


def run(ctx, provider, dim, number, reps, vcycle, label):
    p, l = provider.degree, provider.max_level
    n_cells, n_dofs = provider.n_cells(l), provider.n_dofs(l)
    size = 8 if number == mg.F64 else 4
    ordered = n_cells * (p + 1) ** dim <= 1 << 26 and not getattr(ctx, "colour", False)
    print("%s: p = %d, %d cells, %d unknowns, %s, %s" % (label, p, n_cells, n_dofs, "fp64" if size == 8 else "fp32",
                                                       "ordered assembly" if ordered else "colour by colour"))
    x = provider.seeded_vector(l, 3).astype(np.float64 if size == 8 else np.float32)
    if vcycle:
        solver = mg.MultigridSolver(ctx, provider, 3, 3, 1, number)
        op, sm = solver.matrix(l), solver.smoother(l)
    else:
        solver, op = None, mg.LaplaceOperator.from_cube(ctx, provider, l, number)
        sm = mg.Chebyshev(op, 20.0, 3, 15)
    src, dst, b = ctx.vector(n_dofs, number, data=x), ctx.vector(n_dofs, number), ctx.vector(n_dofs, number, data=x[::-1].copy())
    report("vmult", timed(ctx, reps, lambda: op.vmult(dst, src)), n_dofs, bytes_per_dof(dim, p, size, n_cells, n_dofs, ordered, "vmult"))
    # (degree 3: a step is the first update and two iterations of the recurrence, three operator applications)
    t = timed(ctx, reps, lambda: sm.step(dst, b))
    report("Chebyshev step / 3", t / 3, n_dofs, bytes_per_dof(dim, p, size, n_cells, n_dofs, ordered, "chebyshev"))
    if solver is not None:
        s64, d64 = ctx.vector(n_dofs, data=x.astype(np.float64)), ctx.vector(n_dofs)
        t = timed(ctx, max(3, reps // 4), lambda: solver.vmult(d64, s64))
        print("  %-22s %9.3f ms  %8.3f GDoF/s" % ("V-cycle", t * 1e3, n_dofs / t * 1e-9))
        solver.close()
    else:
        sm.clear()
        op.clear()
    for v in (src, dst, b):
        v.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--refine", type=int, default=10)
    ap.add_argument("--refine3d", type=int, default=6)
    ap.add_argument("--number", choices=["f64", "f32"], default="f64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--no-vcycle", action="store_true")
    a = ap.parse_args()
    number = mg.F64 if a.number == "f64" else mg.F32
    print("command: python tools/feq_2d_times.py " + " ".join(sys.argv[1:]))
    ctx = mg.Context(0, options=dict(cell_colour_min=1) if a.colour else None)
    ctx.colour = a.colour
    sq = mg.Square(a.degree, 1, a.refine)
    run(ctx, sq, 2, number, a.reps, not a.no_vcycle, "2D")
    sq.close()
    ctx.close()
    if a.refine3d >= 0:
        ctx = mg.Context(0, options=dict(no_bricks=1))
        cube = mg.Cube(a.degree, 1, a.refine3d)
        run(ctx, cube, 3, number, a.reps, not a.no_vcycle, "3D per-cell path (no_bricks)")
        cube.close()
        ctx.close()


if __name__ == "__main__":
    main()
