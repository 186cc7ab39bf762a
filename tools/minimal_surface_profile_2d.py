#!/usr/bin/env python3
"""Measurements of the solution-dependent coefficient path in two dimensions for profiles/minimal_surface_2d.md, in one
process: the evaluation and the residual kernel, on affine cells (the square) NEXT TO curved cells (the annulus sector
of the same size), both laws, fp64 and fp32, the forms alternating; one refresh of a hierarchy; and the same refresh the
only way it could be done without the 2D entry points (state to the host, tensors in numpy, hierarchy created anew).

Timing: warm-up, then --groups groups of --reps back-to-back launches between two device events on the context's stream.
Byte models, as fractions of the 8 TB/s HBM peak:
  evaluation  3 values stored per point, + 4 loaded per point in the per-point form, + the gathered state (one value per DoF)
  residual    two vectors (state read, result written), + 4 values per point in the per-point form
              (the scratch round trip of the ordered assembly, 2 values per point, is NOT in the model: it is overhead)

Usage: python tools/minimal_surface_profile_2d.py DEGREE N_REFINE [--no-host] [--no-update]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_amd as mg  # noqa: E402

HBM_PEAK = 8.0e12


def timed(ctx, stream, fn, reps, groups):
    for _ in range(3):
        fn()
    ctx.sync()
    out = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / reps)
    return np.array(out)


def smooth_state(sq, l):
    x = sq.dof_coordinates(l)
    return 0.6 * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])) * np.cos(1.3 * x[:, 1]) + 0.2 * x[:, 0] ** 2


def kernels(ctx, stream, args, flat, curved):
    p, n2, l = args.degree, (args.degree + 1) ** 2, flat.max_level
    n_cells, n_dofs = flat.n_cells(l), flat.n_dofs(l)
    ua, uq = smooth_state(flat, l), smooth_state(curved, l)
    unit_a, unit_q, jxw_q = flat.unit_law_coefficient(l), curved.unit_q(l), curved.jxw_q(l)
    for number, dt, size, name in ((mg.F64, np.float64, 8, "fp64"), (mg.F32, np.float32, 4, "fp32")):
        a = mg.LaplaceOperator.from_cube(ctx, flat, l, number, coef_q=unit_a)
        a.enable_coefficient_update(*flat.affine_metric(l))
        q = mg.LaplaceOperator.from_cube(ctx, curved, l, number)
        q.enable_coefficient_update_q(unit_q, jxw_q)
        sa, sq = ctx.vector(n_dofs, number, ua.astype(dt)), ctx.vector(n_dofs, number, uq.astype(dt))
        da, dq = ctx.vector(n_dofs, number), ctx.vector(n_dofs, number)
        print("FE_Q(%d), %d x %d cells, %d DoFs, %s; coef_q %.1f MB, per-point geometry %.1f MB"
              % ((p,) + flat.cells_per_dim2(l) + (n_dofs, name, n_cells * 3 * n2 * size / 1e6, n_cells * 4 * n2 * size / 1e6)))
        rows = []
        ev_a, ev_q = (n_cells * 3 * n2 + n_dofs) * size, (n_cells * 7 * n2 + n_dofs) * size
        rs_a, rs_q = 2 * n_dofs * size, (2 * n_dofs + n_cells * 4 * n2) * size
        for law, lname in ((mg.LAW_UNIT, "unit"), (mg.LAW_MINIMAL_SURFACE, "minimal_surface")):
            rows.append(("evaluate " + lname, lambda law=law: a.evaluate_coefficient(law, sa),
                         lambda law=law: q.evaluate_coefficient(law, sq), ev_a, ev_q))
        for law, lname in ((mg.LAW_UNIT, "unit"), (mg.LAW_MINIMAL_SURFACE, "minimal_surface")):
            rows.append(("residual " + lname, lambda law=law: a.compute_nonlinear_residual(law, da, sa),
                         lambda law=law: q.compute_nonlinear_residual(law, dq, sq), rs_a, rs_q))
        rows.append(("vmult (per-point tensor)", lambda: a.vmult(da, sa), lambda: q.vmult(dq, sq),
                     rs_a + n_cells * 3 * n2 * size, rs_a + n_cells * 3 * n2 * size))
        print("%-26s %-44s %-44s ratio" % ("", "affine (one metric per level)", "per point (curved cells)"))
        for rname, fa, fq, ba, bq in rows:
            ta, tq = [], []
            for _ in range(2):  # alternate the two forms
                ta.append(timed(ctx, stream, fa, args.reps, args.groups))
                tq.append(timed(ctx, stream, fq, args.reps, args.groups))
            ta, tq = np.concatenate(ta), np.concatenate(tq)
            cell = lambda t, b: "%7.1f us (%.1f..%.1f) %.3f of peak" % (t.mean() * 1e6, t.min() * 1e6, t.max() * 1e6,
                                                                       b / t.mean() / HBM_PEAK)
            print("%-26s %-44s %-44s %.2f" % (rname, cell(ta, ba), cell(tq, bq), tq.mean() / ta.mean()), flush=True)
        for o in (a, q):
            o.clear()
        for v in (sa, sq, da, dq):
            v.free()


def update(ctx, stream, args, flat):
    import nonlinear_reference_2d as nr2
    p, lmax = args.degree, flat.max_level
    solver = mg.MultigridSolver(ctx, flat, 2, 2, 1, mg.F32, general=True)
    state = ctx.vector(flat.n_dofs(lmax), data=smooth_state(flat, lmax))
    t = timed(ctx, stream, lambda: solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, state), 1, args.groups)
    print("FE_Q(%d), %d levels, fp32 V-cycle: update_coefficient %.2f ms (min %.2f max %.2f over %d)"
          % (p, flat.n_levels, t.mean() * 1e3, t.min() * 1e3, t.max() * 1e3, args.groups), flush=True)
    if args.no_host:
        solver.close()
        return
    # the route without the entry points: state to the host, tensors in numpy, everything created anew
    R = nr2.interpolation_matrix_1d(flat.gll())
    dofs = [nr2.cell_dofs(flat.idx9_plain(l), p) for l in range(flat.n_levels)]
    refs = [nr2.NonlinearReference2D(p, flat.shape_values(), flat.colloc_grad(), flat.qweights(), flat.idx9(l), flat.idx9_plain(l),
                                     flat.n_dofs(l), flat.cell_nodes(l), True) for l in range(flat.n_levels)]
    t0 = time.perf_counter()
    states = [None] * flat.n_levels
    states[lmax] = state.download()
    t1 = time.perf_counter()
    for l in range(lmax, 0, -1):
        states[l - 1] = nr2.interpolate_to_coarse(R, flat.children(l), dofs[l], dofs[l - 1], flat.n_dofs(l - 1), states[l])
    tensors = [refs[l].coefficient(mg.LAW_MINIMAL_SURFACE, states[l]) for l in range(flat.n_levels)]
    t2 = time.perf_counter()
    scratch = mg.MultigridSolver(ctx, flat, 2, 2, 1, mg.F32, general=True, coef_q=tensors)
    ctx.sync()
    t3 = time.perf_counter()
    scratch.close()
    solver.close()
    print("host route: %.2f s = download %.3f + numpy interpolation and tensors %.2f + operators / transfers / solver %.2f"
          % (t3 - t0, t1 - t0, t2 - t1, t3 - t2), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", type=int)
    ap.add_argument("n_refine", type=int)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-update", action="store_true")
    args = ap.parse_args()
    ctx = mg.Context(0)
    stream = torch.cuda.ExternalStream(int(ctx.stream or 0))
    flat = mg.Square(args.degree, 1, args.n_refine)
    curved = mg.Square(args.degree, 1, args.n_refine, mapped="annulus_sector")
    kernels(ctx, stream, args, flat, curved)
    curved.close()
    if not args.no_update:
        update(ctx, stream, args, flat)
    flat.close()
    ctx.close()


if __name__ == "__main__":
    main()
