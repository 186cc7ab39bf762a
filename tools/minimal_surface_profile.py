#!/usr/bin/env python3
"""Measurements of the solution-dependent coefficient path for profiles/minimal_surface.md:

  kernel   the coefficient-evaluation kernel on one level (warm-up, then --groups groups of --reps back-to-back launches
           between two stream synchronisations; mean and spread of the per-launch time over the groups), its achieved
           bytes/s against the traffic model 6 (p+1)^3 values stored + (p+1)^3 values gathered per cell, as a fraction of
           the 8 TB/s HBM peak; next to it the plain general vmult of the same operator and its fraction
           (model: 6 (p+1)^3 coefficient values per cell + 16 B per DoF of the vectors)
  update   one whole MultigridSolver.update_coefficient of a hierarchy, against the route without it: download the state,
           evaluate the tensors of every level in numpy, create operators / transfers / solver anew through desc.coef_q

  mapped   the per-point kernels of curved cells (mgx_operator_enable_coefficient_update_q) on a shell_sector box of
           2^N_REFINE cells per direction NEXT TO the affine kernels on the Cartesian cube of the same size, alternating
           in one run: evaluation (both laws) and nonlinear residual.  Byte model of an evaluation: the affine one stores
           6 values per point, the per-point one loads 7 and stores 6 (+ one gathered state value per point each)

Usage: python tools/minimal_surface_profile.py kernel DEGREE N_REFINE [--number f64|f32]
       python tools/minimal_surface_profile.py mapped DEGREE N_REFINE [--number f64|f32]
       python tools/minimal_surface_profile.py update DEGREE N_REFINE [--vcycle f32|f64] [--no-host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_amd as mg  # noqa: E402

HBM_PEAK = 8.0e12


def timed(ctx, fn, reps, groups):
    for _ in range(3):
        fn()
    ctx.sync()
    out = []
    for _ in range(groups):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) / reps)
    return np.array(out)


def smooth_state(cube, l):
    x = cube.dof_coordinates(l)
    return 0.6 * np.sin(2 * np.pi * (x[:, 0] + x[:, 1])) * np.cos(1.3 * x[:, 2]) + 0.2 * x[:, 2] ** 2


def kernel(args):
    number, dt, size = (mg.F64, np.float64, 8) if args.number == "f64" else (mg.F32, np.float32, 4)
    ctx = mg.Context(0)
    cube = mg.Cube(args.degree, 1, args.n_refine)
    l, n3 = cube.max_level, (args.degree + 1) ** 3
    op = mg.LaplaceOperator.from_cube(ctx, cube, l, number, coef_q=cube.unit_law_coefficient(l))
    op.enable_coefficient_update(*cube.affine_metric(l))
    u = smooth_state(cube, l)
    state, dst = ctx.vector(u.size, number, u.astype(dt)), ctx.vector(u.size, number)
    n_cells, n_dofs = cube.n_cells(l), cube.n_dofs(l)
    print("FE_Q(%d), %d^3 cells, %d DoFs, %s; coef_q %.1f MB" % (args.degree, cube.cells_per_dim(l), n_dofs, args.number,
                                                                n_cells * 6 * n3 * size / 1e6))
    for name, law in (("evaluate_coefficient unit", mg.LAW_UNIT), ("evaluate_coefficient minimal_surface", mg.LAW_MINIMAL_SURFACE)):
        t = timed(ctx, lambda: op.evaluate_coefficient(law, state), args.reps, args.groups)
        traffic = n_cells * 7 * n3 * size
        print("%-38s %8.1f us (min %.1f max %.1f over %d x %d)  %7.1f GB/s of its model = %.3f of the HBM peak"
              % (name, t.mean() * 1e6, t.min() * 1e6, t.max() * 1e6, args.groups, args.reps, traffic / t.mean() / 1e9,
                 traffic / t.mean() / HBM_PEAK))
    t = timed(ctx, lambda: op.vmult(dst, state), args.reps, args.groups)
    traffic = n_cells * 6 * n3 * size + 2 * size * n_dofs
    print("%-38s %8.1f us (min %.1f max %.1f)  %7.1f GB/s of its model = %.3f of the HBM peak"
          % ("general vmult (same coefficient)", t.mean() * 1e6, t.min() * 1e6, t.max() * 1e6, traffic / t.mean() / 1e9,
             traffic / t.mean() / HBM_PEAK))
    t = timed(ctx, lambda: op.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, dst, state), args.reps, args.groups)
    print("%-38s %8.1f us (min %.1f max %.1f)" % ("nonlinear residual minimal_surface", t.mean() * 1e6, t.min() * 1e6, t.max() * 1e6))


def mapped(args):
    number, dt, size = (mg.F64, np.float64, 8) if args.number == "f64" else (mg.F32, np.float32, 4)
    ctx = mg.Context(0)
    p, n3 = args.degree, (args.degree + 1) ** 3
    flat = mg.Cube(p, 1, args.n_refine)
    curved = mg.Cube(p, n_refine=args.n_refine, box=(1, 1, 1), origin=-0.9, h0=1.9, geometry="shell_sector")
    l = flat.max_level
    assert curved.n_cells(l) == flat.n_cells(l) and curved.n_dofs(l) == flat.n_dofs(l)
    n_cells, n_dofs = flat.n_cells(l), flat.n_dofs(l)
    a = mg.LaplaceOperator.from_cube(ctx, flat, l, number, coef_q=flat.unit_law_coefficient(l))
    a.enable_coefficient_update(*flat.affine_metric(l))
    q = mg.LaplaceOperator.from_cube(ctx, curved, l, number)
    q.enable_coefficient_update_q(curved.coef_q(l), curved.jxw_q(l))
    ua, uq = smooth_state(flat, l), smooth_state(curved, l)
    sa, sq = ctx.vector(n_dofs, number, ua.astype(dt)), ctx.vector(n_dofs, number, uq.astype(dt))
    da, dq = ctx.vector(n_dofs, number), ctx.vector(n_dofs, number)
    print("FE_Q(%d), %d^3 cells, %d DoFs, %s; coef_q %.1f MB, per-point geometry %.1f MB"
          % (p, flat.cells_per_dim(l), n_dofs, args.number, n_cells * 6 * n3 * size / 1e6, n_cells * 7 * n3 * size / 1e6))
    rows = []
    for name, law in (("evaluate unit", mg.LAW_UNIT), ("evaluate minimal_surface", mg.LAW_MINIMAL_SURFACE)):
        rows.append((name, lambda law=law: a.evaluate_coefficient(law, sa), lambda law=law: q.evaluate_coefficient(law, sq),
                     n_cells * 7 * n3 * size, n_cells * 14 * n3 * size))
    # residual: the affine form streams no tensor; the per-point form loads 6 (unit law) / 7 values per point; both
    # gather the state, store (p+1)^3 local values per cell and read them again in the ordered assembly
    base = n_cells * 2 * n3 * size + 2 * size * n_dofs
    rows.append(("residual unit", lambda: a.compute_nonlinear_residual(mg.LAW_UNIT, da, sa),
                 lambda: q.compute_nonlinear_residual(mg.LAW_UNIT, dq, sq), base, base + n_cells * 6 * n3 * size))
    rows.append(("residual minimal_surface", lambda: a.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, da, sa),
                 lambda: q.compute_nonlinear_residual(mg.LAW_MINIMAL_SURFACE, dq, sq), base, base + n_cells * 7 * n3 * size))
    print("%-26s %-42s %-42s ratio" % ("", "affine (one metric per level)", "per point (curved cells)"))
    for name, fa, fq, ba, bq in rows:
        ta, tq = [], []
        for _ in range(2):  # alternate the two forms
            ta.append(timed(ctx, fa, args.reps, args.groups))
            tq.append(timed(ctx, fq, args.reps, args.groups))
        ta, tq = np.concatenate(ta), np.concatenate(tq)
        cell = lambda t, b: "%7.1f us (%.1f..%.1f) %.3f of peak" % (t.mean() * 1e6, t.min() * 1e6, t.max() * 1e6,
                                                                   b / t.mean() / HBM_PEAK)
        print("%-26s %-42s %-42s %.2f (bytes: %.2f)" % (name, cell(ta, ba), cell(tq, bq), tq.mean() / ta.mean(), bq / ba))


def update(args):
    import nonlinear_reference as nr
    vnumber = mg.F32 if args.vcycle == "f32" else mg.F64
    ctx = mg.Context(0)
    cube = mg.Cube(args.degree, 1, args.n_refine)
    lmax, p = cube.max_level, args.degree
    solver = mg.MultigridSolver(ctx, cube, 2, 2, 1, vnumber, general=True)
    state = ctx.vector(cube.n_dofs(lmax), data=smooth_state(cube, lmax))
    t = timed(ctx, lambda: solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, state), 1, args.groups)
    print("FE_Q(%d), %d^3 cells, %d levels, %s V-cycle: update_coefficient %.2f ms (min %.2f max %.2f over %d)"
          % (p, cube.cells_per_dim(lmax), cube.n_levels, args.vcycle, t.mean() * 1e3, t.min() * 1e3, t.max() * 1e3, args.groups))
    if args.no_host:
        return
    # the route without the entry point: state to the host, tensors in numpy, everything created anew
    R = nr.interpolation_matrix_1d(cube.gll())
    dofs = [nr.cell_dofs(cube.idx27_plain(l), p) for l in range(cube.n_levels)]
    refs = [nr.NonlinearReference(p, cube.shape_values(), cube.colloc_grad(), cube.qweights(), cube.idx27(l), cube.idx27_plain(l),
                                  cube.n_dofs(l), *cube.affine_metric(l)) for l in range(cube.n_levels)]
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        states = [None] * cube.n_levels
        states[lmax] = state.download()
        t1 = time.perf_counter()
        for l in range(lmax, 0, -1):
            states[l - 1] = nr.interpolate_to_coarse(R, cube.children(l), dofs[l], dofs[l - 1], cube.n_dofs(l - 1), states[l])
        tensors = [refs[l].coefficient(mg.LAW_MINIMAL_SURFACE, states[l]) for l in range(cube.n_levels)]
        t2 = time.perf_counter()
        scratch = mg.MultigridSolver(ctx, cube, 2, 2, 1, vnumber, general=True, coef_q=tensors)
        ctx.sync()
        t3 = time.perf_counter()
        scratch.close()
        times.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    for tt in times:
        print("host route: %.2f s = download %.3f + numpy interpolation and tensors %.2f + operators / transfers / solver %.2f"
              % tt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "mapped", "update"])
    ap.add_argument("degree", type=int)
    ap.add_argument("n_refine", type=int)
    ap.add_argument("--number", choices=["f64", "f32"], default="f64")
    ap.add_argument("--vcycle", choices=["f64", "f32"], default="f32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    {"kernel": kernel, "mapped": mapped, "update": update}[args.what](args)


if __name__ == "__main__":
    main()
