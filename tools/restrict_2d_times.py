"""Time per call of the two-dimensional restriction alone (mgx_restrict_and_add on quadrilaterals, restrict_2d_kernel colour
by colour) between the two finest levels of the square [-0.9, 1]^2, in fp64 and in fp32 in the same process: device events
around groups of `--repeat` back-to-back calls, the two number types alternating group by group, `--groups` groups each.
The prolongation of the same level pair is timed next to it in the same way.

    python tools/restrict_2d_times.py [degree=4] [n_refine=10] [--repeat 20] [--groups 9]

Prints, per form, the best and the median group, in microseconds per call.  The script uses nothing but Square,
LaplaceOperator and Transfer, so the same file runs on an earlier commit for a comparison; nothing here is a pass
criterion."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=4)
    ap.add_argument("n_refine", nargs="?", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--groups", type=int, default=9)
    a = ap.parse_args()
    ctx = mg.Context(0)
    sq = mg.Square(a.degree, 1, a.n_refine)
    l = sq.max_level
    nc, nf = sq.n_dofs(l - 1), sq.n_dofs(l)
    print("FE_Q(%d), %d -> %d cells, %d -> %d unknowns, %d calls per group, %d groups per form"
          % (a.degree, sq.n_cells(l), sq.n_cells(l - 1), nf, nc, a.repeat, a.groups))
    forms = {}
    for name, number, dt in (("f64", mg.F64, np.float64), ("f32", mg.F32, np.float32)):
        ops = [mg.LaplaceOperator.from_cube(ctx, sq, k, number) for k in (l - 1, l)]
        tr = mg.Transfer(ops[0], ops[1], sq.children(l), sq.prolong_1d())
        fine = ctx.vector(nf, number, data=sq.seeded_vector(l, 12).astype(dt))
        coarse = ctx.vector(nc, number)
        forms["restrict_and_add " + name] = (lambda tr=tr, coarse=coarse, fine=fine: tr.restrict_and_add(coarse, fine), (ops, tr, fine, coarse))
        forms["prolongate " + name] = (lambda tr=tr, coarse=coarse, fine=fine: tr.prolongate(fine, coarse), None)
    stream = torch.cuda.ExternalStream(ctx.stream)
    times = {name: [] for name in forms}
    for fn, _ in forms.values():
        for _ in range(3):
            fn()
    ctx.sync()
    with torch.cuda.stream(stream):
        for _ in range(a.groups):
            for name, (fn, _) in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(a.repeat):
                    fn()
                t1.record(stream)
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / a.repeat)
    for name, t in times.items():
        print("%-22s best %9.2f us  median %9.2f us  (%s)" % (name, min(t), float(np.median(t)), " ".join("%.1f" % v for v in t)))
    for _, keep in forms.values():
        if keep:
            ops, tr, fine, coarse = keep
            tr.clear()
            for v in (fine, coarse):
                v.free()
            for o in ops:
                o.clear()
    sq.close()
    ctx.close()


if __name__ == "__main__":
    main()
