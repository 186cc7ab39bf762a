"""What Neumann faces cost: the merged Chebyshev step of the DG-SIP operator (tools/matvec_dg_cheby.py's loop,
Hermite-like basis) on the harness mesh with three sides of the box Neumann sides -- the variant kernels and the 3^6-row
table of inverse diagonals -- against the same mesh with all sides Dirichlet, in one process.

    python tools/dg_neumann_times.py [--cases 4:18,8:15] [--numbers f32,f64] [--nsteps 50] [--rounds 3] [--sides 1,2,5]

--cases degree:refinement steps (4:18 is 64^3 cells, 8:15 is 32^3, the sizes bench.py times).  The two operators are
timed in alternation, `rounds` times each, every round the best of three averages over nsteps steps.  The yardstick is
the all-Dirichlet rate and the margin the spread of its rounds: a Neumann face does less work than a Dirichlet face, so
a Neumann rate below the slowest all-Dirichlet round needs an explanation."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def rate(ctx, op, vectors, nsteps):
    rhs, out, inp = vectors
    best = 1e10
    for _ in range(3):
        ctx.sync()
        t = time.perf_counter()
        for _ in range(nsteps):
            op.vmult_with_chebyshev_update(rhs, 2, 0.6, 0.2, out, inp)
            out, inp = inp, out
        ctx.sync()
        best = min(best, (time.perf_counter() - t) / nsteps)
    return op.m() / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4:18,8:15")
    ap.add_argument("--numbers", default="f32,f64")
    ap.add_argument("--nsteps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sides", default="1,2,5")
    a = ap.parse_args()
    sides = tuple(int(f) for f in a.sides.split(","))
    ctx = mg.Context(0)
    print("merged Chebyshev step, Hermite-like basis, DoFs/s; Neumann sides %s against all sides Dirichlet" % (sides,))
    for case in a.cases.split(","):
        p, steps = (int(v) for v in case.split(":"))
        cells, jac = mg.dg_cheby_mesh(steps)
        for name in a.numbers.split(","):
            number = mg.F32 if name == "f32" else mg.F64
            ops, vecs = {}, {}
            rng = np.random.default_rng(0)
            for key, marked in (("dirichlet", ()), ("neumann", sides)):
                nb, _ = mg.dg_box_neighbours(cells, neumann_sides=marked)
                ops[key] = mg.DGLaplaceOperator(ctx, p, mg.DG_HERMITE, nb, jac, number)
            n = ops["dirichlet"].m()
            shared = [ops["dirichlet"].initialize_dof_vector(rng.random(n)), ops["dirichlet"].initialize_dof_vector(),
                      ops["dirichlet"].initialize_dof_vector()]
            rates = {"dirichlet": [], "neumann": []}
            for _ in range(a.rounds):
                for key in ("dirichlet", "neumann"):
                    for v in shared[1:]:
                        v.zero()
                    rates[key].append(rate(ctx, ops[key], shared, a.nsteps))
            d, nm = rates["dirichlet"], rates["neumann"]
            print("p=%d %s %s cells %d DoFs: all-Dirichlet %s (min %.4e max %.4e)  Neumann %s (best %.4e)  best/best %.4f  %s"
                  % (p, name, "x".join(map(str, cells)), n, " ".join("%.4e" % r for r in d), min(d), max(d),
                     " ".join("%.4e" % r for r in nm), max(nm), max(nm) / max(d),
                     "within the all-Dirichlet spread or above" if max(nm) >= min(d) else "BELOW the all-Dirichlet spread"))
            for v in shared:
                v.free()
            for op in ops.values():
                op.clear()
    ctx.close()


if __name__ == "__main__":
    main()
