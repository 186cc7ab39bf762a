"""Times of the device right-hand side and L2 error of the DG-SIP operator (DGLaplaceOperator.compute_rhs,
compute_l2_error) against the yardstick the issue names -- one mgx_dg_vmult of the same fp64 operator -- and against
the host numpy path of tools/poisson_dg_plain.py that they replace, all in one process.

    python tools/dg_rhs_times.py [degree=3] [n_refine=6] [--dim 2|3] [--number f64|f32] [--repeat 20] [--no-host]

The mesh is that of tools/poisson_dg_plain.py: [-0.9, 1]^dim, one cell refined n_refine times, cells in z-order; f and
g = u are the harness's sine products (evaluated in the kernel) or the same values sampled.  Device times are HIP
events on the context's stream around `repeat` calls after a warm-up call, best of three windows; compute_l2_error
ends with its copy of the four sums to the host, which the events include.  The host path is timed once by the wall
clock (it takes seconds).  Prints one table row per quantity and the three ratios."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_amd as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("degree", nargs="?", type=int, default=3)
    ap.add_argument("n_refine", nargs="?", type=int, default=6)
    ap.add_argument("--dim", type=int, choices=[2, 3], default=3)
    ap.add_argument("--number", choices=["f64", "f32"], default="f64")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dim, p = a.dim, a.degree
    number = mg.F64 if a.number == "f64" else mg.F32
    ctx = mg.Context(0)
    cells = (1 << a.n_refine,) * dim
    h = 1.9 / cells[0]
    nb, ijk = mg.dg_box_neighbours(cells, "z")
    op = mg.DGLaplaceOperator(ctx, p, mg.DG_HERMITE, nb, np.eye(dim) * h, number, dim=dim)
    op.set_cell_positions((-0.9,) * dim, ijk)
    n, nc = op.m(), len(ijk)
    k = 3 * np.pi
    u = mg.DGFunction.sine_product(1.0, (k,) * dim, (0.0,) * dim)
    f = mg.DGFunction.sine_product(dim * k * k, (k,) * dim, (0.0,) * dim)
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.default_stream()

    def device_time(call):
        call()
        ctx.sync()
        best = 1e30
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.repeat):
                call()
            e1.record(stream)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e-3 / a.repeat)
        return best

    b, x, y = op.initialize_dof_vector(), op.initialize_dof_vector(np.ones(n)), op.initialize_dof_vector()
    t = {}
    t["vmult"] = device_time(lambda: op.vmult(y, x))
    t["rhs sine f"] = device_time(lambda: op.compute_rhs(b, f))
    t["rhs sine f, g"] = device_time(lambda: op.compute_rhs(b, f, u))
    t["l2 error sine"] = device_time(lambda: op.compute_l2_error(b, u))
    rhs_dev = b.download()[:n].astype(float)
    host = None
    if not a.no_host:
        # the host path of tools/poisson_dg_plain.py (lines 59-74 and 86-87 there), and the values for the sampled kind
        t0 = time.perf_counter()
        S, xq, wq = op.basis_1d()
        Sd, wd = S, wq
        for _ in range(dim - 1):
            Sd, wd = np.kron(S, Sd), np.kron(wq, wd)
        wd = wd * h ** dim
        ref = np.stack(np.meshgrid(*([xq] * dim), indexing="ij"), axis=-1)[..., ::-1].reshape(-1, dim)
        pts = -0.9 + h * (ijk.astype(float)[:, None, :] + ref[None, :, :])
        uq = np.prod(np.sin(k * pts), axis=-1)
        fq = dim * k * k * uq
        rhs = (fq * wd) @ Sd
        t["host numpy rhs"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        uh = b.download()[:n].astype(float).reshape(nc, -1) @ Sd.T
        host = float(np.sum(wd * (uh - uq) ** 2)), nc * h ** dim
        t["host numpy l2 error"] = time.perf_counter() - t0
        op.compute_rhs(b, f)
        print("device f-only vector against the host formula: %.2e" % (abs(b.download()[:n] - rhs.ravel()).max() / abs(rhs).max()))
        fv = ctx.vector(fq.size, mg.F64, data=fq.ravel())
        fs = mg.DGFunction.sampled(fv)
        t["rhs sampled f"] = device_time(lambda: op.compute_rhs(b, fs))
        us = mg.DGFunction.sampled(ctx.vector(uq.size, mg.F64, data=uq.ravel()))
        op.compute_rhs(b, f, u)
        t["l2 error sampled"] = device_time(lambda: op.compute_l2_error(b, us))
        dev = op.compute_l2_error(b, us)
        print("device sums %.12e %.12e, host sums %.12e %.12e" % (dev[0], dev[1], host[0], host[1]))
    print("DoFs %d, cells %d, p = %d, dim = %d, %s; seconds per call" % (n, nc, p, dim, a.number))
    for name, v in t.items():
        print("  %-22s %.6e  (%.3f of one vmult, %.3e DoFs/s)" % (name, v, v / t["vmult"], n / v))
    print("ratios: rhs (sine f, g) / vmult %.3f   l2 error (sine) / vmult %.3f" % (t["rhs sine f, g"] / t["vmult"], t["l2 error sine"] / t["vmult"])
          + ("" if a.no_host else "   host rhs / device rhs %.0f   host l2 / device l2 %.0f"
             % (t["host numpy rhs"] / t["rhs sine f, g"], t["host numpy l2 error"] / t["l2 error sine"])))
    assert np.isfinite(rhs_dev).all()
    op.clear()
    ctx.close()


if __name__ == "__main__":
    main()
