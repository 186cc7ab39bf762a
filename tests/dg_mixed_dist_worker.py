"""Worker of the decomposed DG test with Neumann faces (one process per rank over gloo, all ranks on the one GPU): the
DG operator, the merged Chebyshev update and the merged CG iteration on a block-decomposed box with Neumann sides that
the partition cuts, against the single-domain restatement (tests/dg_mixed_reference.py) on the same global mesh.
argv: degree basis steps number(f32|f64) sides(comma separated face numbers 2d+s)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], tuple(int(f) for f in sys.argv[5].split(",")), dist, rank,
        world)
    dist.barrier()
    dist.destroy_process_group()


def run(p, basis, steps, number, sides, dist, rank, world, say=print):
    import multigrid_amd as mg

    import dg_mixed_reference as mx

    num = mg.F64 if number == "f64" else mg.F32
    tol = 2e-11 if num == mg.F64 else 5e-5
    cells, jac = mg.dg_cheby_mesh(steps)
    procs = mg.process_grid(world)
    part = mg.dg_box_partition(cells, procs, rank)
    ijk = part["ijk"]
    # the owned cells with their positions in the whole box: faces towards another rank are cells (ghosts) and stay
    nb = mg.dg_box_set_sides(cells, ijk, part["neighbours"], sides)
    cut = [f for f in sides if procs[f // 2] == 1 and max(procs) > 1]
    assert cut, "no Neumann side is cut by the partition"
    for f in cut:                                        # every rank holds a piece of such a side
        assert (nb[:, f] == mg.DG_NEUMANN).any(), (rank, f)
    ctx = mg.Context(0)
    comm = mg.Communicator(ctx, dist)  # noqa: F841  (the context keeps the transport it installs)
    op = mg.DGLaplaceOperator(ctx, p, basis, nb, jac, num, part["n_ghost"], part["exchange"])
    o = mx.mixed_oracle(p, basis, cells, jac, sides)
    rng = np.random.default_rng(5)   # the same global vectors on every rank
    x, xo, rhs = (rng.standard_normal(o.shape) for _ in range(3))
    mine = lambda a: a[ijk[:, 2], ijk[:, 1], ijk[:, 0]].ravel()   # noqa: E731
    n = op.m()

    def owned(v):
        return v.download()[:n].astype(float)

    def rel(a, b):
        return abs(a - b).max() / abs(b).max()

    src, dst = op.initialize_dof_vector(mine(x)), op.initialize_dof_vector()
    op.vmult(dst, src)
    assert rel(owned(dst), mine(o.vmult(x))) < tol, "vmult"
    b = op.initialize_dof_vector(mine(rhs))
    op.vmult_residual(dst, b, src)
    assert rel(owned(dst), mine(rhs - o.vmult(x))) < tol, "residual"
    op.jacobi_vmult(dst, b)
    assert rel(owned(dst), mine(o.jacobi_vmult(rhs))) < 5 * tol, "jacobi"
    for idx in (0, 1, 2):
        sol, old = op.initialize_dof_vector(mine(x)), op.initialize_dof_vector(mine(xo))
        op.vmult_with_chebyshev_update(b, idx, 0.6, 0.2, sol, old)
        new_ref, old_ref = o.vmult_with_chebyshev_update(rhs, idx, 0.6, 0.2, x, xo)
        assert rel(owned(sol), mine(new_ref)) < 5 * tol, ("cheb", idx)
        assert rel(owned(old), mine(old_ref)) < 5 * tol, ("cheb old", idx)
    # merged CG iterations: the sums cover every rank's owned cells
    r, q, pv = (rng.standard_normal(o.shape) for _ in range(3))
    R, Q, Pv, X = (op.initialize_dof_vector(mine(a)) for a in (r, q, pv, x))
    sums = op.vmult_with_cg_update(0.37, 0.81, R, Q, Pv, X)
    p_ref = 0.81 * pv + q
    q_ref = o.vmult(p_ref)
    assert rel(owned(Q), mine(q_ref)) < 5 * tol and rel(owned(X), mine(x + 0.37 * pv)) < 5 * tol, "cg update"
    ref = np.array([(q_ref * p_ref).sum(), (r * r).sum(), (q_ref * r).sum(), (q_ref * q_ref).sum()])
    assert np.allclose(sums, ref, rtol=100 * tol, atol=100 * tol * abs(ref).max()), ("cg sums", sums, ref)
    m = np.tile(op.lumped_mass_inverse(), int(np.prod(cells))).reshape(o.shape)
    R, Q, Pv = (op.initialize_dof_vector(mine(a)) for a in (r, q, pv))
    sums = op.vmult_with_pcg_sums(R, Q, Pv)
    q_ref = o.vmult(pv)
    assert rel(owned(Q), mine(q_ref)) < 5 * tol, "pcg q"
    ref = np.array([(q_ref * pv).sum(), (r * m * r).sum(), (q_ref * m * r).sum(), (q_ref * m * q_ref).sum()])
    assert np.allclose(sums, ref, rtol=100 * tol, atol=100 * tol * abs(ref).max()), ("pcg sums", sums, ref)
    say("rank %d dg mixed ok: %d owned cells, %d ghost cells, Neumann sides %s, cut %s" % (rank, len(ijk), part["n_ghost"], sides, cut),
        flush=True)
    op.clear()
    ctx.close()


if __name__ == "__main__":
    main()
