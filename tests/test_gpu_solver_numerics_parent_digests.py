"""The host numerics of the solvers (the CG run as a Lanczos process of the eigenvalue estimates, SolverCG with its
ReductionControl, the Chebyshev factors, the tail of vmult_with_residual_update, the level timers, the DG level) are
written once, in multigrid_amd/csrc/mgx_krylov.hpp, for FE_Q and DG alike.  Folding the copies may change nothing that is
computed: BITWISE against the commit before it.  tests/golden/solver_numerics_parent_digests.json holds the SHA-256 of
the raw bytes of every result below, recorded from a build of that commit with tools/solver_numerics_digests.py, which
runs all_digests() of this file.  The tool was run on that commit twice, one process each; only results in which the
commit reproduced itself are kept: 92 of 100 digests.  Dropped (DROPPED below): history and solution of the FE_Q
solve_cg() and of the solve with control = (5, 0., 1e-3) in all four cases -- the last bits of the FE_Q CG residuals
differ from process to process on that commit (p = 4, fp32, controlled solve: the last residual is
0.0047904284728159195 in some runs and 0.00479042847281592 in others, with that commit's library and with this one
alike).  What those solves must still reproduce is recorded beside them and was equal in every run: iteration count,
length of the history and, for the controlled solve, the status it returns; and the residual history itself is recorded
as numbers and compared within HISTORY_RTOL (below: 8.7e-10 with an fp64 V-cycle, 7.6e-4 with an fp32 one).  The tool
records under the scheduling thresholds of tests/conftest.py.

Cases:
  * FE_Q: MultigridSolver on Cube(p, n_refine=2), p = 2 and 4, V-cycle in fp64 and fp32: mgx_smoother_info of every
    level as raw bytes (level 0: the degree from Varga's estimate); iterations, cg_history and solution of solve_cg();
    the same with control = (5, 0., 1e-3) together with the status it returns (MGX_ERR_NOT_CONVERGED where the commit
    before returned it); iteration counts and status of both once more on their own; sums and both vectors of one
    vmult_with_residual_update; vmult and step of a fourth-kind Chebyshev smoother on the finest level; wall_times()
    after one timed solve (shape and level-0 count; no entry may be negative; the times are not compared);
  * DG on FE_Q: DGMultigridSolver on Cube(2, n_refine=2) (64 cells: the restriction into FE_Q runs as plain launches),
    Hermite-like basis, fp32 and fp64: smoother_info, one vmult, iterations and solution of solve_cg;
  * plain DG multigrid, fp32 and fp64: 3D p = 2 from a 1x1x1 box on three levels, 2D p = 3 from a 3x2 box on two levels,
    the hp hierarchy "3d-hp" of tests/dg_hp_reference.py, and that one with a Neumann side: smoother_info of every level,
    one vmult, iterations and solution of solve_cg, sums and both vectors of one vmult_with_residual_update.
No Lanczos run of these cases has more than 64 rows: the bisection route of the DG estimate beyond that is covered by
tests/test_krylov_host.py."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_numerics_parent_digests.json")
NUMBERS = (("f64", mg.F64), ("f32", mg.F32))
FE_Q_DEGREES = (2, 4)
# not reproduced by the commit before from one process to the next, so not recorded
DROPPED = ["feq-p%d-%s-solve_cg%s" % (p, tag, which) for p in (2, 4) for tag in ("f64", "f32") for which in ("", "-5-iterations")]
# What stands for them: the recorded cg_history (keys "...-history", lists of numbers, not digests) within HISTORY_RTOL =
# steps x condition x addends x eps: a history has up to 8 steps, each passes a perturbation on through alpha and beta
# with at most the condition of the preconditioned operator (below 1e2: the iteration contracts by 0.07 per step), and
# what is not reproduced is the order of a sum.  fp64 V-cycle: the fp64 partial sums of the dot products over the 4913
# DoFs of the finest level.  fp32 V-cycle: on top of that the fp32 sums inside the cycle that add the contributions of
# the up to 8 cells around a DoF in the order they arrive, which is the larger term
HISTORY_RTOL = {"f64": 8 * 1e2 * 4913 * np.finfo(np.float64).eps, "f32": 8 * 1e2 * 8 * np.finfo(np.float32).eps}
# (name, degree, basis, coarse cells, n_levels, hierarchy, neumann sides)
PLAIN = [("plain-3d-p2-1x1x1-L3", 2, mg.DG_HERMITE, (1, 1, 1), 3, None, ()),
         ("plain-2d-p3-3x2-L2", 3, mg.DG_HERMITE, (3, 2), 2, None, ()),
         ("plain-3d-hp", 3, mg.DG_GAUSS, (3, 2, 1), None, [(1, 0), (3, 0), (3, 1)], ()),
         ("plain-3d-hp-neumann", 3, mg.DG_GAUSS, (3, 2, 1), None, [(1, 0), (3, 0), (3, 1)], (1,))]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def info_bytes(call, *args):
    i = mg._lib.SmootherInfo()
    mg.check(call(*args, C.byref(i)))
    return np.frombuffer(bytes(i), dtype=np.uint8)


def fe_q_digests(ctx, p, tag, number):
    out, name = {}, "feq-p%d-%s-" % (p, tag)
    cube = mg.Cube(p, 1, 2)
    S = mg.MultigridSolver(ctx, cube, 3, 3, 1, number)
    lmax = cube.max_level
    for l in range(cube.n_levels):
        out[name + "smoother-info-L%d" % l] = digest(info_bytes(ctx.lib.mgx_smoother_get_info, S.smoother(l).h))
    its, _ = S.solve_cg()
    out[name + "solve_cg"] = digest(np.int64(its), S.cg_history(), S.get_solution().download())
    out[name + "solve_cg-iterations"] = digest(np.int64([its, len(S.cg_history())]))
    out[name + "solve_cg-history"] = [float(v) for v in S.cg_history()]
    status = 0
    try:
        its, _ = S.solve_cg(control=(5, 0., 1e-3))
    except mg.MgxError as e:
        status, its = e.status, -1
    out[name + "solve_cg-5-iterations"] = digest(np.int64([status, its]), S.cg_history(), S.get_solution().download())
    out[name + "solve_cg-5-iterations-status"] = digest(np.int64([status, its, len(S.cg_history())]))
    out[name + "solve_cg-5-iterations-history"] = [float(v) for v in S.cg_history()]
    n = cube.n_dofs(lmax)
    res, upd = (ctx.vector(n, data=cube.seeded_vector(lmax, s)) for s in (8, 9))
    sums = S.vmult_with_residual_update(res, upd, 0.25)
    out[name + "residual-update"] = digest(sums, res.download(), upd.download())
    cheb = mg.Chebyshev(S.matrix(lmax), 20., 3, 15, polynomial="fourth_kind")
    b, x = ctx.vector(n, number, cube.seeded_vector(lmax, 7)), ctx.vector(n, number)
    out[name + "fourth-kind-info"] = digest(info_bytes(ctx.lib.mgx_smoother_get_info, cheb.h))
    cheb.vmult(x, b)
    out[name + "fourth-kind-vmult"] = digest(x.download())
    cheb.step(x, b)
    out[name + "fourth-kind-step"] = digest(x.download())
    cheb.clear()
    S.enable_timings(True)
    S.wall_times()
    S.solve_cg()
    t = S.wall_times()
    assert (t >= 0).all(), t
    out[name + "wall-times-shape-and-level-0-count"] = digest(np.int64(t.shape), t[0, 1])
    S.close()
    cube.close()
    return out


def dg_hybrid_digests(ctx, tag, number):
    out, name = {}, "dg-feq-p2-%s-" % tag
    cube = mg.Cube(2, 1, 2)
    S = mg.DGMultigridSolver(ctx, cube, mg.DG_HERMITE, 3, number)
    out[name + "smoother-info"] = digest(info_bytes(ctx.lib.mgx_dg_solver_smoother_info, S.h))
    rng = np.random.default_rng(11)
    src, dst = S.initialize_dof_vector(rng.standard_normal(S.m())), S.initialize_dof_vector()
    S.vmult(dst, src)
    out[name + "vmult"] = digest(dst.download())
    sol = S.initialize_dof_vector()
    its, _ = S.solve_cg(src, sol, 1e-9)
    out[name + "solve_cg"] = digest(np.int64(its), sol.download())
    S.close()
    cube.close()
    return out


def dg_plain_digests(ctx, case, tag, number):
    name, p, basis, cells, n_levels, hierarchy, neumann = case
    out, name = {}, "%s-%s-" % (name, tag)
    S = mg.DGPlainMultigridSolver(ctx, p, basis, cells, np.eye(len(cells)) * 0.7, n_levels, 3, number, neumann_sides=neumann,
                                  hierarchy=hierarchy)
    for l in range(S.n_levels):
        out[name + "smoother-info-L%d" % l] = digest(info_bytes(ctx.lib.mgx_dg_plain_solver_smoother_info, S.h, l))
    rng = np.random.default_rng(len(name))
    a, u = rng.standard_normal(S.m()), rng.standard_normal(S.m())
    src, dst = S.initialize_dof_vector(a), S.initialize_dof_vector()
    S.vmult(dst, src)
    out[name + "vmult"] = digest(dst.download())
    sol = S.initialize_dof_vector()
    its, _ = S.solve_cg(src, sol, 1e-9)
    out[name + "solve_cg"] = digest(np.int64(its), sol.download())
    res, upd = S.initialize_dof_vector(a), S.initialize_dof_vector(u)
    sums = S.vmult_with_residual_update(res, upd, -0.37)
    out[name + "residual-update"] = digest(sums, res.download(), upd.download())
    S.close()
    return out


def all_digests():
    ctx = mg.Context(0)
    out = {}
    try:
        for tag, number in NUMBERS:
            for p in FE_Q_DEGREES:
                out.update(fe_q_digests(ctx, p, tag, number))
            out.update(dg_hybrid_digests(ctx, tag, number))
            for case in PLAIN:
                out.update(dg_plain_digests(ctx, case, tag, number))
        return out
    finally:
        ctx.close()


def test_solver_numerics_are_bitwise_those_of_the_commit_before_the_fold():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = all_digests()
    assert set(golden) == set(got) - set(DROPPED)
    def same(name, a, b):
        if isinstance(b, str):
            return a == b
        return len(a) == len(b) and np.allclose(a, b, rtol=HISTORY_RTOL["f32" if "-f32-" in name else "f64"], atol=0.)

    differ = [name for name in sorted(golden) if not same(name, got[name], golden[name])]
    assert not differ, "%d of %d results differ from the recorded ones: %s" % (len(differ), len(golden), differ[:20])
