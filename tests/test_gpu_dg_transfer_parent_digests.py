"""The DG-to-DG level transfers of mesh steps and of degree steps run one kernel template and one host object
(mgx_dg_transfer.hip, DGLevelStep in mgx_dg_api.cpp).  Merging them may change nothing that is computed: BITWISE against
the commit before the merge.  tests/golden/dg_transfer_parent_digests.json holds the SHA-256 of the raw bytes of every
result below, recorded from a build of that commit with tools/dg_transfer_digests.py, which runs all_digests() of this
file.  Both operations add: every destination starts from seeded random values.

Cases, each in fp64 and fp32 and in both directions (a sized case is there for the paths named with it):
  * mesh step in 3D, p = 1 ... 9: coarse box 1x1x1 (one parent, one workgroup); 3x2x1 in z-order (children[c][k] = 8 c + k:
    the table is not read) and with lexicographic fine order (the table is read; several workgroups from p = 4 on, a
    partly filled last one, one parent per workgroup from p = 6);
  * mesh step in 2D, p = 1 ... 9: box 1x1; box 13x5 in both orders (65 parents against at most 64 per workgroup: two
    workgroups, the last partly filled, at every degree);
  * degree step, all 36 pairs pc < pf: 19 cells in 3D and 67 in 2D (primes: the last workgroup is partly filled whatever
    the number of cells per workgroup), and one cell in either dimension for the pairs (2,1), (9,1), (9,8);
  * the host path of both solver entry points: one fp64 V-cycle (vmult) on a seeded vector of DGPlainMultigridSolver on
    two levels from a 2x1x1 box at p = 2 (mgx_dg_plain_solver_create) and of the hierarchy p = 1 -> 2 on that box
    (mgx_dg_hp_solver_create)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dg_transfer_parent_digests.json")
NUMBERS = (("f64", mg.F64), ("f32", mg.F32))
DEGREES = range(1, 10)
PAIRS = [(pf, pc) for pf in range(2, 10) for pc in range(1, pf)]
# (coarse box, ordering of the cells of both levels)
MESH_BOXES = [((1, 1, 1), "z"), ((3, 2, 1), "z"), ((3, 2, 1), "lexicographic"),
              ((1, 1), "z"), ((13, 5), "z"), ((13, 5), "lexicographic")]
# (cells, dim, pairs)
DEGREE_SIZES = [(19, 3, PAIRS), (67, 2, PAIRS), (1, 3, [(2, 1), (9, 1), (9, 8)]), (1, 2, [(2, 1), (9, 1), (9, 8)])]
# (name, DGPlainMultigridSolver arguments after (ctx, degree, basis, coarse_cells, jacobian0): n_levels, hierarchy)
SOLVERS = [("solver-h-p2-2x1x1-L2", 2, None), ("solver-hp-p1-p2-2x1x1", None, [(1, 0), (2, 0)])]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def both_directions(ctx, T, name, number, n_fine, n_coarse, seed):
    """{name-prolongate: digest of fine, name-restrict: digest of coarse} with seeded sources and destinations"""
    rng = np.random.default_rng(seed)
    f0, c0 = rng.standard_normal(n_fine), rng.standard_normal(n_coarse)
    fine, coarse = ctx.vector(n_fine, number, f0), ctx.vector(n_coarse, number, c0)
    T.prolongate_and_add(fine, coarse)
    out = {name + "-prolongate": digest(fine.download())}
    fine, coarse = ctx.vector(n_fine, number, f0), ctx.vector(n_coarse, number, c0)
    T.restrict_and_add(coarse, fine)
    out[name + "-restrict"] = digest(coarse.download())
    return out


def mesh_step_digests(ctx):
    out = {}
    for box, ordering in MESH_BOXES:
        dim = len(box)
        children = mg.dg_box_children(box, ordering, ordering)
        for p in DEGREES:
            for tag, number in NUMBERS:
                T = mg.DGLevelTransfer(ctx, p, p % 3, children, number)
                n = len(children) * (p + 1) ** dim
                name = "mesh-%dd-p%d-%s-%s-%s" % (dim, p, "x".join(map(str, box)), ordering, tag)
                out.update(both_directions(ctx, T, name, number, n << dim, n, 1000 * p + 10 * dim + len(children)))
                T.clear()
    return out


def degree_step_digests(ctx):
    out = {}
    for n_cells, dim, pairs in DEGREE_SIZES:
        for pf, pc in pairs:
            for tag, number in NUMBERS:
                T = mg.DGDegreeTransfer(ctx, pf, pc, (pf + pc) % 3, n_cells, number, dim)
                name = "degree-%dd-p%d-p%d-n%d-%s" % (dim, pc, pf, n_cells, tag)
                out.update(both_directions(ctx, T, name, number, n_cells * (pf + 1) ** dim, n_cells * (pc + 1) ** dim,
                                           1000 * pf + 100 * pc + 10 * dim + n_cells))
                T.clear()
    return out


def solver_digests(ctx):
    out = {}
    for name, n_levels, hierarchy in SOLVERS:
        S = mg.DGPlainMultigridSolver(ctx, 2, mg.DG_HERMITE, (2, 1, 1), np.eye(3), n_levels, vcycle_number=mg.F64, hierarchy=hierarchy)
        src = S.initialize_dof_vector(np.random.default_rng(len(name)).standard_normal(S.m()))
        dst = S.initialize_dof_vector()
        S.vmult(dst, src)
        out[name + "-vmult"] = digest(dst.download())
        S.close()
    return out


def all_digests():
    ctx = mg.Context(0)
    try:
        return {**mesh_step_digests(ctx), **degree_step_digests(ctx), **solver_digests(ctx)}
    finally:
        ctx.close()


def test_transfers_and_v_cycles_are_bitwise_those_of_the_commit_before_the_merge():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = all_digests()
    assert sorted(got) == sorted(golden)
    differ = [name for name in sorted(got) if got[name] != golden[name]]
    assert not differ, "%d of %d results differ from the recorded ones: %s" % (len(differ), len(got), differ[:20])
