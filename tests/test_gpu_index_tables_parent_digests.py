"""First-owner masks, cell colours and patch multiplicities of the FE_Q set-up come from one host header
(mgx_index_tables.hpp), one mgx_transfer_create serves both dimensions and the 2D launchers run the list loop of the 3D
ones.  None of that may change what is computed: BITWISE against the commit before the change.
tests/golden/index_tables_parent_digests.json holds the SHA-256 of the raw bytes of every result below, recorded from a
build of that commit with tools/index_tables_digests.py (twice, in two processes: every case is free of atomics, and
the two recordings agreed).  Sources and destinations are seeded random vectors, fp64 and fp32.

  * 2D, Square(p, 1, 2) and Square(p, n_refine=1, box=(3, 2)), p = 1, 2, 4: on every level vmult with the diagonal
    coefficient and with a sheared jacobian on the default context (ordered assembly) and on one with cell_colour_min=1
    (colour launches), and the inverse diagonal; prolongate, prolongate_and_add and restrict_and_add with and without
    constraints; on MultigridSolver(ctx, square, general=True) interpolate_to_coarse into a NaN-filled vector,
    compute_nonlinear_residual with both laws on both contexts, update_coefficient + get_coefficient on every level;
  * 2D DG over FE_Q: DGMultigridSolver on Square(2, 1, 1) (4 cells: the greedy colours) and on Square(3, 1, 2) (16 cells:
    the four classes): restrict_to_cg, vmult_residual_and_restrict_to_cg, prolongate_add_cg_to_dg, one vmult;
  * 3D, Cube(p, 1, 2), p = 2, 4: prolongate and prolongate_and_add with and without constraints; on the general=True
    hierarchy interpolate_to_coarse and update_coefficient + get_coefficient.  (No colour launch of the general kernel
    and no restriction in 3D: tests/test_index_tables_host.py pins the order array itself, and
    tests/test_gpu_transfer_routes.py covers every restriction route.)"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_tables_parent_digests.json")
NUMBERS = (("f64", mg.F64, np.float64), ("f32", mg.F32, np.float32))
SHEAR = [[1.0, 0.35], [0.15, 0.8]]
SQUARES = {"1x1-r2": dict(n_subdiv=1, n_refine=2), "3x2-r1": dict(n_refine=1, box=(3, 2))}
DEGREES_2D = (1, 2, 4)
DEGREES_3D = (2, 4)
LAWS = (("unit", mg.LAW_UNIT), ("minsurf", mg.LAW_MINIMAL_SURFACE))
DG_SQUARES = {"p2-2x2": (2, 1, 1), "p3-4x4": (3, 1, 2)}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seeded(name, n, dt=np.float64):
    """the seeded random vector of a case: the same values on every run and in every process"""
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal(n).astype(dt)


def operator_digests(ctx, tag, mesh, l, number, dt):
    """vmult into a seeded destination and the inverse diagonal of the level operator"""
    op = mg.LaplaceOperator.from_cube(ctx, mesh, l, number)
    n = mesh.n_dofs(l)
    src, dst = ctx.vector(n, number, seeded(tag + "-src", n, dt)), ctx.vector(n, number, seeded(tag + "-dst", n, dt))
    op.vmult(dst, src)
    out = {tag + "-vmult": digest(dst.download())}
    op.compute_diagonal()
    out[tag + "-inverse-diagonal"] = digest(op.get_matrix_diagonal_inverse().download())
    op.clear()
    return out


def transfer_digests(ctx, tag, mesh, l, number, dt, restrict):
    ops = [mg.LaplaceOperator.from_cube(ctx, mesh, k, number) for k in (l - 1, l)]
    tr = mg.Transfer(ops[0], ops[1], mesh.children(l), mesh.prolong_1d())
    nc, nf = mesh.n_dofs(l - 1), mesh.n_dofs(l)
    xc, xf = seeded(tag + "-coarse", nc, dt), seeded(tag + "-fine", nf, dt)
    out = {}
    for bc in (False, True):
        name = tag + ("-bc" if bc else "-plain")
        coarse, fine = ctx.vector(nc, number, xc), ctx.vector(nf, number, xf)
        tr.prolongate(fine, coarse, with_constraints=bc)
        out[name + "-prolongate"] = digest(fine.download())
        fine.upload(xf)
        tr.prolongate_and_add(fine, coarse, with_constraints=bc)
        out[name + "-prolongate-add"] = digest(fine.download())
        if restrict:
            fine.upload(xf)
            tr.restrict_and_add(coarse, fine, with_constraints=bc)
            out[name + "-restrict-add"] = digest(coarse.download())
    tr.clear()
    for o in ops:
        o.clear()
    return out


def interpolation_digests(ctx, tag, mesh, solver):
    out = {}
    for l in range(1, mesh.n_levels):
        nc, nf = mesh.n_dofs(l - 1), mesh.n_dofs(l)
        fine, coarse = ctx.vector(nf, data=seeded("%s-L%d-fine" % (tag, l), nf)), ctx.vector(nc, data=np.full(nc, np.nan))
        solver.transfer_dp(l).interpolate_to_coarse(coarse, fine)
        out["%s-L%d-interpolate" % (tag, l)] = digest(coarse.download())
    return out


def coefficient_digests(ctx, tag, mesh, solver):
    """(last: it changes the solver's operators)"""
    n = mesh.n_dofs(mesh.max_level)
    solver.update_coefficient(mg.LAW_MINIMAL_SURFACE, ctx.vector(n, data=0.3 * seeded(tag + "-state", n)))
    out = {}
    for l in range(mesh.n_levels):
        out["%s-L%d-coefficient-f64" % (tag, l)] = digest(solver.matrix_dp(l).get_coefficient().download())
        out["%s-L%d-coefficient-f32" % (tag, l)] = digest(solver.matrix(l).get_coefficient().download())
    return out


def residual_digests(ctx, tag, mesh, solver):
    out = {}
    for l in range(mesh.n_levels):
        n = mesh.n_dofs(l)
        for ntag, number, dt in NUMBERS:
            op = solver.matrix_dp(l) if number == mg.F64 else solver.matrix(l)
            state = ctx.vector(n, number, 0.3 * seeded("%s-L%d-state" % (tag, l), n, dt))
            for law_tag, law in LAWS:
                name = "%s-L%d-residual-%s-%s" % (tag, l, law_tag, ntag)
                dst = ctx.vector(n, number, seeded(name, n, dt))
                op.compute_nonlinear_residual(law, dst, state)
                out[name] = digest(dst.download())
    return out


def square_digests(ctx, colour_ctx):
    out = {}
    for mesh_tag, args in SQUARES.items():
        for p in DEGREES_2D:
            plain, sheared = mg.Square(p, **args), mg.Square(p, jacobian=SHEAR, **args)
            for form, sq in (("diagonal", plain), ("sheared", sheared)):
                for route, c in (("ordered", ctx), ("colours", colour_ctx)):
                    for l in range(sq.n_levels):
                        for ntag, number, dt in NUMBERS:
                            tag = "2d-%s-p%d-%s-%s-L%d-%s" % (mesh_tag, p, form, route, l, ntag)
                            out.update(operator_digests(c, tag, sq, l, number, dt))
            for l in range(1, plain.n_levels):
                for ntag, number, dt in NUMBERS:
                    out.update(transfer_digests(ctx, "2d-%s-p%d-L%d-%s" % (mesh_tag, p, l, ntag), plain, l, number, dt, True))
            for route, c in (("ordered", ctx), ("colours", colour_ctx)):
                tag = "2d-%s-p%d-general-%s" % (mesh_tag, p, route)
                solver = mg.MultigridSolver(c, plain, 2, 2, 1, mg.F32, general=True)
                out.update(interpolation_digests(c, tag, plain, solver))
                out.update(residual_digests(c, tag, plain, solver))
                out.update(coefficient_digests(c, tag, plain, solver))
                solver.close()
            plain.close()
            sheared.close()
    return out


def dg_digests(ctx):
    out = {}
    for mesh_tag, (p, n_subdiv, n_refine) in DG_SQUARES.items():
        sq = mg.Square(p, n_subdiv, n_refine)
        for ntag, number, dt in NUMBERS:
            S = mg.DGMultigridSolver(ctx, sq, mg.DG_HERMITE, 3, number)
            tag = "dg-%s-%s" % (mesh_tag, ntag)
            m, ncg = S.m(), sq.n_dofs(sq.max_level)
            dg = lambda name: ctx.vector(m, number, seeded(tag + name, m, dt))  # noqa: E731
            cg = lambda name: ctx.vector(ncg, number, seeded(tag + name, ncg, dt))  # noqa: E731
            dst = cg("-restrict-dst")
            S.restrict_to_cg(dst, dg("-restrict-src"))
            out[tag + "-restrict"] = digest(dst.download())
            dst = cg("-merged-dst")
            S.vmult_residual_and_restrict_to_cg(dst, dg("-merged-rhs"), dg("-merged-lhs"))
            out[tag + "-residual-restrict"] = digest(dst.download())
            dst = dg("-prolongate-dst")
            S.prolongate_add_cg_to_dg(dst, cg("-prolongate-src"))
            out[tag + "-prolongate"] = digest(dst.download())
            src, dst = S.initialize_dof_vector(seeded(tag + "-vmult-src", m)), S.initialize_dof_vector()
            S.vmult(dst, src)
            out[tag + "-vmult"] = digest(dst.download())
            S.close()
        sq.close()
    return out


def cube_digests(ctx):
    out = {}
    for p in DEGREES_3D:
        cube = mg.Cube(p, 1, 2)
        for l in range(1, cube.n_levels):
            for ntag, number, dt in NUMBERS:
                out.update(transfer_digests(ctx, "3d-p%d-L%d-%s" % (p, l, ntag), cube, l, number, dt, False))
        tag = "3d-p%d-general" % p
        solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F32, general=True)
        out.update(interpolation_digests(ctx, tag, cube, solver))
        out.update(coefficient_digests(ctx, tag, cube, solver))
        solver.close()
        cube.close()
    return out


def all_digests():
    ctx, colour_ctx = mg.Context(0), mg.Context(0, options=dict(cell_colour_min=1))
    try:
        return {**square_digests(ctx, colour_ctx), **dg_digests(ctx), **cube_digests(ctx)}
    finally:
        colour_ctx.close()
        ctx.close()


def test_results_are_bitwise_those_of_the_commit_before_the_tables_were_shared():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = all_digests()
    assert sorted(got) == sorted(golden)
    differ = [name for name in sorted(got) if got[name] != golden[name]]
    assert not differ, "%d of %d results differ from the recorded ones: %s" % (len(differ), len(got), differ[:20])
