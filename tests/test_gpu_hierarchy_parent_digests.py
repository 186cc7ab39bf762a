"""One builder (mgx_hierarchy.cpp) assembles the FE_Q hierarchy of the cube and of the square: level operators in two
precisions, the geometry for coefficient updates, the two transfer chains, right-hand sides and boundary data.  None of
that may change what a hierarchy holds or computes: BITWISE against the commit before the change.
tests/golden/hierarchy_parent_digests.json holds the SHA-256 of the raw bytes of every result below, recorded from a
build of that commit with tools/hierarchy_digests.py (twice, in two processes: every case is free of atomics, and the
two recordings agreed).

  * 2D, Square(p, 1, 2) and Square(p, n_refine=1, box=(3, 2), jacobian=SHEAR), p = 1, 3, with an fp32 and an fp64
    V-cycle: the plain hierarchy with and without per_point, the general one with coef_q=None and with a caller's list
    (1.5 x the unit-law tensor on the finest level, None below); the mapped Square(2, 1, 1, "annulus_sector") on the
    general routes.  On every level: the right-hand side, the coefficient of both operators ("none" where an operator
    has no per-point tensor), prolongate of both chains with and without constraints.  General routes: the nonlinear
    residual with both laws on the finest level ("refused" on the fp32 operator of curved cells, whose geometry is kept
    with the fp64 one), then update_coefficient with both laws and the coefficients of every level.  Square(3, 1, 2),
    fp64, plain: solve_cg iterations and the solution;
  * 3D, Cube(2, 1, 2): the plain host-rhs hierarchy in both precisions (right-hand side of level 0, prolongate);
    general=True with jacobian=None, with a sheared jacobian and with a caller's coef_q; the per-point route on
    Cube(2, n_refine=1, box=(2, 2, 2), geometry="sheared") and on Cube(2, n_refine=1, shell=6, problem="cube").  General
    routes: the coefficients of every level after creation and after update_coefficient, interpolate_to_coarse into a
    NaN-filled vector.  (No 3D vmult, restriction, device right-hand side or solve: those may use atomics, and the
    parity, transfer-route and distributed tests cover them.  No host right-hand side of the 3D levels 1 and 2 either:
    the two recordings of the commit before differed there.)"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hierarchy_parent_digests.json")
NUMBERS = (("f32", mg.F32, np.float32), ("f64", mg.F64, np.float64))
SHEAR = [[1.0, 0.35], [0.15, 0.8]]
SHEAR_3D = [[1.0, 0.2, 0.1], [0.05, 0.9, 0.15], [0.1, 0.0, 1.1]]
SQUARES = {"1x1-r2": dict(n_subdiv=1, n_refine=2), "3x2-r1-sheared": dict(n_refine=1, box=(3, 2), jacobian=SHEAR)}
DEGREES_2D = (1, 3)
LAWS = (("unit", mg.LAW_UNIT), ("minsurf", mg.LAW_MINIMAL_SURFACE))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seeded(name, n, dt=np.float64):
    """the seeded random vector of a case: the same values on every run and in every process"""
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal(n).astype(dt)


def dtype_of(number):
    return np.float64 if number == mg.F64 else np.float32


def scaled_finest(mesh):
    """a caller's coef_q list: 1.5 x the unit-law tensor on the finest level, the hierarchy's own below"""
    return [None] * mesh.max_level + [1.5 * mesh.unit_law_coefficient(mesh.max_level)]


def coefficient_digests(tag, mesh, solver):
    out = {}
    for l in range(mesh.n_levels):
        for name, op in (("f64", solver.matrix_dp(l)), ("vcycle", solver.matrix(l))):
            try:
                out["%s-L%d-coefficient-%s" % (tag, l, name)] = digest(op.get_coefficient().download())
            except mg.MgxError:  # separable or one-tensor operator
                out["%s-L%d-coefficient-%s" % (tag, l, name)] = "none"
    return out


def rhs_digests(tag, mesh, solver, levels=None):
    levels = range(mesh.n_levels) if levels is None else levels
    return {"%s-L%d-rhs" % (tag, l): digest(solver.get_vector(l, "rhs").download()) for l in levels}


def prolongate_digests(ctx, tag, mesh, solver):
    out = {}
    for l in range(1, mesh.n_levels):
        nc, nf = mesh.n_dofs(l - 1), mesh.n_dofs(l)
        for chain, tr, number in (("f64", solver.transfer_dp(l), mg.F64), ("vcycle", solver.transfer(l), solver.vnumber)):
            dt = dtype_of(number)
            name = "%s-L%d-%s" % (tag, l, chain)
            for bc in (False, True):
                coarse = ctx.vector(nc, number, seeded(name + "-coarse", nc, dt))
                fine = ctx.vector(nf, number, seeded(name + "-fine", nf, dt))
                tr.prolongate(fine, coarse, with_constraints=bc)
                out[name + ("-bc" if bc else "-plain") + "-prolongate"] = digest(fine.download())
    return out


def interpolation_digests(ctx, tag, mesh, solver):
    out = {}
    for l in range(1, mesh.n_levels):
        nc, nf = mesh.n_dofs(l - 1), mesh.n_dofs(l)
        fine, coarse = ctx.vector(nf, data=seeded("%s-L%d-fine" % (tag, l), nf)), ctx.vector(nc, data=np.full(nc, np.nan))
        solver.transfer_dp(l).interpolate_to_coarse(coarse, fine)
        out["%s-L%d-interpolate" % (tag, l)] = digest(coarse.download())
    return out


def residual_digests(ctx, tag, mesh, solver):
    """compute_nonlinear_residual with both laws on the finest level, in both precisions"""
    out, l = {}, mesh.max_level
    n = mesh.n_dofs(l)
    for name, op, number in (("f64", solver.matrix_dp(l), mg.F64), ("vcycle", solver.matrix(l), solver.vnumber)):
        dt = dtype_of(number)
        state = ctx.vector(n, number, 0.3 * seeded(tag + "-residual-state", n, dt))
        for law_tag, law in LAWS:
            key = "%s-residual-%s-%s" % (tag, law_tag, name)
            dst = ctx.vector(n, number, seeded(key, n, dt))
            try:
                op.compute_nonlinear_residual(law, dst, state)
                out[key] = digest(dst.download())
            except mg.MgxError:  # curved cells: the geometry is kept with the fp64 operator only
                out[key] = "refused"
    return out


def update_digests(ctx, tag, mesh, solver, laws):
    """(last: it changes the solver's operators)"""
    out, n = {}, mesh.n_dofs(mesh.max_level)
    for law_tag, law in laws:
        solver.update_coefficient(law, ctx.vector(n, data=0.3 * seeded(tag + "-state", n)))
        out.update(coefficient_digests("%s-updated-%s" % (tag, law_tag), mesh, solver))
    return out


def plain_digests(ctx, tag, mesh, solver):
    return {**rhs_digests(tag, mesh, solver), **coefficient_digests(tag, mesh, solver),
            **prolongate_digests(ctx, tag, mesh, solver)}


def general_digests_2d(ctx, tag, mesh, number):
    out = {}
    for route, coef_q in (("unit", None), ("caller", scaled_finest(mesh))):
        name = "%s-general-%s" % (tag, route)
        solver = mg.MultigridSolver(ctx, mesh, 2, 2, 1, number, general=True, coef_q=coef_q)
        out.update(plain_digests(ctx, name, mesh, solver))
        out.update(residual_digests(ctx, name, mesh, solver))
        out.update(update_digests(ctx, name, mesh, solver, LAWS))
        solver.close()
    return out


def square_digests(ctx):
    out = {}
    for mesh_tag, args in SQUARES.items():
        for p in DEGREES_2D:
            sq = mg.Square(p, **args)
            for ntag, number, _ in NUMBERS:
                tag = "2d-%s-p%d-%s" % (mesh_tag, p, ntag)
                for per_point in (False, True):
                    solver = mg.MultigridSolver(ctx, sq, 2, 2, 1, number, per_point=per_point)
                    out.update(plain_digests(ctx, tag + ("-per-point" if per_point else "-plain"), sq, solver))
                    solver.close()
                out.update(general_digests_2d(ctx, tag, sq, number))
            sq.close()
    sq = mg.Square(2, 1, 1, mapped="annulus_sector")
    for ntag, number, _ in NUMBERS:
        out.update(general_digests_2d(ctx, "2d-annulus-p2-" + ntag, sq, number))
    sq.close()
    sq = mg.Square(3, 1, 2)
    solver = mg.MultigridSolver(ctx, sq, 3, 3, 1, mg.F64)
    its, _ = solver.solve_cg()
    out["2d-1x1-r2-p3-f64-solve-cg-iterations"] = digest(np.array([its], dtype=np.int64))
    out["2d-1x1-r2-p3-f64-solve-cg-solution"] = digest(solver.get_solution().download())
    solver.close()
    sq.close()
    return out


def general_digests_3d(ctx, tag, cube, **kwargs):
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, mg.F32, general=True, **kwargs)
    out = coefficient_digests(tag, cube, solver)
    out.update(interpolation_digests(ctx, tag, cube, solver))
    out.update(update_digests(ctx, tag, cube, solver, LAWS[1:]))
    solver.close()
    return out


def cube_digests(ctx):
    out = {}
    cube = mg.Cube(2, 1, 2)
    for ntag, number, _ in NUMBERS:
        solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, number)
        tag = "3d-p2-plain-" + ntag
        # (level 0 only: the cube assembles its host right-hand side with OpenMP and atomic adds, and the sums of the
        # levels with more than one cell were not the same bits in two recordings of the commit before)
        out.update(rhs_digests(tag, cube, solver, levels=(0,)))
        out.update(prolongate_digests(ctx, tag, cube, solver))
        solver.close()
    out.update(general_digests_3d(ctx, "3d-p2-general-identity", cube))
    out.update(general_digests_3d(ctx, "3d-p2-general-sheared", cube, jacobian=SHEAR_3D))
    out.update(general_digests_3d(ctx, "3d-p2-general-caller", cube, coef_q=scaled_finest(cube)))
    cube.close()
    for tag, args in (("3d-p2-box-sheared", dict(box=(2, 2, 2), geometry="sheared")), ("3d-p2-shell6", dict(shell=6, problem="cube"))):
        cube = mg.Cube(2, n_refine=1, **args)
        out.update(general_digests_3d(ctx, tag + "-general", cube))
        cube.close()
    return out


def all_digests():
    ctx = mg.Context(0)
    try:
        return {**square_digests(ctx), **cube_digests(ctx)}
    finally:
        ctx.close()


def test_hierarchies_are_bitwise_those_of_the_commit_before_the_builder_was_shared():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = all_digests()
    assert sorted(got) == sorted(golden)
    differ = [name for name in sorted(got) if got[name] != golden[name]]
    assert not differ, "%d of %d results differ from the recorded ones: %s" % (len(differ), len(got), differ[:20])
