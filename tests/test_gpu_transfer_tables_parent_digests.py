"""The assembly and transfer tables of the FE_Q set-up -- ordered assembly, brick cell lists, patch table, block table of
the fused forms, its scratch CSR -- are built by plain host functions (mgx_transfer_tables.hpp) with one node rule
(mgx_index_tables.hpp).  None of that may change what is computed: BITWISE against the commit before the change.
tests/golden/transfer_tables_parent_digests.json holds the SHA-256 of the raw bytes of every result below and the route
lines of the set-up trace, recorded from a build of that commit with tools/transfer_tables_digests.py (twice, in two
processes: every case is free of atomics, and the two recordings agreed).  3D, fp64 and fp32, seeded random vectors;
the thresholds are those of the suite (brick_min 1, restrict_colour_min 8), set as context options.

  * ordered assembly: Cube(p, 3, 1), p = 1, 2, 4, brick_min above every level: vmult and the inverse diagonal on both
    levels, restrict_and_add with constraints (the assembly route: 27 parents are not colourable by index mod 8);
  * colour launches: Cube(p, 1, 2), p = 1, 2, 4: restrict_and_add onto the 8 parents of level 1, with and without
    constraints;
  * brick-level forms: Cube(2, 1, 4), Cube(4, 1, 3), Cube(5, 1, 3), Cube(8, 1, 2) under the three schedule settings of
    tests/test_gpu_schedules.py: one V-cycle (solver.vmult) and compute_diagonal on the two finest levels -- fused
    residual + restriction in colour launches (eight colours) and in scratch form (two classes, one launch), fused
    prolongation, brick cell lists.
(No atomic restriction route: its last bits are not reproducible.)"""
import contextlib
import hashlib
import json
import os
import tempfile
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_tables_parent_digests.json")
NUMBERS = (("f64", mg.F64, np.float64), ("f32", mg.F32, np.float32))
SUITE = dict(brick_min=1, restrict_colour_min=8, trace=1)
DEGREES = (1, 2, 4)
BRICK_CUBES = ((2, 1, 4), (4, 1, 3), (5, 1, 3), (8, 1, 2))
# (the three settings of tests/test_gpu_schedules.py, as context options)
SCHEDULES = {"eight": dict(free_max_bricks=0),
             "two": dict(free_max_bricks=4000000000, free_one_max=0),
             "one": dict(free_max_bricks=4000000000, free_one_max=4000000000)}
ROUTE_WORDS = ("ordered assembly", "restriction in", "fused residual + restriction", "fused prolongation", "coarse colouring")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seeded(name, n, dt=np.float64):
    """the seeded random vector of a case: the same values on every run and in every process"""
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal(n).astype(dt)


@contextlib.contextmanager
def set_up_trace(lines):
    """appends to `lines` the route lines the library writes to stderr inside the block, each once"""
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            for s in f.read().decode(errors="replace").splitlines():
                s = s[s.index("_create:") + 9:].strip() if "_create:" in s else ""
                if any(w in s for w in ROUTE_WORDS) and s not in lines:
                    lines.append(s)


def context(**options):
    return mg.Context(0, options=dict(SUITE, **options))


def operator_digests(ctx, tag, cube, l, number, dt, routes):
    with set_up_trace(routes):
        op = mg.LaplaceOperator.from_cube(ctx, cube, l, number)
    n = cube.n_dofs(l)
    src, dst = ctx.vector(n, number, seeded(tag + "-src", n, dt)), ctx.vector(n, number, seeded(tag + "-dst", n, dt))
    op.vmult(dst, src)
    out = {tag + "-vmult": digest(dst.download())}
    op.compute_diagonal()
    out[tag + "-inverse-diagonal"] = digest(op.get_matrix_diagonal_inverse().download())
    op.clear()
    return out


def restrict_digests(ctx, tag, cube, l, number, dt, constraints, routes):
    with set_up_trace(routes):
        ops = [mg.LaplaceOperator.from_cube(ctx, cube, k, number) for k in (l - 1, l)]
        tr = mg.Transfer(ops[0], ops[1], cube.children(l), cube.prolong_1d())
    nc, nf = cube.n_dofs(l - 1), cube.n_dofs(l)
    out = {}
    for bc in constraints:
        coarse, fine = ctx.vector(nc, number, seeded(tag + "-coarse", nc, dt)), ctx.vector(nf, number, seeded(tag + "-fine", nf, dt))
        tr.restrict_and_add(coarse, fine, with_constraints=bc)
        out[tag + ("-bc" if bc else "-plain") + "-restrict-add"] = digest(coarse.download())
    tr.clear()
    for o in ops:
        o.clear()
    return out


def assembly_digests():
    out, ctx = {}, context(brick_min=4000000000)
    for p in DEGREES:
        cube = mg.Cube(p, 3, 1)
        for ntag, number, dt in NUMBERS:
            tag, routes = "assembly-p%d-%s" % (p, ntag), []
            for l in range(cube.n_levels):
                out.update(operator_digests(ctx, "%s-L%d" % (tag, l), cube, l, number, dt, routes))
            out.update(restrict_digests(ctx, tag + "-L1", cube, 1, number, dt, (True,), routes))
            out[tag + "-routes"] = routes
        cube.close()
    ctx.close()
    return out


def colour_digests():
    out, ctx = {}, context()
    for p in DEGREES:
        cube = mg.Cube(p, 1, 2)
        for ntag, number, dt in NUMBERS:
            tag, routes = "colours-p%d-%s" % (p, ntag), []
            out.update(restrict_digests(ctx, tag + "-L2", cube, 2, number, dt, (False, True), routes))
            out[tag + "-routes"] = routes
        cube.close()
    ctx.close()
    return out


def brick_digests():
    out = {}
    for p, ns, nr in BRICK_CUBES:
        cube = mg.Cube(p, ns, nr)
        l, n = cube.max_level, cube.n_dofs(cube.max_level)
        for schedule, options in SCHEDULES.items():
            ctx = context(**options)
            for ntag, number, dt in NUMBERS:
                tag, routes = "bricks-p%d-r%d-%s-%s" % (p, nr, schedule, ntag), []
                with set_up_trace(routes):
                    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, number)
                src, dst = ctx.vector(n, data=seeded(tag + "-src", n)), ctx.vector(n, data=seeded(tag + "-dst", n))
                solver.vmult(dst, src)
                out[tag + "-vcycle"] = digest(dst.download())
                for k in (l - 1, l):
                    A = solver.matrix(k)
                    A.compute_diagonal()
                    out["%s-L%d-inverse-diagonal" % (tag, k)] = digest(A.get_matrix_diagonal_inverse().download())
                out[tag + "-routes"] = routes
                solver.close()
            ctx.close()
        cube.close()
    return out


def all_digests():
    return {**assembly_digests(), **colour_digests(), **brick_digests()}


def test_results_are_bitwise_those_of_the_commit_before_the_tables_became_host_functions():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = all_digests()
    assert sorted(got) == sorted(golden)
    differ = [name for name in sorted(got) if got[name] != golden[name]]
    assert not differ, "%d of %d results differ from the recorded ones: %s" % (len(differ), len(got), differ[:20])
    # the routes the cases claim are the ones that ran
    routes = {name: " | ".join(v) for name, v in got.items() if name.endswith("-routes")}
    for name, lines in routes.items():
        if name.startswith("assembly"):
            assert "ordered assembly of the per-cell kernel" in lines, (name, lines)
            assert "restriction in one launch, ordered assembly with constraints" in lines, (name, lines)
        elif name.startswith("colours"):
            assert "restriction in 8 colour launches" in lines, (name, lines)
        else:
            # (fused prolongation: never on the one-launch schedule, on the two-class schedule of these few bricks only
            # above degree 4 -- fused_prolong_blocker of mgx_api.cpp)
            schedule, p = name.split("-")[3], int(name.split("-")[1][1:])
            form = "colour launches" if schedule == "eight" else "scratch form"
            assert "fused residual + restriction yes (%s)" % form in lines, (name, lines)
            assert ("fused prolongation yes" in lines) == (schedule == "eight" or (schedule == "two" and p > 4)), (name, lines)
