"""The first Chebyshev iteration from a zero start (kChebInit, profile form 5) keeps the right-hand side it gathered
and forms x_1 = f0 D^-1 b from it again at write-out instead of loading b a second time.  Nothing it computes may
change by that:

  * BITWISE against the commit before the change: tests/golden/cheb_init_parent_digests.json holds the SHA-256 of the
    raw bytes of smoother.vmult from a zero start (Chebyshev degree 3, first kind) and of the following smoother.step,
    recorded from a build of that commit with tools/cheb_init_digests.py (which runs the cases of this file).  The two
    cases on (5,1,3) were recorded from that commit with the collect pass of the per-item diagonal table made
    deterministic (diag_table_kernel, the one the library has now): without it the table takes, item by item, whichever
    brick wrote last, and on that mesh the commit reproduces none of its own results from one set-up to the next
    (three runs, three digests); with it the commit reproduces every other digest of this file unchanged;
  * against the oracle (cheb_vmult, cheb_step) at 1e-12 in fp64 and 2e-5 in fp32 (the oracle in its fp32 mode);
  * with several bricks per workgroup (the kept value must survive the gather of the next brick, which is issued before
    the write-out): 2.1 M DoFs with 16 resident workgroups, 4 bricks each per colour launch, against the default grid.

Cases (p, ns, nr, number): every degree that changes the shape of the kernels (p <= 4: 4^3-cell bricks and the second
pipeline, p >= 5: 2^3-cell bricks and the first one; p = 9: sliced sweeps), each on eight colour launches with the second
pipeline (mgx_macro2.hip) and without it (mgx_macro.hip, no_macro_v2); (4,1,3) and (4,3,2) also on the two-class and the
one-launch schedule (FREE); (4,1,3) without the per-item table of the inverse diagonal (no_diag_table: the diagonal is
streamed, two operands gathered per value), on eight colours and on two classes.  The sheared box is there as well, but
its operator has the full tensor, gets no brick schedule and never runs form 5: a separable operator whose diagonal is
not uniform per brick item does not exist on the meshes of this project, the option is what reaches that path.
Whether form 5 ran is read from mgx_profile_read and asserted."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle_view import oracle_for  # noqa: E402

FORM_CHEB_INIT = 5
BIG = 4000000000
EIGHT, EIGHT_V1 = {"free_max_bricks": 0}, {"free_max_bricks": 0, "no_macro_v2": 1}
TWO, ONE = {"free_max_bricks": BIG, "free_one_max": 0}, {"free_max_bricks": BIG, "free_one_max": BIG}
MESHES = [(1, 1, 4, "f64"), (2, 1, 4, "f64"), (4, 1, 3, "f64"), (4, 3, 2, "f64"), (5, 1, 3, "f64"), (8, 1, 2, "f64"),
          (9, 1, 2, "f64"), (4, 1, 3, "f32"), (8, 1, 2, "f32")]
SHEARED = ("sheared", 4, 2, "f64")


def _cases():
    out = []
    for m in MESHES:
        out += [(m, "eight", EIGHT), (m, "eight-v1", EIGHT_V1)]
        if m in ((4, 1, 3, "f64"), (4, 3, 2, "f64")):
            out += [(m, "two", TWO), (m, "one", ONE)]
    m = (4, 1, 3, "f64")
    out += [(m, "eight-streamed-diagonal", dict(EIGHT, no_diag_table=1)), (m, "two-streamed-diagonal", dict(TWO, no_diag_table=1))]
    out += [(SHEARED, "eight", EIGHT), (SHEARED, "eight-v1", EIGHT_V1)]
    return out


CASES = _cases()
# (4,1,5): 512 bricks, 64 per colour launch; macro_wg_per_cu_x16 = 1: 256 CUs / 16 = 16 workgroups, 4 bricks each
MULTI = (4, 1, 5, "f64")
MULTI_CASES = [("eight-16wg", dict(EIGHT, macro_wg_per_cu_x16=1)), ("eight", EIGHT)]


def case_name(mesh, tag):
    return "-".join(str(v) for v in mesh) + "-" + tag


def make_cube(mesh):
    if mesh[0] == "sheared":
        return mg.Cube(mesh[1], n_refine=mesh[2], box=(1, 1, 1), origin=-0.9, h0=1.9, geometry="sheared", problem="cube")
    return mg.Cube(*mesh[:3])


def make_oracle(cube, mesh):
    vfloat = mesh[3] == "f32"
    if mesh[0] == "sheared":
        return oracle_for(cube, mesh[1], 1, mesh[2], degree=3, n_cycles=1, geometry="sheared", problem="cube", origin=-0.9, h0=1.9)
    return oracle_for(cube, *mesh[:3], degree=3, n_cycles=1, vfloat=vfloat)


def rhs_of(cube, mesh):
    b = cube.seeded_vector(cube.max_level, 22)
    return b.astype(np.float32).astype(np.float64) if mesh[3] == "f32" else b


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def smoother_results(cube, mesh, opts, b):
    """smoother.vmult from a zero start and the following step on the finest level of the solver's hierarchy (pre-smoothing
    form: Chebyshev degree 3, first kind); returns both and the launches of form 5"""
    vnum = mg.F32 if mesh[3] == "f32" else mg.F64
    ctx = mg.Context(0, options=opts)
    solver = mg.MultigridSolver(ctx, cube, 3, 3, 1, vnum)
    try:
        l = cube.max_level
        A, sm = solver.matrix(l), solver.smoother(l)
        bd, xd = ctx.vector(b.size, vnum, b), ctx.vector(b.size, vnum, np.full(b.size, np.nan))
        ctx.profile_enable(True)
        A.set_profiled(True)
        ctx.profile_read(FORM_CHEB_INIT)
        sm.vmult(xd, bd)
        x1 = xd.download()
        n5 = ctx.profile_read(FORM_CHEB_INIT)[0]
        A.set_profiled(False)
        ctx.profile_enable(False)
        sm.step(xd, bd)
        return x1, xd.download(), n5
    finally:
        solver.close()
        ctx.close()


def multi_results(cube, opts, b):
    """the same two applications of a Chebyshev smoother (degree 3) on the finest level alone"""
    ctx = mg.Context(0, options=opts)
    op = mg.LaplaceOperator.from_cube(ctx, cube, cube.max_level, number=mg.F64)
    sm = mg.Chebyshev(op, 20., 3, 15)
    try:
        bd, xd = ctx.vector(b.size, mg.F64, b), ctx.vector(b.size, mg.F64, np.full(b.size, np.nan))
        ctx.profile_enable(True)
        op.set_profiled(True)
        ctx.profile_read(FORM_CHEB_INIT)
        sm.vmult(xd, bd)
        x1 = xd.download()
        n5 = ctx.profile_read(FORM_CHEB_INIT)[0]
        op.set_profiled(False)
        ctx.profile_enable(False)
        sm.step(xd, bd)
        return x1, xd.download(), n5
    finally:
        sm.clear()
        op.clear()
        ctx.close()


def all_digests(only=()):
    """{case:vmult|step -> digest} of every case of this file (only: of the cases whose name starts with one of these)
    with the library that is loaded (tools/cheb_init_digests.py)"""
    out, cubes = {}, {}
    wanted = lambda name: not only or any(name.startswith(o) for o in only)  # noqa: E731
    for mesh, tag, opts in CASES:
        if not wanted(case_name(mesh, tag)):
            continue
        if mesh not in cubes:
            cubes[mesh] = make_cube(mesh)
        x1, x2, _ = smoother_results(cubes[mesh], mesh, opts, rhs_of(cubes[mesh], mesh))
        out[case_name(mesh, tag) + ":vmult"], out[case_name(mesh, tag) + ":step"] = digest(x1), digest(x2)
    for c in cubes.values():
        c.close()
    if any(wanted(case_name(MULTI, tag)) for tag, _ in MULTI_CASES):
        cube = make_cube(MULTI)
        for tag, opts in MULTI_CASES:
            if wanted(case_name(MULTI, tag)):
                x1, x2, _ = multi_results(cube, opts, rhs_of(cube, MULTI))
                out[case_name(MULTI, tag) + ":vmult"], out[case_name(MULTI, tag) + ":step"] = digest(x1), digest(x2)
        cube.close()
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cheb_init_parent_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


_cubes, _refs = {}, {}


def cube_of(mesh):
    if mesh not in _cubes:
        _cubes[mesh] = make_cube(mesh)
    return _cubes[mesh]


def refs_of(mesh):
    """right-hand side and the oracle's two results, computed once per mesh and number type"""
    if mesh not in _refs:
        cube = cube_of(mesh)
        orc = make_oracle(cube, mesh)
        b = rhs_of(cube, mesh)
        x1 = orc.cheb_vmult(cube.max_level, b)
        _refs[mesh] = (b, x1, orc.cheb_step(cube.max_level, x1, b))
        orc.close()
    return _refs[mesh]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for c in _cubes.values():
        c.close()
    _cubes.clear()
    _refs.clear()


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("mesh,tag,opts", CASES, ids=[case_name(m, t) for m, t, _ in CASES])
def test_zero_start_and_step_bitwise_and_against_the_oracle(golden, mesh, tag, opts):
    cube = cube_of(mesh)
    b, ref1, ref2 = refs_of(mesh)
    x1, x2, n5 = smoother_results(cube, mesh, opts, b)
    name = case_name(mesh, tag)
    if mesh[0] != "sheared":
        assert n5 > 0, "%s: the first-iterate form did not run" % name
    tol = 2e-5 if mesh[3] == "f32" else 1e-12
    e1, e2 = rel(x1.astype(np.float64), ref1), rel(x2.astype(np.float64), ref2)
    print("%s: form-5 launches %d, vmult against the oracle %.3e, step %.3e (bound %g)" % (name, n5, e1, e2, tol))
    assert digest(x1) == golden[name + ":vmult"], "%s: smoother.vmult differs from the build before the change" % name
    assert digest(x2) == golden[name + ":step"], "%s: smoother.step differs from the build before the change" % name
    assert e1 < tol, "%s: smoother.vmult against the oracle %g" % (name, e1)
    assert e2 < tol, "%s: smoother.step against the oracle %g" % (name, e2)


def test_several_bricks_per_workgroup(golden):
    cube = make_cube(MULTI)
    try:
        b = rhs_of(cube, MULTI)
        res = {}
        for tag, opts in MULTI_CASES:
            x1, x2, n5 = multi_results(cube, opts, b)
            assert n5 > 0, "%s: the first-iterate form did not run" % tag
            name = case_name(MULTI, tag)
            assert digest(x1) == golden[name + ":vmult"], "%s: smoother.vmult differs from the build before the change" % name
            assert digest(x2) == golden[name + ":step"], "%s: smoother.step differs from the build before the change" % name
            res[tag] = (x1, x2)
        assert np.array_equal(res["eight-16wg"][0], res["eight"][0]) and np.array_equal(res["eight-16wg"][1], res["eight"][1])
    finally:
        cube.close()
