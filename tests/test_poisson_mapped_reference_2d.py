"""The numpy restatement of a linear problem on a Square (tests/poisson_mapped_reference_2d.py) and the problem
description of the 2D provider (include/mgx_square.h: mgx_square_problem, mgx_square_problem_*) pinned on the CPU: the
provider's four arrays are those the reference computes from the cell nodes, on the box, the sheared box, the annulus
sector and the disc; on the box with the box's own problem the reference is the existing host right-hand side and L2
error; a polynomial of the element's degree is reproduced; the dense solve converges on the disc; and the provider's
host code runs clean under AddressSanitizer and UBSan in a program of its own (tests/square_problem_check.cpp).

CONVERGENCE names the degree and the level pair of the disc whose error ratio test_gpu_poisson_mapped_2d.py asks of the
device as well.  Measured with the reference alone (u = sin(2 pi (x + y)), contrast 0), L2 errors of the dense solve on
levels 1, 2, 3:
    p = 2:  1.987e-01  2.110e-02  4.798e-03   ratios  9.42  4.40   (0.8 * 2^3 =  6.4: the pair (2, 3) misses it)
    p = 3:  5.010e-02  7.790e-03  4.048e-04   ratios  6.43  19.24  (0.8 * 2^4 = 12.8: the pair (1, 2) misses it)
so p = 3 with the levels (2, 3), ratio 19.24."""
import os
import subprocess

import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
import poisson_mapped_reference_2d as pm  # noqa: E402
from test_gpu_feq_2d import SHEAR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_amd", "csrc")

# degree and level pair of the convergence check on the disc (see above)
CONVERGENCE = dict(p=3, levels=(2, 3))

GEOMETRIES = ("box", "sheared", "sector", "ball")
PROBLEMS = (("cube", 0.0), ("shell", 1.0), ("shell", 1.0e6))


def make_square(geometry, p, n_refine=None):
    """box: 3 x 2 roots refined once; sheared: the same under SHEAR; sector: 2 x 3 roots of the annulus sector refined
    once; ball: the disc, level 2 -- the meshes of test_gpu_poisson_mapped_2d.py (its disc: level 3)"""
    if geometry == "ball":
        return mg.Square(p, n_refine=2 if n_refine is None else n_refine, mapped="ball")
    if geometry == "sector":
        return mg.Square(p, box=(2, 3), n_refine=1 if n_refine is None else n_refine, h0=1.9 / 3, mapped="annulus_sector")
    return mg.Square(p, box=(3, 2), n_refine=1 if n_refine is None else n_refine, h0=1.9 / 3,
                     jacobian=SHEAR if geometry == "sheared" else None)


def problems(kind, contrast):
    return mg.SquareProblem(kind, contrast), pm.Problem(kind, contrast)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


@pytest.mark.parametrize("p", [1, 2, 4, 7])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_provider_arrays(geometry, p):
    """coef_q, rhs_quadrature, solution_q and bc_value of every level against the reference, 1e-13 relative"""
    sq = make_square(geometry, p)
    for l in range(sq.n_levels):
        R = pm.PoissonMappedReference2D.from_square(sq, l)
        n2 = (p + 1) ** 2
        for kind, contrast in PROBLEMS:
            P, Pr = problems(kind, contrast)
            coef = sq.problem_coef_q(l, P)
            assert coef.shape == (sq.n_cells(l), 3, n2)
            assert rel(coef, R.coef_q(Pr)) < 1e-13
            assert rel(sq.problem_rhs_quadrature(l, P), R.rhs_quadrature(Pr)) < 1e-13
            assert rel(sq.problem_solution_q(l, P), R.solution_q(Pr)) < 1e-13
            bc = sq.problem_bc_value(l, P)
            assert bc.shape == (sq.n_constrained(l),)
            assert rel(bc, R.bc_value(Pr)) < 1e-13
    sq.close()


@pytest.mark.parametrize("p", [1, 3, 4])
def test_reference_is_the_host_problem_of_the_box(p):
    """box + the box's own problem: the reference's right-hand side is Square.rhs, its error Square.l2_error, and the
    provider's boundary values are Square.bc"""
    sq = make_square("box", p)
    P, Pr = problems("cube", 0.0)
    for l in range(sq.n_levels):
        R = pm.PoissonMappedReference2D.from_square(sq, l)
        assert rel(R.rhs(Pr), sq.rhs(l)) < 1e-12
        assert np.array_equal(R.rhs(Pr)[sq.constrained(l)], np.zeros(sq.n_constrained(l)))
        u = sq.seeded_vector(l, 5)
        assert abs(R.l2_error(Pr, u) - sq.l2_error(l, u)) < 1e-12 * sq.l2_error(l, u)
        index, value = sq.bc(l)
        assert np.array_equal(index, sq.constrained(l)) and rel(sq.problem_bc_value(l, P), value) < 1e-14
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 3, 5])
def test_consistency_with_the_operator(p):
    """affine box, a = 1: for u = (1 + x)^p (1 - y / 2)^p + x y, a polynomial of degree <= p per direction, the
    right-hand side with f = -lap u equals A u on the free rows (the element reproduces u, the rule integrates the
    products exactly)"""
    sq = make_square("box", p)
    l = sq.max_level
    R = pm.PoissonMappedReference2D.from_square(sq, l)
    x, y = R.dof_xy[:, 0], R.dof_xy[:, 1]
    u = (1 + x) ** p * (1 - y / 2) ** p + x * y
    xq, yq = R.x_q[..., 0], R.x_q[..., 1]
    lap = (p * (p - 1) * (1 + xq) ** max(p - 2, 0) * (1 - yq / 2) ** p if p > 1 else 0.0) + \
          (p * (p - 1) / 4 * (1 + xq) ** p * (1 - yq / 2) ** max(p - 2, 0) if p > 1 else 0.0)
    coef = R.ref.U
    u_bc = np.zeros_like(u)
    u_bc[R.constrained] = u[R.constrained]
    rhs = R.residual(coef, u_bc, -lap * R.jxw_q)
    u_free = u - u_bc
    Au = R.ref.apply(coef, u_free)
    free = R.ref.free
    assert np.abs(rhs[free] - Au[free]).max() < 1e-11 * np.abs(Au[free]).max()
    sq.close()


def test_summation_orders_agree():
    """the reference's right-hand side with the cells added forward, reversed and in extended precision: the spread is
    rounding, at contrast 1 and at 1e6"""
    sq = make_square("ball", 3)
    l = sq.max_level
    R = pm.PoissonMappedReference2D.from_square(sq, l)
    for contrast, bound in ((1.0, 1e-13), (1.0e6, 1e-12)):
        Pr = pm.Problem("shell", contrast)
        fwd, rev, ext = R.rhs(Pr), R.rhs(Pr, reverse=True), R.rhs(Pr, dtype=np.longdouble).astype(np.float64)
        assert rel(fwd, rev) < bound and rel(fwd, ext) < bound
    sq.close()


def test_convergence_on_the_disc():
    """contrast 0: the L2 error of the dense solve falls by at least 0.8 * 2^(p+1) between the levels of CONVERGENCE"""
    p, (coarse, fine) = CONVERGENCE["p"], CONVERGENCE["levels"]
    Pr, errors = pm.Problem("shell", 0.0), []
    for level in (coarse, fine):
        sq = make_square("ball", p, n_refine=level)
        R = pm.PoissonMappedReference2D.from_square(sq, level)
        errors.append(R.l2_error(Pr, R.solve(Pr)))
        sq.close()
    print("disc p = %d, levels %d, %d: errors %.3e %.3e, ratio %.2f" % (p, coarse, fine, errors[0], errors[1], errors[0] / errors[1]))
    assert errors[0] / errors[1] >= 0.8 * 2 ** (p + 1)


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tests/square_problem_check.cpp with the provider's host sources, under AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("square_problem") / "square_problem_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "square_problem_check.cpp")] +
                   [os.path.join(CSRC, f) for f in ("mgx_square.cpp", "mgx_cube.cpp", "mgx_bricks.cpp")], check=True)
    return exe


@pytest.mark.parametrize("p", [1, 4])
def test_provider_on_the_host_under_sanitizers(check_program, p):
    """the four accessors and the host side of mgx_square_solver_create_problem on all four geometries in a program of its
    own: no sanitizer report, every refusal an MGX_ERR_INVALID_ARGUMENT, every level described, and the arrays those of
    the library (weighted sums)"""
    out = subprocess.run([check_program, str(p)], check=True, capture_output=True, timeout=120).stdout.decode()
    lines = [ln.split() for ln in out.splitlines()]
    tail = {ln[0]: ln[1] for ln in lines if len(ln) == 2}
    assert tail == {"refused": "28", "described": "18", "done": "1"}
    weights = lambda a: 1.0 + np.arange(a.size) % 7
    seen = 0
    for geometry in GEOMETRIES:
        sq = make_square(geometry, p)
        for kind in ("cube", "shell"):
            P = mg.SquareProblem(kind, 1.0e6)
            for l in range(sq.n_levels):
                row = [ln for ln in lines if ln[:3] == [geometry, kind, str(l)]]
                assert len(row) == 1
                arrays = (sq.problem_coef_q(l, P), sq.problem_rhs_quadrature(l, P), sq.problem_solution_q(l, P),
                          sq.problem_bc_value(l, P))
                for text, a in zip(row[0][3:], arrays):
                    a = a.ravel()
                    assert abs(float(text) - (a * weights(a)).sum()) <= 1e-12 * (np.abs(a) * weights(a)).sum()
                seen += 1
        sq.close()
    assert seen == 18
