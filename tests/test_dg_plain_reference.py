"""Properties that pin tests/dg_plain_reference.py -- the numpy restatement of MultigridSolverDGPlain
(common/multigrid_solver_dg_plain.h:55-595) the GPU tests compare against -- independently of the product, and the
compile check of the shim's MultigridSolverDGPlain mirror.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_plain_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHEARED = dg.cheby_mesh(0)[1]
BASES = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]


@pytest.mark.parametrize("kind", BASES)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5])
def test_prolongation_reproduces_polynomials(p, kind):
    """a polynomial of degree <= p lies in the space of both levels: its coefficients on the coarse level,
    prolongated, are its coefficients on the fine level (measured <= 1.1e-11)"""
    o = ref.DGPlainOracle(p, kind, (2, 1, 1), SHEARED, 2)
    a = np.array([0.3, -0.5, 0.7])
    fn = lambda x: (1.0 + x @ a) ** p   # noqa: E731
    coarse, fine = o.level[0].interpolate(fn), o.level[1].interpolate(fn)
    assert abs(o.prolongate(1, coarse) - fine).max() < 1e-10 * abs(fine).max()


@pytest.mark.parametrize("kind", BASES)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 7, 9])
def test_embedding_preserves_the_mass_matrix_and_is_mirror_symmetric(p, kind):
    o = dg.DGOracle(p, kind, (1, 1, 1), np.eye(3))
    P = ref.embedding_1d(p, kind)
    mass = o.S.T @ (o.wq[:, None] * o.S)            # on [0, 1]; a child has half the length
    np.testing.assert_allclose(sum(P[c].T @ (0.5 * mass) @ P[c] for c in (0, 1)), mass, atol=1e-12 * abs(mass).max())
    # the basis is invariant under x -> 1 - x with the functions in reverse order
    np.testing.assert_allclose(P[1], P[0][::-1, ::-1], atol=1e-12)
    # the parent's functions sum to one, and so do the children's
    np.testing.assert_allclose(P.sum(axis=2), 1.0, atol=1e-12)


@pytest.mark.parametrize("p,kind,cells", [(2, dg.HERMITE, (2, 1, 1)), (3, dg.GAUSS, (1, 2, 1)), (4, dg.GAUSS_LOBATTO, (1, 1, 2))])
def test_restriction_is_the_transpose_of_prolongation(p, kind, cells):
    o = ref.DGPlainOracle(p, kind, cells, SHEARED, 2)
    rng = np.random.default_rng(p)
    c, f = rng.standard_normal(o.level[0].shape), rng.standard_normal(o.level[1].shape)
    lhs, rhs = np.vdot(o.restrict(1, f), c), np.vdot(f, o.prolongate(1, c))
    assert abs(lhs - rhs) < 1e-13 * np.linalg.norm(f) * np.linalg.norm(c) * 8
    # the children of cell (i, j, k) are the cells 2 (i, j, k) + (kx, ky, kz): a swapped axis shows on the non-cubic box
    last = tuple(n - 1 for n in o.level[0].shape[:3])
    e = np.zeros(o.level[0].shape)
    e[last] = 1.0
    fine = o.prolongate(1, e)
    inside = np.zeros(o.level[1].shape, dtype=bool)
    inside[2 * last[0]:, 2 * last[1]:, 2 * last[2]:] = True
    assert abs(fine[inside]).min() > 0 and abs(fine[~inside]).max() == 0


def test_level_zero_follows_the_coarse_solver_rule():
    """level 0: range 1e-5 -> [min(0.9 lambda_max, lambda_min), lambda_max], Varga's degree, CG until 1e-10"""
    o = ref.DGPlainOracle(3, dg.HERMITE, (2, 1, 1), SHEARED, 3)
    i0 = o.info[0]
    assert i0["cg_its"] < int(np.prod(o.level[0].shape)) and 7 <= i0["degree"] <= 21
    assert i0["theta"] - i0["delta"] == pytest.approx(min(0.9 * i0["lambda_max"], i0["lambda_min"]), rel=1e-12)
    A = o.level[0].dense_matrix()
    # lambda_max / 1.2 and lambda_min are the extreme Ritz values of the preconditioned operator
    n = A.shape[0]
    Pinv = np.array([o.level[0].jacobi_vmult(col.reshape(o.level[0].shape)).ravel() for col in np.eye(n)]).T
    ev = np.sort(np.linalg.eigvals(Pinv @ A).real)
    # (Ritz values lie inside the spectrum; CG has run to a residual of 1e-10, so the extreme ones have converged)
    assert ev[0] * (1 - 1e-10) <= i0["lambda_min"] <= 1.01 * ev[0]
    assert 0.99 * ev[-1] <= i0["lambda_max"] / 1.2 <= ev[-1] * (1 + 1e-10)
    # ... so the Chebyshev iteration solves the level to about 1e-5
    b = np.random.default_rng(0).standard_normal(o.level[0].shape)
    x = o.v_cycle(b, 0)
    assert np.linalg.norm(b - o.level[0].vmult(x)) < 1e-3 * np.linalg.norm(b)
    assert [o.info[1]["degree"], o.info[2]["degree"]] == [3, 2] and o.info[1]["cg_its"] == 15


def test_v_cycle_is_symmetric_positive_definite():
    o = ref.DGPlainOracle(2, dg.HERMITE, (2, 1, 1), SHEARED, 2)
    shape = o.level[1].shape
    n = int(np.prod(shape))
    M = np.array([o.v_cycle(col.reshape(shape)).ravel() for col in np.eye(n)]).T
    assert abs(M - M.T).max() < 1e-10 * abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
    # M and A symmetric positive definite: the preconditioned operator has a real positive spectrum
    ev = np.linalg.eigvals(M @ o.level[1].dense_matrix())
    assert abs(ev.imag).max() < 1e-8 and ev.real.min() > 0


def test_residual_update_sums_are_consistent():
    o = ref.DGPlainOracle(2, dg.GAUSS, (1, 1, 1), SHEARED, 2)
    rng = np.random.default_rng(1)
    r, u = rng.standard_normal(o.level[1].shape), rng.standard_normal(o.level[1].shape)
    new, mg, sums = o.vmult_with_residual_update(r, u, 0.0)
    assert sums[0] == sums[1] == pytest.approx(np.vdot(o.v_cycle(r), r)) and new is not None
    new, mg, sums = o.vmult_with_residual_update(r, u, -0.37)
    np.testing.assert_allclose(new, r - 0.37 * u)
    np.testing.assert_allclose(mg, o.v_cycle(r - 0.37 * u))
    assert sums[0] - sums[1] == pytest.approx(np.vdot(mg, r))


def test_shim_mirrors_the_plain_dg_solver_and_compiles(tmp_path):
    """include/multigrid_shim.hpp: MultigridSolverDGPlain declares the reference's public members
    (multigrid_solver_dg_plain.h:303-445) and a translation unit that names them compiles"""
    import re
    src = open(os.path.join(ROOT, "include", "multigrid_shim.hpp")).read()
    body = src[src.index("  class MultigridSolverDGPlain"):]
    body = body[:body.index("\n  };")]
    need = {"solve_cg", "vmult", "vmult_with_residual_update", "do_matvec", "do_matvec_smoother"}
    assert need <= set(re.findall(r"\b([a-z_0-9]+)\(", body))
    tu = tmp_path / "shim_plain_check.cpp"
    tu.write_text("""
#include "multigrid_shim.hpp"
using namespace multigrid;
template <int p, typename Number, int type>
double drive(const Context &ctx)
{
  const int    cells[3] = {2, 1, 1};
  const double jac[9]   = {0.5, 0, 0, 0, 1, 0, 0, 0, 1};
  MultigridSolverDGPlain<3, p, Number, double, type> mg(ctx, cells, jac, 3, 3);
  Vector<double> rhs, sol, res, upd;
  mg.matrix_dg_dp.initialize_dof_vector(rhs);
  mg.matrix_dg_dp.initialize_dof_vector(sol);
  mg.matrix_dg_dp.initialize_dof_vector(res);
  mg.matrix_dg_dp.initialize_dof_vector(upd);
  const std::pair<unsigned int, double> its = mg.solve_cg(rhs, sol, 1e-9);
  mg.vmult(sol, rhs);
  const std::array<double, 2> sums = mg.vmult_with_residual_update(res, upd, -0.5);
  mg.do_matvec();
  mg.do_matvec_smoother();
  return its.second + sums[0] + sums[1] + mg.smoother_info(0).lambda_max + (double)mg.matrix.size();
}
template double drive<3, float, 0>(const Context &);
template double drive<4, double, 2>(const Context &);
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(tu)], check=True)
