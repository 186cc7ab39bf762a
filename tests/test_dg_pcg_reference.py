"""The numpy restatement of the lumped-mass PCG (tests/dg_pcg_reference.py) on the CPU: the preconditioner table
against an integral it must equal, the merged recurrence against textbook PCG, its fp32 run against the fp64 one, and
the breakdown guard.  No GPU."""
import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_pcg_reference as pcg
import dg_reference_2d as ref2

KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])


def box_3d(kind):
    """2 x 2 x 2 cells, p = 3, the Jacobian of the harness mesh after 3 steps"""
    cells, jac = dg.cheby_mesh(3)
    assert cells == (2, 2, 2)
    return dg.DGOracle(3, kind, cells, jac), pcg.lumped_mass_inverse(3, kind, jac)


def box_2d(kind):
    """3 x 2 cells, p = 4, sheared"""
    return ref2.DGOracle2D(4, kind, (3, 2), SHEARED_2D), pcg.lumped_mass_inverse(4, kind, SHEARED_2D)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", range(1, 10))
def test_table_is_the_integral_of_the_basis_functions(p, kind):
    """the (p+1)-point rule integrates a polynomial of degree p exactly: the lumped mass of function i is its integral"""
    xq, wq = dg.gauss01(p + 4)
    exact = np.array([np.sum(wq * f(xq)) for f in dg.basis_1d(p, kind)])
    line = pcg.lumped_line(p, kind)
    assert np.allclose(line, exact, rtol=1e-12, atol=1e-15)
    assert (line > 0).all(), line.min()
    assert np.isclose(line.sum(), 1.0, rtol=1e-12)      # the functions sum to one
    for jac in (dg.cheby_mesh(5)[1], SHEARED_2D):
        dim = jac.shape[0]
        t = pcg.lumped_mass_inverse(p, kind, jac)
        assert t.shape == ((p + 1) ** dim,) and np.isfinite(t).all() and (t > 0).all()
        assert np.isclose((1.0 / t).sum(), abs(np.linalg.det(jac)), rtol=1e-12)   # the cell's volume
        # x fastest
        i = p  # last function along x, first along the others
        assert np.isclose(1.0 / t[i], abs(np.linalg.det(jac)) * line[p] * line[0] ** (dim - 1), rtol=1e-12)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("box", [box_3d, box_2d], ids=["3d", "2d"])
def test_merged_recurrence_equals_textbook_pcg(box, kind):
    o, m = box(kind)
    b = np.random.default_rng(3 + kind).random(o.shape)        # rhs in [0, 1), as solver_dg/program.cc:157-158
    x_ref, h_ref = pcg.textbook_pcg(o.vmult, m, b, 20)
    x, h, stalled = pcg.merged_pcg(o.vmult, m, b, 20)
    err = abs(x - x_ref).max() / abs(x_ref).max()
    print("merged vs textbook: x %.2e, history %.2e" % (err, abs(h / h_ref - 1).max()))
    assert stalled == -1
    assert err < 1e-12
    assert np.allclose(h, h_ref, rtol=1e-9)
    assert h[20] < h[0]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("box", [box_3d, box_2d], ids=["3d", "2d"])
def test_fp32_run_stays_close_to_fp64(box, kind):
    o, m = box(kind)
    b = np.random.default_rng(5 + kind).random(o.shape)
    x64, h64, _ = pcg.merged_pcg(o.vmult, m, b, 10)
    x32, h32, stalled = pcg.merged_pcg(o.vmult, m, b, 10, np.float32)
    err = abs(x32 - x64).max() / abs(x64).max()
    print("fp32 vs fp64 restatement: x %.2e, history %.2e" % (err, abs(h32 - h64).max() / h64.max()))
    assert stalled == -1 and x32.dtype == np.float32
    assert err < 5e-6
    assert abs(h32 - h64).max() / h64.max() < 5e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_guard_zero_right_hand_side(dtype):
    o, m = box_2d(dg.GAUSS)
    x, h, stalled = pcg.merged_pcg(o.vmult, m, np.zeros(o.shape), 5, dtype)
    assert stalled == 0 and not x.any() and not h.any()
    assert pcg.stop_iteration(h, 0.0, 1, stalled) == 0 and pcg.stop_iteration(h, 1e-6, 4, stalled) == 0


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_guard_more_iterations_than_unknowns(kind):
    """1 x 1 cell, p = 1: 4 unknowns, 12 iterations -- the residual reaches rounding level and the recurrence breaks down
    or goes on with numbers of that size; either way everything stays finite and x is the solution"""
    o = ref2.DGOracle2D(1, kind, (1, 1), SHEARED_2D)
    m = pcg.lumped_mass_inverse(1, kind, SHEARED_2D)
    b = np.random.default_rng(9).random(o.shape)
    x, h, stalled = pcg.merged_pcg(o.vmult, m, b, 12)
    assert np.isfinite(x).all() and np.isfinite(h).all()
    exact = np.linalg.solve(o.dense_matrix(), b.ravel()).reshape(o.shape)
    assert abs(x - exact).max() / abs(exact).max() < 1e-10
    assert -1 <= stalled < 12
    assert pcg.stop_iteration(h, 0.0, 1, stalled) <= 12


def test_stopping_rule():
    h = np.array([1.0, 0.25, 1e-2, 1e-4, 1e-6, 1e-8, 1e-10])
    assert pcg.stop_iteration(h, 1e-2, 1) == 3        # sqrt(1e-4) = 1e-2
    assert pcg.stop_iteration(h, 1e-2, 2) == 4        # rounded up to a multiple of 2
    assert pcg.stop_iteration(h, 1e-2, 4) == 4
    assert pcg.stop_iteration(h, 1e-2, 5) == 5
    assert pcg.stop_iteration(h, 1e-9, 1) == 6        # not met: all iterations
    assert pcg.stop_iteration(h, 0.0, 1) == 6
    assert pcg.stop_iteration(h, 1e-2, 4, stalled_at=2) == 2
