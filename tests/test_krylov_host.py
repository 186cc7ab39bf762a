"""The host numerics every solver shares (multigrid_amd/csrc/mgx_krylov.hpp: the CG loop, SolverCG with its
ReductionControl, the Lanczos estimate with both rules for the Ritz values, the Chebyshev interval and factors) without a
device: tests/krylov_check.cpp runs them on plain loops over std::vector<double>, built with AddressSanitizer and UBSan
(no library is preloaded: the program has its own main), and this test compares what it prints with numpy.

The matrix of n points is A = tridiag(-1, d_i, -1) with d_i = 2 + (i mod 3), the preconditioner M = diag(d), the start
vector of an estimate (i mod 11) - mean.

The case n = 100 with 100 iterations allowed and the rule "dense up to 64 rows" stops after 29 steps -- the residual is
below 1e-10 there, as in the numpy restatement of the loop below --, so its Lanczos matrix has 29 rows and goes to the
dense solver; it is checked as the 5-iteration case is.  The route beyond 64 rows is taken by the same case on
tridiag(-1, 2, -1) ("laplace"): 100 rows, the dense solver is not called, same checks."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("krylov") / "krylov_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "krylov_check.cpp"), os.path.join(ROOT, "multigrid_amd", "csrc", "mgx_dg_host.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=300).stdout.decode()
    vals = {}
    for line in out.splitlines():
        case, key, *v = line.split()
        vals.setdefault(case, {})[key] = np.array([float(a) for a in v])
    assert vals["done"]["done"][0] == 1
    assert all(c["status"][0] == 0 for c in vals.values() if "status" in c)
    return vals


def matrix(n, laplace=False):
    d = np.full(n, 2.) if laplace else 2. + np.arange(n) % 3
    return np.diag(d) - np.eye(n, k=1) - np.eye(n, k=-1), d


def cg(A, d, r, max_its, keep_going):
    """the loop restated: (iterations, x, residual norms, Lanczos diagonal, off-diagonal)"""
    x, hist, diag, off = np.zeros(len(r)), [np.linalg.norm(r)], [], []
    rz = alpha = beta = 0.
    it, dirn = 0, None
    while it < max_its and keep_going(hist[-1], hist[0]):
        rz_old, z = rz, r / d
        rz = r @ z
        if it > 0:
            beta = rz / rz_old
        dirn = z if it == 0 else z + beta * dirn
        h = A @ dirn
        alpha_old, alpha = alpha, rz / (dirn @ h)
        x, r = x + alpha * dirn, r - alpha * h
        hist.append(np.linalg.norm(r))
        it += 1
        if it > 1:
            off.append(np.sqrt(beta) / alpha_old)
        diag.append(1. / alpha if it == 1 else 1. / alpha + beta / alpha_old)
    return it, x, np.array(hist), np.array(diag), np.array(off)


def start_vector(n):
    v = (np.arange(n) % 11).astype(float)
    return v - v.mean()


def extremes(diag, off):
    lam = np.linalg.eigvalsh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
    return lam[0], lam[-1]


def check_against_own_entries(c, iterations, tol=1e-12):
    """extremes of the printed Lanczos matrix; lambda_max carries the factor 1.2"""
    lo, hi, its = c["spectrum"]
    assert its == iterations and len(c["diag"]) == iterations and len(c["off"]) == iterations - 1
    wlo, whi = extremes(c["diag"], c["off"])
    assert lo == pytest.approx(wlo, rel=tol) and hi == pytest.approx(1.2 * whi, rel=tol)


def test_full_lanczos_run_gives_the_spectrum_of_the_preconditioned_matrix(printed):
    A, d = matrix(12)
    lam = np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d)))
    lo, hi, its = printed["lanczos-n12-full"]["spectrum"]
    assert its == 12
    assert lo == pytest.approx(lam[0], rel=1e-10) and hi / 1.2 == pytest.approx(lam[-1], rel=1e-10)


def test_five_iterations(printed):
    check_against_own_entries(printed["lanczos-n12-five"], 5)
    _, _, _, diag, off = cg(*matrix(12), start_vector(12), 5, lambda res, res0: res > 1e-10)
    np.testing.assert_allclose(printed["lanczos-n12-five"]["diag"], diag, rtol=1e-12)
    np.testing.assert_allclose(printed["lanczos-n12-five"]["off"], off, rtol=1e-12)


def test_empty_estimate(printed):
    assert list(printed["lanczos-n1"]["spectrum"]) == [1., 1., 0.]
    assert len(printed["lanczos-n1"]["diag"]) == 0


def test_dense_up_to_64_rows_and_bisection_beyond(printed):
    its = cg(*matrix(100), start_vector(100), 100, lambda res, res0: res > 1e-10)[0]
    assert its == 29
    short = printed["lanczos-n100-dense64"]
    check_against_own_entries(short, its)
    assert short["dense_calls"][0] == 1
    long = printed["lanczos-laplace-n100-dense64"]
    check_against_own_entries(long, 100)
    assert long["dense_calls"][0] == 0


def test_both_rules_agree_on_the_same_entries(printed):
    c = printed["lanczos-n40"]
    check_against_own_entries(c, 15)
    assert c["dense_calls"][0] == 1
    np.testing.assert_allclose(c["bisection"], c["dense"], rtol=1e-12)
    assert c["spectrum"][0] == c["dense"][0] and c["spectrum"][1] == 1.2 * c["dense"][1]


def test_breakdown_ends_the_estimate_with_the_rows_so_far(printed):
    c = printed["lanczos-n12-breakdown"]
    assert np.isfinite(c["spectrum"]).all()
    check_against_own_entries(c, 2)
    np.testing.assert_array_equal(c["diag"], printed["lanczos-n12-five"]["diag"][:2])


def test_solve(printed):
    A, d = matrix(12)
    above = lambda res, res0: res > 1e-16 and res > 1e-9 * res0  # noqa: E731
    its, x, hist, _, _ = cg(A, d, np.ones(12), 100, above)
    c = printed["solve-n12"]
    n_its, res0, res, still_above, rate = c["result"]
    assert its == 12 and n_its == 12
    assert c["true_residual"][0] <= 1e-12
    assert len(c["history"]) == 13 and c["history"][0] == res0 == np.sqrt(12.) and c["history"][-1] == res
    np.testing.assert_allclose(c["history"][:10], hist[:10], rtol=1e-9)
    assert not still_above and n_its < 100  # converged by either caller's rule
    assert rate == pytest.approx((res / res0) ** (1. / 12), rel=1e-12)


def test_solve_stopped_by_the_iteration_limit(printed):
    A, d = matrix(12)
    its, x, hist, _, _ = cg(A, d, np.ones(12), 3, lambda res, res0: res > 1e-16 and res > 1e-9 * res0)
    n_its, res0, res, still_above, _ = printed["solve-n12-three"]["result"]
    assert its == 3 and n_its == 3
    assert hist[-1] / hist[0] == pytest.approx(0.0531840562, abs=1e-10)
    assert res / res0 == pytest.approx(hist[-1] / hist[0], abs=1e-12)
    assert len(printed["solve-n12-three"]["history"]) == 4
    # not converged by either caller's rule: FE_Q "it >= max_iterations", DG "still above the tolerance"
    assert n_its >= 3 and still_above == 1


def test_breakdown_ends_a_solve_above_the_tolerance(printed):
    """the guards act in solve as well: two steps counted, and the result says that the stopping rule was not met"""
    n_its, res0, res, still_above, _ = printed["solve-n12-breakdown"]["result"]
    assert n_its == 2 and still_above == 1
    np.testing.assert_array_equal(printed["solve-n12-breakdown"]["history"], printed["solve-n12"]["history"][:3])


def test_chebyshev_first_kind_factors(printed):
    lambda_max, smoothing_range, degree = 2., 20., 5
    a = lambda_max / smoothing_range
    theta, delta = (lambda_max + a) / 2, (lambda_max - a) / 2
    np.testing.assert_allclose(printed["chebyshev-first"]["interval"], [a, theta, delta, degree], rtol=1e-15)
    want, rho, sigma = [1. / theta], delta / theta, theta / delta
    for _ in range(degree - 1):
        rho_next = 1. / (2. * sigma - rho)
        want += [rho_next * rho, 2. * rho_next / delta]
        rho = rho_next
    np.testing.assert_allclose(printed["chebyshev-first"]["factors"], want, rtol=1e-14)


def test_chebyshev_fourth_kind_factors(printed):
    lambda_max = 2.
    want = [4. / (3. * lambda_max)]
    for k in range(4):
        want += [(2 * k + 1) / (2 * k + 5), (8 * k + 12) / (lambda_max * (2 * k + 5))]
    np.testing.assert_allclose(printed["chebyshev-fourth"]["factors"], want, rtol=1e-15)


def test_varga_degree(printed):
    lambda_min, lambda_max, eps = 0.3, 1.9, 1e-3
    a = min(0.9 * lambda_max, lambda_min)
    sigma = (1. - np.sqrt(a / lambda_max)) / (1. + np.sqrt(a / lambda_max))
    degree = 1 + int(np.log(1. / eps + np.sqrt(1. / eps ** 2 - 1.)) / np.log(1. / sigma))
    got = printed["chebyshev-varga"]["interval"]
    assert got[3] == degree == 10
    np.testing.assert_allclose(got[:3], [a, (lambda_max + a) / 2, (lambda_max - a) / 2], rtol=1e-15)
