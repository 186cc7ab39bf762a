// mgx_krylov.hpp -- the host numerics every solver shares, without the device: the CG loop, SolverCG
// and estimate_eigenvalues built from it, the Chebyshev interval and factors.
// The device work of a CG step is the caller's: an `ops` object with four members, each returning a status of mgx.h,
//   precondition_dot(&rz)    z = M^-1 r and r.z
//   direction(beta, first)   d = z (first) or d = z + beta d
//   vmult_dot(&dh)           h = A d and d.h
//   update(alpha, &res)      x += alpha d where there is an x, r -= alpha h and |r|
// Read by mgx_api.cpp (FE_Q) and mgx_dg_api.cpp (DG); tests/krylov_check.cpp runs it on std::vector.
#pragma once

#include "../../include/mgx.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mgx::krylov
{
  inline bool positive_finite(double v) { return v > 0. && std::isfinite(v); }

  // The loop: while keep_going() and fewer than max_iterations steps are done.  A step whose r.z or d.A d is not a
  // positive finite number ends the iteration and is not counted (fp32 on a level that CG has solved to rounding).
  // Every finished step goes to after_step(number of the step = 1, 2, ..., alpha, alpha_old, beta, |r| after it).
  template <typename Ops, typename KeepGoing, typename AfterStep>
  int cg_iterate(Ops &ops, unsigned max_iterations, KeepGoing keep_going, AfterStep after_step)
  {
    double rz = 0, rz_old = 0, dh = 0, res = 0, alpha = 0, alpha_old = 0, beta = 0;
    int    status = MGX_OK;
    for (unsigned it = 0; it < max_iterations && keep_going();)
      {
        rz_old = rz;
        if ((status = ops.precondition_dot(&rz)) != MGX_OK || !positive_finite(rz))
          break;
        if (it > 0)
          beta = rz / rz_old;
        if ((status = ops.direction(beta, it == 0)) != MGX_OK || (status = ops.vmult_dot(&dh)) != MGX_OK || !positive_finite(dh))
          break;
        alpha_old = alpha;
        alpha     = rz / dh;
        if ((status = ops.update(alpha, &res)) != MGX_OK)
          break;
        after_step((int)++it, alpha, alpha_old, beta, res);
      }
    return status;
  }

  // SolverCG with ReductionControl(max_iterations, abs_tol, reduction)
  struct SolveResult
  {
    unsigned iterations = 0;
    double   res0 = 0, res = 0;
    bool     above_tolerance = false; // the stopping rule still asks for a step
    double   reduction_rate() const { return iterations ? std::pow(res / res0, 1.0 / iterations) : 1.0; }
  };

  // from a residual of norm res0; history receives res0 and |r| after every step, iterations and reduction_rate what
  // their names say (each may be null).  Whether the outcome is a failure is the caller's rule: iterations against
  // max_iterations, or above_tolerance.
  template <typename Ops>
  int solve(Ops &ops, double res0, unsigned max_iterations, double abs_tol, double reduction, std::vector<double> *history,
            SolveResult &out, unsigned *iterations = nullptr, double *reduction_rate = nullptr)
  {
    out = SolveResult{0, res0, res0, false};
    if (history)
      history->assign(1, res0);
    const auto above  = [&] { return out.res > abs_tol && out.res > reduction * out.res0; };
    const int  status = cg_iterate(ops, max_iterations, above, [&](int iteration, double, double, double, double res) {
      out.iterations = (unsigned)iteration;
      out.res        = res;
      if (history)
        history->push_back(res);
    });
    out.above_tolerance = above();
    if (iterations)
      *iterations = out.iterations;
    if (reduction_rate)
      *reduction_rate = out.reduction_rate(); // multigrid_solver.h:491-492
    return status;
  }

  // estimate_eigenvalues: number of eigenvalues below x of the symmetric tridiagonal matrix d[n], e[n - 1] (Sturm sequence)
  inline int sturm_count(int n, const double *d, const double *e, double x)
  {
    int    count = 0;
    double q     = d[0] - x;
    if (q < 0)
      ++count;
    for (int i = 1; i < n; ++i)
      {
        if (q == 0)
          q = 1e-300;
        q = d[i] - x - e[i - 1] * e[i - 1] / q;
        if (q < 0)
          ++count;
      }
    return count;
  }

  // its smallest and largest eigenvalue by bisection
  inline void tridiag_extreme(int n, const double *d, const double *e, double &lo, double &hi)
  {
    double gl = d[0], gu = d[0];
    for (int i = 0; i < n; ++i)
      {
        const double r = (i > 0 ? std::fabs(e[i - 1]) : 0) + (i < n - 1 ? std::fabs(e[i]) : 0);
        gl             = std::min(gl, d[i] - r);
        gu             = std::max(gu, d[i] + r);
      }
    for (int which = 0; which < 2; ++which)
      {
        const int k = which == 0 ? 1 : n;
        double    a = gl, b = gu;
        for (int it = 0; it < 200; ++it)
          {
            const double m = 0.5 * (a + b);
            if (m == a || m == b)
              break;
            if (sturm_count(n, d, e, m) >= k)
              b = m;
            else
              a = m;
          }
        (which == 0 ? lo : hi) = 0.5 * (a + b);
      }
  }

  // the Lanczos matrix of a CG run: diag[m], off[m - 1]
  struct Tridiagonal
  {
    std::vector<double> diag, off;
  };

  // The rule for its extreme eigenvalues (the two routes differ in the last bits, and recorded results pin both).
  // FE_Q (no sym_eig): bisection always.  DG: the dense symmetric solver (sym_eig of mgx_dg_host.cpp: eigenvalues
  // ascending) up to 64 rows -- its Jacobi sweeps cost m^3 each --, bisection beyond
  struct RitzRule
  {
    void (*sym_eig)(int n, std::vector<double> A, std::vector<double> &lambda, std::vector<double> &V) = nullptr;
    void operator()(const Tridiagonal &T, double &lo, double &hi) const
    {
      const int m = (int)T.diag.size();
      if (!sym_eig || m > 64)
        return tridiag_extreme(m, T.diag.data(), T.off.data(), lo, hi);
      std::vector<double> Tm((size_t)m * m, 0.0), lam, V;
      for (int i = 0; i < m; ++i)
        {
          Tm[i * m + i] = T.diag[i];
          if (i + 1 < m)
            Tm[i * m + i + 1] = Tm[(i + 1) * m + i] = T.off[i];
        }
      sym_eig(m, Tm, lam, V);
      lo = lam.front();
      hi = lam.back();
    }
  };

  // CG from a residual of norm res0, stopped at 1e-10 (IterationNumberControl(max_iterations, 1e-10)), as a Lanczos
  // process, into info.cg_iterations, lambda_min and lambda_max = 1.2 x the largest Ritz value; 1, 1 without a step.
  // entries (may be null) receives the Lanczos matrix.
  template <typename Ops>
  int lanczos_estimate(Ops &ops, double res0, int max_iterations, RitzRule ritz_rule, mgx_smoother_info &info,
                       Tridiagonal *entries = nullptr)
  {
    Tridiagonal local, &T = entries ? *entries : local;
    T                  = Tridiagonal{};
    double    res      = res0;
    const int status   = cg_iterate(
      ops, (unsigned)std::max(0, max_iterations), [&] { return res > 1e-10; },
      [&](int iteration, double alpha, double alpha_old, double beta, double res_now) {
        if (iteration > 1)
          T.off.push_back(std::sqrt(beta) / alpha_old);
        T.diag.push_back(iteration == 1 ? 1. / alpha : 1. / alpha + beta / alpha_old);
        res = res_now;
      });
    info.cg_iterations = (int)T.diag.size();
    info.lambda_min = info.lambda_max = 1.;
    if (status == MGX_OK && !T.diag.empty())
      {
        ritz_rule(T, info.lambda_min, info.lambda_max);
        info.lambda_max = 1.2 * info.lambda_max; // the largest Ritz value with its safety factor
      }
    return status;
  }

  // PreconditionChebyshev: theta, delta and (degree < 0: numbers::invalid_unsigned_int) the degree of info from its
  // lambda_min / lambda_max.  smoothing_range > 1: [lambda_max / range, lambda_max]; otherwise [min(0.9 lambda_max,
  // lambda_min), lambda_max] and Varga's estimate of the degree that reduces the error by it.  Returns the lower end.
  inline double chebyshev_interval(double smoothing_range, int degree, mgx_smoother_info &info)
  {
    const double a =
      smoothing_range > 1. ? info.lambda_max / smoothing_range : std::min(0.9 * info.lambda_max, info.lambda_min);
    if (degree < 0)
      {
        const double actual_range = info.lambda_max / a;
        const double sigma        = (1. - std::sqrt(1. / actual_range)) / (1. + std::sqrt(1. / actual_range));
        const double eps          = smoothing_range;
        degree = 1 + (int)(std::log(1. / eps + std::sqrt(1. / eps / eps - 1.)) / std::log(1. / sigma));
      }
    info.degree = degree;
    info.delta  = (info.lambda_max - a) * 0.5;
    info.theta  = (info.lambda_max + a) * 0.5;
    return a;
  }

  // factor of the first step, and factor1 / factor2 of iteration k = 0, 1, ... of the recurrence (in this order: the
  // first kind carries rho_k along).  fourth_kind (multigrid_solver.h:951-952): delta is lambda_max
  struct ChebyshevFactors
  {
    double theta, delta, rhok;
    bool   fourth_kind;
    explicit ChebyshevFactors(const mgx_smoother_info &info, bool fourth_kind = false)
      : theta(info.theta), delta(info.delta), rhok(info.delta / info.theta), fourth_kind(fourth_kind)
    {}
    double first() const { return fourth_kind ? 4. / (3. * delta) : 1. / theta; }
    void   next(int k, double &f1, double &f2)
    {
      if (fourth_kind)
        {
          f1 = (2. * k + 1.) / (2. * k + 5.);
          f2 = (8. * k + 12.) / (delta * (2. * k + 5.));
          return;
        }
      const double sigma = theta / delta, rhokp = 1. / (2. * sigma - rhok);
      f1   = rhokp * rhok;
      f2   = 2. * rhokp / delta;
      rhok = rhokp;
    }
  };
} // namespace mgx::krylov
