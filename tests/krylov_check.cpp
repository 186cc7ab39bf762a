// The host numerics of multigrid_amd/csrc/mgx_krylov.hpp on plain loops over std::vector<double>, without a device:
// tests/test_krylov_host.py builds this program under AddressSanitizer and UBSan together with mgx_dg_host.cpp (for
// sym_eig), runs it and compares the printed values with numpy.  Every line is "<case> <key> <values ...>".
// The matrix of n points: A = tridiag(-1, d_i, -1) with d_i = 2 + (i mod 3), preconditioner M = diag(d); the cases named
// "laplace" take d_i = 2.
#include "../multigrid_amd/csrc/mgx_dg_host.hpp"
#include "../multigrid_amd/csrc/mgx_krylov.hpp"

#include <cstdio>
#include <string>
#include <vector>

// what mgx_dg_host.cpp asks of the library around it (the library records the message for mgx_last_error)
namespace mgx
{
  int report_error(int code, const char *) { return code; }
} // namespace mgx

namespace kr = mgx::krylov;
using Vec    = std::vector<double>;

static double dot(const Vec &a, const Vec &b)
{
  double s = 0;
  for (size_t i = 0; i < a.size(); ++i)
    s += a[i] * b[i];
  return s;
}

struct VectorOps
{
  int n;
  Vec dg, x, r, z, d, h;
  int zero_dh_at = 0, vmults = 0; // vmult_dot number zero_dh_at reports d.A d = 0
  VectorOps(int n, bool laplace, const Vec &r0)
    : n(n)
    , dg(n)
    , x(n, 0.)
    , r(r0)
    , z(n)
    , d(n)
    , h(n)
  {
    for (int i = 0; i < n; ++i)
      dg[i] = laplace ? 2. : 2. + (i % 3);
  }
  void apply(Vec &out, const Vec &in) const
  {
    for (int i = 0; i < n; ++i)
      out[i] = dg[i] * in[i] - (i > 0 ? in[i - 1] : 0.) - (i + 1 < n ? in[i + 1] : 0.);
  }
  int precondition_dot(double *rz)
  {
    for (int i = 0; i < n; ++i)
      z[i] = r[i] / dg[i];
    *rz = dot(r, z);
    return MGX_OK;
  }
  int direction(double beta, bool first)
  {
    for (int i = 0; i < n; ++i)
      d[i] = first ? z[i] : z[i] + beta * d[i];
    return MGX_OK;
  }
  int vmult_dot(double *dh)
  {
    apply(h, d);
    *dh = ++vmults == zero_dh_at ? 0. : dot(d, h);
    return MGX_OK;
  }
  int update(double alpha, double *res)
  {
    for (int i = 0; i < n; ++i)
      {
        x[i] += alpha * d[i];
        r[i] -= alpha * h[i];
      }
    *res = std::sqrt(dot(r, r));
    return MGX_OK;
  }
};

static void print(const std::string &name, const char *key, const Vec &v)
{
  std::printf("%s %s", name.c_str(), key);
  for (double a : v)
    std::printf(" %.17g", a);
  std::printf("\n");
}

static int dense_calls = 0;
static void counted_sym_eig(int n, Vec A, Vec &lambda, Vec &V)
{
  ++dense_calls;
  mgx::dg::sym_eig(n, A, lambda, V);
}

// v_i = (i mod 11) - mean
static Vec start_vector(int n)
{
  Vec    v(n);
  double mean = 0;
  for (int i = 0; i < n; ++i)
    mean += i % 11;
  mean /= n;
  for (int i = 0; i < n; ++i)
    v[i] = i % 11 - mean;
  return v;
}

// one estimate; dense: the rule "dense up to 64 rows", else bisection.  Prints the spectrum (lambda_max with its factor
// 1.2), the Lanczos matrix and how often the dense solver ran
static kr::Tridiagonal estimate(const std::string &name, int n, int max_its, bool dense, bool laplace = false, int zero_dh_at = 0)
{
  const Vec r0 = start_vector(n);
  VectorOps ops(n, laplace, r0);
  ops.zero_dh_at = zero_dh_at;
  mgx_smoother_info I{};
  kr::Tridiagonal   T;
  dense_calls = 0;
  const int status =
    kr::lanczos_estimate(ops, std::sqrt(dot(r0, r0)), max_its, dense ? kr::RitzRule{counted_sym_eig} : kr::RitzRule{}, I, &T);
  print(name, "status", {(double)status});
  print(name, "spectrum", {I.lambda_min, I.lambda_max, (double)I.cg_iterations});
  print(name, "diag", T.diag);
  print(name, "off", T.off);
  print(name, "dense_calls", {(double)dense_calls});
  return T;
}

static void solve(const std::string &name, int n, unsigned max_its, int zero_dh_at = 0)
{
  const Vec b(n, 1.);
  VectorOps ops(n, false, b);
  ops.zero_dh_at = zero_dh_at;
  Vec       history;
  kr::SolveResult R;
  const int status = kr::solve(ops, std::sqrt(dot(b, b)), max_its, 1e-16, 1e-9, &history, R);
  Vec Ax(n);
  ops.apply(Ax, ops.x);
  for (int i = 0; i < n; ++i)
    Ax[i] -= b[i];
  print(name, "status", {(double)status});
  print(name, "result", {(double)R.iterations, R.res0, R.res, R.above_tolerance ? 1. : 0., R.reduction_rate()});
  print(name, "true_residual", {std::sqrt(dot(Ax, Ax))});
  print(name, "history", history);
}

int main()
{
  estimate("lanczos-n12-full", 12, 12, false);
  estimate("lanczos-n12-five", 12, 5, false);
  estimate("lanczos-n1", 1, 5, false);
  estimate("lanczos-n100-dense64", 100, 100, true);
  estimate("lanczos-laplace-n100-dense64", 100, 100, true, true);
  {
    // both rules on the same entries
    const kr::Tridiagonal T = estimate("lanczos-n40", 40, 15, true);
    double lo = 0, hi = 0;
    kr::RitzRule{}(T, lo, hi);
    print("lanczos-n40", "bisection", {lo, hi});
    kr::RitzRule{counted_sym_eig}(T, lo, hi);
    print("lanczos-n40", "dense", {lo, hi});
  }
  estimate("lanczos-n12-breakdown", 12, 12, false, false, 3);
  solve("solve-n12", 12, 100);
  solve("solve-n12-three", 12, 3);
  solve("solve-n12-breakdown", 12, 100, 3);
  {
    mgx_smoother_info I{};
    I.lambda_min = 0.1;
    I.lambda_max = 2.;
    const double a = kr::chebyshev_interval(20., 5, I);
    print("chebyshev-first", "interval", {a, I.theta, I.delta, (double)I.degree});
    kr::ChebyshevFactors F(I);
    Vec                  f{F.first()};
    for (int k = 0; k < I.degree - 1; ++k)
      {
        double f1, f2;
        F.next(k, f1, f2);
        f.push_back(f1);
        f.push_back(f2);
      }
    print("chebyshev-first", "factors", f);
    I.delta = I.lambda_max; // mgx_smoother_set_polynomial_type
    kr::ChebyshevFactors F4(I, true);
    f.assign(1, F4.first());
    for (int k = 0; k < 4; ++k)
      {
        double f1, f2;
        F4.next(k, f1, f2);
        f.push_back(f1);
        f.push_back(f2);
      }
    print("chebyshev-fourth", "factors", f);
    I.lambda_min = 0.3;
    I.lambda_max = 1.9;
    const double a0 = kr::chebyshev_interval(1e-3, -1, I);
    print("chebyshev-varga", "interval", {a0, I.theta, I.delta, (double)I.degree});
  }
  std::printf("done done 1\n");
  return 0;
}
