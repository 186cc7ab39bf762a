// mgx_dg_host.cpp -- host numerics of the DG operator (mgx_dg_host.hpp) and the entry points of include/mgx_dg.h that
// need neither a context nor the device: the affine box of matvec_dg_cheby, neighbour and child tables of a box of
// cells.  Pure host code in fp64 (C++17): Gauss and Gauss-Lobatto points, the three element bases, the generalised
// eigenproblem behind JacobiTransformed, the embedding of a cell's space into those of its halves, geometry factors
// and the transformed diagonal.
//
// Reference behaviour (not code): common/laplace_operator_dg.h -- JacobiTransformed :2028-2256,
// LocalBasisTransformer :92-350.
#include "mgx_dg_host.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace mgx
{
  int report_error(int code, const char *message); // mgx_api.cpp: message for mgx_last_error()
}

using namespace mgx::dg;

namespace
{
  // ---- 1D data ----
  struct Poly1 // c * prod (x - r_k)
  {
    double              c = 1;
    std::vector<double> r;
    double val(double x) const
    {
      double v = c;
      for (double rk : r)
        v *= x - rk;
      return v;
    }
    double der(double x) const
    {
      double s = 0;
      for (size_t m = 0; m < r.size(); ++m)
        {
          double v = c;
          for (size_t k = 0; k < r.size(); ++k)
            if (k != m)
              v *= x - r[k];
          s += v;
        }
      return s;
    }
    void normalise(double x, double value) { c *= value / val(x); }
  };

  // roots of the Jacobi polynomial P^(al,al)_m mapped to [0,1]: eigenvalues of the Jacobi matrix
  std::vector<double> jacobi_roots01(int m, double al)
  {
    std::vector<double> out;
    if (m <= 0)
      return out;
    std::vector<double> J((size_t)m * m, 0.0), lam, V;
    for (int k = 1; k < m; ++k)
      {
        const double s = 2 * k + 2 * al;
        const double bk =
          2.0 / s * std::sqrt(k * (k + al) * (k + al) * (k + 2 * al) / ((s - 1) * (s + 1)));
        J[(k - 1) * m + k] = J[k * m + k - 1] = bk;
      }
    sym_eig(m, J, lam, V);
    for (double x : lam)
      out.push_back(0.5 * (x + 1));
    return out;
  }

  void gauss01(int n, std::vector<double> &x, std::vector<double> &w)
  {
    x = jacobi_roots01(n, 0.0);
    w.resize(n);
    for (int i = 0; i < n; ++i)
      {
        // Newton polish on the Legendre polynomial, weight 1 / ((1 - t^2) P_n'(t)^2) on [0,1]
        double t = 2 * x[i] - 1, dp = 0;
        for (int it = 0; it < 3; ++it)
          {
            double p0 = 1, p1 = t;
            for (int k = 2; k <= n; ++k)
              {
                const double pk = ((2 * k - 1) * t * p1 - (k - 1) * p0) / k;
                p0 = p1;
                p1 = pk;
              }
            if (n == 1)
              {
                p0 = 1;
                p1 = t;
              }
            dp = n * (t * p1 - p0) / (t * t - 1);
            if (it < 2)
              t -= p1 / dp;
          }
        x[i] = 0.5 * (t + 1);
        w[i] = 1.0 / ((1 - t * t) * dp * dp);
      }
  }

  std::vector<Poly1> lagrange(const std::vector<double> &nodes)
  {
    std::vector<Poly1> out(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i)
      {
        for (size_t k = 0; k < nodes.size(); ++k)
          if (k != i)
            out[i].r.push_back(nodes[k]);
        out[i].normalise(nodes[i], 1.0);
      }
    return out;
  }

  // FE_DGQHermite's 1D functions (deal.II Polynomials::HermiteLikeInterpolation, external, restated
  // from its documented construction): p_0 is the only function with a value at x = 0, p_0 and p_1
  // the only ones with a derivative there (mirror image at x = 1), p_0 is L2-orthogonal to p_1, the
  // inner functions are Lagrange polynomials in the roots of the Jacobi polynomial P^(4,4)_{p-3}
  // times x^2 (1-x)^2, and all functions sum to one (hence p_1'(0) = -p_0'(0), which
  // laplace_operator_dg.h:1190-1198 relies on).  Degree 1: hat functions, 2: Bernstein.
  std::vector<Poly1> hermite_like(int p)
  {
    std::vector<Poly1> out(p + 1);
    if (p == 0)
      return out;
    if (p == 1)
      {
        out[0].r = {1.0};
        out[0].c = -1;
        out[1].r = {0.0};
        return out;
      }
    if (p == 2)
      {
        out[0].r = {1.0, 1.0};
        out[1].r = {0.0, 1.0};
        out[1].c = -2;
        out[2].r = {0.0, 0.0};
        return out;
      }
    const std::vector<double> inner = jacobi_roots01(p - 3, 4.0);
    Poly1                     q0, q1;
    q0.r = {1.0, 1.0};
    q1.r = {0.0, 1.0, 1.0};
    for (double x : inner)
      {
        q0.r.push_back(x);
        q1.r.push_back(x);
      }
    std::vector<double> xq, wq;
    gauss01(p + 2, xq, wq); // exact to degree 2p + 3 >= deg(x q0 q1) = 2p
    double i0 = 0, i1 = 0;
    for (size_t k = 0; k < xq.size(); ++k)
      {
        i0 += wq[k] * q0.val(xq[k]) * q1.val(xq[k]);
        i1 += wq[k] * xq[k] * q0.val(xq[k]) * q1.val(xq[k]);
      }
    Poly1 p0 = q0;
    p0.r.push_back(i1 / i0);
    p0.normalise(0.0, 1.0);
    Poly1 p1 = q1;
    p1.c     = -p0.der(0.0) / q1.der(0.0);
    out[0]   = p0;
    out[1]   = p1;
    for (size_t j = 0; j < inner.size(); ++j)
      {
        Poly1 f;
        f.r = {0.0, 0.0, 1.0, 1.0};
        for (size_t k = 0; k < inner.size(); ++k)
          if (k != j)
            f.r.push_back(inner[k]);
        f.normalise(inner[j], 1.0);
        out[2 + j] = f;
      }
    auto mirror = [](const Poly1 &f) {
      Poly1 m;
      m.c = f.c * ((f.r.size() % 2) ? -1.0 : 1.0);
      for (double r : f.r)
        m.r.push_back(1.0 - r);
      return m;
    };
    out[p - 1] = mirror(p1);
    out[p]     = mirror(p0);
    return out;
  }

  // inverse of a dense n x n matrix (row-major), Gauss-Jordan with partial pivoting; false: singular
  bool invert(int n, std::vector<double> Bm, std::vector<double> &inv)
  {
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      inv[i * n + i] = 1;
    for (int col = 0; col < n; ++col)
      {
        int piv = col;
        for (int r = col + 1; r < n; ++r)
          if (std::abs(Bm[r * n + col]) > std::abs(Bm[piv * n + col]))
            piv = r;
        if (std::abs(Bm[piv * n + col]) < 1e-14)
          return false;
        for (int k = 0; k < n; ++k)
          {
            std::swap(Bm[piv * n + k], Bm[col * n + k]);
            std::swap(inv[piv * n + k], inv[col * n + k]);
          }
        const double dinv = 1.0 / Bm[col * n + col];
        for (int k = 0; k < n; ++k)
          {
            Bm[col * n + k] *= dinv;
            inv[col * n + k] *= dinv;
          }
        for (int r = 0; r < n; ++r)
          if (r != col)
            {
              const double f = Bm[r * n + col];
              for (int k = 0; k < n; ++k)
                {
                  Bm[r * n + k] -= f * Bm[col * n + k];
                  inv[r * n + k] -= f * inv[col * n + k];
                }
            }
      }
    return true;
  }

  // the p + 1 functions of the element basis MGX_DG_* on [0,1]; xq: the (p+1)-point Gauss rule (the nodes of
  // MGX_DG_GAUSS)
  std::vector<Poly1> element_basis(int p, int basis, const std::vector<double> &xq)
  {
    if (basis == MGX_DG_HERMITE)
      return hermite_like(p);
    if (basis == MGX_DG_GAUSS)
      return lagrange(xq);
    std::vector<double> nodes{0.0};
    for (double x : jacobi_roots01(p - 1, 1.0))
      nodes.push_back(x);
    nodes.push_back(1.0);
    return lagrange(nodes);
  }
} // namespace

namespace mgx::dg
{
  void sym_eig(int n, std::vector<double> A, std::vector<double> &lambda, std::vector<double> &V)
  {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      V[i * n + i] = 1;
    for (int sweep = 0; sweep < 100; ++sweep)
      {
        double off = 0, dia = 0;
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j)
            (i == j ? dia : off) += A[i * n + j] * A[i * n + j];
        if (off <= 1e-30 * dia)
          break;
        for (int p = 0; p < n - 1; ++p)
          for (int q = p + 1; q < n; ++q)
            {
              if (std::abs(A[p * n + q]) < 1e-300)
                continue;
              const double theta = (A[q * n + q] - A[p * n + p]) / (2 * A[p * n + q]);
              const double tt    = (theta >= 0 ? 1.0 : -1.0) / (std::abs(theta) + std::sqrt(theta * theta + 1));
              const double cs = 1 / std::sqrt(tt * tt + 1), sn = tt * cs;
              for (int k = 0; k < n; ++k)
                {
                  const double akp = A[k * n + p], akq = A[k * n + q];
                  A[k * n + p] = cs * akp - sn * akq;
                  A[k * n + q] = sn * akp + cs * akq;
                }
              for (int k = 0; k < n; ++k)
                {
                  const double apk = A[p * n + k], aqk = A[q * n + k];
                  A[p * n + k] = cs * apk - sn * aqk;
                  A[q * n + k] = sn * apk + cs * aqk;
                }
              for (int k = 0; k < n; ++k)
                {
                  const double vkp = V[k * n + p], vkq = V[k * n + q];
                  V[k * n + p] = cs * vkp - sn * vkq;
                  V[k * n + q] = sn * vkp + cs * vkq;
                }
            }
      }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int i, int j) { return A[i * n + i] < A[j * n + j]; });
    lambda.resize(n);
    std::vector<double> Vs((size_t)n * n);
    for (int e = 0; e < n; ++e)
      {
        lambda[e] = A[order[e] * n + order[e]];
        for (int k = 0; k < n; ++k)
          Vs[k * n + e] = V[k * n + order[e]];
      }
    V.swap(Vs);
  }

  int build_1d(int p, int basis, Host1D &h, std::string &why)
  {
    const int n = p + 1;
    h.n         = n;
    gauss01(n, h.xq, h.wq);
    const std::vector<Poly1> fe  = element_basis(p, basis, h.xq);
    const std::vector<Poly1> col = lagrange(h.xq);
    h.S.assign(n * n, 0);
    h.SD.assign(n * n, 0);
    h.D.assign(n * n, 0);
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i)
        {
          h.S[q * n + i]  = fe[i].val(h.xq[q]);
          h.SD[q * n + i] = fe[i].der(h.xq[q]);
          h.D[q * n + i]  = col[i].der(h.xq[q]);
        }
    for (int s = 0; s < 2; ++s)
      for (int i = 0; i < n; ++i)
        {
          h.b[s][i]  = col[i].val(s);
          h.g[s][i]  = col[i].der(s);
          h.fb[s][i] = fe[i].val(s);
          h.fg[s][i] = fe[i].der(s);
        }
    h.hderiv = fe[0].der(0.0);
    {
      // embedding of FE_Q(p) (nodal in the Gauss-Lobatto points g_q) into this basis on one cell:
      // sum_i d_i phi_i(g_q) = c_q, i.e. d = B^-1 c with B[q][i] = phi_i(g_q)
      // (LocalBasisTransformer type 1, laplace_operator_dg.h:103-135, applied at :1802, :1881)
      std::vector<double> nodes{0.0};
      for (double x : jacobi_roots01(n - 2, 1.0))
        nodes.push_back(x);
      nodes.push_back(1.0);
      if (n == 1)
        nodes = {0.5};
      std::vector<double> Bm(n * n);
      for (int q = 0; q < n; ++q)
        for (int i = 0; i < n; ++i)
          Bm[q * n + i] = fe[i].val(nodes[q]);
      if (!invert(n, Bm, h.P1))
        {
          why = "element basis is not unisolvent in the Gauss-Lobatto nodes";
          return MGX_ERR_UNSUPPORTED;
        }
    }
    {
      // embedding into the two halves of the cell: sum_i P_h[i][j] phi_i(x_q) = phi_j((x_q + h) / 2) in the Gauss
      // points x_q, i.e. P_h = S^-1 V_h (the spaces are nested: any unisolvent set of points gives the same matrix)
      std::vector<double> Sinv;
      if (!invert(n, h.S, Sinv))
        {
          why = "element basis is not unisolvent in the Gauss points";
          return MGX_ERR_UNSUPPORTED;
        }
      h.embed.assign(2 * n * n, 0.0);
      for (int half = 0; half < 2; ++half)
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j)
            {
              double v = 0;
              for (int q = 0; q < n; ++q)
                v += Sinv[i * n + q] * fe[j].val(0.5 * (h.xq[q] + half));
              h.embed[(half * n + i) * n + j] = v;
            }
    }

    // generalised eigenproblem lapl v = lambda mass v (laplace_operator_dg.h:179-215)
    std::vector<double> mass(n * n, 0), lapl(n * n, 0), cfirst(n * n, 0);
    const double        pen = double(n) * n;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        {
          double m = 0, l = 0, cf = 0;
          for (int q = 0; q < n; ++q)
            {
              m += h.wq[q] * h.S[q * n + i] * h.S[q * n + j];
              l += h.wq[q] * h.SD[q * n + i] * h.SD[q * n + j];
              cf += h.wq[q] * h.S[q * n + i] * h.SD[q * n + j];
            }
          mass[i * n + j]   = m;
          cfirst[i * n + j] = cf;
          l += h.fb[0][i] * h.fb[0][j] * pen + 0.5 * (h.fg[0][i] * h.fb[0][j] + h.fg[0][j] * h.fb[0][i]);
          l += h.fb[1][i] * h.fb[1][j] * pen - 0.5 * (h.fg[1][i] * h.fb[1][j] + h.fg[1][j] * h.fb[1][i]);
          lapl[i * n + j] = l;
        }
    // Cholesky mass = L L^T
    std::vector<double> L(n * n, 0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j)
        {
          double s = mass[i * n + j];
          for (int k = 0; k < j; ++k)
            s -= L[i * n + k] * L[j * n + k];
          if (i == j)
            {
              if (s <= 0)
                {
                  why = "1D mass matrix is not positive definite";
                  return MGX_ERR_UNSUPPORTED;
                }
              L[i * n + i] = std::sqrt(s);
            }
          else
            L[i * n + j] = s / L[j * n + j];
        }
    // C = L^-1 lapl L^-T
    auto solve_lower = [&](std::vector<double> &B) { // B <- L^-1 B (columns)
      for (int col_ = 0; col_ < n; ++col_)
        for (int i = 0; i < n; ++i)
          {
            double s = B[i * n + col_];
            for (int k = 0; k < i; ++k)
              s -= L[i * n + k] * B[k * n + col_];
            B[i * n + col_] = s / L[i * n + i];
          }
    };
    std::vector<double> Cm = lapl;
    solve_lower(Cm);
    std::vector<double> Ct(n * n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        Ct[i * n + j] = Cm[j * n + i];
    solve_lower(Ct);
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j)
        Ct[i * n + j] = Ct[j * n + i] = 0.5 * (Ct[i * n + j] + Ct[j * n + i]);
    std::vector<double> Q;
    sym_eig(n, Ct, h.lambda, Q);
    // E = L^-T Q
    h.E.assign(n * n, 0);
    for (int e = 0; e < n; ++e)
      for (int i = n - 1; i >= 0; --i)
        {
          double s = Q[i * n + e];
          for (int k = i + 1; k < n; ++k)
            s -= L[k * n + i] * h.E[k * n + e];
          h.E[i * n + e] = s / L[i * n + i];
        }
    // Eigenvectors even ones first, odd ones behind (each group by ascending eigenvalue): the cell kernel
    // applies E in even-odd form (mul_E).  The operator is invariant under x -> 1 - x, so every
    // eigenvector of a simple eigenvalue has a parity; a pair that does not (degenerate eigenvalues) keeps
    // the ascending order and the dense product.
    {
      std::vector<int> parity(n, 0);
      bool             pure = true;
      for (int e = 0; e < n; ++e)
        {
          double even = 0, odd = 0, nrm = 0;
          for (int i = 0; i < n; ++i)
            {
              even += std::fabs(h.E[i * n + e] - h.E[(n - 1 - i) * n + e]);
              odd += std::fabs(h.E[i * n + e] + h.E[(n - 1 - i) * n + e]);
              nrm += std::fabs(h.E[i * n + e]);
            }
          parity[e] = even <= 1e-9 * nrm ? 1 : (odd <= 1e-9 * nrm ? -1 : 0);
          pure      = pure && parity[e] != 0;
        }
      const int n_even = (int)std::count(parity.begin(), parity.end(), 1);
      h.e_parity = pure && n_even == n - n / 2;
      if (h.e_parity)
        {
          std::vector<int> order;
          for (int pass = 1; pass >= -1; pass -= 2)
            for (int e = 0; e < n; ++e)
              if (parity[e] == pass)
                order.push_back(e);
          std::vector<double> E2(n * n), l2(n);
          for (int k = 0; k < n; ++k)
            {
              l2[k] = h.lambda[order[k]];
              for (int i = 0; i < n; ++i)
                E2[i * n + k] = h.E[i * n + order[k]];
            }
          h.E.swap(E2);
          h.lambda.swap(l2);
        }
    }
    // 1D forms in the eigenvector basis
    h.lt.assign(n, 0);
    h.ct.assign(n, 0);
    for (int s = 0; s < 2; ++s)
      {
        h.beta[s].assign(n, 0);
        h.gamma[s].assign(n, 0);
      }
    for (int e = 0; e < n; ++e)
      {
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j)
            {
              double l = 0;
              for (int q = 0; q < n; ++q)
                l += h.wq[q] * h.SD[q * n + i] * h.SD[q * n + j];
              h.lt[e] += h.E[i * n + e] * l * h.E[j * n + e];
              h.ct[e] += h.E[i * n + e] * cfirst[i * n + j] * h.E[j * n + e];
            }
        for (int s = 0; s < 2; ++s)
          for (int i = 0; i < n; ++i)
            {
              h.beta[s][e] += h.E[i * n + e] * h.fb[s][i];
              h.gamma[s][e] += h.E[i * n + e] * h.fg[s][i];
            }
      }
    return MGX_OK;
  }

  int build_geometry(const double J[9], int p, Geometry &g, std::string &why)
  {
    const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) +
                       J[2] * (J[3] * J[7] - J[4] * J[6]);
    if (!(std::abs(det) > 0))
      {
        why = "singular cell Jacobian";
        return MGX_ERR_INVALID_ARGUMENT;
      }
    double inv[3][3]; // inv[a][i] = d xi_a / d x_i
    inv[0][0] = (J[4] * J[8] - J[5] * J[7]) / det;
    inv[0][1] = (J[2] * J[7] - J[1] * J[8]) / det;
    inv[0][2] = (J[1] * J[5] - J[2] * J[4]) / det;
    inv[1][0] = (J[5] * J[6] - J[3] * J[8]) / det;
    inv[1][1] = (J[0] * J[8] - J[2] * J[6]) / det;
    inv[1][2] = (J[2] * J[3] - J[0] * J[5]) / det;
    inv[2][0] = (J[3] * J[7] - J[4] * J[6]) / det;
    inv[2][1] = (J[1] * J[6] - J[0] * J[7]) / det;
    inv[2][2] = (J[0] * J[4] - J[1] * J[3]) / det;
    double G[3][3];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c)
        G[a][c] = inv[a][0] * inv[c][0] + inv[a][1] * inv[c][1] + inv[a][2] * inv[c][2];
    const double ad = std::abs(det);
    g.dim  = 3;
    g.K[0] = ad * G[0][0];
    g.K[1] = ad * G[1][1];
    g.K[2] = ad * G[2][2];
    g.K[3] = ad * G[0][1];
    g.K[4] = ad * G[0][2];
    g.K[5] = ad * G[1][2];
    for (int d = 0; d < 3; ++d)
      {
        const double nrm = std::sqrt(G[d][d]);
        for (int a = 0; a < 3; ++a)
          g.cn[d][a] = G[d][a] / nrm;
        g.fw[d]    = ad * nrm;
        g.sigma[d] = double(p + 1) * (p + 1) * std::abs(g.cn[d][d]); // penalty_factor = 1 (:47)
      }
    return MGX_OK;
  }

  int build_geometry_2d(const double J[4], int p, Geometry &g, std::string &why)
  {
    g = Geometry{};
    g.dim = 2;
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(J[i]))
        {
          why = "cell Jacobian with an entry that is not finite";
          return MGX_ERR_INVALID_ARGUMENT;
        }
    const double det = J[0] * J[3] - J[1] * J[2];
    if (!(det > 0) || !std::isfinite(det))
      {
        why = "cell Jacobian with a determinant that is not positive";
        return MGX_ERR_INVALID_ARGUMENT;
      }
    // inv[a][i] = d xi_a / d x_i
    const double inv[2][2] = {{J[3] / det, -J[1] / det}, {-J[2] / det, J[0] / det}};
    double       G[2][2];
    for (int a = 0; a < 2; ++a)
      for (int c = 0; c < 2; ++c)
        G[a][c] = inv[a][0] * inv[c][0] + inv[a][1] * inv[c][1];
    g.K[0] = det * G[0][0];
    g.K[1] = det * G[1][1];
    g.K[2] = det * G[0][1];
    for (int d = 0; d < 2; ++d)
      {
        const double nrm = std::sqrt(G[d][d]);
        for (int a = 0; a < 2; ++a)
          g.cn[d][a] = G[d][a] / nrm;
        g.fw[d]    = det * nrm;
        g.sigma[d] = double(p + 1) * (p + 1) * std::abs(g.cn[d][d]); // penalty_factor = 1 (:47)
      }
    return MGX_OK;
  }

  namespace
  {
    void transformed_diagonal_2d(const Host1D &h, const Geometry &g, const int *kind, std::vector<double> &diag)
    {
      const int n = h.n;
      diag.assign((size_t)n * n, 0.0);
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          {
            const int e[2] = {i, j};
            double    v    = g.K[0] * h.lt[i] + g.K[1] * h.lt[j] + 2 * g.K[2] * h.ct[i] * h.ct[j];
            for (int f = 0; f < 4; ++f)
              {
                const int    d = f / 2, s = f % 2;
                const double fbnd = kind[f] == kDirichlet ? 1.0 : (kind[f] == kNeumann ? 0.0 : 0.5);
                const double sgn  = s ? 1.0 : -1.0;
                const double be = h.beta[s][e[d]], ga = h.gamma[s][e[d]];
                const double vn = g.cn[d][d] * be * ga + g.cn[d][1 - d] * be * be * h.ct[e[1 - d]];
                v += g.fw[d] * (2 * fbnd * g.sigma[d] * be * be - 2 * fbnd * sgn * vn);
              }
            diag[j * n + i] = v;
          }
    }
  } // namespace

  void transformed_diagonal(const Host1D &h, const Geometry &g, const int *kind, std::vector<double> &diag)
  {
    if (g.dim == 2)
      return transformed_diagonal_2d(h, g, kind, diag);
    const int n = h.n;
    diag.assign((size_t)n * n * n, 0.0);
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          {
            const int e[3] = {i, j, k};
            double    v    = g.K[0] * h.lt[i] + g.K[1] * h.lt[j] + g.K[2] * h.lt[k] +
                       2 * (g.K[3] * h.ct[i] * h.ct[j] + g.K[4] * h.ct[i] * h.ct[k] + g.K[5] * h.ct[j] * h.ct[k]);
            for (int f = 0; f < 6; ++f)
              {
                const int    d = f / 2, s = f % 2;
                const double fbnd = kind[f] == kDirichlet ? 1.0 : (kind[f] == kNeumann ? 0.0 : 0.5);
                const double sgn  = s ? 1.0 : -1.0;
                const double be = h.beta[s][e[d]], ga = h.gamma[s][e[d]];
                double       vn = g.cn[d][d] * be * ga;
                for (int a = 0; a < 3; ++a)
                  if (a != d)
                    vn += g.cn[d][a] * be * be * h.ct[e[a]];
                v += g.fw[d] * (2 * fbnd * g.sigma[d] * be * be - 2 * fbnd * sgn * vn);
              }
            diag[(k * n + j) * n + i] = v;
          }
  }
} // namespace mgx::dg

extern "C" {

int mgx_dg_degree_embedding(int fine_degree, int coarse_degree, int basis, double *e1d)
{
  if (!e1d)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_degree_embedding: null argument");
  if (basis < MGX_DG_HERMITE || basis > MGX_DG_GAUSS)
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_degree_embedding: basis must be MGX_DG_HERMITE, _GAUSS_LOBATTO or _GAUSS");
  if (fine_degree < 1 || fine_degree > MGX_MAX_DEGREE || coarse_degree < 1 || coarse_degree > MGX_MAX_DEGREE)
    return mgx::report_error(MGX_ERR_UNSUPPORTED,
                             ("mgx_dg_degree_embedding: degrees must be in 1.." + std::to_string(MGX_MAX_DEGREE)).c_str());
  if (coarse_degree >= fine_degree)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, ("mgx_dg_degree_embedding: coarse degree " + std::to_string(coarse_degree) +
                                                        " must be below the fine degree " + std::to_string(fine_degree))
                                                         .c_str());
  // sum_i E[i][j] phi^f_i(x_q) = phi^c_j(x_q) in the Gauss points x_q of the fine space, i.e. E = S_f^-1 V (the spaces
  // are nested: any unisolvent set of points gives the same matrix)
  const int           nf = fine_degree + 1, nc = coarse_degree + 1;
  std::vector<double> xf, wf, xc, wc;
  gauss01(nf, xf, wf);
  gauss01(nc, xc, wc);
  const std::vector<Poly1> fine = element_basis(fine_degree, basis, xf), coarse = element_basis(coarse_degree, basis, xc);
  std::vector<double>      S((size_t)nf * nf), Sinv;
  for (int q = 0; q < nf; ++q)
    for (int i = 0; i < nf; ++i)
      S[q * nf + i] = fine[i].val(xf[q]);
  if (!invert(nf, S, Sinv))
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_degree_embedding: element basis is not unisolvent in the Gauss points");
  for (int i = 0; i < nf; ++i)
    for (int j = 0; j < nc; ++j)
      {
        double v = 0;
        for (int q = 0; q < nf; ++q)
          v += Sinv[i * nf + q] * coarse[j].val(xf[q]);
        e1d[i * nc + j] = v;
      }
  return MGX_OK;
}

int mgx_dg_cheby_mesh(int n_cell_steps, int cells[3], double jacobian[9])
{
  if (n_cell_steps < 0 || n_cell_steps > 30 || !cells || !jacobian)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_cheby_mesh: invalid argument");
  for (int d = 0; d < 3; ++d)
    {
      const double left = -1.0 + 0.05 * (d + 1), right = 0.95 - 0.06 * d;
      cells[d]          = (d < n_cell_steps % 3 ? 2 : 1) << (n_cell_steps / 3);
      const double h    = (right - left) / cells[d];
      for (int r = 0; r < 3; ++r)
        jacobian[r * 3 + d] = ((r == d ? 1.0 : 0.0) + 0.12 * (r + 1) * (d + 1)) * h;
    }
  return MGX_OK;
}

int mgx_dg_box_neighbours(const int cells[3], int ordering, int32_t *neighbours, int32_t *cell_ijk)
{
  if (!cells || !neighbours || cells[0] < 1 || cells[1] < 1 || cells[2] < 1)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_neighbours: invalid argument");
  const uint64_t n = (uint64_t)cells[0] * cells[1] * cells[2];
  if (n >= (1ull << 31))
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_box_neighbours: more than 2^31 cells");
  std::vector<uint32_t> order(n), position(n);
  std::iota(order.begin(), order.end(), 0u);
  auto ijk = [&](uint32_t lex, int out[3]) {
    out[0] = lex % cells[0];
    out[1] = (lex / cells[0]) % cells[1];
    out[2] = lex / ((uint64_t)cells[0] * cells[1]);
  };
  if (ordering == 1)
    {
      auto spread = [](uint64_t v) { // bits of v to every third position
        uint64_t r = 0;
        for (int bit = 0; bit < 21; ++bit)
          r |= ((v >> bit) & 1ull) << (3 * bit);
        return r;
      };
      std::vector<uint64_t> key(n);
      for (uint32_t c = 0; c < n; ++c)
        {
          int p[3];
          ijk(c, p);
          key[c] = spread(p[0]) | (spread(p[1]) << 1) | (spread(p[2]) << 2);
        }
      std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    }
  for (uint32_t c = 0; c < n; ++c)
    position[order[c]] = c;
  for (uint32_t c = 0; c < n; ++c)
    {
      int p[3];
      ijk(order[c], p);
      if (cell_ijk)
        for (int d = 0; d < 3; ++d)
          cell_ijk[(size_t)c * 3 + d] = p[d];
      const uint64_t stride[3] = {1, (uint64_t)cells[0], (uint64_t)cells[0] * cells[1]};
      for (int d = 0; d < 3; ++d)
        {
          neighbours[(size_t)c * 6 + 2 * d] = p[d] > 0 ? (int32_t)position[order[c] - stride[d]] : MGX_DG_BOUNDARY;
          neighbours[(size_t)c * 6 + 2 * d + 1] =
            p[d] + 1 < cells[d] ? (int32_t)position[order[c] + stride[d]] : MGX_DG_BOUNDARY;
        }
    }
  return MGX_OK;
}

int mgx_dg_box_children(const int coarse_cells[3], int coarse_ordering, int fine_ordering, uint32_t *children)
{
  if (!coarse_cells || !children || coarse_cells[0] < 1 || coarse_cells[1] < 1 || coarse_cells[2] < 1)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_children: invalid argument");
  const uint64_t nc = (uint64_t)coarse_cells[0] * coarse_cells[1] * coarse_cells[2];
  if (8 * nc >= (1ull << 31))
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_box_children: more than 2^31 fine cells");
  const int fine_cells[3] = {2 * coarse_cells[0], 2 * coarse_cells[1], 2 * coarse_cells[2]};
  std::vector<int32_t> nb(6 * (size_t)8 * nc), cijk(3 * (size_t)nc), fijk(3 * (size_t)8 * nc);
  if (const int status = mgx_dg_box_neighbours(coarse_cells, coarse_ordering, nb.data(), cijk.data()); status != MGX_OK)
    return status;
  if (const int status = mgx_dg_box_neighbours(fine_cells, fine_ordering, nb.data(), fijk.data()); status != MGX_OK)
    return status;
  std::vector<uint32_t> at(8 * (size_t)nc); // lexicographic position of a fine cell -> its number
  for (uint32_t f = 0; f < 8 * nc; ++f)
    at[fijk[3 * (size_t)f] + (size_t)fine_cells[0] * (fijk[3 * (size_t)f + 1] + (size_t)fine_cells[1] * fijk[3 * (size_t)f + 2])] = f;
  for (uint32_t c = 0; c < nc; ++c)
    for (int k = 0; k < 8; ++k)
      {
        const size_t x = 2 * (size_t)cijk[3 * (size_t)c] + (k & 1), y = 2 * (size_t)cijk[3 * (size_t)c + 1] + ((k >> 1) & 1),
                     z = 2 * (size_t)cijk[3 * (size_t)c + 2] + (k >> 2);
        children[8 * (size_t)c + k] = at[x + fine_cells[0] * (y + fine_cells[1] * z)];
      }
  return MGX_OK;
}

namespace
{
  // numbering of a box of two dimensions: order[c] = lexicographic position of cell c (x fastest)
  std::vector<uint32_t> box_order_2d(const int cells[2], int ordering)
  {
    const uint64_t        n = (uint64_t)cells[0] * cells[1];
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (ordering == 1)
      {
        auto spread = [](uint64_t v) { // bits of v to every second position
          uint64_t r = 0;
          for (int bit = 0; bit < 31; ++bit)
            r |= ((v >> bit) & 1ull) << (2 * bit);
          return r;
        };
        std::vector<uint64_t> key(n);
        for (uint32_t c = 0; c < n; ++c)
          key[c] = spread(c % cells[0]) | (spread(c / cells[0]) << 1);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
      }
    return order;
  }
} // namespace

int mgx_dg_box_neighbours_2d(const int cells[2], int ordering, int32_t *neighbours, int32_t *cell_ij)
{
  if (!cells || !neighbours || cells[0] < 1 || cells[1] < 1)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_neighbours_2d: invalid argument");
  const uint64_t n = (uint64_t)cells[0] * cells[1];
  if (n >= (1ull << 31))
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_box_neighbours_2d: more than 2^31 cells");
  const std::vector<uint32_t> order = box_order_2d(cells, ordering);
  std::vector<uint32_t>       position(n);
  for (uint32_t c = 0; c < n; ++c)
    position[order[c]] = c;
  const uint64_t stride[2] = {1, (uint64_t)cells[0]};
  for (uint32_t c = 0; c < n; ++c)
    {
      const int p[2] = {(int)(order[c] % cells[0]), (int)(order[c] / cells[0])};
      for (int d = 0; d < 2; ++d)
        {
          if (cell_ij)
            cell_ij[(size_t)c * 2 + d] = p[d];
          neighbours[(size_t)c * 4 + 2 * d] = p[d] > 0 ? (int32_t)position[order[c] - stride[d]] : MGX_DG_BOUNDARY;
          neighbours[(size_t)c * 4 + 2 * d + 1] =
            p[d] + 1 < cells[d] ? (int32_t)position[order[c] + stride[d]] : MGX_DG_BOUNDARY;
        }
    }
  return MGX_OK;
}

int mgx_dg_box_set_sides(int dim, const int *cells, uint32_t n_cells, const int32_t *cell_pos, const int *side_kind,
                         int32_t *neighbours)
{
  if ((dim != 2 && dim != 3) || !cells || !cell_pos || !side_kind || !neighbours)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_set_sides: dim must be 2 or 3 and no argument null");
  for (int d = 0; d < dim; ++d)
    if (cells[d] < 1)
      return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_set_sides: cells must be positive");
  for (int f = 0; f < 2 * dim; ++f)
    if (side_kind[f] != MGX_DG_BOUNDARY && side_kind[f] != MGX_DG_NEUMANN)
      return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_set_sides: a side is MGX_DG_BOUNDARY or MGX_DG_NEUMANN");
  // checked before anything is written: a table that does not belong to these positions stays as it is
  for (int pass = 0; pass < 2; ++pass)
    for (uint32_t c = 0; c < n_cells; ++c)
      for (int d = 0; d < dim; ++d)
        {
          const int32_t p = cell_pos[(size_t)c * dim + d];
          if (pass == 0 && (p < 0 || p >= cells[d]))
            return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_set_sides: cell position outside the box");
          for (int s = 0; s < 2; ++s)
            {
              int32_t   &entry   = neighbours[((size_t)c * dim + d) * 2 + s];
              const bool at_side = s == 0 ? p == 0 : p + 1 == cells[d];
              if (pass == 0 && at_side != (entry < 0))
                return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_set_sides: the neighbour table has a boundary entry "
                                                                   "inside the box or a cell behind one of its sides");
              if (pass == 1 && at_side)
                entry = side_kind[2 * d + s];
            }
        }
  return MGX_OK;
}

int mgx_dg_box_children_2d(const int coarse_cells[2], int coarse_ordering, int fine_ordering, uint32_t *children)
{
  if (!coarse_cells || !children || coarse_cells[0] < 1 || coarse_cells[1] < 1)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_box_children_2d: invalid argument");
  const uint64_t nc = (uint64_t)coarse_cells[0] * coarse_cells[1];
  if (4 * nc >= (1ull << 31))
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_dg_box_children_2d: more than 2^31 fine cells");
  const int                   fine_cells[2] = {2 * coarse_cells[0], 2 * coarse_cells[1]};
  const std::vector<uint32_t> corder = box_order_2d(coarse_cells, coarse_ordering), forder = box_order_2d(fine_cells, fine_ordering);
  std::vector<uint32_t>       at(4 * (size_t)nc); // lexicographic position of a fine cell -> its number
  for (uint32_t f = 0; f < 4 * nc; ++f)
    at[forder[f]] = f;
  for (uint32_t c = 0; c < nc; ++c)
    for (int k = 0; k < 4; ++k)
      {
        const size_t x = 2 * (size_t)(corder[c] % coarse_cells[0]) + (k & 1), y = 2 * (size_t)(corder[c] / coarse_cells[0]) + (k >> 1);
        children[4 * (size_t)c + k] = at[x + fine_cells[0] * y];
      }
  return MGX_OK;
}

} // extern "C"
