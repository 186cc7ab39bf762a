// mgx_element.hpp -- host only: what the mesh providers (mgx_cube.cpp, mgx_square.cpp) share.  The 1D element data of
// FE_Q(p) are defined once, in mgx_cube.cpp: these tables feed every kernel, and one definition built by one compiler
// with one set of flags keeps them the same bits in both dimensions.
#pragma once
#include "../../include/mgx.h"

#include <cstdint>
#include <vector>

namespace mgx
{
  int report_error(int code, const char *message); // mgx_api.cpp: message for mgx_last_error()

  // ---- 1D element data: FE_Q(p) on Gauss-Lobatto nodes, QGauss(p+1) ----
  struct Basis
  {
    static constexpr int kMaxN = MGX_MAX_DEGREE + 1;
    int    p = 0, n = 0;
    double gll[kMaxN], gq[kMaxN], gw[kMaxN];
    double S[kMaxN * kMaxN], D[kMaxN * kMaxN], P1[2 * kMaxN * kMaxN];
  };

  using ld = long double;
  void legendre(int n, ld x, ld &P, ld &dP);
  ld   lagrange_value(const std::vector<ld> &x, int i, ld t);
  ld   lagrange_derivative(const std::vector<ld> &x, int i, ld t);
  void make_basis(Basis &b, int p);

  // the seeded vector of a level: entry i is a splitmix64 hash of (seed, grid id of DoF i) mapped to [-1, 1), so that it
  // is the same function of the grid whatever the numbering of the DoFs
  inline void seeded_fill(uint64_t seed, const uint32_t *dof_grid, uint32_t n, double *out)
  {
#pragma omp parallel for schedule(static)
    for (uint32_t i = 0; i < n; ++i)
      {
        uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)dof_grid[i] + 1);
        z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out[i] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
      }
  }
} // namespace mgx
