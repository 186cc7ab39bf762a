// Runs the problem description of the two-dimensional provider (include/mgx_square.h: mgx_square_problem, the four
// mgx_square_problem_* accessors, the host side of mgx_square_solver_create_problem) on the box, the sheared box, the
// annulus sector and the disc, into arrays of exactly the documented sizes, and prints lines "<key> <numbers>" for
// tests/test_poisson_mapped_reference_2d.py.  Built from the provider's host sources with AddressSanitizer and UBSan; no
// device, no library: the few entry points of the device layer the sources refer to are stand-ins below, and the
// stand-in of the hierarchy builder asks for every level's description (the tensor, the boundary values) and stops.
//
// Arguments: the degree.  Output per geometry g in {box, sheared, sector, ball} and problem k in {cube, shell}:
//   "<g> <k> <level> <sum coef_q> <sum rhs_quadrature> <sum solution_q> <sum bc_value>" for every level (sum: of v[i] (1 + i mod 7)),
// then "refused <n>" (the refusals that came back as MGX_ERR_INVALID_ARGUMENT), "described <n>" (level descriptions the
// builder's stand-in received) and "done 1".
#include "../include/mgx_square.h"
#include "../multigrid_amd/csrc/mgx_hierarchy.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// ---- stand-ins of the device layer ----
static std::string last_error;
static int         described = 0;
namespace mgx
{
  int report_error(int code, const char *message)
  {
    last_error = message ? message : "";
    return code;
  }
  int build_hierarchy(mgx_context_t, int n_levels, int, int, int, const DescribeLevel &describe, mgx_cube_solver *)
  {
    for (int l = 0; l < n_levels; ++l)
      {
        LevelDesc d;
        if (const int status = describe(l, d); status != MGX_OK)
          return status;
        // what the builder would read: the tensor of every point, the boundary lists
        double s = 0;
        for (size_t i = 0; i < (size_t)d.op.n_cells * 3 * (d.op.degree + 1) * (d.op.degree + 1); ++i)
          s += d.op.coef_q[i];
        for (uint32_t i = 0; i < d.bc_count; ++i)
          s += d.bc_value[i] + d.bc_index[i];
        if (!(s == s) || d.rhs != nullptr)
          return report_error(MGX_ERR_INVALID_ARGUMENT, "stand-in: bad level description");
        ++described;
      }
    return report_error(MGX_ERR_UNSUPPORTED, "stand-in: no device");
  }
  int abandon_hierarchy(int status, mgx_cube_solver *) { return status; }
} // namespace mgx
extern "C" {
const char *mgx_last_error(void) { return last_error.c_str(); }
int         mgx_malloc(mgx_context_t, void **, size_t) { return MGX_ERR_UNSUPPORTED; }
int         mgx_free(mgx_context_t, void *) { return MGX_ERR_UNSUPPORTED; }
int         mgx_upload(mgx_context_t, void *, const void *, size_t) { return MGX_ERR_UNSUPPORTED; }
int         mgx_sync(mgx_context_t) { return MGX_ERR_UNSUPPORTED; }
int         mgx_solver_compute_rhs(mgx_solver_t, int, const double *) { return MGX_ERR_UNSUPPORTED; }
int         mgx_solver_compute_rhs_2d(mgx_solver_t, int, const double *) { return MGX_ERR_UNSUPPORTED; }
}

// sum of v[i] (1 + i mod 7): entries that cancel in the plain sum (u is odd on these meshes) do not cancel here
static double sum(const std::vector<double> &v)
{
  double s = 0;
  for (size_t i = 0; i < v.size(); ++i)
    s += v[i] * (double)(1 + i % 7);
  return s;
}

int main(int argc, char **argv)
{
  if (argc != 2)
    return 2;
  const int    p  = std::atoi(argv[1]);
  const size_t n2 = (size_t)(p + 1) * (p + 1);
  const double shear[4] = {1.0, 0.35, 0.15, 0.8};
  int          refused = 0;
  for (int g = 0; g < 4; ++g)
    {
      static const char  *names[4] = {"box", "sheared", "sector", "ball"};
      mgx_square_t        sq       = nullptr;
      mgx_square_box_desc bd;
      bd.degree   = p;
      bd.n_refine = 1;
      bd.roots[0] = g == 2 ? 2 : 3;
      bd.roots[1] = g == 2 ? 3 : 2;
      bd.origin   = -0.9;
      bd.h0       = 1.9 / 3;
      bd.jacobian = g == 1 ? shear : nullptr;
      const int status = g == 3   ? mgx_square_create_ball(p, 2, &sq)
                         : g == 2 ? mgx_square_create_mapped(&bd, MGX_SQUARE_GEOMETRY_ANNULUS_SECTOR, &sq)
                                  : mgx_square_create_box(&bd, &sq);
      if (status != MGX_OK)
        return 3;
      for (int k = 0; k < 2; ++k)
        {
          const mgx_square_problem problem = {k == 0 ? MGX_SQUARE_PROBLEM_CUBE : MGX_SQUARE_PROBLEM_SHELL, 1.0e6};
          for (int l = 0; l < mgx_square_n_levels(sq); ++l)
            {
              const size_t        nc = mgx_square_n_cells(sq, l);
              std::vector<double> coef(nc * 3 * n2), rhs(nc * n2), sol(nc * n2), bc(mgx_square_n_constrained(sq, l));
              if (mgx_square_problem_coef_q(sq, l, &problem, coef.data()) != MGX_OK ||
                  mgx_square_problem_rhs_quadrature(sq, l, &problem, rhs.data()) != MGX_OK ||
                  mgx_square_problem_solution_q(sq, l, &problem, sol.data()) != MGX_OK ||
                  mgx_square_problem_bc_value(sq, l, &problem, bc.data()) != MGX_OK)
                return 4;
              std::printf("%s %s %d %.17g %.17g %.17g %.17g\n", names[g], k == 0 ? "cube" : "shell", l, sum(coef), sum(rhs), sum(sol),
                          sum(bc));
            }
          // the host side of the solver: every level described, then the stand-in's refusal, nothing left behind
          mgx_cube_solver out;
          if (mgx_square_solver_create_problem((mgx_context_t)&described, sq, MGX_F64, 3, 1, &problem, &out) != MGX_ERR_UNSUPPORTED)
            return 5;
        }
      // refusals: no problem, an unknown kind, a negative contrast, a level that does not exist
      std::vector<double>      out((size_t)mgx_square_n_cells(sq, 0) * 3 * n2);
      const mgx_square_problem unknown = {7, 0.}, negative = {MGX_SQUARE_PROBLEM_SHELL, -1.}, fine = {MGX_SQUARE_PROBLEM_CUBE, 0.};
      mgx_cube_solver          solver;
      refused += mgx_square_problem_coef_q(sq, 0, nullptr, out.data()) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_problem_rhs_quadrature(sq, 0, &unknown, out.data()) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_problem_solution_q(sq, 0, &negative, out.data()) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_problem_bc_value(sq, 99, &fine, out.data()) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_problem_bc_value(sq, 0, &fine, nullptr) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_solver_create_problem((mgx_context_t)&described, sq, MGX_F64, 3, 1, nullptr, &solver) == MGX_ERR_INVALID_ARGUMENT;
      refused += mgx_square_solver_create_problem((mgx_context_t)&described, sq, MGX_F64, 3, 1, &unknown, &solver) == MGX_ERR_INVALID_ARGUMENT;
      mgx_square_destroy(sq);
    }
  std::printf("refused %d\ndescribed %d\ndone 1\n", refused, described);
  return 0;
}
