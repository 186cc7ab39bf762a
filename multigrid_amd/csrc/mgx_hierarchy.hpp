// mgx_hierarchy.hpp -- host only: one builder of the FE_Q hierarchy (mgx_cube_solver) for the cube and the square.  A
// provider describes its levels one at a time; the builder owns the handle arrays, the rule which precisions share an
// operator, the geometry for coefficient updates, the two transfer chains, mgx_solver_desc and the failure path.
#pragma once
#include "../../include/mgx_cube.h"

#include <functional>
#include <vector>

namespace mgx
{
  // What a level looks like.  The object lives until the operators of its level exist: `scratch` and the exchange lists
  // are the place for what is built for that level only (a replicated unit-law tensor, the neighbour arrays).  What
  // `transfer`, rhs and bc_* point to has to live until the builder returns.
  struct LevelDesc
  {
    mgx_operator_desc op;          // the fp64 operator, coef_q as chosen by the provider; op.exchange is the builder's
    bool              decomposed = false; // `exchange` is filled: plan ids 2 level (fp64 operator), 2 level + 1 (V-cycle)
    mgx_exchange_desc exchange;
    const uint32_t   *neighbor_index[27];
    int               neighbor_rank[27];
    uint32_t          neighbor_count[27];
    // geometry for coefficient updates: none, affine (metric, det: on the operators of both precisions) or per point
    // (unit_q, jxw_q: kept once, in fp64 with matrix_dp; mgx_solver_update_coefficient writes the tensor of an fp32
    // V-cycle operator from it)
    enum { no_geometry, affine, per_point } geometry = no_geometry;
    double              metric[6] = {0, 0, 0, 0, 0, 0}, det = 0;
    const double       *unit_q = nullptr, *jxw_q = nullptr;
    mgx_transfer_desc   transfer;  // level > 0
    const double       *rhs = nullptr, *bc_value = nullptr;
    const uint32_t     *bc_index = nullptr;
    uint32_t            bc_count = 0;
    std::vector<double> scratch;
  };

  // fills the description of level `level`; a status other than MGX_OK (reported by the callee) ends the build
  using DescribeLevel = std::function<int(int level, LevelDesc &)>;

  int build_hierarchy(mgx_context_t ctx, int n_levels, int vnumber, int degree_pre, int n_cycles, const DescribeLevel &describe,
                      mgx_cube_solver *out);

  // the failure path: destroys what exists of *out and reports `status` with the error text of the failed call
  int abandon_hierarchy(int status, mgx_cube_solver *out);
} // namespace mgx
