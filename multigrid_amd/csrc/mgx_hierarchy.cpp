// mgx_hierarchy.cpp -- the FE_Q hierarchy of mgx_cube_solver_create* and mgx_square_solver_create* (mgx_hierarchy.hpp).
// Pure host code; the device work is behind mgx.h.
#include "mgx_hierarchy.hpp"
#include "mgx_element.hpp"

#include <cstring>
#include <string>

int mgx::abandon_hierarchy(int status, mgx_cube_solver *out)
{
  const std::string keep = mgx_last_error(); // the destroy calls below must not hide the cause
  mgx_cube_solver_destroy(out);
  return mgx::report_error(status, keep.c_str());
}

int mgx::build_hierarchy(mgx_context_t ctx, int nl, int vnumber, int degree_pre, int n_cycles, const DescribeLevel &describe,
                         mgx_cube_solver *out)
{
  std::memset(out, 0, sizeof(*out));
  out->n_levels    = nl;
  out->matrix      = new mgx_operator_t[nl]();
  out->matrix_dp   = new mgx_operator_t[nl]();
  out->transfer    = new mgx_transfer_t[nl]();
  out->transfer_dp = new mgx_transfer_t[nl]();
  std::vector<mgx_transfer_desc> transfer(nl);
  std::vector<const double *>    rhs(nl), bcv(nl);
  std::vector<const uint32_t *>  bci(nl);
  std::vector<uint32_t>          bcn(nl);
  int                            status = MGX_OK;
  for (int l = 0; l < nl && status == MGX_OK; ++l)
    {
      LevelDesc d;
      status = describe(l, d);
      if (status != MGX_OK)
        break;
      transfer[l] = d.transfer;
      rhs[l] = d.rhs, bci[l] = d.bc_index, bcv[l] = d.bc_value, bcn[l] = d.bc_count;
      if (d.decomposed)
        {
          d.exchange.plan_id = 2 * l;
          d.op.exchange      = &d.exchange;
        }
      d.op.number = MGX_F64;
      status      = mgx_operator_create(ctx, &d.op, &out->matrix_dp[l]);
      if (status != MGX_OK)
        break;
      if (vnumber == MGX_F64)
        out->matrix[l] = out->matrix_dp[l];
      else
        {
          d.op.number        = MGX_F32;
          d.exchange.plan_id = 2 * l + 1;
          status             = mgx_operator_create(ctx, &d.op, &out->matrix[l]);
        }
      // (the entry points of the two dimensions differ in their refusals and in the number of metric entries they read)
      const bool two = d.op.dim == 2;
      if (d.geometry == LevelDesc::per_point && status == MGX_OK)
        {
          const auto enable = two ? mgx_operator_enable_coefficient_update_q_2d : mgx_operator_enable_coefficient_update_q;
          status            = enable(out->matrix_dp[l], d.unit_q, d.jxw_q);
        }
      if (d.geometry == LevelDesc::affine && status == MGX_OK)
        {
          const auto enable = two ? mgx_operator_enable_coefficient_update_2d : mgx_operator_enable_coefficient_update;
          status            = enable(out->matrix_dp[l], d.metric, d.det);
          if (status == MGX_OK && out->matrix[l] != out->matrix_dp[l])
            status = enable(out->matrix[l], d.metric, d.det);
        }
    }
  for (int l = 1; l < nl && status == MGX_OK; ++l)
    {
      status = mgx_transfer_create(out->matrix_dp[l - 1], out->matrix_dp[l], &transfer[l], &out->transfer_dp[l]);
      if (status != MGX_OK)
        break;
      if (vnumber == MGX_F64)
        out->transfer[l] = out->transfer_dp[l];
      else
        status = mgx_transfer_create(out->matrix[l - 1], out->matrix[l], &transfer[l], &out->transfer[l]);
    }
  if (status == MGX_OK)
    {
      mgx_solver_desc sd;
      sd.n_levels    = nl;
      sd.degree_pre  = degree_pre;
      sd.n_cycles    = n_cycles;
      sd.matrix      = out->matrix;
      sd.matrix_dp   = out->matrix_dp;
      sd.transfer    = out->transfer;
      sd.transfer_dp = out->transfer_dp;
      sd.rhs         = rhs.data();
      sd.bc_index    = bci.data();
      sd.bc_value    = bcv.data();
      sd.bc_count    = bcn.data();
      status         = mgx_solver_create(ctx, &sd, &out->solver);
    }
  return status == MGX_OK ? MGX_OK : abandon_hierarchy(status, out);
}

extern "C" int mgx_cube_solver_destroy(mgx_cube_solver *s)
{
  if (!s)
    return MGX_OK;
  mgx_solver_destroy(s->solver);
  // transfers reference their level operators: release them first
  for (int l = 0; l < s->n_levels; ++l)
    {
      if (s->transfer && s->transfer_dp && s->transfer_dp[l] != s->transfer[l])
        mgx_transfer_destroy(s->transfer_dp[l]);
      if (s->transfer)
        mgx_transfer_destroy(s->transfer[l]);
    }
  for (int l = 0; l < s->n_levels; ++l)
    {
      if (s->matrix && s->matrix_dp && s->matrix_dp[l] != s->matrix[l])
        mgx_operator_destroy(s->matrix_dp[l]);
      if (s->matrix)
        mgx_operator_destroy(s->matrix[l]);
    }
  delete[] s->matrix;
  delete[] s->matrix_dp;
  delete[] s->transfer;
  delete[] s->transfer_dp;
  std::memset(s, 0, sizeof(*s));
  return MGX_OK;
}
