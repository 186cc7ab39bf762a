// mgx_api.cpp -- implementation of the C ABI declared in include/mgx.h: host-side control flow of
// LaplaceOperator / PreconditionChebyshev / MGTransferMatrixFree / MultigridSolver on top of the
// HIP kernels.  Reference citations (file:line) are relative to the reference root; deal.II
// semantics follow SURVEY.md 8a rows R, S, T and Appendix D.
#include "../../include/mgx.h"
#include "mgx_bricks.hpp"
#include "mgx_device_memory.hpp"
#include "mgx_index_tables.hpp"
#include "mgx_internal.hpp"
#include "mgx_krylov.hpp"
#include "mgx_transfer_tables.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types only: the library is bound at run time (dlopen), single-GPU users need no RCCL

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace mgx;

namespace
{
  thread_local std::string g_last_error;

  int fail(int code, const std::string &msg)
  {
    g_last_error = msg;
    return code;
  }

  inline size_t number_size(int number) { return number == MGX_F64 ? 8 : 4; }

  // MGX_TRACE=1 prints the host-side control flow to stderr (debugging aid); set by the first
  // context created with it
  bool g_trace = false;
  bool trace_on() { return g_trace; }
#define MGX_TRACE(...)                  \
  do                                    \
    {                                   \
      if (trace_on())                   \
        {                               \
          std::fprintf(stderr, "[mgx] " __VA_ARGS__); \
          std::fputc('\n', stderr);     \
          std::fflush(stderr);          \
        }                               \
    }                                   \
  while (0)
} // namespace

int mgx::report_error(int code, const char *message) { return fail(code, message ? message : ""); }

// The environment carries the thresholds a deployment may want to tune, nothing else: no variable
// changes what is computed or selects a diagnostic / cross-check code path.  Those are options of
// a context, set explicitly with mgx_context_set_option (tests, A/B timings, tools).
#ifndef MGX_CELLS_FORM
#define MGX_CELLS_FORM 0
#endif
extern "C" int mgx_has_cells_form(void) { return MGX_CELLS_FORM; }
extern "C" int64_t mgx_live_device_allocations(void) { return mgx::live_device_allocations().load(); }

mgx::Tunables mgx::Tunables::from_environment()
{
  Tunables t;
  auto     num = [](const char *name, uint32_t dflt) {
    const char *e = std::getenv(name);
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : dflt;
  };
  t.trace               = std::getenv("MGX_TRACE") != nullptr;
  t.brick_min           = num("MGX_BRICK_MIN", t.brick_min);
  t.brick_min_from_env  = std::getenv("MGX_BRICK_MIN") != nullptr;
  t.overlap_min         = num("MGX_OVERLAP_MIN_BRICKS", t.overlap_min);
  t.restrict_colour_min = num("MGX_RESTRICT_COLOUR_MIN", t.restrict_colour_min);
  t.cell_colour_min     = num("MGX_CELL_COLOUR_MIN", t.cell_colour_min);
  t.free_max_bricks     = num("MGX_FREE_MAX_BRICKS", t.free_max_bricks);
  t.free_one_max        = num("MGX_FREE_ONE_MAX", t.free_one_max);
  t.graph_max_dofs      = num("MGX_GRAPH_MAX_DOFS", t.graph_max_dofs);
  return t;
}

bool mgx::Tunables::set(const std::string &name, double value)
{
  const bool     on = value != 0.;
  const uint32_t u  = value <= 0. ? 0u : (value >= 4294967295. ? 0xFFFFFFFFu : (uint32_t)value);
  struct Entry
  {
    const char *name;
    bool       *flag;
    uint32_t   *number;
  };
  const Entry table[] = {
    {"trace", &trace, nullptr},
    {"brick_min", nullptr, &brick_min},
    {"overlap_min_bricks", nullptr, &overlap_min},
    {"restrict_colour_min", nullptr, &restrict_colour_min},
    {"cell_colour_min", nullptr, &cell_colour_min},
    {"free_max_bricks", nullptr, &free_max_bricks},
    {"free_one_max", nullptr, &free_one_max},
    {"graph_max_dofs", nullptr, &graph_max_dofs},
    // code-path selectors (numerically equivalent paths; tests compare them)
    {"general_kernel", &general_kernel, nullptr},
    {"no_bricks", &no_bricks, nullptr},
#if MGX_CELLS_FORM // cross-check builds only (make crosscheck)
    {"cells_form", &cells_form, nullptr},
    {"brick_wide_max", nullptr, &wide_max},
#endif
    {"macro_wg_per_cu_x16", nullptr, &macro_wg_x16},
    {"no_diag_table", &no_diag_table, nullptr},
    {"no_macro_v2", &no_macro_v2, nullptr},
    {"no_general_bricks", &no_general_bricks, nullptr},
    {"general_brick_min", nullptr, &general_brick_min},
    {"fused_prolong_min_bricks", nullptr, &fused_prolong_min_bricks},
    {"roctx", &roctx, nullptr},
    {"no_fused_init", &no_fused_init, nullptr},
    {"no_fused_restrict", &no_fused_restrict, nullptr},
    {"no_fused_prolong", &no_fused_prolong, nullptr},
    {"force_fused_transfers", &force_fused_transfers, nullptr},
    {"transfer_v1", &transfer_v1, nullptr},
    {"restrict_atomic", &restrict_atomic, nullptr},
    {"exchange_unfused", &exchange_unfused, nullptr},
    {"no_graph", &no_graph, nullptr},
    {"dg_no_overlap", &dg_no_overlap, nullptr},
    {"dg_unmerged_restrict", &dg_unmerged_restrict, nullptr},
    {"no_fused_decomposed", &no_fused_decomposed, nullptr},
    {"no_fused_assembly", &no_fused_assembly, nullptr},
    {"no_fused_residual", &no_fused_residual, nullptr},
    {"no_restrict_scratch", &no_restrict_scratch, nullptr},
    // emulation of a rank of a decomposed mesh on one GPU (tools/rank_emulation.py): the results are WRONG
    {"rccl_selftest", &rccl_selftest, nullptr},
  };
  for (const Entry &e : table)
    if (name == e.name)
      {
        if (e.flag)
          *e.flag = on;
        else
          *e.number = u;
        if (name == "brick_min")
          brick_min_from_env = true; // taken as given (no p <= 2 doubling)
        return true;
      }
  return false;
}

struct ExchangePlan
{
  std::vector<uint32_t> not_owned_host; // DoFs a lower rank holds as well (host copy of not_owned_dev)
  int                    plan_id = 0, number = MGX_F64, self_pos = 0;
  std::vector<int>       rank;
  std::vector<uint32_t>  count;
  std::vector<uint32_t *> index_dev;
  std::vector<void *>    send, recv;
  uint32_t              *shared_dev = nullptr, *not_owned_dev = nullptr;
  uint32_t               n_shared = 0, n_not_owned = 0;
  void                  *own_buf = nullptr;
  // fused form: one pack launch over the concatenated lists, one ordered unpack launch over the
  // interface DoFs (CSR of their contributions in ascending rank order, 255 = the rank's own sum)
  std::vector<uint32_t>  start;              // [n_neighbors + 1] offsets into the concatenation
  uint32_t              *all_index_dev = nullptr, *csr_start_dev = nullptr, *csr_pos_dev = nullptr;
  uint8_t               *all_seg_dev = nullptr, *csr_k_dev = nullptr;
  bool                   fused = false;
};

// RCCL entry points, bound lazily.  The process may already hold an RCCL (torch bundles one): that
// instance is reused so that only one RCCL runtime is active.
struct RcclApi
{
  void *lib = nullptr;
  decltype(&ncclGetUniqueId)    GetUniqueId    = nullptr;
  decltype(&ncclCommInitRank)   CommInitRank   = nullptr;
  decltype(&ncclCommDestroy)    CommDestroy    = nullptr;
  decltype(&ncclGroupStart)     GroupStart     = nullptr;
  decltype(&ncclGroupEnd)       GroupEnd       = nullptr;
  decltype(&ncclSend)           Send           = nullptr;
  decltype(&ncclRecv)           Recv           = nullptr;
  decltype(&ncclAllReduce)      AllReduce      = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  bool load()
  {
    if (lib)
      return true;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names)
      if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD)))
        break;
    if (!lib)
      for (const char *n : names)
        if ((lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL)))
          break;
    if (!lib)
      return false;
#define MGX_RCCL_SYM(name)                                        \
  name = reinterpret_cast<decltype(name)>(dlsym(lib, "nccl" #name)); \
  if (!name)                                                      \
    {                                                             \
      lib = nullptr;                                              \
      return false;                                               \
    }
    MGX_RCCL_SYM(GetUniqueId)
    MGX_RCCL_SYM(CommInitRank)
    MGX_RCCL_SYM(CommDestroy)
    MGX_RCCL_SYM(GroupStart)
    MGX_RCCL_SYM(GroupEnd)
    MGX_RCCL_SYM(Send)
    MGX_RCCL_SYM(Recv)
    MGX_RCCL_SYM(AllReduce)
    MGX_RCCL_SYM(GetErrorString)
#undef MGX_RCCL_SYM
    return true;
  }
};
static RcclApi &rccl_api()
{
  static RcclApi api;
  return api;
}

struct mgx_context_s
{
  int         device = 0;
  Tunables    tun; // environment switches, read once in mgx_context_create
  DeviceArena mem{"mgx_context"}; // partial_dev, result_dev, ar_dev
  hipStream_t stream = nullptr;
  bool        borrowed_stream = false; // the stream of the context of the decomposed hierarchy above (agglomerated levels)
  // interface exchange overlapped with the interior bricks: side stream and the two events that
  // order it against `stream` (created with the communicator)
  hipStream_t side     = nullptr;
  hipEvent_t  ev_iface = nullptr, ev_side = nullptr;
  double     *partial_dev = nullptr; // kDotBlocks block partials
  double     *result_dev  = nullptr; // 4 scalars
  double     *result_host = nullptr; // pinned
  // cell-loop launch profiling (mgx_profile_*)
  bool                                        profile = false;
  struct Bracket
  {
    hipEvent_t start, stop;
    int        form, launches;
  };
  std::vector<Bracket> ev_pool, ev_used;
  // domain decomposition
  bool                                      has_comm = false;
  mgx_comm_desc                             comm{};
  // native transport: RCCL send/recv and allreduce on `stream`, no host synchronisation
  ncclComm_t                                nccl = nullptr;
  bool                                      use_rccl = false;
  int                                       rccl_rank = 0, rccl_size = 1;
  double                                   *ar_dev = nullptr; // allreduce scratch (8 doubles)
  std::vector<std::pair<size_t, struct ExchangePlan *>> plans; // (vector length, plan) for dot products
};

struct mgx_operator_s
{
  mgx_context_t ctx = nullptr;
  DeviceArena   mem{"mgx_operator"}; // every device buffer of the operator and of its exchange plan
  OperatorData  d;
  double        S[kMaxN * kMaxN], D[kMaxN * kMaxN], w[kMaxN];
  bool          has_diag = false;
  bool          profiled = false;
  uint32_t     *global_index_dev = nullptr; // optional numbering-independent index (smoother start vector)
  double        start_sum = 0, start_count = 0; // sum of (index mod 11) and number of the owned DoFs
  std::unique_ptr<ExchangePlan> plan;       // interface exchange of a decomposed mesh
  // fused PCG (mgx_vmult_with_cg_update): partial sums, their result, carrier of the brick loop
  double  *cg_partials = nullptr, *cg_result = nullptr;
  void    *cg_carrier  = nullptr;
  bool     constrained_last = false; // the constrained DoFs are exactly [n_dofs - n_constrained, n_dofs)
  // solution-dependent coefficient (mgx_operator_enable_coefficient_update): affine geometry of the level,
  // M = J^-1 J^-T [xx,yy,zz,xy,xz,yz] and det J
  bool     coef_update  = false;
  double   metric[6]    = {0, 0, 0, 0, 0, 0};
  double   det_jacobian = 0;
  // ... or (mgx_operator_enable_coefficient_update_q) the per-point geometry of curved cells in the operator's number
  // type: unit_q [n_cells][6][n^3] = JxW_q J^-1 J^-T, jxw_q [n_cells][n^3] = JxW_q; nullptr: affine geometry
  void    *unit_q = nullptr, *jxw_q = nullptr;
};

struct mgx_smoother_s
{
  mgx_operator_t    op = nullptr;
  DeviceArena       mem{"mgx_smoother"};
  mgx_smoother_info info{};
  void             *x_old = nullptr, *tmp = nullptr;
  void             *x_old2 = nullptr; // third iterate buffer (odd number of fused iterations in step())
  // AdditionalData::PolynomialType::fourth_kind (multigrid_solver.h:951-952): info.delta = lambda_max
  bool              fourth_kind = false;
  double            range_a     = 0; // lower end of the smoothing range (first-kind delta / theta)
  // the arguments of mgx_smoother_create, for mgx_solver_update_coefficient which re-creates the smoother with them
  double            req_range  = 0;
  int               req_degree = 0, req_eig_its = 0;
  // factor of the first step, and factor1 / factor2 of iteration k = 0, 1, ... of the recurrence
  krylov::ChebyshevFactors factors() const { return krylov::ChebyshevFactors(info, fourth_kind); }
};

struct mgx_transfer_s
{
  mgx_operator_t coarse = nullptr, fine = nullptr;
  DeviceArena    mem{"mgx_transfer"};
  TransferData   d;
  void          *scratch = nullptr; // decomposed mesh: coarse-level scratch of restrict_and_add
  // mgx_interpolate_to_coarse (built at its first call): 1D interpolation matrix [(2p+1)(p+1)] in the number type and
  // the coarse cells' entity ownership (bit e: first cell in cell order that contains entity e)
  void          *interp_1d  = nullptr;
  uint32_t      *own_coarse = nullptr;
};

struct mgx_solver_s
{
  mgx_context_t               ctx = nullptr;
  DeviceArena                 mem{"mgx_solver"};
  int                         n_levels = 0, degree = 0, n_cycles = 1, vnumber = MGX_F64;
  std::vector<mgx_operator_t> matrix, matrix_dp;
  std::vector<mgx_transfer_t> transfer, transfer_dp;
  std::vector<mgx_smoother_t> smooth;
  std::vector<double *>       solution, rhs, residual;         // fp64 (multigrid_solver.h:709-719)
  std::vector<void *>         defect, t, solution_update;      // V-cycle precision (:725-735)
  std::vector<uint32_t *>     bc_index_dev;
  std::vector<double *>       bc_value_dev, bc_zero_dev;
  std::vector<uint32_t>       bc_count;
  double                     *cg_r = nullptr, *cg_z = nullptr, *cg_d = nullptr, *cg_h = nullptr;
  bool                        timing = false;
  std::vector<double>         timings; // n_levels*6
  // The V-cycle below `graph_level` is a fixed sequence of small, launch-latency-bound kernels on
  // fixed buffers: it is captured into a HIP graph on its second execution and replayed afterwards
  int             graph_level = -1, graph_calls = 0;
  bool            graph_failed = false;
  hipGraph_t      graph = nullptr;
  hipGraphExec_t  graph_exec = nullptr;
  // Agglomeration of the coarse levels of a decomposed hierarchy (mgx_solver_set_agglomeration):
  // the V-cycle below agg_level runs on agg_solver, an undecomposed copy of those levels that
  // every rank holds on a context of its own (no exchange, graph replay)
  mgx_solver_t    agg_solver = nullptr;
  int             agg_level  = -1;
  int             agg_offset = 0;       // level agg_level of this solver is level agg_level + agg_offset of agg_solver (its finest)
  uint32_t       *agg_map    = nullptr; // device [n_dofs(agg_level)]: local DoF -> DoF of agg_solver's level
  uint8_t        *agg_owned  = nullptr; // device: 1 where this rank owns the DoF
  hipEvent_t      agg_in = nullptr, agg_out = nullptr;
  std::vector<double> agg_host;         // callback transport: staging of the allreduce
  std::vector<double> cg_history;       // residual norms of the last solve_cg: start, then one per iteration
  // mgx_solver_update_coefficient: the fp64 state on every level (the finest entry is unused), allocated at the first call
  std::vector<double *> nl_state;
};

namespace
{
  int read_result(mgx_context_t ctx, double *out)
  {
    MGX_HIP(hipMemcpyAsync(ctx->result_host, ctx->result_dev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP(hipStreamSynchronize(ctx->stream));
    *out = ctx->result_host[0];
    return MGX_OK;
  }

  // in-place sum of a few host doubles over the ranks
  int comm_allreduce(mgx_context_t ctx, double *values, int count)
  {
    if (!ctx->has_comm)
      return MGX_OK;
    if (ctx->use_rccl)
      {
        if (count > 8)
          return fail(MGX_ERR_INVALID_ARGUMENT, "comm_allreduce: more than 8 values");
        RcclApi &R = rccl_api();
        MGX_HIP(hipMemcpyAsync(ctx->ar_dev, values, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
        if (R.AllReduce(ctx->ar_dev, ctx->ar_dev, (size_t)count, ncclDouble, ncclSum, ctx->nccl, ctx->stream) != ncclSuccess)
          return fail(MGX_ERR_HIP, "ncclAllReduce failed");
        MGX_HIP(hipMemcpyAsync(values, ctx->ar_dev, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
        MGX_HIP(hipStreamSynchronize(ctx->stream));
        return MGX_OK;
      }
    if (!ctx->comm.allreduce_sum || ctx->comm.allreduce_sum(ctx->comm.user, values, count) != 0)
      return fail(MGX_ERR_HIP, "allreduce_sum callback failed");
    return MGX_OK;
  }

  // x.y over the DoFs this rank owns, summed over the ranks (Vector::operator* / l2_norm with
  // MPI_Allreduce in the reference).  The exchange plan is looked up by the vector length.
  // plan: the ownership plan of the operator the vectors belong to.  nullptr on a decomposed
  // context: looked up by the vector length among the registered operators, which must be
  // unambiguous (the public mgx_dot / mgx_l2_norm take no operator).
  int dot(mgx_context_t ctx, int number, const void *x, const void *y, size_t n, double *out,
          const ExchangePlan *plan = nullptr)
  {
    launch_dot(ctx->stream, number, x, y, n, ctx->partial_dev, ctx->result_dev);
    MGX_TRY(read_result(ctx, out));
    if (!ctx->has_comm)
      return MGX_OK;
    if (!plan)
      {
        for (auto &pr : ctx->plans)
          if (pr.first == n)
            {
              // (operators of one level in two number types share the lists: same sizes)
              if (plan && (plan->n_not_owned != pr.second->n_not_owned || plan->n_shared != pr.second->n_shared))
                return fail(MGX_ERR_INVALID_ARGUMENT, "dot: two operators of this context have vectors of this length but "
                                                      "different ownership; reductions need the operator");
              plan = pr.second;
            }
        if (!plan)
          return fail(MGX_ERR_INVALID_ARGUMENT, "dot: no operator with vectors of this length is registered on this "
                                                "decomposed context (duplicated interface DoFs could not be discounted)");
      }
    if (plan->n_not_owned > 0)
      {
        double dup = 0;
        launch_dot_list(ctx->stream, number, x, y, plan->not_owned_dev, plan->n_not_owned, ctx->partial_dev,
                        ctx->result_dev);
        MGX_TRY(read_result(ctx, &dup));
        *out -= dup;
      }
    return comm_allreduce(ctx, out, 1);
  }

  // Vector::compress(add) for duplicated interface DoFs: every rank ends up with the sum of all
  // sharers' entries, added in ascending rank order on every rank (bitwise identical copies).
  // post (fused exchange plans only; returns with *post_done = true): the Chebyshev update of the interface DoFs and
  // of the constrained rows inside the unpack launch
  int exchange_add(mgx_operator_t op, void *vec, hipStream_t on = nullptr, const BrickLaunch *post = nullptr,
                   bool *post_done = nullptr)
  {
    ExchangePlan *P = op->plan.get();
    if (!P)
      return MGX_OK;
    mgx_context_t ctx = op->ctx;
    hipStream_t   s   = on ? on : ctx->stream;
    const int     num = op->d.number;
    if (P->fused)
      launch_pack_all(s, num, P->send.data(), P->start.data(), (int)P->rank.size(), vec, P->all_index_dev,
                      P->all_seg_dev, P->start.back());
    else
      {
        for (size_t k = 0; k < P->rank.size(); ++k)
          launch_pack(s, num, P->send[k], vec, P->index_dev[k], P->count[k]);
        launch_pack(s, num, P->own_buf, vec, P->shared_dev, P->n_shared);
        launch_constrained_set(s, num, vec, 0.0, P->shared_dev, P->n_shared);
      }
    if (ctx->use_rccl)
      {
        // one group of point-to-point operations on the context's stream: ordered after the pack
        // kernels and before the unpack kernels by the stream itself, the host does not wait
        RcclApi             &R  = rccl_api();
        const ncclDataType_t dt = num == MGX_F64 ? ncclDouble : ncclFloat;
        bool                 ok = R.GroupStart() == ncclSuccess;
        // MGX_RCCL_SELFTEST on a one-rank communicator: every neighbour is the rank itself, so one
        // GPU runs the launch sequence of a rank of a decomposed mesh (tools/rank_emulation.py)
        const bool to_self = ctx->tun.rccl_selftest && ctx->rccl_size == 1;
        for (size_t k = 0; ok && k < P->rank.size(); ++k)
          {
            const int peer = to_self ? 0 : P->rank[k];
            ok = ok && R.Send(P->send[k], P->count[k], dt, peer, ctx->nccl, s) == ncclSuccess;
            ok = ok && R.Recv(P->recv[k], P->count[k], dt, peer, ctx->nccl, s) == ncclSuccess;
          }
        ok = (R.GroupEnd() == ncclSuccess) && ok;
        if (!ok)
          return fail(MGX_ERR_HIP, "RCCL exchange failed");
      }
    else
      {
        MGX_HIP(hipStreamSynchronize(s));
        if (!ctx->comm.exchange ||
            ctx->comm.exchange(ctx->comm.user, P->plan_id, num, (int)P->rank.size(), P->rank.data(),
                               P->count.data(), P->send.data(), P->recv.data()) != 0)
          return fail(MGX_ERR_HIP, "exchange callback failed");
      }
    if (P->fused && post && post_done)
      {
        launch_unpack_ordered_cheb(s, num, P->recv.data(), (int)P->rank.size(), vec, P->shared_dev, P->csr_start_dev,
                                   P->csr_k_dev, P->csr_pos_dev, P->n_shared, *post, op->d.constrained, op->d.n_constrained);
        *post_done = true;
      }
    else if (P->fused)
      launch_unpack_ordered(s, num, P->recv.data(), (int)P->rank.size(), vec, P->shared_dev, P->csr_start_dev,
                            P->csr_k_dev, P->csr_pos_dev, P->n_shared);
    else
      for (size_t k = 0; k <= P->rank.size(); ++k)
        {
          if ((int)k == P->self_pos)
            launch_unpack_add(s, num, vec, P->own_buf, P->shared_dev, P->n_shared);
          if (k < P->rank.size())
            launch_unpack_add(s, num, vec, P->recv[k], P->index_dev[k], P->count[k]);
        }
    MGX_HIP(hipGetLastError());
    return MGX_OK;
  }


  // side stream + events of the overlapped interface exchange (created with the communicator)
  int ensure_side_stream(mgx_context_t ctx)
  {
    if (ctx->side)
      return MGX_OK;
    MGX_HIP(hipSetDevice(ctx->device));
    MGX_HIP(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    MGX_HIP(hipEventCreateWithFlags(&ctx->ev_iface, hipEventDisableTiming));
    MGX_HIP(hipEventCreateWithFlags(&ctx->ev_side, hipEventDisableTiming));
    return MGX_OK;
  }

  // compute units of the context's device: what the persistent grids are sized by
  uint32_t context_cus(mgx_context_t ctx)
  {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    return (uint32_t)std::max(1, cus);
  }

  // HIP-event bracket around the cell loop of a profiled operator
  struct ProfileBracket
  {
    mgx_context_t          ctx;
    bool                   on;
    mgx_context_s::Bracket ev;
    ProfileBracket(mgx_operator_t op, int form)
      : ctx(op->ctx)
      , on(op->ctx->profile && op->profiled)
    {
      if (!on)
        return;
      if (ctx->ev_pool.empty())
        {
          if (hipEventCreate(&ev.start) != hipSuccess || hipEventCreate(&ev.stop) != hipSuccess)
            {
              on = false;
              return;
            }
        }
      else
        {
          ev = ctx->ev_pool.back();
          ctx->ev_pool.pop_back();
        }
      ev.form     = form;
      ev.launches = op->d.bricks.available() ? op->d.bricks.n_colours : 1;
      (void)hipEventRecord(ev.start, ctx->stream);
    }
    ~ProfileBracket()
    {
      if (on)
        {
          (void)hipEventRecord(ev.stop, ctx->stream);
          ctx->ev_used.push_back(ev);
        }
    }
  };

  // The brick loop of a level followed, on a decomposed mesh, by the completion of the interface
  // DoFs: exchange of their partial sums in `carrier`, then `fix(stream)` = the list kernel(s) that
  // apply the fused post-operation to them (they were never flagged LAST).
  // Split schedule (BrickData::n_iface_groups > 0): the bricks on the rank interface run first,
  // colour by colour; the exchange and the list kernels go to the side stream behind an event and
  // overlap with the interior bricks, which touch no interface DoF.  (The reference's explicit
  // exchange, laplace_operator_dg.h:986-1057, packs the send-side data first but waits for all
  // requests before its cell loop; deal.II's own loops overlap inside MatrixFree.)  With the callback transport the host blocks in the exchange
  // while the interior launches, enqueued before, execute.
  // Finish(stream, first, count) (colour-free schedule only, `free_schedule`): completes the DoFs
  // [first, first + count) of the operator's list of brick-surface DoFs (launch_surf_finish); the
  // first n_surf_shared of them are the rank-interface DoFs, whose sums go to the carrier.
  // post / post_done: the fix as the post-operation of the unpack launch where the exchange plan allows (exchange_add)
  template <typename Launch, typename Fix, typename Finish>
  int brick_loop_with_exchange(mgx_operator_t op, int form, void *carrier, Launch launch, Fix fix, bool free_schedule,
                               Finish finish, const BrickLaunch *post = nullptr, bool *post_done = nullptr)
  {
    mgx_context_t    ctx = op->ctx;
    hipStream_t      s   = ctx->stream;
    const BrickData &bd  = op->d.bricks;
    const int        ng = free_schedule ? bd.fr.n_groups : bd.n_colours, ni = free_schedule ? bd.fr.n_iface_groups : bd.n_iface_groups;
    const uint32_t   n_sh = bd.fr.n_surf_shared, n_all = bd.fr.n_surf_dofs;
    if (!op->plan || ni == 0 || !ctx->side)
      {
        {
          ProfileBracket pb(op, form);
          launch(s, 0, ng);
          if (free_schedule)
            finish(s, 0u, n_all);
        }
        if (op->plan)
          {
            bool done = false;
            MGX_TRY(exchange_add(op, carrier, nullptr, post, post ? &done : nullptr));
            if (!done)
              fix(s);
            if (post_done)
              *post_done = done;
          }
        return MGX_OK;
      }
    {
      ProfileBracket pb(op, form);
      launch(s, 0, ni);
      if (free_schedule)
        finish(s, 0u, n_sh); // the interface sums are complete after the interface bricks
      MGX_HIP(hipEventRecord(ctx->ev_iface, s));
      MGX_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_iface, 0));
      launch(s, ni, ng); // enqueued before the (possibly host-blocking) exchange
      if (free_schedule)
        finish(s, n_sh, n_all - n_sh);
    }
    {
      bool done = false;
      MGX_TRY(exchange_add(op, carrier, ctx->side, post, post ? &done : nullptr));
      if (!done)
        fix(ctx->side);
      if (post_done)
        *post_done = done;
    }
    MGX_HIP(hipEventRecord(ctx->ev_side, ctx->side));
    MGX_HIP(hipStreamWaitEvent(s, ctx->ev_side, 0));
    return MGX_OK;
  }
  template <typename Launch, typename Fix>
  int brick_loop_with_exchange(mgx_operator_t op, int form, void *carrier, Launch launch, Fix fix)
  {
    return brick_loop_with_exchange(op, form, carrier, launch, fix, false, [](hipStream_t, uint32_t, uint32_t) {});
  }

  // dst = A src on the unconstrained rows (constrained rows untouched).  identity_rows (per-cell
  // kernel only): also dst = src on the constrained rows, set by the launch that zeroes dst when the
  // constrained DoFs are the tail of the vector; *identity_done tells the caller whether it was
  int apply_plain(mgx_operator_t op, void *dst, const void *src, bool identity_rows = false,
                  bool *identity_done = nullptr)
  {
    if (identity_done)
      *identity_done = false;
    hipStream_t s = op->ctx->stream;
    if (op->d.bricks.available())
      {
        BrickLaunch l; // dst = A src, the partial sums travel in dst itself
        l.mode          = kPlain;
        l.src           = src;
        l.out           = dst;
        l.carrier       = dst;
        l.free_schedule = op->d.bricks.fr.available();
        return brick_loop_with_exchange(
          op, kPlain, dst, [&](hipStream_t st, int g0, int g1) { launch_brick_loop(st, op->d, l.groups(g0, g1)); },
          [](hipStream_t) {}, l.free_schedule,
          [&](hipStream_t st, uint32_t first, uint32_t count) { launch_surf_finish(st, op->d, l, first, count); });
      }
    ProfileBracket pb(op, kPlain);
    if (op->d.gbricks.fr.available() && !op->plan)
      {
        // general operator on its brick schedule: one launch over the bricks, one over the DoFs on brick surfaces
        BrickLaunch l;
        l.mode    = kPlain;
        l.src     = src;
        l.out     = dst;
        l.carrier = dst;
        launch_general_bricks(s, op->d, dst, src);
        launch_surf_finish(s, op->d, l, 0, op->d.gbricks.fr.n_surf_dofs, nullptr, 0, &op->d.gbricks.fr);
        return MGX_OK;
      }
    if (op->d.asm_start)
      {
        // ordered assembly: the cell loop writes every entry of dst (and the identity rows with it when
        // the constrained DoFs are the tail of the vector)
        const bool tail = identity_rows && identity_done && op->constrained_last;
        launch_cell_loop(s, op->d, dst, src, tail ? src : nullptr, op->d.n_dofs - op->d.n_constrained);
        if (tail)
          *identity_done = true;
        return exchange_add(op, dst);
      }
    // "zero dst within the loop" (laplace_operator.h:590)
    if (identity_rows && identity_done && op->constrained_last && op->d.n_dofs < (1u << 22))
      {
        // small levels are launch-bound: one launch instead of the two fill kernels of a memset
        // plus the copy of the constrained rows
        launch_zero_head_copy_tail(s, op->d.number, dst, src, op->d.n_dofs - op->d.n_constrained, op->d.n_dofs);
        *identity_done = true;
      }
    else
      MGX_HIP(hipMemsetAsync(dst, 0, number_size(op->d.number) * op->d.n_dofs, s));
    launch_cell_loop(s, op->d, dst, src);
    return exchange_add(op, dst); // no-op on a single rank
  }

  // Profiler ranges (context option "roctx"): the reference brackets its phases with LIKWID markers -- fmg_solver,
  // cg_solver, matvec, matvec_sp in the driver (poisson_cube/program.cc:282,309,348,369) and vmult_cheby_<level> around
  // the smoother's operator applications (laplace_operator.h:732-739); the same names go to roctx here, so that a
  // rocprofv3 --marker-trace of a run can be cut by level and phase.  The library is bound at run time.
  struct Roctx
  {
    int (*push)(const char *) = nullptr;
    int (*pop)()              = nullptr;
    Roctx()
    {
      for (const char *n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
        if (void *lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))
          {
            push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
            pop  = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
            if (push && pop)
              return;
          }
      push = nullptr;
      pop  = nullptr;
    }
  };
  Roctx &roctx()
  {
    static Roctx r;
    return r;
  }
  inline void range_push(mgx_context_t ctx, const char *name)
  {
    if (ctx->tun.roctx && roctx().push)
      (void)roctx().push(name);
  }
  inline void range_pop(mgx_context_t ctx)
  {
    if (ctx->tun.roctx && roctx().pop)
      (void)roctx().pop();
  }


  // the sum the launch before has left: decomposed, duplicated interface DoFs must count once -- dot() with the plan
  int fused_sum(mgx_operator_t A, const void *a, const void *b, double *out)
  {
    return A->ctx->has_comm ? dot(A->ctx, A->d.number, a, b, A->d.n_dofs, out, A->plan.get()) : read_result(A->ctx, out);
  }

  // The four steps of a CG iteration (mgx_krylov.hpp) on an FE_Q operator with vectors of its number type.  Mixed precision
  // (r32, z32 set): the fp32 defect is written along with r, the direction reads the fp32 result z32 of the preconditioner
  template <typename PreconditionDot>
  struct CGOps
  {
    mgx_operator_t  A;
    void           *x, *r, *z, *d, *h;
    PreconditionDot precondition_dot;
    float          *r32 = nullptr;
    const float    *z32 = nullptr;
    int direction(double beta, bool first)
    {
      hipStream_t s = A->ctx->stream;
      if (first)
        launch_copy_cast(s, d, A->d.number, z32 ? (const void *)z32 : z, z32 ? MGX_F32 : A->d.number, A->d.n_dofs);
      else if (z32)
        launch_xpby_f64_f32(s, (double *)d, z32, beta, A->d.n_dofs);
      else
        launch_xpby(s, A->d.number, d, z, beta, A->d.n_dofs);
      return MGX_OK;
    }
    int vmult_dot(double *dh)
    {
      MGX_TRY(mgx_vmult(A, h, d));
      return dot(A->ctx, A->d.number, d, h, A->d.n_dofs, dh, A->plan.get());
    }
    int update(double alpha, double *res)
    {
      mgx_context_t ctx = A->ctx;
      if (r32)
        launch_cg_update_f32copy(ctx->stream, (double *)x, (double *)r, (const double *)d, (const double *)h, alpha, A->d.n_dofs,
                                 r32, ctx->partial_dev, ctx->result_dev);
      else
        launch_cg_update(ctx->stream, A->d.number, x, r, d, h, alpha, A->d.n_dofs, ctx->partial_dev, ctx->result_dev);
      MGX_TRY(fused_sum(A, r, r, res));
      *res = std::sqrt(*res);
      return MGX_OK;
    }
  };

  // a timed part of the FE_Q V-cycle, as a range under the name of the phase
  LevelTimer stopwatch(mgx_solver_t S, int level, int slot) { return LevelTimer(S->ctx, S->timing, &S->timings[6 * level], level, slot, true); }
} // namespace

mgx::LevelTimer::LevelTimer(mgx_context_t ctx, bool timed, double *times, int level, int part, bool with_ranges)
  : ctx(ctx), slot(timed ? times + part : nullptr), ranges(with_ranges && ctx->tun.roctx)
{
  if (ranges)
    {
      // the phases print_wall_times() reports (multigrid_solver.h:348-371), the smoother under the reference's marker name
      static const char *const names[6] = {"mg_mv", "restrict", "prolongate", "inhomBC", "mg_vec", "vmult_cheby"};
      char                     buf[48];
      std::snprintf(buf, sizeof(buf), "%s_%d", (level == 0 && part == 0) ? "coarse_solver" : names[part], level);
      range_push(ctx, buf);
    }
  if (slot)
    {
      (void)hipStreamSynchronize(ctx->stream);
      t0 = std::chrono::steady_clock::now();
    }
}

mgx::LevelTimer::~LevelTimer()
{
  if (slot)
    {
      (void)hipStreamSynchronize(ctx->stream);
      *slot += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  if (ranges)
    range_pop(ctx);
}

int mgx::residual_update_finish(hipStream_t s, int number, const void *cycle_result, double *residual, double *update, double factor,
                                size_t n_free, size_t n, double *partials, double *sums_dev, double out[2])
{
  double sums[4];
  const uint32_t used = launch_residual_post(s, number, cycle_result, residual, update, factor, n_free, n, partials);
  launch_reduce4(s, partials, used, nullptr, sums_dev);
  MGX_HIP(hipGetLastError());
  MGX_HIP(hipMemcpyAsync(sums, sums_dev, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  MGX_HIP(hipStreamSynchronize(s));
  out[0] = sums[0];
  out[1] = sums[1];
  return MGX_OK;
}

// Point-to-point exchange of packed device buffers with the context's transport (native RCCL group
// on the stream, or the blocking callback), for the parts of the ABI implemented in other
// translation units (the DG ghost-cell update); allreduce of a few host doubles likewise
int mgx::exchange_buffers(mgx_context_t ctx, int plan_id, int number, int n_neighbors, const int *ranks,
                          const uint32_t *counts, void *const *send, void *const *recv, hipStream_t stream)
{
  MGX_REQUIRE(ctx && ctx->has_comm, "exchange_buffers: no communicator on this context");
  hipStream_t s = stream ? stream : ctx->stream;
  if (ctx->use_rccl)
    {
      RcclApi             &R  = rccl_api();
      const ncclDataType_t dt = number == MGX_F64 ? ncclDouble : ncclFloat;
      const bool           to_self = ctx->tun.rccl_selftest && ctx->rccl_size == 1;
      bool                 ok = R.GroupStart() == ncclSuccess;
      for (int k = 0; ok && k < n_neighbors; ++k)
        {
          const int peer = to_self ? 0 : ranks[k];
          ok = ok && R.Send(send[k], counts[k], dt, peer, ctx->nccl, s) == ncclSuccess;
          ok = ok && R.Recv(recv[k], counts[k], dt, peer, ctx->nccl, s) == ncclSuccess;
        }
      ok = (R.GroupEnd() == ncclSuccess) && ok;
      return ok ? MGX_OK : fail(MGX_ERR_HIP, "RCCL exchange failed");
    }
  MGX_HIP(hipStreamSynchronize(s));
  if (!ctx->comm.exchange || ctx->comm.exchange(ctx->comm.user, plan_id, number, n_neighbors, ranks, counts, send, recv) != 0)
    return fail(MGX_ERR_HIP, "exchange callback failed");
  return MGX_OK;
}

hipStream_t mgx::side_stream_begin(mgx_context_t ctx)
{
  if (!ctx || !ctx->side || hipEventRecord(ctx->ev_iface, ctx->stream) != hipSuccess ||
      hipStreamWaitEvent(ctx->side, ctx->ev_iface, 0) != hipSuccess)
    return nullptr;
  return ctx->side;
}

int mgx::side_stream_end(mgx_context_t ctx)
{
  MGX_REQUIRE(ctx && ctx->side, "side_stream_end: no side stream");
  MGX_HIP(hipEventRecord(ctx->ev_side, ctx->side));
  MGX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
  return MGX_OK;
}

int mgx::allreduce_sum(mgx_context_t ctx, double *values, int count) { return comm_allreduce(ctx, values, count); }
int mgx::operator_dim(mgx_operator_t op) { return op->d.dim; }

// x.y over the first n entries of two vectors whose leading part is owned by this rank without
// duplicates (DG vectors: owned cells, then ghost cells), summed over the ranks
int mgx::dot_owned_prefix(mgx_context_t ctx, int number, const void *x, const void *y, size_t n, double *out)
{
  launch_dot(ctx->stream, number, x, y, n, ctx->partial_dev, ctx->result_dev);
  MGX_TRY(read_result(ctx, out));
  return comm_allreduce(ctx, out, 1);
}

bool mgx::context_has_comm(mgx_context_t ctx) { return ctx && ctx->has_comm; }

const mgx::Tunables &mgx::context_tunables(mgx_context_t ctx) { return ctx->tun; }

extern "C" {

const char *mgx_last_error(void) { return g_last_error.c_str(); }
const char *mgx_version(void) { return "mgx 0.1 (gfx950)"; }

int mgx_context_create(mgx_context_t *out, int device)
{
  MGX_REQUIRE(out != nullptr, "mgx_context_create: null output");
  int        count = 0;
  hipError_t e     = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return fail(MGX_ERR_NO_DEVICE, "mgx_context_create: no HIP device available (there is no CPU fallback)");
  MGX_REQUIRE(device >= 0 && device < count, "mgx_context_create: device index out of range");
  MGX_HIP(hipSetDevice(device));
  std::unique_ptr<mgx_context_s, int (*)(mgx_context_t)> ctx(new mgx_context_s, mgx_context_destroy);
  ctx->device = device;
  ctx->tun    = Tunables::from_environment();
  g_trace     = g_trace || ctx->tun.trace;
  MGX_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  MGX_TRY(ctx->mem.alloc(&ctx->partial_dev, kDotBlocks));
  MGX_TRY(ctx->mem.alloc(&ctx->result_dev, 4));
  MGX_HIP(hipHostMalloc((void **)&ctx->result_host, sizeof(double) * 4));
  *out = ctx.release();
  return MGX_OK;
}

int mgx_context_set_option(mgx_context_t ctx, const char *name, double value)
{
  MGX_REQUIRE(ctx && name, "mgx_context_set_option: null argument");
  if (!ctx->tun.set(name, value))
    return fail(MGX_ERR_INVALID_ARGUMENT, std::string("mgx_context_set_option: unknown option '") + name + "'");
  g_trace = g_trace || ctx->tun.trace;
  return MGX_OK;
}

int mgx_context_destroy(mgx_context_t ctx)
{
  if (!ctx)
    return MGX_OK;
  if (ctx->borrowed_stream)
    (void)hipDeviceSynchronize(); // the stream's owner may be gone already
  else
    (void)hipStreamSynchronize(ctx->stream);
  (void)hipHostFree(ctx->result_host);
  if (ctx->nccl)
    (void)rccl_api().CommDestroy(ctx->nccl);
  for (auto *pool : {&ctx->ev_pool, &ctx->ev_used})
    for (auto &ev : *pool)
      {
        (void)hipEventDestroy(ev.start);
        (void)hipEventDestroy(ev.stop);
      }
  if (ctx->side)
    (void)hipStreamDestroy(ctx->side);
  if (ctx->ev_iface)
    (void)hipEventDestroy(ctx->ev_iface);
  if (ctx->ev_side)
    (void)hipEventDestroy(ctx->ev_side);
  if (!ctx->borrowed_stream)
    (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return MGX_OK;
}

int mgx_sync(mgx_context_t ctx)
{
  MGX_REQUIRE(ctx, "mgx_sync: null context");
  MGX_HIP(hipStreamSynchronize(ctx->stream));
  return MGX_OK;
}

int mgx_device_memory_info(mgx_context_t ctx, size_t *free_bytes, size_t *total_bytes)
{
  MGX_REQUIRE(ctx && free_bytes && total_bytes, "mgx_device_memory_info: null argument");
  MGX_HIP(hipSetDevice(ctx->device));
  MGX_HIP(hipMemGetInfo(free_bytes, total_bytes));
  return MGX_OK;
}

void *mgx_context_stream(mgx_context_t ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int mgx_context_set_comm(mgx_context_t ctx, const mgx_comm_desc *comm)
{
  MGX_REQUIRE(ctx && comm && comm->exchange && comm->allreduce_sum && comm->size >= 1 && comm->rank >= 0 &&
                comm->rank < comm->size,
              "mgx_context_set_comm: bad communicator");
  ctx->comm     = *comm;
  ctx->has_comm = comm->size > 1;
  if (ctx->has_comm)
    MGX_TRY(ensure_side_stream(ctx));
  return MGX_OK;
}

int mgx_rccl_unique_id(void *id128)
{
  MGX_REQUIRE(id128, "mgx_rccl_unique_id: null argument");
  static_assert(sizeof(ncclUniqueId) == MGX_RCCL_ID_BYTES, "ncclUniqueId size");
  RcclApi &R = rccl_api();
  if (!R.load())
    return fail(MGX_ERR_UNSUPPORTED, "mgx_rccl_unique_id: librccl not found");
  ncclUniqueId id;
  if (R.GetUniqueId(&id) != ncclSuccess)
    return fail(MGX_ERR_HIP, "ncclGetUniqueId failed");
  std::memcpy(id128, &id, sizeof(id));
  return MGX_OK;
}

int mgx_context_set_rccl(mgx_context_t ctx, int rank, int size, const void *id128)
{
  MGX_REQUIRE(ctx && id128 && size >= 1 && rank >= 0 && rank < size, "mgx_context_set_rccl: bad argument");
  MGX_REQUIRE(!ctx->nccl, "mgx_context_set_rccl: communicator already set");
  RcclApi &R = rccl_api();
  if (!R.load())
    return fail(MGX_ERR_UNSUPPORTED, "mgx_context_set_rccl: librccl not found");
  MGX_HIP(hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  const ncclResult_t r = R.CommInitRank(&ctx->nccl, size, id, rank);
  if (r != ncclSuccess)
    {
      ctx->nccl = nullptr;
      return fail(MGX_ERR_HIP, std::string("ncclCommInitRank failed: ") + R.GetErrorString(r));
    }
  MGX_TRY(ctx->mem.alloc(&ctx->ar_dev, 8));
  ctx->rccl_rank = rank;
  ctx->rccl_size = size;
  ctx->has_comm  = size > 1 || ctx->tun.rccl_selftest;
  if (ctx->has_comm)
    MGX_TRY(ensure_side_stream(ctx));
  ctx->use_rccl  = true;
  return MGX_OK;
}

int mgx_context_use_rccl(mgx_context_t ctx, int enable)
{
  MGX_REQUIRE(ctx, "mgx_context_use_rccl: null context");
  if (enable)
    MGX_REQUIRE(ctx->nccl, "mgx_context_use_rccl: no RCCL communicator on this context");
  else
    MGX_REQUIRE(ctx->comm.exchange && ctx->comm.allreduce_sum, "mgx_context_use_rccl: no callback transport to fall back to");
  MGX_HIP(hipStreamSynchronize(ctx->stream));
  ctx->use_rccl = enable != 0;
  return MGX_OK;
}

int mgx_copy_device(mgx_context_t ctx, void *dst, const void *src, size_t bytes)
{
  MGX_REQUIRE(ctx && (bytes == 0 || (dst && src)), "mgx_copy_device: null argument");
  if (bytes)
    {
      MGX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      MGX_HIP(hipStreamSynchronize(ctx->stream));
    }
  return MGX_OK;
}

int mgx_range_push(mgx_context_t ctx, const char *name)
{
  MGX_REQUIRE(ctx && name, "mgx_range_push: null argument");
  range_push(ctx, name);
  return MGX_OK;
}

int mgx_range_pop(mgx_context_t ctx)
{
  MGX_REQUIRE(ctx, "mgx_range_pop: null context");
  range_pop(ctx);
  return MGX_OK;
}

int mgx_profile_enable(mgx_context_t ctx, int enable)
{
  MGX_REQUIRE(ctx, "mgx_profile_enable: null context");
  ctx->profile = enable != 0;
  return MGX_OK;
}

int mgx_profile_read(mgx_context_t ctx, int form, uint64_t *launches, double *total_ms)
{
  MGX_REQUIRE(ctx && launches && total_ms, "mgx_profile_read: null argument");
  MGX_HIP(hipStreamSynchronize(ctx->stream));
  double                              sum = 0;
  uint64_t                            n   = 0;
  std::vector<mgx_context_s::Bracket> keep;
  for (auto &ev : ctx->ev_used)
    {
      if (ev.form != form)
        {
          keep.push_back(ev);
          continue;
        }
      float ms = 0;
      MGX_HIP(hipEventElapsedTime(&ms, ev.start, ev.stop));
      sum += ms;
      n += (uint64_t)ev.launches;
      ctx->ev_pool.push_back(ev);
    }
  ctx->ev_used.swap(keep);
  *launches = n;
  *total_ms = sum;
  return MGX_OK;
}

int mgx_malloc(mgx_context_t ctx, void **dptr, size_t bytes)
{
  MGX_REQUIRE(ctx && dptr, "mgx_malloc: null argument");
  MGX_HIP(hipMalloc(dptr, bytes ? bytes : 8));
  return MGX_OK;
}

int mgx_free(mgx_context_t ctx, void *dptr)
{
  MGX_REQUIRE(ctx, "mgx_free: null context");
  if (dptr)
    {
      MGX_HIP(hipStreamSynchronize(ctx->stream));
      MGX_HIP(hipFree(dptr));
    }
  return MGX_OK;
}

int mgx_upload(mgx_context_t ctx, void *dptr, const void *hptr, size_t bytes)
{
  MGX_REQUIRE(ctx && (bytes == 0 || (dptr && hptr)), "mgx_upload: null argument");
  if (bytes)
    {
      MGX_HIP(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, ctx->stream));
      MGX_HIP(hipStreamSynchronize(ctx->stream));
    }
  return MGX_OK;
}

int mgx_download(mgx_context_t ctx, void *hptr, const void *dptr, size_t bytes)
{
  MGX_REQUIRE(ctx && (bytes == 0 || (dptr && hptr)), "mgx_download: null argument");
  if (bytes)
    {
      MGX_HIP(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
      MGX_HIP(hipStreamSynchronize(ctx->stream));
    }
  return MGX_OK;
}

int mgx_memset_zero(mgx_context_t ctx, void *dptr, size_t bytes)
{
  MGX_REQUIRE(ctx && (bytes == 0 || dptr), "mgx_memset_zero: null argument");
  if (bytes)
    MGX_HIP(hipMemsetAsync(dptr, 0, bytes, ctx->stream));
  return MGX_OK;
}

int mgx_copy_cast(mgx_context_t ctx, void *dst, int dn, const void *src, int sn, size_t n)
{
  MGX_REQUIRE(ctx && (n == 0 || (dst && src)), "mgx_copy_cast: null argument");
  launch_copy_cast(ctx->stream, dst, dn, src, sn, n);
  return MGX_OK;
}

int mgx_add_cast(mgx_context_t ctx, void *dst, int dn, const void *src, int sn, size_t n)
{
  MGX_REQUIRE(ctx && (n == 0 || (dst && src)), "mgx_add_cast: null argument");
  launch_add_cast(ctx->stream, dst, dn, src, sn, n);
  return MGX_OK;
}

int mgx_sadd(mgx_context_t ctx, int number, void *x, double s, double a, const void *v, size_t n)
{
  MGX_REQUIRE(ctx && (n == 0 || (x && v)), "mgx_sadd: null argument");
  launch_sadd(ctx->stream, number, x, s, a, v, n);
  return MGX_OK;
}

int mgx_dot(mgx_context_t ctx, int number, const void *x, const void *y, size_t n, double *result)
{
  MGX_REQUIRE(ctx && result && (n == 0 || (x && y)), "mgx_dot: null argument");
  return dot(ctx, number, x, y, n, result);
}

int mgx_l2_norm(mgx_context_t ctx, int number, const void *x, size_t n, double *result)
{
  MGX_REQUIRE(ctx && result && (n == 0 || x), "mgx_l2_norm: null argument");
  double s = 0;
  MGX_TRY(dot(ctx, number, x, x, n, &s));
  *result = std::sqrt(s);
  return MGX_OK;
}

/* reductions over the DoFs a rank owns, with the ownership taken from the operator itself (mgx_dot finds
 * it through the vector length) */
int mgx_operator_dot(mgx_operator_t op, const void *x, const void *y, double *result)
{
  MGX_REQUIRE(op && x && y && result, "mgx_operator_dot: null argument");
  return dot(op->ctx, op->d.number, x, y, op->d.n_dofs, result, op->plan.get());
}

int mgx_operator_l2_norm(mgx_operator_t op, const void *x, double *result)
{
  MGX_REQUIRE(op && x && result, "mgx_operator_l2_norm: null argument");
  double s = 0;
  MGX_TRY(dot(op->ctx, op->d.number, x, x, op->d.n_dofs, &s, op->plan.get()));
  *result = std::sqrt(s);
  return MGX_OK;
}

int mgx_set_entries(mgx_context_t ctx, int number, void *v, const uint32_t *idx_host, const double *val_host,
                    uint32_t count)
{
  MGX_REQUIRE(ctx && (count == 0 || (v && idx_host && val_host)), "mgx_set_entries: null argument");
  if (count == 0)
    return MGX_OK;
  DeviceArena tmp("mgx_set_entries");
  uint32_t *idx_dev = nullptr;
  double   *val_dev = nullptr;
  MGX_TRY(tmp.alloc(&idx_dev, count));
  MGX_TRY(tmp.alloc(&val_dev, count));
  MGX_HIP(hipMemcpyAsync(idx_dev, idx_host, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
  MGX_HIP(hipMemcpyAsync(val_dev, val_host, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
  launch_scatter_values(ctx->stream, number, v, idx_dev, val_dev, count);
  MGX_HIP(hipStreamSynchronize(ctx->stream)); // (the host arrays are the caller's, in flight until here)
  return MGX_OK;
}

/* ------------------------------------------------------------------------------------------
 * LaplaceOperator
 * ------------------------------------------------------------------------------------------ */
} // extern "C"

// The stages of mgx_operator_create, in the order it calls them.  Every device buffer goes to the operator's arena:
// a stage that fails leaves nothing behind that mgx_operator_destroy would not free.
namespace
{
  constexpr size_t kAssemblyMaxEntries = (size_t)1 << 26; // ordered assembly up to this many local values per level

  // what depends on the dimension of a level (mgx_operator_desc::dim) beyond mgx_index_tables.hpp: entries of the
  // symmetric coefficient tensor
  inline int desc_dim(const mgx_operator_desc *desc) { return desc->dim == 2 ? 2 : 3; }
  inline int n_tensor_entries(int dim) { return dim == 2 ? 3 : 6; }
  // the entry points that exist in three dimensions only
  inline int refuse_2d(const mgx::OperatorData &d, const char *who, const char *why)
  {
    if (d.dim != 2)
      return MGX_OK;
    return fail(MGX_ERR_UNSUPPORTED, std::string(who) + ": not on a two-dimensional operator (" + why + ")");
  }

  // G = D S: derivative of the nodal basis at the quadrature points, G[q n + i], accumulated in R
  template <typename R>
  void nodal_gradient(const mgx_operator_s &op, R *G)
  {
    const int n = op.d.p + 1;
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i)
        {
          R g = 0;
          for (int r = 0; r < n; ++r)
            g += (R)op.D[q * n + r] * op.S[r * n + i];
          G[q * n + i] = g;
        }
  }

  // host-side validation of operand shapes before any kernel can touch them
  int validate_operator_desc(mgx_context_t ctx, const mgx_operator_desc *desc, mgx_operator_t *out)
  {
    MGX_REQUIRE(ctx && desc && out, "mgx_operator_create: null argument");
    MGX_REQUIRE(desc->degree >= 1 && desc->degree <= MGX_MAX_DEGREE, "mgx_operator_create: degree must be 1..9");
    MGX_REQUIRE(desc->number == MGX_F32 || desc->number == MGX_F64, "mgx_operator_create: bad number type");
    MGX_REQUIRE(desc->n_cells > 0 && desc->n_dofs > 0, "mgx_operator_create: empty level");
    MGX_REQUIRE(desc->idx27 && desc->shape_values && desc->colloc_grad && desc->qweights,
                "mgx_operator_create: missing table");
    MGX_REQUIRE(desc->n_constrained == 0 || desc->constrained, "mgx_operator_create: missing constrained list");
    MGX_REQUIRE(desc->dim == 0 || desc->dim == 2 || desc->dim == 3, "mgx_operator_create: dim must be 2 or 3 (0: 3)");
    if (desc->dim == 2 && desc->exchange)
      return fail(MGX_ERR_UNSUPPORTED, "mgx_operator_create: a two-dimensional operator with an exchange plan (one rank only)");
    if (desc->dim == 2 && ctx->has_comm)
      return fail(MGX_ERR_UNSUPPORTED, "mgx_operator_create: a two-dimensional operator on a context with a communicator (one rank only)");
    const int    p         = desc->degree;
    const int    ne        = n_entities(desc_dim(desc));
    const size_t n_entries = ne * (size_t)desc->n_cells;
    for (int pass = 0; pass < 2; ++pass)
      {
        const uint32_t *tab = pass == 0 ? desc->idx27 : desc->idx27_plain;
        if (!tab)
          continue;
        for (size_t i = 0; i < n_entries; ++i)
          {
            const uint32_t b = tab[i];
            if (b == MGX_INVALID_INDEX)
              continue;
            if ((uint64_t)b + (uint32_t)entity_size((int)(i % ne), p) > desc->n_dofs)
              return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: compressed index out of range");
          }
      }
    for (uint32_t i = 0; i < desc->n_constrained; ++i)
      if (desc->constrained[i] >= desc->n_dofs)
        return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: constrained index out of range");
    if (!desc->coef_q && desc->dim == 2) // [xx, yy, xy]
      MGX_REQUIRE(desc->coef[0] > 0 && desc->coef[0] * desc->coef[1] - desc->coef[2] * desc->coef[2] > 0,
                  "mgx_operator_create: the coefficient tensor is not positive definite");
    else if (!desc->coef_q)
      {
        // the one coefficient tensor of an affine mesh (xx yy zz xy xz yz) must be positive definite
        const double *c  = desc->coef;
        const double  m2 = c[0] * c[1] - c[3] * c[3];
        const double  m3 = c[0] * (c[1] * c[2] - c[5] * c[5]) - c[3] * (c[3] * c[2] - c[5] * c[4]) +
                          c[4] * (c[3] * c[5] - c[1] * c[4]);
        MGX_REQUIRE(c[0] > 0 && m2 > 0 && m3 > 0, "mgx_operator_create: the coefficient tensor is not positive definite");
      }
    return MGX_OK;
  }

  // are the constrained DoFs exactly [n_dofs - n_constrained, n_dofs)?  (any order inside the list)
  bool constrained_are_last(const mgx_operator_desc *desc)
  {
    std::vector<uint8_t> seen(desc->n_constrained, 0);
    bool                 last = true;
    for (uint32_t i = 0; i < desc->n_constrained && last; ++i)
      {
        const uint32_t c = desc->constrained[i];
        last             = c >= desc->n_dofs - desc->n_constrained && !seen[c - (desc->n_dofs - desc->n_constrained)];
        if (last)
          seen[c - (desc->n_dofs - desc->n_constrained)] = 1;
      }
    return last;
  }

  // 1D tables of the element in the operator's number type (Basis1D<T>); decides d.separable
  int upload_basis(mgx_operator_s &op)
  {
    OperatorData &d = op.d;
    const int     n = d.p + 1;
    // 1D mass and stiffness matrices of the separable form, M = S^T W S, K = S^T D^T W D S
    double M1[kMaxN * kMaxN], K1[kMaxN * kMaxN];
    {
      long double G[kMaxN * kMaxN];
      nodal_gradient(op, G);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
          {
            long double m = 0, k = 0;
            for (int q = 0; q < n; ++q)
              {
                m += (long double)op.w[q] * op.S[q * n + i] * op.S[q * n + j];
                k += (long double)op.w[q] * G[q * n + i] * G[q * n + j];
              }
            M1[i * n + j] = (double)m;
            K1[i * n + j] = (double)k;
          }
    }
    auto fill_basis = [&](auto &b) {
      using T = std::remove_reference_t<decltype(b.S[0])>;
      for (int i = 0; i < n * n; ++i)
        {
          b.S[i] = (T)op.S[i];
          b.D[i] = (T)op.D[i];
        }
      for (int i = 0; i < n; ++i)
        b.w[i] = (T)op.w[i];
      const int H = n / 2;
      auto      eo = [&](auto &E, const double *A) {
        for (int a = 0; a < H; ++a)
          {
            for (int i = 0; i < H; ++i)
              {
                E.ee[a * H + i] = (T)(0.5 * (A[a * n + i] + A[a * n + n - 1 - i]));
                E.eo[a * H + i] = (T)(0.5 * (A[a * n + i] - A[a * n + n - 1 - i]));
              }
            E.mc[a] = (n % 2) ? (T)A[a * n + H] : (T)0;
          }
        E.mhh = (n % 2) ? (T)A[H * n + H] : (T)0;
      };
      eo(b.mass, M1);
      eo(b.lapl, K1);
    };
    // the separable fast path needs the symmetry A[a][b] = A[n-1-a][n-1-b] of M and K (true for
    // any symmetric node/quadrature set); MGX_GENERAL_KERNEL=1 forces the quadrature-point form
    for (int a = 0; a < n && d.separable; ++a)
      for (int bb = 0; bb < n; ++bb)
        if (std::fabs(M1[a * n + bb] - M1[(n - 1 - a) * n + n - 1 - bb]) > 1e-12 ||
            std::fabs(K1[a * n + bb] - K1[(n - 1 - a) * n + n - 1 - bb]) > 1e-10 * std::fabs(K1[0]))
          d.separable = false;
    if (d.number == MGX_F64)
      {
        Basis1D<double> b{};
        fill_basis(b);
        return op.mem.upload_bytes(&d.basis, &b, sizeof(b));
      }
    Basis1D<float> b{};
    fill_basis(b);
    return op.mem.upload_bytes(&d.basis, &b, sizeof(b));
  }

  // general branch: G = D S for the diagonal of the general cell matrix; the per-point coefficient in the
  // operator's number type
  int upload_general_tables(mgx_operator_s &op, const mgx_operator_desc *desc)
  {
    OperatorData       &d = op.d;
    const int           n = d.p + 1;
    std::vector<double> G((size_t)n * n);
    nodal_gradient(op, G.data());
    MGX_TRY(op.mem.upload_as(d.number, &d.grad_1d, G.data(), G.size()));
    if (desc->coef_q)
      MGX_TRY(op.mem.upload_as(d.number, &d.coef_q, desc->coef_q,
                               (size_t)desc->n_cells * n_tensor_entries(d.dim) * n_local_values(d.dim, d.p)));
    return MGX_OK;
  }

  // Cell colouring for the general branch: greedy over the cells in their order, two cells
  // conflict if they share a mesh entity that carries DoFs (its first DoF is the key).  On the
  // structured meshes of the provider this gives the 8 parity classes.  More than 32 colours:
  // keep the single launch with atomics.
  int colour_cells(mgx_operator_s &op, const mgx_operator_desc *desc)
  {
    const CellColouring colours = colour_cells_greedy(desc->idx27, n_entities(op.d.dim), desc->n_cells, desc->n_dofs, op.d.p);
    if (colours.more_than_32)
      return MGX_OK;
    MGX_TRY(upload_colours(op.mem, op.d.cell_colours, colours));
    MGX_TRACE("operator_create: %u cells in %d colours", desc->n_cells, colours.n);
    return MGX_OK;
  }

  // device tables of a reduced-colour schedule (bricks.fr and gbricks.fr); the counts of `fr` that differ between
  // the two are the caller's
  int upload_free_schedule(DeviceArena &mem, FreeSchedule &fr, FreeHost &fh, uint32_t n_bricks, int number)
  {
    fr.n_surf      = fh.n_surf;
    fr.n_surf_dofs = (uint32_t)fh.surf_dof.size();
    fh.surf_dof.push_back(0);
    fh.surf_pos.push_back(0);
    MGX_TRY(mem.upload(&fr.surf_off, fh.surf_off));
    MGX_TRY(mem.upload(&fr.surf_dof, fh.surf_dof));
    MGX_TRY(mem.upload(&fr.surf_start, fh.surf_start));
    MGX_TRY(mem.upload(&fr.surf_pos, fh.surf_pos));
    MGX_TRY(mem.alloc(&fr.priv, (size_t)n_bricks * fh.n_surf * number_size(number) + 16));
    return mem.upload(&fr.ent, fh.ent);
  }

  // brick schedule for the atomic-free cell loop (mgx_brick.hip); MGX_NO_BRICKS=1 keeps the
  // per-cell kernel (A/B measurements)
  int build_brick_schedule(mgx_operator_s &op, const mgx_operator_desc *desc, const Tunables &tun)
  {
    OperatorData &d = op.d;
    const int     p = d.p;
    BrickHost   bh;
    std::string why;
    const mgx_exchange_desc *ex = desc->exchange;
    // The eight colour launches of a brick loop cost about 80 us however small the level is; below
    // that the per-cell kernel (all cells of the level in one launch, atomic scatter) is faster.
    // Measured cross-over with the macro-element kernel on MI355X (tools/time_matvec.py): p = 4 and
    // p = 8 between 216 and 512 bricks (512: 0.082 vs 0.098 ms, 0.090 vs 0.134 ms), p = 2 between 512
    // and 1728 bricks (512: 0.042 vs 0.028 ms).  MGX_BRICK_MIN overrides the threshold as given.
    const uint32_t brick_min   = tun.brick_min_from_env ? tun.brick_min : (p <= 2 ? 2 * tun.brick_min : tun.brick_min);
    const uint32_t brick_cells = p <= 4 ? 64u : 8u;
    // Decomposed mesh: from this many bricks per rank on, the bricks on the rank interface are
    // launched first and the exchange overlaps with the interior bricks.  The split costs one
    // small (latency-bound) launch per colour; DESIGN.md 6 has the measured break-even.
    const uint32_t overlap_min = tun.overlap_min;
    if (desc->n_dofs >= 0x3FFFFFFFu)
      {
        MGX_TRACE("operator_create: per-cell kernel (%u DoFs do not fit the 30-bit entity index)", desc->n_dofs);
        return MGX_OK;
      }
    if (desc->n_cells / brick_cells < brick_min)
      {
        MGX_TRACE("operator_create: per-cell kernel (%u bricks < %u)", desc->n_cells / brick_cells, brick_min);
        return MGX_OK;
      }
    if (!build_bricks(p, desc->n_cells, desc->n_dofs, desc->idx27, desc->idx27_plain, desc->brick_colour,
                      ex ? ex->shared : nullptr, ex ? ex->n_shared : 0, ex && desc->n_cells / brick_cells >= overlap_min, bh,
                      why))
      {
        MGX_TRACE("operator_create: per-cell kernel (%s)", why.c_str());
        return MGX_OK;
      }
    BrickData &b = d.bricks;
    b.n_bricks   = bh.n_bricks;
    b.n_colours  = bh.n_colours;
    b.n_iface_groups = bh.n_iface_groups;
    b.order      = bh.order;
    for (int c = 0; c <= bh.n_colours; ++c)
      b.colour_start[c] = bh.colour_start[c];
    // device table word: bits 0..29 first DoF, bit 30 FIRST, bit 31 LAST (mgx_brick.hip)
    for (size_t i = 0; i < bh.ent_base.size(); ++i)
      if (bh.ent_base[i] != MGX_INVALID_INDEX)
        bh.ent_base[i] |= (uint32_t)(bh.ent_flags[i] & 3u) << 30;
    MGX_TRY(op.mem.upload(&b.ent_base, bh.ent_base));
    b.ent_flags = nullptr;
    if (d.separable)
      {
        // write-out order of the macro-element kernel (mgx_macro.hip)
        std::vector<uint32_t> map;
        build_item_map(p, map);
        MGX_TRY(op.mem.upload(&b.item_map, map));
        {
          // ... and of its second pipeline (mgx_macro2.hip): interior of the brick first
          std::vector<uint32_t> map2;
          build_item_map2(p, map2);
          MGX_TRY(op.mem.upload(&b.item_map2, map2));
        }
        // Reduced-colour schedule of the plain / residual / Chebyshev forms (mgx_macro.hip, FREE): one
        // class (one launch per level) on levels with at most free_one_max bricks, two classes up to
        // free_max_bricks
        const int n_classes = b.n_bricks <= tun.free_one_max ? 1 : 2;
        FreeHost  fh;
        if (!MGX_MACRO_PAIRS && !tun.cells_form && b.n_bricks <= tun.free_max_bricks &&
            (uint64_t)desc->n_dofs * number_size(d.number) < 0xFFFFFFF0ull &&
            build_free_schedule(p, bh, desc->n_dofs, ex ? ex->shared : nullptr, ex ? ex->n_shared : 0,
                                bh.n_iface_groups > 0, n_classes, map, fh) &&
            (size_t)b.n_bricks * fh.n_surf * number_size(d.number) < 0xFFFFFFF0ull && fh.n_groups <= 8)
          {
            FreeSchedule &fr  = b.fr;
            fr.n_classes      = n_classes;
            fr.n_groups       = fh.n_groups;
            fr.n_iface_groups = fh.n_iface_groups;
            for (int g = 0; g <= fh.n_groups; ++g)
              fr.group_start[g] = fh.group_start[g];
            fr.n_surf_shared = fh.n_surf_shared;
            MGX_TRY(upload_free_schedule(op.mem, fr, fh, b.n_bricks, d.number));
            MGX_TRACE("operator_create: reduced-colour schedule, %d classes, %d groups, %u private values per brick, %u "
                      "private DoFs (%u shared)",
                      n_classes, fr.n_groups, fr.n_surf, fr.n_surf_dofs, fr.n_surf_shared);
          }
      }
    MGX_TRACE("operator_create: %u bricks, %d colours", b.n_bricks, b.n_colours);
    return MGX_OK;
  }

  // Brick form of the general tensor branch (mgx_kernels.hip, brick_general_kernel): p = 4, one rank, vectors and
  // coefficient array below the 4 GB of a 32-bit element offset, cells in bricks (hyper_shell and every structured
  // mapped mesh of mgx_cube): the one-launch schedule of the macro-element kernel -- every entity on a brick surface
  // private -- with its finish kernel.  vmult only; the other forms of a general operator keep the per-cell kernel.
  int build_general_brick_schedule(mgx_operator_s &op, const mgx_operator_desc *desc)
  {
    OperatorData &d = op.d;
    const int     p = d.p;
    BrickHost   bh;
    std::string why;
    FreeHost    fh;
    std::vector<uint32_t> map;
    build_item_map(p, map);
    if (build_bricks(p, desc->n_cells, desc->n_dofs, desc->idx27, desc->idx27_plain, nullptr, nullptr, 0, false, bh, why) &&
        build_free_schedule(p, bh, desc->n_dofs, nullptr, 0, false, 1, map, fh) && fh.n_groups == 1 &&
        (size_t)bh.n_bricks * fh.n_surf * number_size(d.number) < 0xFFFFFFF0ull)
      {
        BrickData &g = d.gbricks;
        g.n_bricks   = bh.n_bricks;
        FreeSchedule &fr = g.fr;
        fr.n_classes = 1;
        fr.n_groups  = 1;
        fr.group_start[0] = 0;
        fr.group_start[1] = bh.n_bricks;
        fr.n_surf_shared = 0;
        MGX_TRY(op.mem.upload(&g.order_dev, bh.order));
        MGX_TRY(op.mem.upload(&g.item_map, map));
        MGX_TRY(upload_free_schedule(op.mem, fr, fh, bh.n_bricks, d.number));
        MGX_TRACE("operator_create: general branch on %u bricks, %u private values per brick, %u private DoFs", bh.n_bricks,
                  fr.n_surf, fr.n_surf_dofs);
      }
    else
      MGX_TRACE("operator_create: general branch without bricks (%s)", why.c_str());
    return MGX_OK;
  }

  // Ordered assembly for the per-cell kernels: levels without a brick schedule and without cell
  // colours.  For every DoF the positions (cell (p+1)^3 + local index) of its contributions in
  // ascending cell order, from the compressed index table (read_dof_values_compressed,
  // vector_access_reduced.h:153-229; constrained entities contribute nothing).  Larger levels than
  // kAssemblyMaxEntries keep the one launch with atomic adds (last bits not reproducible).
  int build_ordered_assembly(mgx_operator_s &op, const mgx_operator_desc *desc)
  {
    OperatorData &d = op.d;
    const size_t  n_local = n_local_values(d.dim, d.p) * desc->n_cells;
    if (d.bricks.available() || d.cell_colours.order || n_local > kAssemblyMaxEntries)
      return MGX_OK;
    const IndexRows a = ordered_assembly(desc->idx27, d.dim, desc->n_cells, desc->n_dofs, d.p);
    MGX_TRY(op.mem.upload(&d.asm_start, a.start));
    MGX_TRY(op.mem.upload(&d.asm_pos, a.pos));
    MGX_TRY(op.mem.alloc(&d.cell_scratch, number_size(d.number) * n_local));
    MGX_TRACE("operator_create: ordered assembly of the per-cell kernel (%zu contributions)", a.pos.size() - 1);
    return MGX_OK;
  }

  // smoother start vector statistics over the DoFs this rank owns
  void start_vector_statistics(mgx_operator_s &op, const mgx_operator_desc *desc)
  {
    std::vector<uint8_t> skip(desc->n_dofs, 0);
    if (desc->exchange)
      for (uint32_t i = 0; i < desc->exchange->n_not_owned; ++i)
        skip[desc->exchange->not_owned[i]] = 1;
    double sum = 0, cnt = 0;
    for (uint32_t i = 0; i < desc->n_dofs; ++i)
      if (!skip[i])
        {
          sum += (double)((desc->global_index ? desc->global_index[i] : i) % 11u);
          cnt += 1;
        }
    op.start_sum   = sum;
    op.start_count = cnt;
  }

  // interface exchange of a decomposed mesh: lists, buffers (the operator's arena holds those it allocates itself;
  // the caller's and the communicator's stay theirs) and the tables of the fused pack / ordered unpack
  int build_exchange_plan(mgx_operator_s &op, const mgx_operator_desc *desc, const Tunables &tun)
  {
    mgx_context_t            ctx = op.ctx;
    const OperatorData      &d   = op.d;
    const mgx_exchange_desc &e   = *desc->exchange;
    MGX_REQUIRE(ctx->has_comm, "mgx_operator_create: exchange plan given but no communicator set on the context");
    MGX_REQUIRE(e.n_neighbors >= 0 && (e.n_neighbors == 0 || (e.neighbor_rank && e.count && e.index)),
                "mgx_operator_create: incomplete exchange plan");
    auto P     = std::make_unique<ExchangePlan>();
    P->plan_id = e.plan_id;
    P->number  = d.number;
    const size_t es = number_size(d.number);
    const int    my_rank = (ctx->nccl && !ctx->comm.exchange) ? ctx->rccl_rank : ctx->comm.rank;
    // MGX_RCCL_SELFTEST: a one-rank communicator may name itself as neighbour (tools/rccl_selftest.py)
    const bool   selftest = tun.rccl_selftest;
    for (int k = 0; k < e.n_neighbors; ++k)
      {
        MGX_REQUIRE(selftest ||
                      (e.neighbor_rank[k] != my_rank && (k == 0 || e.neighbor_rank[k] > e.neighbor_rank[k - 1])),
                    "mgx_operator_create: neighbour ranks must be ascending and differ from the own rank");
        for (uint32_t i = 0; i < e.count[k]; ++i)
          if (e.index[k][i] >= desc->n_dofs)
            return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: exchange index out of range");
        if (e.neighbor_rank[k] < my_rank)
          P->self_pos = k + 1;
        P->rank.push_back(e.neighbor_rank[k]);
        P->count.push_back(e.count[k]);
        uint32_t *idx = nullptr;
        MGX_TRY(op.mem.upload(&idx, e.index[k], e.count[k], 1));
        P->index_dev.push_back(idx);
        void *sb = e.send_buf ? e.send_buf[k] : nullptr, *rb = e.recv_buf ? e.recv_buf[k] : nullptr;
        bool own = !(sb && rb);
        if (own && ctx->comm.alloc_device)
          {
            sb  = ctx->comm.alloc_device(ctx->comm.user, es * (e.count[k] + 1));
            rb  = ctx->comm.alloc_device(ctx->comm.user, es * (e.count[k] + 1));
            own = false;
            MGX_REQUIRE(sb && rb, "mgx_operator_create: the communicator's alloc_device failed");
          }
        if (own)
          {
            MGX_TRY(op.mem.alloc(&sb, es * (e.count[k] + 1)));
            MGX_TRY(op.mem.alloc(&rb, es * (e.count[k] + 1)));
          }
        P->send.push_back(sb);
        P->recv.push_back(rb);
      }
    for (uint32_t i = 0; i < e.n_shared; ++i)
      if (e.shared[i] >= desc->n_dofs)
        return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: shared index out of range");
    {
      // Dirichlet DoFs are never exchanged: their rows are the identity on every rank, and the
      // interface post-operations assume the two lists to be disjoint (mgx.h, mgx_exchange_desc)
      std::vector<uint8_t> is_constrained(desc->n_dofs, 0);
      for (uint32_t i = 0; i < desc->n_constrained; ++i)
        is_constrained[desc->constrained[i]] = 1;
      for (uint32_t i = 0; i < e.n_shared; ++i)
        if (is_constrained[e.shared[i]])
          return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: a constrained DoF is listed as shared; leave "
                                                "Dirichlet DoFs out of the exchange plan");
      for (int k = 0; k < e.n_neighbors; ++k)
        for (uint32_t i = 0; i < e.count[k]; ++i)
          if (is_constrained[e.index[k][i]])
            return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_operator_create: a constrained DoF is listed for exchange; "
                                                  "leave Dirichlet DoFs out of the exchange plan");
    }
    P->n_shared    = e.n_shared;
    P->n_not_owned = e.n_not_owned;
    P->not_owned_host.assign(e.not_owned, e.not_owned + e.n_not_owned);
    MGX_TRY(op.mem.upload(&P->shared_dev, e.shared, e.n_shared, 1));
    MGX_TRY(op.mem.upload(&P->not_owned_dev, e.not_owned, e.n_not_owned, 1));
    MGX_TRY(op.mem.alloc(&P->own_buf, es * (e.n_shared + 1)));
    // fused pack / ordered unpack tables
    if (e.n_neighbors <= 32 && e.n_neighbors < 255 && !tun.exchange_unfused)
      {
        P->start.assign(e.n_neighbors + 1, 0);
        for (int k = 0; k < e.n_neighbors; ++k)
          P->start[k + 1] = P->start[k] + e.count[k];
        const uint32_t        total = P->start.back();
        std::vector<uint32_t> all_index(total + 1, 0);
        std::vector<uint8_t>  all_seg(total + 1, 0);
        for (int k = 0; k < e.n_neighbors; ++k)
          for (uint32_t i = 0; i < e.count[k]; ++i)
            {
              all_index[P->start[k] + i] = e.index[k][i];
              all_seg[P->start[k] + i]   = (uint8_t)k;
            }
        // contributions per interface DoF in ascending rank order, own sum at self_pos
        std::vector<uint32_t> slot(desc->n_dofs, MGX_INVALID_INDEX);
        for (uint32_t j = 0; j < e.n_shared; ++j)
          slot[e.shared[j]] = j;
        std::vector<uint32_t> cnt(e.n_shared + 1, 0);
        bool                  ok = true;
        for (int k = 0; k < e.n_neighbors && ok; ++k)
          for (uint32_t i = 0; i < e.count[k]; ++i)
            {
              const uint32_t j = slot[e.index[k][i]];
              if (j == MGX_INVALID_INDEX)
                {
                  ok = false; // an exchanged DoF that is not in the shared list: keep the plain form
                  break;
                }
              cnt[j]++;
            }
        if (ok)
          {
            std::vector<uint32_t> cs(e.n_shared + 1, 0);
            for (uint32_t j = 0; j < e.n_shared; ++j)
              cs[j + 1] = cs[j] + cnt[j] + 1;
            std::vector<uint8_t>  ck(cs.back() + 1, 0);
            std::vector<uint32_t> cp(cs.back() + 1, 0), fill(cs.begin(), cs.end() - 1);
            for (int k = 0; k <= e.n_neighbors; ++k)
              {
                if (k == P->self_pos)
                  for (uint32_t j = 0; j < e.n_shared; ++j)
                    ck[fill[j]++] = 255;
                if (k < e.n_neighbors)
                  for (uint32_t i = 0; i < e.count[k]; ++i)
                    {
                      const uint32_t j = slot[e.index[k][i]];
                      ck[fill[j]]   = (uint8_t)k;
                      cp[fill[j]++] = i;
                    }
              }
            MGX_TRY(op.mem.upload(&P->all_index_dev, all_index));
            MGX_TRY(op.mem.upload(&P->all_seg_dev, all_seg));
            MGX_TRY(op.mem.upload(&P->csr_start_dev, cs));
            MGX_TRY(op.mem.upload(&P->csr_k_dev, ck));
            MGX_TRY(op.mem.upload(&P->csr_pos_dev, cp));
            P->fused = true;
          }
      }
    ctx->plans.push_back({(size_t)desc->n_dofs, P.get()});
    op.plan = std::move(P);
    return MGX_OK;
  }
} // namespace

extern "C" {

int mgx_operator_create(mgx_context_t ctx, const mgx_operator_desc *desc, mgx_operator_t *out)
{
  MGX_TRY(validate_operator_desc(ctx, desc, out));
  // failures below return through the destroy function, which frees what the operator's arena holds by then
  std::unique_ptr<mgx_operator_s, int (*)(mgx_operator_t)> op(new mgx_operator_s, mgx_operator_destroy);
  op->ctx              = ctx;
  op->constrained_last = constrained_are_last(desc);
  const Tunables &tun  = ctx->tun;
  const int       p = desc->degree, n = p + 1;
  const int       dim = desc_dim(desc);
  const size_t    n_entries = n_entities(dim) * (size_t)desc->n_cells;
  OperatorData   &d  = op->d;
  d.dim            = dim;
  d.p              = p;
  d.number         = desc->number;
  d.n_cells        = desc->n_cells;
  d.n_dofs         = desc->n_dofs;
  d.n_constrained  = desc->n_constrained;
  for (int i = 0; i < 6; ++i)
    d.coef[i] = desc->coef[i];
  std::memcpy(op->S, desc->shape_values, sizeof(double) * n * n);
  std::memcpy(op->D, desc->colloc_grad, sizeof(double) * n * n);
  std::memcpy(op->w, desc->qweights, sizeof(double) * n);
  d.full_tensor      = !desc->coef_q && (dim == 2 ? desc->coef[2] != 0. : (desc->coef[3] != 0. || desc->coef[4] != 0. || desc->coef[5] != 0.));
  const bool general = d.full_tensor || desc->coef_q; // quadrature-point operation with the full tensor
  d.separable        = !tun.general_kernel && !general;
  d.cells_form       = tun.cells_form;
  d.wide_max         = tun.wide_max;
  d.macro_wg_x16     = tun.macro_wg_x16;
  d.n_cus            = context_cus(ctx);
  d.macro_v2         = !tun.no_macro_v2;
  MGX_HIP(hipSetDevice(ctx->device));
  MGX_TRY(op->mem.upload(&d.idx27, desc->idx27, n_entries));
  if (desc->idx27_plain)
    MGX_TRY(op->mem.upload(&d.idx27_plain, desc->idx27_plain, n_entries));
  MGX_TRY(op->mem.upload(&d.constrained, desc->constrained, desc->n_constrained, 1));
  MGX_TRY(upload_basis(*op));
  MGX_TRY(op->mem.alloc(&d.inv_diag, number_size(d.number) * d.n_dofs));
  if (general)
    MGX_TRY(upload_general_tables(*op, desc));
  // (two dimensions: every form, the separable one too -- a level without the ordered assembly runs colour by colour,
  // never with atomics)
  if ((general || dim == 2) &&
      (desc->n_cells >= tun.cell_colour_min || n_local_values(dim, p) * desc->n_cells > kAssemblyMaxEntries))
    {
      MGX_TRY(colour_cells(*op, desc));
      if (dim == 2 && !d.cell_colours.order)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_operator_create: a two-dimensional level that needs more than 32 cell colours "
                                         "(and is too large for, or was told not to use, the ordered assembly)");
    }
  // (builds without the cell-by-cell cross-check kernels schedule bricks only where the macro-element
  // kernel runs: separable operator, vector below the 4 GB of a buffer descriptor)
  const bool macro_covers = d.separable && (uint64_t)desc->n_dofs * number_size(d.number) < 0xFFFFFFF0ull;
  if (dim == 3 && !tun.no_bricks && !general && (MGX_CELLS_FORM ? (p <= 4 || d.separable) : macro_covers))
    MGX_TRY(build_brick_schedule(*op, desc, tun));
  if (dim == 3 && general && p == 4 && !desc->exchange && !tun.no_bricks && !tun.no_general_bricks && desc->n_dofs < 0x3FFFFFFFu &&
      (uint64_t)desc->n_dofs * number_size(d.number) < 0xFFFFFFF0ull &&
      desc->n_cells / 64 >= tun.general_brick_min)
    MGX_TRY(build_general_brick_schedule(*op, desc));
  MGX_TRY(build_ordered_assembly(*op, desc));
  start_vector_statistics(*op, desc);
  if (desc->global_index)
    MGX_TRY(op->mem.upload(&op->global_index_dev, desc->global_index, desc->n_dofs));
  if (desc->exchange)
    MGX_TRY(build_exchange_plan(*op, desc, tun));
  *out = op.release();
  return MGX_OK;
}

int mgx_operator_exchange_buffers(mgx_operator_t op, int k, void **send, void **recv, uint32_t *count, int *rank)
{
  MGX_REQUIRE(op && op->plan && k >= 0 && k < (int)op->plan->rank.size(), "mgx_operator_exchange_buffers: bad argument");
  if (send)
    *send = op->plan->send[k];
  if (recv)
    *recv = op->plan->recv[k];
  if (count)
    *count = op->plan->count[k];
  if (rank)
    *rank = op->plan->rank[k];
  return MGX_OK;
}

int mgx_exchange_add(mgx_operator_t op, void *vec)
{
  MGX_REQUIRE(op && vec, "mgx_exchange_add: null argument");
  return exchange_add(op, vec);
}

int mgx_operator_destroy(mgx_operator_t op)
{
  if (!op)
    return MGX_OK;
  (void)hipStreamSynchronize(op->ctx->stream);
  if (op->plan)
    {
      ExchangePlan *P = op->plan.get();
      auto         &v = op->ctx->plans;
      v.erase(std::remove_if(v.begin(), v.end(), [P](const std::pair<size_t, ExchangePlan *> &x) { return x.second == P; }),
              v.end());
    }
  delete op;
  return MGX_OK;
}

uint32_t mgx_operator_n_dofs(mgx_operator_t op) { return op ? op->d.n_dofs : 0; }

int mgx_operator_set_profiled(mgx_operator_t op, int profiled)
{
  MGX_REQUIRE(op, "mgx_operator_set_profiled: null operator");
  op->profiled = profiled != 0;
  return MGX_OK;
}
int      mgx_operator_number(mgx_operator_t op) { return op ? op->d.number : -1; }
int      mgx_operator_dim(mgx_operator_t op) { return op ? op->d.dim : -1; }

int mgx_vmult(mgx_operator_t op, void *dst, const void *src)
{
  MGX_REQUIRE(op && dst && src, "mgx_vmult: null argument");
  MGX_REQUIRE(dst != src, "mgx_vmult: dst and src must not alias (laplace_operator.h:573-601)");
  hipStream_t s = op->ctx->stream;
  bool identity_done = false;
  MGX_TRY(apply_plain(op, dst, src, true, &identity_done));
  // dst[c] = src[c] on constrained rows (:592-593)
  if (!identity_done)
    launch_constrained_copy(s, op->d.number, dst, src, op->d.constrained, op->d.n_constrained);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_vmult_residual(mgx_operator_t op, const void *rhs, const void *lhs, void *res)
{
  MGX_REQUIRE(op && rhs && lhs && res, "mgx_vmult_residual: null argument");
  MGX_REQUIRE(res != lhs && res != rhs, "mgx_vmult_residual: residual must not alias rhs/lhs");
  hipStream_t s = op->ctx->stream;
  if (op->d.bricks.available())
    {
      // zeroing (:617-623) and rhs - A lhs (:624-631) are fused into the brick loop; interface
      // DoFs hold partial sums of A lhs: complete them, then rhs - (.)
      BrickLaunch l; // res = rhs - A lhs, the partial sums travel in res itself
      l.mode          = kResidual;
      l.src           = lhs;
      l.rhs           = rhs;
      l.out           = res;
      l.carrier       = res;
      l.free_schedule = op->d.bricks.fr.available();
      MGX_TRY(brick_loop_with_exchange(
        op, kResidual, res, [&](hipStream_t st, int g0, int g1) { launch_brick_loop(st, op->d, l.groups(g0, g1)); },
        [&](hipStream_t st) {
          launch_list_residual(st, op->d.number, res, rhs, op->plan->shared_dev, op->plan->n_shared);
        },
        l.free_schedule,
        [&](hipStream_t st, uint32_t first, uint32_t count) { launch_surf_finish(st, op->d, l, first, count); }));
    }
  else
    {
      MGX_TRY(apply_plain(op, res, lhs));
      launch_rhs_minus(s, op->d.number, res, rhs, op->d.n_dofs); // :624-631
    }
  // res[c] -= lhs[c] on constrained rows (:632-633); the loop never touches them
  launch_constrained_residual(s, op->d.number, res, rhs, lhs, op->d.constrained, op->d.n_constrained);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

/* LaplaceOperator::vmult_with_cg_update (laplace_operator.h:638-719) */
int mgx_vmult_with_cg_update(mgx_operator_t op, double alpha, double beta, const void *r, void *q, void *p, void *x,
                             void *scratch, double sums[4])
{
  MGX_REQUIRE(op && r && q && p && x && sums, "mgx_vmult_with_cg_update: null argument");
  MGX_REQUIRE(q != p && q != x && p != x && r != q && r != p && r != x, "mgx_vmult_with_cg_update: vectors must not alias");
  mgx_context_t ctx = op->ctx;
  hipStream_t   s   = ctx->stream;
  const int     num = op->d.number;
  const size_t  n   = op->d.n_dofs;
  constexpr uint32_t kCapacity = 1u << 16; // quadruples
  if (!op->cg_partials)
    {
      MGX_TRY(op->mem.alloc(&op->cg_partials, 4 * (size_t)kCapacity));
      MGX_TRY(op->mem.alloc(&op->cg_result, 4));
    }
  bool fused = op->d.bricks.available() && op->d.separable && op->d.bricks.item_map && !op->plan;
  if (fused)
    {
      // the brick loop reads q (the preconditioned residual) while neighbouring bricks already hold
      // partial sums of the new q = A p: those travel in a separate carrier vector
      void *carrier = scratch;
      if (!carrier)
        {
          if (!op->cg_carrier)
            MGX_TRY(op->mem.alloc(&op->cg_carrier, number_size(num) * n));
          carrier = op->cg_carrier;
        }
      uint32_t used = 0;
      {
        ProfileBracket pb(op, kCgUpdate);
        fused = num == MGX_F64 ? launch_macro_cg_update_f64(s, op->d, alpha, beta, r, q, p, x, carrier, op->cg_partials,
                                                            kCapacity - 2048, &used)
                               : launch_macro_cg_update_f32(s, op->d, alpha, beta, r, q, p, x, carrier, op->cg_partials,
                                                            kCapacity - 2048, &used);
      }
      if (fused)
        {
          // constrained rows: the vector updates of the before-loop hook; the cell loop leaves q = 0 there
          used += launch_cg_list_update(s, num, op->d.constrained, op->d.n_constrained, alpha, beta, r, q, p, x,
                                        op->cg_partials + 4 * (size_t)used);
          launch_reduce4(s, op->cg_partials, used, nullptr, op->cg_result);
          MGX_HIP(hipMemcpyAsync(sums, op->cg_result, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
          MGX_HIP(hipStreamSynchronize(s));
          MGX_HIP(hipGetLastError());
          return MGX_OK;
        }
    }
  // levels without the fused kernel / decomposed meshes: the same operations one after the other
  launch_cg_pre(s, num, x, p, q, alpha, beta, n);
  MGX_TRY(apply_plain(op, q, p)); // constrained rows stay zero, as in the reference's cell loop
  if (!ctx->has_comm)
    {
      const uint32_t used = launch_dot4(s, num, q, p, r, n, op->cg_partials);
      launch_reduce4(s, op->cg_partials, used, nullptr, op->cg_result);
      MGX_HIP(hipMemcpyAsync(sums, op->cg_result, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
      MGX_HIP(hipStreamSynchronize(s));
    }
  else
    {
      MGX_TRY(dot(ctx, num, q, p, n, &sums[0], op->plan.get()));
      MGX_TRY(dot(ctx, num, r, r, n, &sums[1], op->plan.get()));
      MGX_TRY(dot(ctx, num, q, r, n, &sums[2], op->plan.get()));
      MGX_TRY(dot(ctx, num, q, q, n, &sums[3], op->plan.get()));
    }
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

// Cells of a brick level in launches whose cells share no DoF (mgx::brick_cell_lists: 64 lists); plain adds in an order
// that does not depend on the run.
// The cells go to the device, into memory of `mem` (the caller's: it outlives the launches), the offsets to `list_start`.
static int upload_brick_cell_lists(mgx_operator_t op, DeviceArena &mem, std::vector<uint32_t> &list_start, CellLists &out)
{
  const BrickData &bd = op->d.bricks;
  // (cells per brick: 64 or 8)
  IndexRows built = brick_cell_lists(bd.order.data(), bd.colour_start, bd.n_colours, op->d.n_cells / bd.n_bricks);
  const std::vector<uint32_t> &lists = built.pos;
  list_start.swap(built.start);
  hipStream_t s         = op->ctx->stream;
  uint32_t   *lists_dev = nullptr;
  MGX_TRY(mem.alloc(&lists_dev, lists.size() + 1));
  MGX_HIP(hipMemcpyAsync(lists_dev, lists.data(), sizeof(uint32_t) * lists.size(), hipMemcpyHostToDevice, s));
  MGX_HIP(hipStreamSynchronize(s)); // (`lists` is pageable host memory in flight until here)
  out = CellLists(lists_dev, list_start.data(), (int)list_start.size() - 1);
  return MGX_OK;
}

int mgx_compute_residual(mgx_operator_t op, void *dst, const void *src, const void *rhs_q)
{
  MGX_REQUIRE(op && dst, "mgx_compute_residual: null argument");
  MGX_REQUIRE(dst != src, "mgx_compute_residual: dst and src must not alias");
  MGX_TRY(refuse_2d(op->d, "mgx_compute_residual", "right-hand sides of a two-dimensional problem are assembled on the host"));
  // (the boundary values are gathered through the table that also names the constrained DoFs)
  MGX_REQUIRE(op->d.idx27_plain, "mgx_compute_residual: the operator was created without idx27_plain");
  hipStream_t  s     = op->ctx->stream;
  const size_t bytes = number_size(op->d.number) * op->d.n_dofs;
  // temporaries of this call, released on every path out of it (after the stream has drained)
  DeviceArena tmp("mgx_compute_residual");
  tmp.drain_before_release(s);
  if (!src) // homogeneous boundary values
    {
      void *zero = nullptr;
      MGX_TRY(tmp.zeros(&zero, bytes, s));
      src = zero;
    }
  MGX_HIP(hipMemsetAsync(dst, 0, bytes, s));
  // assembly without atomics, as for the diagonal (mgx_compute_diagonal): brick lists, then the cell colours -- only
  // where there is no ordered assembly --, then the ordered assembly (or atomics)
  std::vector<uint32_t> list_start;
  CellLists             lists;
  if (op->d.bricks.available())
    MGX_TRY(upload_brick_cell_lists(op, tmp, list_start, lists));
  else if (op->d.cell_colours.order && !op->d.asm_start)
    lists = op->d.cell_colours.lists();
  launch_cell_residual(s, op->d, dst, src, rhs_q, lists);
  MGX_HIP(hipGetLastError());
  return exchange_add(op, dst); // dst.compress(add), laplace_operator.h:843
}

/* ------------------------------------------------------------------------------------------
 * Solution-dependent coefficient of the general branch (MinimalSurfaceOperator, minimal_surface/program.cc:103-200)
 * ------------------------------------------------------------------------------------------ */
// the operator of a solution-dependent coefficient has a per-point tensor
static int require_coef_q(mgx_operator_t op, const char *who)
{
  if (op->d.coef_q)
    return MGX_OK;
  return fail(MGX_ERR_UNSUPPORTED, std::string(who) + ": the operator has no per-point coefficient (separable or "
                                     "one-tensor-per-mesh branch); create it with mgx_operator_desc::coef_q set, e.g. to the "
                                     "unit-law tensor JxW_q J^-1 J^-T");
}

// an affine geometry replaces a per-point one, which a kernel in flight may read
static int release_point_geometry(mgx_operator_t op)
{
  if (op->unit_q)
    {
      MGX_HIP(hipStreamSynchronize(op->ctx->stream));
      op->mem.release(op->unit_q);
      op->mem.release(op->jxw_q);
      op->unit_q = op->jxw_q = nullptr;
    }
  return MGX_OK;
}

// per-point geometry: unit_q [n_cells][n_tensor][n_q] = JxW_q J^-1 J^-T with a positive diagonal, jxw_q [n_cells][n_q] > 0
static int set_point_geometry(mgx_operator_t op, const double *unit_q, const double *jxw_q, const char *who)
{
  MGX_TRY(require_coef_q(op, who));
  const size_t nq = n_local_values(op->d.dim, op->d.p), nc = op->d.n_cells, nt = (size_t)n_tensor_entries(op->d.dim);
  const size_t nd = (size_t)op->d.dim; // the diagonal entries come first: [xx,yy,zz,...] / [xx,yy,xy]
  bool         ok = true;
  for (size_t c = 0; c < nc && ok; ++c)
    for (size_t q = 0; q < nq && ok; ++q)
      {
        ok = jxw_q[c * nq + q] > 0.; // (false for NaN)
        for (size_t k = 0; k < nd && ok; ++k)
          ok = unit_q[(c * nt + k) * nq + q] > 0.;
      }
  MGX_REQUIRE(ok, std::string(who) + ": JxW_q and the diagonal of JxW_q J^-1 J^-T must be positive at every quadrature point");
  // (a failed upload leaves the new arrays to the operator's arena and the present geometry in place)
  void *u_dev = nullptr, *w_dev = nullptr;
  MGX_TRY(op->mem.upload_as(op->d.number, &u_dev, unit_q, nc * nt * nq));
  MGX_TRY(op->mem.upload_as(op->d.number, &w_dev, jxw_q, nc * nq));
  MGX_HIP(hipStreamSynchronize(op->ctx->stream)); // a kernel in flight may read the geometry this call replaces
  op->mem.release(op->unit_q);
  op->mem.release(op->jxw_q);
  op->unit_q      = u_dev;
  op->jxw_q       = w_dev;
  op->coef_update = true;
  return MGX_OK;
}

// affine geometry: M = J^-1 J^-T ([xx,yy,zz,xy,xz,yz] / [xx,yy,xy]) is symmetric positive definite (leading minors), det J > 0
static int set_affine_geometry(mgx_operator_t op, const double *metric, double det_jacobian, const char *who)
{
  MGX_TRY(require_coef_q(op, who));
  double m[6] = {0, 0, 0, 0, 0, 0};
  std::copy(metric, metric + n_tensor_entries(op->d.dim), m);
  bool ok = det_jacobian > 0. && m[0] > 0.;
  if (op->d.dim == 2)
    ok = ok && m[0] * m[1] - m[2] * m[2] > 0.;
  else
    ok = ok && m[0] * m[1] - m[3] * m[3] > 0. &&
         m[0] * (m[1] * m[2] - m[5] * m[5]) - m[3] * (m[3] * m[2] - m[5] * m[4]) + m[4] * (m[3] * m[5] - m[1] * m[4]) > 0.;
  MGX_REQUIRE(ok, std::string(who) + ": the metric must be positive definite and det J > 0");
  MGX_TRY(release_point_geometry(op));
  std::copy(m, m + 6, op->metric);
  op->det_jacobian = det_jacobian;
  op->coef_update  = true;
  return MGX_OK;
}

static int refuse_3d(mgx_operator_t op, const char *who, const char *instead)
{
  if (op->d.dim == 2)
    return MGX_OK;
  return fail(MGX_ERR_UNSUPPORTED, std::string(who) + ": not on a three-dimensional operator (call " + instead + ")");
}

/* LaplaceOperator<2,...>::compute_residual (laplace_operator.h:804-845): mgx_compute_residual with (p+1)^2 points per cell.
 * The cells are added up as every two-dimensional result is -- the ordered assembly or the cell colours, never atomics. */
int mgx_compute_residual_2d(mgx_operator_t op, void *dst, const void *src, const void *rhs_q)
{
  MGX_REQUIRE(op && dst, "mgx_compute_residual_2d: null argument");
  MGX_REQUIRE(dst != src, "mgx_compute_residual_2d: dst and src must not alias");
  MGX_TRY(refuse_3d(op, "mgx_compute_residual_2d", "mgx_compute_residual"));
  // (the boundary values are gathered through the table that also names the constrained DoFs)
  MGX_REQUIRE(op->d.idx27_plain, "mgx_compute_residual_2d: the operator was created without idx27_plain");
  hipStream_t  s     = op->ctx->stream;
  const size_t bytes = number_size(op->d.number) * op->d.n_dofs;
  // temporaries of this call, released on every path out of it (after the stream has drained)
  DeviceArena tmp("mgx_compute_residual_2d");
  tmp.drain_before_release(s);
  if (!src) // homogeneous boundary values
    {
      void *zero = nullptr;
      MGX_TRY(tmp.zeros(&zero, bytes, s));
      src = zero;
    }
  if (!op->d.asm_start) // the cell colours add to dst; the ordered assembly writes it
    MGX_HIP(hipMemsetAsync(dst, 0, bytes, s));
  launch_cell_residual_2d(s, op->d, dst, src, rhs_q);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

/* MultigridSolver<2,...>::compute_l2_error (multigrid_solver.h:298-343) against a function given at the quadrature
 * points: sums = { sum (u_h - u_q)^2 JxW_q, sum JxW_q }, formed in fp64 in a fixed order */
int mgx_compute_l2_error_2d(mgx_operator_t op, const void *vec, const void *u_q, const void *jxw_q, double sums[2])
{
  MGX_REQUIRE(op && vec && u_q && jxw_q && sums, "mgx_compute_l2_error_2d: null argument");
  MGX_TRY(refuse_3d(op, "mgx_compute_l2_error_2d", "the host's error evaluation, mgx_cube_l2_error"));
  MGX_REQUIRE(op->d.idx27_plain, "mgx_compute_l2_error_2d: the operator was created without idx27_plain");
  hipStream_t    s  = op->ctx->stream;
  const uint32_t nb = l2_error_grid_2d(op->d.p, op->d.n_cells);
  DeviceArena    tmp("mgx_compute_l2_error_2d");
  tmp.drain_before_release(s);
  double *partials = nullptr, *result = nullptr;
  MGX_TRY(tmp.alloc(&partials, 4 * (size_t)nb));
  MGX_TRY(tmp.alloc(&result, 4));
  launch_l2_error_2d(s, op->d, vec, u_q, jxw_q, partials);
  launch_reduce4(s, partials, nb, nullptr, result);
  MGX_HIP(hipGetLastError());
  double host[4];
  MGX_HIP(hipMemcpyAsync(host, result, sizeof(host), hipMemcpyDeviceToHost, s));
  MGX_HIP(hipStreamSynchronize(s));
  sums[0] = host[0], sums[1] = host[1];
  return MGX_OK;
}

/* MinimalSurfaceOperator<2,...>::initialize (minimal_surface/program.cc:112-117 with dimension = 2, :73): the mapping data
 * evaluate_coefficient and compute_residual read, for affine cells */
int mgx_operator_enable_coefficient_update_2d(mgx_operator_t op, const double metric[3], double det_jacobian)
{
  MGX_REQUIRE(op && metric, "mgx_operator_enable_coefficient_update_2d: null argument");
  MGX_TRY(refuse_3d(op, "mgx_operator_enable_coefficient_update_2d", "mgx_operator_enable_coefficient_update"));
  return set_affine_geometry(op, metric, det_jacobian, "mgx_operator_enable_coefficient_update_2d");
}

/* the same for curved cells: the per-point mapping data of MatrixFree<2> (minimal_surface/program.cc:125-131, inverse_jacobian
 * and JxW of every quadrature point) */
int mgx_operator_enable_coefficient_update_q_2d(mgx_operator_t op, const double *unit_q, const double *jxw_q)
{
  MGX_REQUIRE(op && unit_q && jxw_q, "mgx_operator_enable_coefficient_update_q_2d: null argument");
  MGX_TRY(refuse_3d(op, "mgx_operator_enable_coefficient_update_q_2d", "mgx_operator_enable_coefficient_update_q"));
  return set_point_geometry(op, unit_q, jxw_q, "mgx_operator_enable_coefficient_update_q_2d");
}

int mgx_operator_enable_coefficient_update(mgx_operator_t op, const double metric[6], double det_jacobian)
{
  MGX_REQUIRE(op && metric, "mgx_operator_enable_coefficient_update: null argument");
  MGX_TRY(refuse_2d(op->d, "mgx_operator_enable_coefficient_update",
                    "the arrays of this call are three-dimensional: call mgx_operator_enable_coefficient_update_2d"));
  return set_affine_geometry(op, metric, det_jacobian, "mgx_operator_enable_coefficient_update");
}

int mgx_operator_enable_coefficient_update_q(mgx_operator_t op, const double *unit_q, const double *jxw_q)
{
  MGX_REQUIRE(op && unit_q && jxw_q, "mgx_operator_enable_coefficient_update_q: null argument");
  MGX_TRY(refuse_2d(op->d, "mgx_operator_enable_coefficient_update_q",
                    "the arrays of this call are three-dimensional: call mgx_operator_enable_coefficient_update_q_2d"));
  return set_point_geometry(op, unit_q, jxw_q, "mgx_operator_enable_coefficient_update_q");
}

static int require_coefficient_update(mgx_operator_t op, int law, const char *who)
{
  const std::string w(who);
  MGX_REQUIRE(law == MGX_LAW_UNIT || law == MGX_LAW_MINIMAL_SURFACE, w + ": unknown law");
  if (op->ctx->has_comm || op->plan)
    return fail(MGX_ERR_UNSUPPORTED, w + ": not on a decomposed mesh (single rank only)");
  // (a two-dimensional operator that was not enabled: the refusal every 2D operator met before the _2d calls existed)
  if (op->d.dim == 2 && !op->coef_update)
    return fail(MGX_ERR_UNSUPPORTED, w + ": not on a two-dimensional operator without a geometry: call "
                                         "mgx_operator_enable_coefficient_update_2d (affine cells) or "
                                         "mgx_operator_enable_coefficient_update_q_2d (curved cells) first");
  MGX_REQUIRE(op->coef_update, w + ": call mgx_operator_enable_coefficient_update (affine geometry of the level) or "
                                   "mgx_operator_enable_coefficient_update_q (curved cells) first");
  MGX_REQUIRE(op->d.idx27_plain, w + ": the operator was created without idx27_plain (the state is read with its boundary values)");
  return MGX_OK;
}

int mgx_evaluate_coefficient(mgx_operator_t op, int law, const void *state)
{
  MGX_REQUIRE(op && state, "mgx_evaluate_coefficient: null argument");
  MGX_TRY(require_coefficient_update(op, law, "mgx_evaluate_coefficient"));
  launch_evaluate_coefficient(op->ctx->stream, op->d, op->d.coef_q, op->d.number, law == MGX_LAW_MINIMAL_SURFACE, op->metric,
                              op->det_jacobian, op->unit_q, op->jxw_q, state);
  MGX_HIP(hipGetLastError());
  op->has_diag = false; // the inverse diagonal belongs to the previous coefficient
  return MGX_OK;
}

int mgx_operator_get_coefficient(mgx_operator_t op, const void **dptr, size_t *n)
{
  MGX_REQUIRE(op && dptr && n, "mgx_operator_get_coefficient: null argument");
  if (!op->d.coef_q)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_operator_get_coefficient: the operator has no per-point coefficient");
  *dptr = op->d.coef_q;
  *n    = (size_t)op->d.n_cells * n_tensor_entries(op->d.dim) * n_local_values(op->d.dim, op->d.p);
  return MGX_OK;
}

int mgx_compute_nonlinear_residual(mgx_operator_t op, int law, void *dst, const void *state)
{
  MGX_REQUIRE(op && dst && state, "mgx_compute_nonlinear_residual: null argument");
  MGX_REQUIRE(dst != state, "mgx_compute_nonlinear_residual: dst and state must not alias");
  MGX_TRY(require_coefficient_update(op, law, "mgx_compute_nonlinear_residual"));
  hipStream_t s  = op->ctx->stream;
  const bool  ms = law == MGX_LAW_MINIMAL_SURFACE;
  // atomic-free assembly only: the ordered assembly where the level has it, else colour by colour
  if (!op->d.asm_start && !op->d.cell_colours.order)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_compute_nonlinear_residual: the level has neither cell colours nor the ordered-assembly "
                                     "tables (more than 32 colours): no reproducible assembly");
  CellLists lists; // none: the ordered assembly, which comes first where the level has it (dst is written)
  if (!op->d.asm_start) // the cell colours: dst is added to
    {
      MGX_HIP(hipMemsetAsync(dst, 0, number_size(op->d.number) * op->d.n_dofs, s));
      lists = op->d.cell_colours.lists();
    }
  launch_cell_nl_residual(s, op->d, ms, op->metric, op->det_jacobian, op->unit_q, op->jxw_q, dst, state, lists);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_compute_diagonal(mgx_operator_t op)
{
  MGX_REQUIRE(op, "mgx_compute_diagonal: null argument");
  hipStream_t s = op->ctx->stream;
  const int   n = op->d.p + 1;
  // 1D diagonal factors: G = D*S is the gradient of the nodal basis at the quadrature points
  double a1d[kMaxN], m1d[kMaxN];
  double G[kMaxN * kMaxN];
  nodal_gradient(*op, G);
  for (int i = 0; i < n; ++i)
    {
      double a = 0, m = 0;
      for (int q = 0; q < n; ++q)
        {
          const double g = G[q * n + i];
          a += op->w[q] * g * g;
          m += op->w[q] * op->S[q * n + i] * op->S[q * n + i];
        }
      a1d[i] = a;
      m1d[i] = m;
    }
  MGX_HIP(hipMemsetAsync(op->d.inv_diag, 0, number_size(op->d.number) * op->d.n_dofs, s));
  // The cell contributions are added up without atomics, in an order that does not depend on the run:
  // brick levels colour by colour (bricks of one launch group share no DoF; inside a brick the cells
  // with the same position m mod 8 in Morton order -- the same child of every parent -- do not touch),
  // cell-coloured levels colour by colour, the others through the ordered assembly (or with atomics).
  DeviceArena lists_mem("mgx_compute_diagonal");
  lists_mem.drain_before_release(s);
  std::vector<uint32_t> list_start;
  CellLists             lists;
  if (op->d.bricks.available())
    MGX_TRY(upload_brick_cell_lists(op, lists_mem, list_start, lists));
  else if (op->d.cell_colours.order)
    lists = op->d.cell_colours.lists();
  launch_cell_diagonal(s, op->d, op->d.inv_diag, a1d, m1d, lists);
  MGX_TRY(exchange_add(op, op->d.inv_diag)); // Vector::compress(add) of the reference's cell_loop
  // set_constrained_entries_to_one + invert (laplace_operator.h:757-765)
  launch_constrained_set(s, op->d.number, op->d.inv_diag, 1.0, op->d.constrained, op->d.n_constrained);
  launch_invert(s, op->d.number, op->d.inv_diag, op->d.n_dofs);
  MGX_HIP(hipGetLastError());
  op->has_diag = true;
  // Is the diagonal the same for every brick (uniform mesh)?  Then the macro-element kernel keeps
  // it in registers instead of streaming it (mgx_macro.hip, DTAB).  MGX_NO_DIAG_TABLE=1: A/B timing.
  for (int which = 0; which < 2; ++which) // the table in the item order of either pipeline of the macro-element kernel
    {
      void          *&slot = which == 0 ? op->d.diag_items : op->d.diag_items2;
      const uint32_t *map  = which == 0 ? op->d.bricks.item_map : op->d.bricks.item_map2;
      op->mem.release(slot);
      slot = nullptr;
      if (!map || !op->d.separable || op->ctx->tun.no_diag_table)
        continue;
      const uint32_t nb = op->d.p <= 4 ? 4 : 2, g = nb * op->d.p + 1, npts = g * g * g;
      DeviceArena    tmp("mgx_compute_diagonal");
      void          *table = nullptr;
      uint32_t      *flag  = nullptr, mismatch = 1;
      MGX_TRY(op->mem.zeros(&table, number_size(op->d.number) * npts, s));
      MGX_TRY(tmp.zeros(&flag, 1, s));
      if (op->d.number == MGX_F64)
        macro_diag_table_f64(s, op->d, map, table, flag);
      else
        macro_diag_table_f32(s, op->d, map, table, flag);
      MGX_HIP(hipMemcpyAsync(&mismatch, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      MGX_HIP(hipStreamSynchronize(s));
      if (mismatch == 0)
        slot = table;
      else
        op->mem.release(table);
      if (which == 0)
        MGX_TRACE("compute_diagonal: diagonal %s per brick item", mismatch == 0 ? "uniform" : "not uniform");
    }
  return MGX_OK;
}

int mgx_get_inverse_diagonal(mgx_operator_t op, const void **dptr)
{
  MGX_REQUIRE(op && dptr, "mgx_get_inverse_diagonal: null argument");
  MGX_REQUIRE(op->has_diag, "mgx_get_inverse_diagonal: call mgx_compute_diagonal first");
  *dptr = op->d.inv_diag;
  return MGX_OK;
}

/* ------------------------------------------------------------------------------------------
 * PreconditionChebyshev
 * ------------------------------------------------------------------------------------------ */
int mgx_smoother_create(mgx_operator_t op, double smoothing_range, int degree, int eig_cg_n_iterations,
                        mgx_smoother_t *out)
{
  MGX_REQUIRE(op && out, "mgx_smoother_create: null argument");
  MGX_REQUIRE(eig_cg_n_iterations > 2, "mgx_smoother_create: eig_cg_n_iterations must be > 2");
  if (!op->has_diag)
    MGX_TRY(mgx_compute_diagonal(op));
  mgx_context_t ctx = op->ctx;
  hipStream_t   s   = ctx->stream;
  const int     num = op->d.number;
  const size_t  n   = op->d.n_dofs, bytes = number_size(num) * n;
  std::unique_ptr<mgx_smoother_s, int (*)(mgx_smoother_t)> sm(new mgx_smoother_s, mgx_smoother_destroy);
  sm->op            = op;
  sm->req_range     = smoothing_range;
  sm->req_degree    = degree;
  sm->req_eig_its   = eig_cg_n_iterations;
  MGX_TRY(sm->mem.alloc(&sm->x_old, bytes));
  MGX_TRY(sm->mem.alloc(&sm->tmp, bytes));
  // estimate_eigenvalues: PCG(D^-1) on v_i = (i mod 11) - mean; Lanczos tridiagonal
  void       *r = nullptr, *z = nullptr, *d = nullptr, *h = sm->tmp, *x = sm->x_old;
  DeviceArena scratch("mgx_smoother_create");
  for (void **v : {&r, &z, &d})
    MGX_TRY(scratch.alloc(v, bytes));
  {
    // deal.II: v_i = (global index of i) mod 11 minus the global mean
    double sc[2] = {op->start_sum, op->start_count};
    MGX_TRY(comm_allreduce(ctx, sc, 2));
    launch_index_mod11(s, num, r, op->global_index_dev, sc[0] / sc[1], n);
  }
  MGX_HIP(hipMemsetAsync(x, 0, bytes, s));
  double res = 0;
  MGX_TRY(mgx_operator_l2_norm(op, r, &res));
  MGX_TRACE("smoother_create: n=%zu eig_its=%d res0=%g", n, eig_cg_n_iterations, res);
  const auto jacobi = [&](double *rz) {
    launch_jacobi_dot(s, num, z, op->d.inv_diag, r, n, ctx->partial_dev, ctx->result_dev);
    return fused_sum(op, r, z, rz);
  };
  CGOps<decltype(jacobi)> ops{op, x, r, z, d, h, jacobi};
  mgx_smoother_info      &info = sm->info; // IterationNumberControl(n_its, 1e-10), extreme Ritz values by bisection
  MGX_TRY(krylov::lanczos_estimate(ops, res, eig_cg_n_iterations, krylov::RitzRule{}, info));
  MGX_HIP(hipStreamSynchronize(s));
  const double a = krylov::chebyshev_interval(smoothing_range, degree, info);
  MGX_TRACE("smoother_create: its=%d lambda=[%g,%g] degree=%d", info.cg_iterations, info.lambda_min, info.lambda_max, info.degree);
  sm->range_a = a;
  *out        = sm.release();
  return MGX_OK;
}

int mgx_smoother_destroy(mgx_smoother_t sm)
{
  if (!sm)
    return MGX_OK;
  (void)hipStreamSynchronize(sm->op->ctx->stream);
  delete sm;
  return MGX_OK;
}

int mgx_smoother_get_info(mgx_smoother_t sm, mgx_smoother_info *info)
{
  MGX_REQUIRE(sm && info, "mgx_smoother_get_info: null argument");
  *info = sm->info;
  return MGX_OK;
}

int mgx_smoother_set_polynomial_type(mgx_smoother_t sm, int polynomial_type)
{
  MGX_REQUIRE(sm, "mgx_smoother_set_polynomial_type: null smoother");
  MGX_REQUIRE(polynomial_type == MGX_CHEBYSHEV_FIRST_KIND || polynomial_type == MGX_CHEBYSHEV_FOURTH_KIND,
              "mgx_smoother_set_polynomial_type: unknown polynomial type");
  sm->fourth_kind = polynomial_type == MGX_CHEBYSHEV_FOURTH_KIND;
  sm->info.delta  = sm->fourth_kind ? sm->info.lambda_max : (sm->info.lambda_max - sm->range_a) * 0.5;
  return MGX_OK;
}

// Levels without a brick schedule, ordered assembly on one rank with the constrained DoFs last: the update is the
// post-operation of the assembly kernel (two launches per iteration instead of three on levels that are launch-bound)
static bool cheb_in_assembly(mgx_operator_t op)
{
  return op->d.asm_start && !op->plan && op->constrained_last && !op->ctx->tun.no_fused_assembly;
}

static void cheb_assembly_iteration(mgx_smoother_t sm, void *x, const void *b, double f1, double f2, bool three_term)
{
  mgx_operator_t op = sm->op;
  ProfileBracket pb(op, three_term ? kCheb : kChebFirst);
  const ChebPost post{sm->x_old, b, op->d.inv_diag, f1, f2, three_term};
  launch_cell_loop(op->ctx->stream, op->d, x, x, nullptr, op->d.n_dofs - op->d.n_constrained, &post);
}

// legacy path (levels without a brick schedule): matvec into tmp, then an elementwise update
static int cheb_loop(mgx_smoother_t sm, void *x, const void *b)
{
  const mgx_smoother_info &I = sm->info;
  mgx_operator_t           op = sm->op;
  hipStream_t              s  = op->ctx->stream;
  if (I.degree < 2 || std::fabs(I.delta) < 1e-40)
    return MGX_OK;
  krylov::ChebyshevFactors F = sm->factors();
  for (int k = 0; k < I.degree - 1; ++k)
    {
      double f1, f2;
      F.next(k, f1, f2);
      if (cheb_in_assembly(op))
        {
          cheb_assembly_iteration(sm, x, b, f1, f2, true);
          continue;
        }
      MGX_TRY(mgx_vmult(op, sm->tmp, x));
      launch_cheb_update(s, op->d.number, kUpdateThreeTerm, x, sm->x_old, b, sm->tmp, op->d.inv_diag, f1, f2, op->d.n_dofs);
    }
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

// One fused Chebyshev iteration on a brick-scheduled level (the counterpart of
// LaplaceOperator::vmult(dst, src, before, after), laplace_operator.h:723-741, with
// PreconditionChebyshev's update as the after-operation):
//   out <- cur + f1 (cur - out) + f2 D^-1 (b - A cur);  kCheb general, kChebFirst without the f1 term,
//   kChebZeroOld with out == 0 on entry.  sm->tmp carries the partial sums of brick-surface DoFs.
static int cheb_fused_iteration(mgx_smoother_t sm, BrickMode mode, const void *cur, const void *old, void *out,
                                const void *b, double f1, double f2, double f0 = 0., const void *coarse = nullptr,
                                const uint32_t *coarse_blocks = nullptr, const TransferData *prolong_tr = nullptr)
{
  mgx_operator_t op = sm->op;
  hipStream_t    s  = op->ctx->stream;
  BrickLaunch l;
  l.mode          = mode;
  l.src           = cur;
  l.rhs           = b;
  l.dinv          = op->d.inv_diag;
  l.old           = old;
  l.out           = out;
  l.carrier       = sm->tmp;
  l.f0            = f0;
  l.f1            = f1;
  l.f2            = f2;
  l.coarse        = const_cast<void *>(coarse);
  l.coarse_blocks = coarse_blocks;
  l.free_schedule = op->d.bricks.fr.available() && on_free_schedule(mode);
  // (reduced-colour schedule on one rank: the update of the constrained rows rides on the finish kernel)
  const bool folded = l.free_schedule && !op->plan;
  // the interface DoFs' partial sums of A cur sit in sm->tmp: complete them and apply the update there.  Decomposed:
  // interface DoFs and constrained rows are updated by the unpack launch of the exchange where the plan allows (post)
  bool post_done = false;
  MGX_TRY(brick_loop_with_exchange(
    op, mode, sm->tmp, [&](hipStream_t st, int g0, int g1) { launch_brick_loop(st, op->d, l.groups(g0, g1)); },
    [&](hipStream_t st) {
      if (mode == kChebFirstProlong) // the shared DoFs start from x + P x_coarse as well (and store it: x_old of the next iteration)
        launch_interface_prolong_cheb(st, op->d.number, *prolong_tr, op->plan->shared_dev, coarse, const_cast<void *>(cur), out, b,
                                      op->d.inv_diag, f2, sm->tmp);
      else
        launch_cheb_constrained(st, op->d.number, mode, cur, out, b, op->d.inv_diag, f1, f2, op->plan->shared_dev,
                                op->plan->n_shared, sm->tmp, old, f0);
    },
    l.free_schedule,
    [&](hipStream_t st, uint32_t first, uint32_t count) {
      // one rank: one call for the whole surface list, which takes the constrained rows along
      launch_surf_finish(st, op->d, l, first, count, folded ? op->d.constrained : nullptr, folded ? op->d.n_constrained : 0u);
    },
    (op->plan && mode != kChebFirstProlong && !op->ctx->tun.exchange_unfused) ? &l : nullptr, &post_done));
  if (!folded && !post_done)
    launch_cheb_constrained(s, op->d.number, mode, cur, out, b, op->d.inv_diag, f1, f2, op->d.constrained,
                            op->d.n_constrained, nullptr, old, f0);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

// vmult (zero start) / step (nonzero start) on a brick-scheduled level.  Every fused iteration
// reads the current iterate (gathered by the cell loop) and x_old, and writes the new iterate into
// a buffer that is not the current one.  The targets rotate over the caller's vector X and the
// smoother's buffers Y (and Z for an odd number of iterations from a nonzero start) such that the
// LAST iterate lands in X: no pointer swap (deal.II swaps solution/solution_old) and no copy, and
// all pointers stay fixed from call to call (which lets the coarse part of the V-cycle be
// replayed as a HIP graph).
// prolong_coarse / prolong_blocks (step only): the coarse-grid correction P x_coarse is added to x on
// the fly by the first iteration (kChebFirstProlong) instead of by a prolongation kernel before the call
static int smoother_apply(mgx_smoother_t sm, void *x, const void *b, bool is_step, const void *prolong_coarse = nullptr,
                          const uint32_t *prolong_blocks = nullptr, const TransferData *prolong_tr = nullptr)
{
  const mgx_smoother_info &I  = sm->info;
  mgx_operator_t           op = sm->op;
  hipStream_t              s  = op->ctx->stream;
  const int                num = op->d.number;
  const size_t             n   = op->d.n_dofs;
  // levels without a brick schedule: matvec + elementwise update
  if (!op->d.bricks.available())
    {
      if (is_step && cheb_in_assembly(op))
        cheb_assembly_iteration(sm, x, b, 0., sm->factors().first(), false);
      else if (is_step)
        {
          MGX_TRY(mgx_vmult(op, sm->tmp, x));
          launch_cheb_update(s, num, kUpdateFirst, x, sm->x_old, b, sm->tmp, op->d.inv_diag, 0., sm->factors().first(), n);
        }
      else
        launch_cheb_update(s, num, kUpdateStart, x, sm->x_old, b, nullptr, op->d.inv_diag, 0., sm->factors().first(), n);
      return cheb_loop(sm, x, b);
    }
  const bool three_term = I.degree >= 2 && std::fabs(I.delta) >= 1e-40;
  const int  n_loop     = three_term ? I.degree - 1 : 0; // iterations of the three-term recurrence
  void      *X = x, *Y = sm->x_old;
  if (!is_step && n_loop >= 1 && op->d.separable && !op->ctx->tun.no_fused_init)
    {
      // Zero initial guess: x_1 = (1/theta) D^-1 b is not stored.  The first loop iteration
      // evaluates it while gathering (kChebInit), the second one again as its x_old (kChebOldInit); from the
      // third on both operands are stored iterates.  Targets alternate so that the last is X.
      const double f0   = sm->factors().first();
      krylov::ChebyshevFactors F = sm->factors();
      void        *cur = nullptr, *old = nullptr;
      for (int k = 0; k < n_loop; ++k)
        {
          double f1, f2;
          F.next(k, f1, f2);
          void *out = ((n_loop - 1 - k) % 2 == 0) ? X : Y;
          MGX_TRY(cheb_fused_iteration(sm, k == 0 ? kChebInit : (k == 1 ? kChebOldInit : kCheb), cur, old, out, b, f1, f2, f0));
          old = cur;
          cur = out;
        }
      return MGX_OK;
    }
  if (!is_step)
    {
      // x_1 = (1/theta) D^-1 b goes where an alternation over {X,Y} ends in X
      void *cur = (n_loop % 2 == 0) ? X : Y, *old = nullptr;
      launch_cheb_init(s, num, cur, b, op->d.inv_diag, sm->factors().first(), n);
      krylov::ChebyshevFactors F = sm->factors();
      for (int k = 0; k < n_loop; ++k)
        {
          double f1, f2;
          F.next(k, f1, f2);
          void *out = (cur == X) ? Y : X;
          MGX_TRY(cheb_fused_iteration(sm, k == 0 ? kChebZeroOld : kCheb, cur, old, out, b, f1, f2)); // k = 0: x_0 = 0
          old = cur;
          cur = out;
        }
      return MGX_OK;
    }
  // step(): 1 + n_loop iterations starting from X
  const int T = 1 + n_loop;
  if (T % 2 == 1 && T >= 3 && !sm->x_old2)
    MGX_TRY(sm->mem.alloc(&sm->x_old2, number_size(num) * n));
  void  *Z = sm->x_old2, *cur = X, *old = nullptr;
  krylov::ChebyshevFactors F = sm->factors();
  for (int k = 1; k <= T; ++k)
    {
      void *out;
      if (T % 2 == 0)
        out = (cur == X) ? Y : X;
      else if (T == 1)
        out = Y; // copied back below
      else
        out = k == 1 ? Y : (k == 2 ? Z : (k == 3 ? X : ((cur == X) ? Y : X)));
      if (k == 1)
        MGX_TRY(cheb_fused_iteration(sm, prolong_blocks ? kChebFirstProlong : kChebFirst, cur, nullptr, out, b, 0., sm->factors().first(), 0.,
                                     prolong_coarse, prolong_blocks, prolong_tr));
      else
        {
          double f1, f2;
          F.next(k - 2, f1, f2);
          MGX_TRY(cheb_fused_iteration(sm, kCheb, cur, old, out, b, f1, f2));
        }
      old = cur;
      cur = out;
    }
  if (cur != X)
    launch_copy_cast(s, X, num, cur, num, n);
  return MGX_OK;
}

int mgx_smoother_vmult(mgx_smoother_t sm, void *x, const void *b)
{
  MGX_REQUIRE(sm && x && b && x != b, "mgx_smoother_vmult: bad argument");
  return smoother_apply(sm, x, b, false);
}

int mgx_smoother_step(mgx_smoother_t sm, void *x, const void *b)
{
  MGX_REQUIRE(sm && x && b && x != b, "mgx_smoother_step: bad argument");
  return smoother_apply(sm, x, b, true);
}

/* ------------------------------------------------------------------------------------------
 * MGTransferMatrixFree (one level pair)
 * ------------------------------------------------------------------------------------------ */
// Fused level transfers on a decomposed mesh (TransferData::ifr_*, ifp_*): the brick loop restricts / prolongates the
// DoFs it completes itself; the DoFs on the rank interface are completed after the exchange, by list kernels that
// need their rows of P spelled out.  P is interpolatory: a fine DoF on a shared mesh entity couples to coarse DoFs of
// that entity only, so the first parent found holds its whole row.  idxc: the coarse operator's index table (host).
static int build_interface_transfer(mgx_transfer_s *tr, const mgx_transfer_desc *desc, const std::vector<uint32_t> &idxc)
{
  mgx_operator_t      fine = tr->fine, coarse = tr->coarse;
  const uint32_t      nsh = fine->plan->n_shared;
  const ExchangePlan &pl = *fine->plan;
  std::vector<uint32_t> shared(nsh);
  if (nsh)
    MGX_HIP(hipMemcpy(shared.data(), pl.shared_dev, sizeof(uint32_t) * nsh, hipMemcpyDeviceToHost));
  std::vector<uint32_t> idxf(27 * (size_t)fine->d.n_cells);
  MGX_HIP(hipMemcpy(idxf.data(), fine->d.idx27, sizeof(uint32_t) * idxf.size(), hipMemcpyDeviceToHost));
  const InterfaceRows rows =
    interface_rows(desc->children, idxf.data(), idxc.data(), coarse->d.n_cells, fine->d.n_dofs, shared.data(), nsh,
                   pl.not_owned_host.data(), pl.not_owned_host.size(), desc->prolong_1d, fine->d.p);
  if (rows.uncovered)
    return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_transfer_create: a shared DoF of the fine level lies in no cell");
  // (an empty list still gets one entry)
  auto upload_w = [&](const std::vector<double> &w, void **dev) {
    return tr->mem.upload_as(fine->d.number, dev, w.data(), w.size(), w.empty() ? 1 : 0);
  };
  auto upload_u = [&](const std::vector<uint32_t> &v, uint32_t **dev) { return tr->mem.upload(dev, v, v.empty() ? 1 : 0); };
  MGX_TRY(upload_u(rows.p_start, &tr->d.ifp_start));
  MGX_TRY(upload_u(rows.p_cdof, &tr->d.ifp_cdof));
  MGX_TRY(upload_w(rows.p_w, &tr->d.ifp_w));
  tr->d.n_ifp = nsh;
  MGX_TRY(upload_u(rows.r_cdof, &tr->d.ifr_cdof));
  MGX_TRY(upload_u(rows.r_start, &tr->d.ifr_start));
  MGX_TRY(upload_u(rows.r_fdof, &tr->d.ifr_fdof));
  MGX_TRY(upload_w(rows.r_w, &tr->d.ifr_w));
  tr->d.n_ifr = (uint32_t)rows.r_cdof.size();
  MGX_TRACE("transfer_create: interface rows: %u shared fine DoFs, %zu entries, %u coarse rows", nsh, rows.n_entries, tr->d.n_ifr);
  return MGX_OK;
}

// Whether the V-cycle (v_cycle_eager) forms the residual and its restriction in one pass of the fine level's cell
// loop, and whether its first post-smoothing step forms x + P x_coarse on the fly: nullptr where it does, else why
// not.  mgx_transfer_create traces the same answers (the smoother degree is known there only as "at least 1").
// Levels on the one-launch schedule run the residual as one launch and the transfers as kernels of their own: the
// fused forms need the eight colour launches, each as long as a brick's whole latency chain on such a level (2 M
// DoFs: 63 instead of 147 us, 52 instead of 180 us) -- except the scratch form of the restriction, one launch itself.
static const char *fused_restrict_blocker(const mgx_transfer_s *tr, const Tunables &tun)
{
  const BrickData &fb         = tr->fine->d.bricks;
  const bool       one_launch = fb.fr.available() && fb.fr.n_classes == 1;
  if (!tr->d.coarse_blocks)
    return "no block table of the coarse level";
  if (one_launch && !tr->d.coarse_scratch)
    return "fine level on the one-launch schedule without the scratch form";
  if (tun.no_fused_residual)
    return "option no_fused_residual";
  return nullptr;
}

// (p <= 4 on the two-class schedule: only from fused_prolong_min_bricks bricks on -- there the two launches + finish of
// a Chebyshev step are each as long as a brick's latency chain; at p = 8 the prolongation kernel costs 0.18 ms on the
// 17 M-DoF level and the fused form wins, 0.945 against 1.004 ms)
static const char *fused_prolong_blocker(const mgx_transfer_s *tr, const Tunables &tun, int smoother_degree)
{
  const mgx_operator_t Af         = tr->fine;
  const BrickData     &fb         = Af->d.bricks;
  const bool           one_launch = fb.fr.available() && fb.fr.n_classes == 1;
  if (!tr->d.coarse_blocks)
    return "no block table of the coarse level";
  if (!fb.item_map || Af->d.cells_form || !Af->d.separable)
    return "fine level not on the macro-element kernel";
  if (tun.no_fused_prolong)
    return "option no_fused_prolong";
  if (smoother_degree < 1)
    return "smoother of degree 0";
  if (one_launch)
    return "fine level on the one-launch schedule";
  if ((uint64_t)Af->d.n_dofs * number_size(Af->d.number) >= 0xFFFFFFF0ull)
    return "fine vector of 4 GB or more";
  if (fb.fr.available() && Af->d.p <= 4 && fb.n_bricks < tun.fused_prolong_min_bricks)
    return "p <= 4 on the two-class schedule below fused_prolong_min_bricks";
  return nullptr;
}

} // extern "C"

// The stages of mgx_transfer_create, in the order it calls them; device buffers go to the transfer's arena.
namespace
{
  // Is the 1D embedding symmetric under reversal of both indices (P1[2p-a][p-j] == P1[a][j])?  Every mirror-symmetric
  // node set gives one that is.  The pipelined kernels and the fused forms apply it in its even-odd form (Basis1D::P1eo),
  // which holds only what the symmetry leaves of P1: any other embedding runs the first-version kernels, which read P1.
  bool embedding_is_symmetric(const double *P1, int p)
  {
    const int n     = p + 1;
    double    scale = 0;
    for (size_t i = 0; i < (size_t)(2 * p + 1) * n; ++i)
      scale = std::max(scale, std::fabs(P1[i]));
    for (int a = 0; a <= 2 * p; ++a)
      for (int j = 0; j <= p; ++j)
        if (std::fabs(P1[a * n + j] - P1[(2 * p - a) * n + (p - j)]) > 1e-12 * scale)
          return false;
    return true;
  }

  // weights 1/multiplicity (multiplicity = number of parent patches sharing a fine DoF), stored
  // compressed as 3^dim entries per parent like deal.II does on uniform meshes, and the ownership of the fine entities.
  // idxf (the fine level's idx27_plain), shift and own are left on the host for build_patch_table.
  int build_weights_and_ownership(mgx_transfer_s &tr, const mgx_transfer_desc *desc, std::vector<uint32_t> &idxf,
                                  std::vector<uint8_t> &shift, std::vector<uint32_t> &own)
  {
    mgx_operator_t coarse = tr.coarse, fine = tr.fine;
    const int      dim = coarse->d.dim, ne = n_entities(dim);
    idxf.resize(ne * (size_t)fine->d.n_cells);
    MGX_HIP(hipMemcpy(idxf.data(), fine->d.idx27_plain, sizeof(uint32_t) * idxf.size(), hipMemcpyDeviceToHost));
    PatchShifts counted = patch_multiplicity_shifts(dim, desc->children, idxf.data(), coarse->d.n_cells, fine->d.n_dofs);
    shift.swap(counted.shift);
    if (dim == 2) // (one rank: the local count is the whole count)
      {
        // three or five cells around a vertex: owner weights as below, one byte per parent entity (patch_owner_weights_2d)
        if (counted.irregular)
          {
            if (desc->weight_shift)
              return fail(MGX_ERR_UNSUPPORTED, "mgx_transfer_create: fine DoF multiplicities other than 1/2/4 together with "
                                               "weight_shift");
            own = first_owner_masks(idxf.data(), ne, fine->d.n_cells, fine->d.n_dofs, coarse->d.p);
            OwnerWeights2D w = patch_owner_weights_2d(desc->children, own.data(), coarse->d.n_cells, coarse->d.p);
            if (!w.consistent)
              return fail(MGX_ERR_UNSUPPORTED, "mgx_transfer_create: owner weights need the fine entities of every parent entity "
                                               "to have their first owner in one parent (children in cell order)");
            shift.swap(w.weight);
            tr.d.owner_weights = true;
          }
        else if (desc->weight_shift && !std::equal(shift.begin(), shift.end(), desc->weight_shift))
          return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_transfer_create: inconsistent weight_shift");
      }
    else
      {
        // Multiplicities other than 1/2/4/8 (three blocks of a multi-block mesh around an edge): the
        // restriction then uses OWNER weights -- a shared fine DoF is restricted by the one parent that
        // owns its entity, with weight 1.  Any weights that add up to one over the parents of a fine
        // DoF give the same R = P^T (P is interpolatory: a fine DoF on a shared entity only couples to
        // coarse DoFs on that entity, which all its parents hold); only the summation order differs.
        // (on a decomposed mesh the local counts miss the parents of other ranks: without the caller's global
        // weight_shift every rank uses owner weights, which need no count at all)
        if (counted.irregular || (coarse->plan && !desc->weight_shift))
          {
            if (desc->weight_shift)
              return fail(MGX_ERR_UNSUPPORTED, "mgx_transfer_create: fine DoF multiplicities other than 1/2/4/8 together with "
                                               "weight_shift");
            std::fill(shift.begin(), shift.end(), (uint8_t)0);
            tr.d.owner_weights = true;
          }
        if (desc->weight_shift) // multiplicities that count the parents of other ranks as well
          for (size_t i = 0; i < shift.size(); ++i)
            {
              if (desc->weight_shift[i] > 3 || desc->weight_shift[i] < shift[i])
                return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_transfer_create: inconsistent weight_shift");
              shift[i] = desc->weight_shift[i];
            }
      }
    MGX_TRY(tr.mem.upload(&tr.d.weight_shift, shift));
    // ownership of the fine entities for the atomic-free prolongation: first cell in cell order (the table was checked
    // when the fine operator was created)
    own = first_owner_masks(idxf.data(), ne, fine->d.n_cells, fine->d.n_dofs, coarse->d.p);
    return tr.mem.upload(&tr.d.own27, own);
  }

  // Two dimensions: the restriction runs over the parents colour by colour -- greedy colours over the unconstrained
  // table (they hold for the constrained one as well)
  int colour_parents(mgx_transfer_s &tr)
  {
    const OperatorData   &c = tr.coarse->d;
    std::vector<uint32_t> idxc(n_entities(c.dim) * (size_t)c.n_cells);
    MGX_HIP(hipMemcpy(idxc.data(), c.idx27_plain, sizeof(uint32_t) * idxc.size(), hipMemcpyDeviceToHost));
    const CellColouring colours = colour_cells_greedy(idxc.data(), n_entities(c.dim), c.n_cells, c.n_dofs, c.p);
    if (colours.more_than_32)
      return fail(MGX_ERR_UNSUPPORTED, "mgx_transfer_create: the coarse cells need more than 32 colours");
    MGX_TRY(upload_colours(tr.mem, tr.d.parent_colours, colours));
    MGX_TRACE("transfer_create: two dimensions, %u parents in %d colours", c.n_cells, colours.n);
    return MGX_OK;
  }

  // patch table of the pipelined kernels (mgx_transfer.hip): the 5^3 mesh entities of the
  // children patch of every parent.  Patch entity layer 0..4 along a direction = (child 0:
  // codes 0,1,2 ; child 1: codes 0,1,2) with child 0's code 2 and child 1's code 0 coinciding.
  // With the table: the check of the coarse cells' colouring by index mod 8 and the route of the restriction.
  int build_patch_table(mgx_transfer_s &tr, const mgx_transfer_desc *desc, bool p1_symmetric, const std::vector<uint32_t> &idxf,
                        const std::vector<uint8_t> &shift, const std::vector<uint32_t> &own)
  {
    mgx_operator_t coarse = tr.coarse, fine = tr.fine;
    const int      p    = coarse->d.p;
    const uint32_t npar = coarse->d.n_cells;
    if (coarse->ctx->tun.transfer_v1)
      {
        MGX_TRACE("transfer_create: no patch table, first-version kernels (option transfer_v1)");
        return MGX_OK;
      }
    if (!p1_symmetric)
      {
        MGX_TRACE("transfer_create: no patch table, first-version kernels (1D embedding not symmetric under reversal)");
        return MGX_OK;
      }
    if (fine->d.n_dofs >= (1u << 29))
      {
        MGX_TRACE("transfer_create: no patch table, first-version kernels (%u fine DoFs: 29-bit index)", fine->d.n_dofs);
        return MGX_OK;
      }
    // owner weights on a decomposed mesh: a fine entity that a lower rank holds as well is restricted
    // there; here it enters with weight 0 (the coarse sums are added over the ranks afterwards)
    std::vector<uint8_t> foreign;
    if (tr.d.owner_weights && fine->plan)
      {
        foreign.assign(fine->d.n_dofs, 0);
        for (uint32_t i : fine->plan->not_owned_host)
          foreign[i] = 1;
      }
    {
      const PatchTable patch = patch_table(desc->children, idxf.data(), own.data(), shift.data(), npar, p, tr.d.owner_weights,
                                           foreign.empty() ? nullptr : foreign.data());
      if (!patch.consistent)
        {
          MGX_TRACE("transfer_create: no patch table, first-version kernels (children patches inconsistent)");
          return MGX_OK;
        }
      MGX_TRY(tr.mem.upload(&tr.d.patch, patch.words));
    }
    // colouring of the coarse cells by index mod 8
    if (npar % 8 == 0 && !coarse->ctx->tun.restrict_atomic)
      {
        std::vector<uint32_t> idxc(27 * (size_t)npar);
        MGX_HIP(hipMemcpy(idxc.data(), coarse->d.idx27_plain, sizeof(uint32_t) * idxc.size(), hipMemcpyDeviceToHost));
        tr.d.coarse_coloured = coloured_by_index_mod_8(idxc.data(), npar, coarse->d.n_dofs, p);
      }
    MGX_TRACE("transfer_create: patch table built, pipelined kernels");
    if (tr.d.coarse_coloured)
      MGX_TRACE("transfer_create: coarse colouring yes (parent index mod 8)");
    else if (npar % 8 != 0)
      MGX_TRACE("transfer_create: coarse colouring no (%u parents, not a multiple of 8)", npar);
    else if (coarse->ctx->tun.restrict_atomic)
      MGX_TRACE("transfer_create: coarse colouring no (option restrict_atomic)");
    else
      MGX_TRACE("transfer_create: coarse colouring no (two parents of one colour share an entity)");
    // the restriction route of launch_t (mgx_transfer.hip)
    if (tr.d.coarse_coloured && npar >= tr.d.colour_min)
      MGX_TRACE("transfer_create: restriction in 8 colour launches");
    else if (coarse->d.asm_start)
      MGX_TRACE("transfer_create: restriction in one launch, ordered assembly with constraints, atomic adds without");
    else
      MGX_TRACE("transfer_create: restriction in one launch, atomic adds");
    return MGX_OK;
  }

  // 1D prolongation matrix into the basis blocks of both operators (the transfer kernels read the
  // coarse one, the fused residual + restriction of the fine level's cell loop the fine one)
  // ... and its even-odd form for the line products of the fused forms (Basis1D::P1eo): the embedding of a parent
  // into its two children is symmetric under reversal of both indices for every node set that is
  int upload_embedding(mgx_transfer_s &tr, const mgx_transfer_desc *desc)
  {
    const int           p = tr.coarse->d.p, n = p + 1;
    const size_t        np1 = (size_t)(2 * p + 1) * n;
    std::vector<double> p1eo;
    {
      const double *P1 = desc->prolong_1d;
      const int     nh = (p + 1) / 2;
      p1eo.assign((size_t)(2 * p + 1) * nh + (p + 1), 0.);
      for (int a = 0; a <= p; ++a)
        for (int j = 0; j < nh; ++j)
          {
            p1eo[(size_t)a * nh + j] = 0.5 * (P1[a * n + j] + P1[a * n + p - j]);
            if (a < p)
              p1eo[(size_t)(p + 1 + a) * nh + j] = 0.5 * (P1[a * n + j] - P1[a * n + p - j]);
          }
      if (p % 2 == 0)
        for (int a = 0; a <= p; ++a)
          p1eo[(size_t)(2 * p + 1) * nh + a] = P1[a * n + p / 2];
    }
    // (two dimensions: the dense embedding into the block of the coarse operator, which the transfer kernels read, and
    // nothing else -- there are no fused forms)
    const bool quads = tr.coarse->d.dim == 2;
    for (mgx_operator_t o : {tr.coarse, tr.fine})
      {
        if (quads && o == tr.fine)
          break;
        const bool   f64 = o->d.number == MGX_F64;
        const size_t at_p1 = f64 ? offsetof(Basis1D<double>, P1) : offsetof(Basis1D<float>, P1);
        const size_t at_eo = f64 ? offsetof(Basis1D<double>, P1eo) : offsetof(Basis1D<float>, P1eo);
        MGX_TRY(tr.mem.copy_as(o->d.number, (char *)o->d.basis + at_p1, desc->prolong_1d, np1));
        if (!quads)
          MGX_TRY(tr.mem.copy_as(o->d.number, (char *)o->d.basis + at_eo, p1eo.data(), p1eo.size()));
      }
    return MGX_OK;
  }

  // Fused residual + restriction (BrickMode kResidualRestrict): needs the fine level on the brick
  // schedule in its separable form, children in forest order (cell c is child c % 8 of parent
  // c / 8, so that a brick's cells are the children of PB^3 sibling parents) and a single rank.
  // (Degree 7 ran the separate kernels until the line products of the embedding took their even-odd form in round 4:
  // V-cycle at 64^3 cells 10.69 ms separate, 9.70 ms fused; before: 8.86 / 9.36 ms at the clocks of round 2.  Degree 8
  // was in the same position while its fused forms spilled.  The option "force_fused_transfers" is a no-op now.)
  // tab: the block table on the host for build_restrict_scratch, empty where the fused forms have none
  int build_fused_blocks(mgx_transfer_s &tr, const mgx_transfer_desc *desc, bool p1_symmetric, std::vector<uint32_t> &tab)
  {
    mgx_operator_t coarse = tr.coarse, fine = tr.fine;
    const int      p    = coarse->d.p;
    const uint32_t npar = coarse->d.n_cells;
    tab.clear();
    const bool fused_pays = p1_symmetric;
    // (decomposed mesh: both levels decomposed alike -- not across an agglomeration -- and interface rows, above)
    if (!(fine->d.bricks.available() && fine->d.separable && (!fine->plan == !coarse->plan) && fused_pays &&
          !coarse->ctx->tun.no_fused_restrict && !(fine->plan && coarse->ctx->tun.no_fused_decomposed)))
      return MGX_OK;
    const int      PB = p <= 4 ? 2 : 1;
    const uint32_t nb = fine->d.bricks.n_bricks, ppb = PB * PB * PB; // parents per brick
    if (!(children_in_forest_order(desc->children, 8 * (size_t)npar) && (uint64_t)nb * ppb == npar &&
          fine->d.bricks.order.size() == nb))
      return MGX_OK;
    std::vector<uint32_t> idxc(27 * (size_t)npar);
    MGX_HIP(hipMemcpy(idxc.data(), coarse->d.idx27, sizeof(uint32_t) * idxc.size(), hipMemcpyDeviceToHost));
    std::vector<uint32_t> idxp(27 * (size_t)npar);
    MGX_HIP(hipMemcpy(idxp.data(), coarse->d.idx27_plain, sizeof(uint32_t) * idxp.size(), hipMemcpyDeviceToHost));
    tab = coarse_block_table(idxc.data(), idxp.data(), fine->d.bricks.order.data(), nb, PB);
    if (tab.empty()) // two parents of a brick disagree on a shared entity
      return MGX_OK;
    if (fine->plan)
      MGX_TRY(build_interface_transfer(&tr, desc, idxc));
    return tr.mem.upload(&tr.d.coarse_blocks, tab);
  }

  // scratch form of the fused residual + restriction: every brick stores its (PB p + 1)^3 restricted values
  // in a block of its own; the coarse vector is assembled from the blocks in brick order
  int build_restrict_scratch(mgx_transfer_s &tr, const std::vector<uint32_t> &tab)
  {
    mgx_operator_t coarse = tr.coarse, fine = tr.fine;
    const int      p  = coarse->d.p;
    const int      PB = p <= 4 ? 2 : 1;
    const uint32_t nb = fine->d.bricks.n_bricks;
    const uint64_t CN = (uint64_t)PB * p + 1, NC = CN * CN * CN;
    // (levels on the reduced-colour schedules only: there a colour launch is as long as a brick's latency chain and
    // one launch instead of eight pays -- 17 M DoFs 179 -> 164 us; on the finest level of C2 the blocks' extra traffic
    // costs more than the seven launch ramps it saves, 1.184 against 1.138 ms)
    if (tab.empty() || !((uint64_t)nb * NC < 0xFFFFFFF0ull && !coarse->ctx->tun.no_restrict_scratch &&
                         nb <= coarse->ctx->tun.free_max_bricks))
      return MGX_OK;
    const IndexRows a = block_assembly(tab.data(), nb, PB, p, coarse->d.n_dofs);
    const size_t scratch_bytes = number_size(fine->d.number) * (size_t)nb * NC;
    MGX_TRY(tr.mem.alloc(&tr.d.coarse_scratch, scratch_bytes));
    MGX_HIP(hipMemset(tr.d.coarse_scratch, 0, scratch_bytes));
    MGX_TRY(tr.mem.upload(&tr.d.cs_start, a.start));
    return tr.mem.upload(&tr.d.cs_pos, a.pos, a.pos.empty() ? 1 : 0);
  }

  // which of the fused transfer forms the V-cycle will run on this level pair, and why not
  void trace_transfer_routes(const mgx_transfer_s &tr, bool p1_symmetric)
  {
    if (!trace_on())
      return;
    mgx_operator_t coarse = tr.coarse, fine = tr.fine;
    // why the block table of the fused forms is missing (the tables' own conditions are checked above)
    const char *no_blocks = !p1_symmetric                        ? "1D embedding not symmetric under reversal"
                            : coarse->ctx->tun.no_fused_restrict ? "option no_fused_restrict"
                            : !fine->d.bricks.available()        ? "fine level without bricks"
                                                                 : "fine level not separable, not in forest order or decomposed differently";
    const char *r = fused_restrict_blocker(&tr, coarse->ctx->tun), *q = fused_prolong_blocker(&tr, coarse->ctx->tun, 1);
    if (r)
      MGX_TRACE("transfer_create: fused residual + restriction no (%s)", tr.d.coarse_blocks ? r : no_blocks);
    else
      MGX_TRACE("transfer_create: fused residual + restriction yes (%s)", tr.d.coarse_scratch ? "scratch form" : "colour launches");
    if (q)
      MGX_TRACE("transfer_create: fused prolongation no (%s)", tr.d.coarse_blocks ? q : no_blocks);
    else
      MGX_TRACE("transfer_create: fused prolongation yes (with a smoother of degree >= 1)");
  }
} // namespace

extern "C" {

int mgx_transfer_create(mgx_operator_t coarse, mgx_operator_t fine, const mgx_transfer_desc *desc,
                        mgx_transfer_t *out)
{
  MGX_REQUIRE(coarse && fine && desc && out && desc->children && desc->prolong_1d,
              "mgx_transfer_create: null argument");
  MGX_REQUIRE(coarse->d.p == fine->d.p && coarse->d.number == fine->d.number,
              "mgx_transfer_create: level operators differ in degree or number type");
  MGX_REQUIRE(coarse->d.idx27_plain && fine->d.idx27_plain,
              "mgx_transfer_create: operators were created without idx27_plain");
  MGX_REQUIRE(coarse->d.dim == fine->d.dim, "mgx_transfer_create: level operators of different dimensions");
  // Two dimensions (mgx_kernels_2d.hip): children in fours, weights and ownership over the 9 entities of a cell, the
  // parents coloured for the restriction.  No patch table, no fused forms: the dense kernels serve every embedding.
  const bool     quads      = coarse->d.dim == 2;
  const uint32_t n_children = quads ? 4u : 8u, npar = coarse->d.n_cells, nfine = fine->d.n_cells;
  MGX_REQUIRE((uint64_t)npar * n_children == nfine,
              quads ? "mgx_transfer_create: fine level must have 4 children per coarse cell (uniform refinement)"
                    : "mgx_transfer_create: fine level must have 8 children per coarse cell (uniform refinement)");
  {
    // (two dimensions: every fine cell is the child of exactly one parent -- the prolongation writes every fine entry once)
    std::vector<uint8_t> seen(quads ? nfine : 0u, 0);
    for (size_t i = 0; i < n_children * (size_t)npar; ++i)
      {
        if (desc->children[i] >= nfine)
          return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_transfer_create: child index out of range");
        if (quads && seen[desc->children[i]]++)
          return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_transfer_create: the children table names a fine cell twice");
      }
  }
  if (!quads)
    MGX_TRACE("transfer_create: parents=%u", npar);
  const bool p1_symmetric = embedding_is_symmetric(desc->prolong_1d, coarse->d.p);
  // failures below return through the destroy function, which frees what the transfer's arena holds by then
  std::unique_ptr<mgx_transfer_s, int (*)(mgx_transfer_t)> tr(new mgx_transfer_s, mgx_transfer_destroy);
  tr->coarse = coarse;
  tr->fine   = fine;
  tr->d.coarse = &coarse->d;
  tr->d.colour_min = coarse->ctx->tun.restrict_colour_min;
  tr->d.fine   = &fine->d;
  tr->d.n_cus  = context_cus(coarse->ctx);
  MGX_TRY(tr->mem.upload(&tr->d.children, desc->children, n_children * (size_t)npar));
  {
    std::vector<uint32_t> idxf, own; // fine idx27_plain, entity ownership of the fine cells
    std::vector<uint8_t>  shift;
    MGX_TRY(build_weights_and_ownership(*tr, desc, idxf, shift, own));
    if (!quads)
      MGX_TRY(build_patch_table(*tr, desc, p1_symmetric, idxf, shift, own));
  }
  if (quads)
    MGX_TRY(colour_parents(*tr));
  MGX_TRY(upload_embedding(*tr, desc));
  if (quads)
    {
      *out = tr.release();
      return MGX_OK;
    }
  {
    std::vector<uint32_t> tab; // block table of the fused forms
    MGX_TRY(build_fused_blocks(*tr, desc, p1_symmetric, tab));
    MGX_TRY(build_restrict_scratch(*tr, tab));
  }
  trace_transfer_routes(*tr, p1_symmetric);
  if (tr->d.owner_weights && !tr->d.patch)
    return fail(MGX_ERR_UNSUPPORTED,
                !p1_symmetric ? "mgx_transfer_create: owner weights need the pipelined transfer kernels, which need a 1D embedding "
                                "symmetric under reversal"
                : coarse->ctx->tun.transfer_v1
                  ? "mgx_transfer_create: owner weights need the pipelined transfer kernels (option transfer_v1 is set)"
                  : "mgx_transfer_create: owner weights need the pipelined transfer kernels (fine level below 2^29 DoFs)");
  *out = tr.release();
  return MGX_OK;
}

int mgx_transfer_destroy(mgx_transfer_t tr)
{
  if (!tr)
    return MGX_OK;
  (void)hipStreamSynchronize(tr->coarse->ctx->stream);
  delete tr;
  return MGX_OK;
}

int mgx_prolongate(mgx_transfer_t tr, void *fine, const void *coarse, int add, int with_constraints)
{
  MGX_REQUIRE(tr && fine && coarse, "mgx_prolongate: null argument");
  launch_prolongate(tr->coarse->ctx->stream, tr->d, fine, coarse, add != 0, with_constraints != 0);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_restrict_and_add(mgx_transfer_t tr, void *coarse, const void *fine, int with_constraints)
{
  MGX_REQUIRE(tr && fine && coarse, "mgx_restrict_and_add: null argument");
  mgx_operator_t cop = tr->coarse;
  hipStream_t    s   = cop->ctx->stream;
  if (!cop->plan)
    {
      launch_restrict_add(s, tr->d, coarse, fine, with_constraints != 0);
      MGX_HIP(hipGetLastError());
      return MGX_OK;
    }
  // decomposed mesh: restrict into a zeroed scratch vector, sum the interface entries over the
  // ranks, then add (adding into `coarse` first would count its existing interface values once
  // per sharing rank)
  const size_t bytes = number_size(cop->d.number) * cop->d.n_dofs;
  if (!tr->scratch)
    MGX_TRY(tr->mem.alloc(&tr->scratch, bytes));
  MGX_HIP(hipMemsetAsync(tr->scratch, 0, bytes, s));
  launch_restrict_add(s, tr->d, tr->scratch, fine, with_constraints != 0);
  MGX_TRY(exchange_add(cop, tr->scratch));
  launch_add_cast(s, coarse, cop->d.number, tr->scratch, cop->d.number, cop->d.n_dofs);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

// 1D matrix of the state interpolation to the coarser level (minimal_surface/program.cc:425-457, FE_Q's
// get_restriction_matrix): r[a (p+1) + i] = value at the coarse Gauss-Lobatto node i of the Lagrange polynomial of the
// fine patch point a (child 0: a = 0..p, child 1: a = p..2p; the children's node sets on [0,1/2] and [1/2,1]); the
// child that contains the node is used (a node on the common face: either gives the same value, child 0 is taken).
static std::vector<double> interpolation_matrix_1d(int p)
{
  using ld = long double;
  const int       n = p + 1, m = 2 * p + 1;
  std::vector<ld> x(n);
  x[0] = 0, x[p] = 1;
  const ld pi = 3.141592653589793238462643383279502884L;
  for (int i = 1; i < p; ++i) // Gauss-Lobatto interior nodes: Newton on P_p'
    {
      ld t = -std::cos(pi * i / p);
      for (int it = 0; it < 100; ++it)
        {
          ld p0 = 1, p1 = t; // Legendre recurrence: P_p(t) and its first two derivatives
          for (int k = 2; k <= p; ++k)
            {
              const ld pk = ((2 * k - 1) * t * p1 - (k - 1) * p0) / k;
              p0 = p1, p1 = pk;
            }
          const ld dP  = p * (p0 - t * p1) / (1 - t * t); // p1 = P_p, p0 = P_{p-1}
          const ld d2P = (2 * t * dP - (ld)p * (p + 1) * p1) / (1 - t * t);
          const ld dt  = dP / d2P;
          t -= dt;
          if (std::fabs(dt) < 1e-19L)
            break;
        }
      x[i] = (t + 1) / 2;
    }
  for (int i = 0; i < n / 2; ++i) // mirror symmetry to the last bit
    x[p - i] = 1 - x[i];
  std::vector<double> r((size_t)m * n, 0.);
  for (int i = 0; i < n; ++i)
    {
      const int child = x[i] > 0.5L ? 1 : 0;
      const ld  xi    = 2 * x[i] - child; // coordinate of the coarse node in the child
      for (int a = 0; a < n; ++a)
        {
          ld v = 1;
          for (int b = 0; b < n; ++b)
            if (b != a)
              v *= (xi - x[b]) / (x[a] - x[b]);
          r[(size_t)(child * p + a) * n + i] = (double)v;
        }
    }
  return r;
}

/* LaplaceProblem::solve, minimal_surface/program.cc:425-457 */
int mgx_interpolate_to_coarse(mgx_transfer_t tr, void *coarse, const void *fine)
{
  MGX_REQUIRE(tr && coarse && fine, "mgx_interpolate_to_coarse: null argument");
  mgx_operator_t cop = tr->coarse, fop = tr->fine;
  const int dim = cop->d.dim, ne = n_entities(dim);
  if (dim == 2 && !cop->coef_update)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_interpolate_to_coarse: not on a two-dimensional transfer whose coarse operator has no "
                                     "geometry: call mgx_operator_enable_coefficient_update_2d or _q_2d on the level operators "
                                     "first (mgx_square_solver_create_general does)");
  if (cop->plan || fop->plan || cop->ctx->has_comm)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_interpolate_to_coarse: not on a decomposed mesh (single rank only)");
  MGX_REQUIRE(cop->d.idx27_plain && fop->d.idx27_plain, "mgx_interpolate_to_coarse: the level operators need idx27_plain");
  hipStream_t s = cop->ctx->stream;
  const int   p = cop->d.p;
  if (!tr->interp_1d)
    {
      // (the Gauss-Lobatto nodes mgx_operator_desc::shape_values is defined on)
      const std::vector<double> r = interpolation_matrix_1d(p);
      // (two dimensions: 9 entities per cell, e = 3 cy + cx, the low 9 bits of the mask)
      std::vector<uint32_t>     idxc((size_t)cop->d.n_cells * ne);
      MGX_HIP(hipMemcpy(idxc.data(), cop->d.idx27_plain, sizeof(uint32_t) * idxc.size(), hipMemcpyDeviceToHost));
      bool                        out_of_range = false;
      const std::vector<uint32_t> own          = first_owner_masks(idxc.data(), ne, cop->d.n_cells, cop->d.n_dofs, p, &out_of_range);
      MGX_REQUIRE(!out_of_range, "mgx_interpolate_to_coarse: index table out of range");
      MGX_TRY(tr->mem.upload(&tr->own_coarse, own));
      MGX_TRY(tr->mem.upload_as(cop->d.number, &tr->interp_1d, r.data(), r.size())); // (last: it marks the tables as built)
    }
  launch_interpolate_to_coarse(s, tr->d, tr->interp_1d, tr->own_coarse, coarse, fine);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

/* ------------------------------------------------------------------------------------------
 * MultigridSolver
 * ------------------------------------------------------------------------------------------ */
int mgx_solver_set_polynomial_type(mgx_solver_t S, int polynomial_type)
{
  MGX_REQUIRE(S, "mgx_solver_set_polynomial_type: null solver");
  // the coarsest level keeps the first kind with the degree from the tolerance (multigrid_solver.h:955-959)
  for (int l = 1; l < S->n_levels; ++l)
    MGX_TRY(mgx_smoother_set_polynomial_type(S->smooth[l], polynomial_type));
  if (S->graph_exec) // the factors are baked into the captured launches
    {
      MGX_HIP(hipStreamSynchronize(S->ctx->stream));
      (void)hipGraphExecDestroy(S->graph_exec);
      (void)hipGraphDestroy(S->graph);
      S->graph_exec  = nullptr;
      S->graph       = nullptr;
      S->graph_calls = 0;
    }
  if (S->agg_solver)
    MGX_TRY(mgx_solver_set_polynomial_type(S->agg_solver, polynomial_type));
  return MGX_OK;
}

int mgx_solver_destroy(mgx_solver_t S)
{
  if (!S)
    return MGX_OK;
  (void)hipStreamSynchronize(S->ctx->stream);
  for (auto sm : S->smooth)
    mgx_smoother_destroy(sm);
  if (S->graph_exec)
    (void)hipGraphExecDestroy(S->graph_exec);
  if (S->graph)
    (void)hipGraphDestroy(S->graph);
  if (S->agg_in)
    (void)hipEventDestroy(S->agg_in);
  if (S->agg_out)
    (void)hipEventDestroy(S->agg_out);
  delete S;
  return MGX_OK;
}

int mgx_solver_create(mgx_context_t ctx, const mgx_solver_desc *desc, mgx_solver_t *out)
{
  MGX_REQUIRE(ctx && desc && out, "mgx_solver_create: null argument");
  MGX_REQUIRE(desc->n_levels >= 1 && desc->matrix && desc->matrix_dp && desc->bc_count,
              "mgx_solver_create: incomplete descriptor");
  MGX_REQUIRE(desc->n_levels == 1 || (desc->transfer && desc->transfer_dp), "mgx_solver_create: missing transfers");
  MGX_REQUIRE(desc->degree_pre >= 1 && desc->n_cycles >= 1, "mgx_solver_create: bad smoother degree / cycle count");
  MGX_TRACE("solver_create: n_levels=%d", desc->n_levels);
  auto S      = std::unique_ptr<mgx_solver_s, int (*)(mgx_solver_t)>(new mgx_solver_s, mgx_solver_destroy);
  S->ctx      = ctx;
  S->n_levels = desc->n_levels;
  S->degree   = desc->degree_pre;
  S->n_cycles = desc->n_cycles;
  S->vnumber  = desc->matrix[0]->d.number;
  S->timings.assign(6 * (size_t)desc->n_levels, 0.);
  const int nl = desc->n_levels;
  S->transfer.assign(nl, nullptr);
  S->transfer_dp.assign(nl, nullptr);
  for (int l = 0; l < nl; ++l)
    {
      MGX_REQUIRE(desc->matrix[l] && desc->matrix_dp[l], "mgx_solver_create: null level operator");
      MGX_REQUIRE(desc->matrix_dp[l]->d.number == MGX_F64, "mgx_solver_create: matrix_dp must be fp64");
      MGX_REQUIRE(desc->matrix[l]->d.number == S->vnumber, "mgx_solver_create: mixed V-cycle number types");
      MGX_REQUIRE(desc->matrix[l]->d.n_dofs == desc->matrix_dp[l]->d.n_dofs, "mgx_solver_create: level size mismatch");
      MGX_REQUIRE(desc->matrix[l]->d.dim == desc->matrix[0]->d.dim && desc->matrix_dp[l]->d.dim == desc->matrix[0]->d.dim,
                  "mgx_solver_create: level operators of different dimensions");
      if (desc->matrix[l]->d.dim == 2 && ctx->has_comm)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_create: a two-dimensional hierarchy on a context with a communicator (one rank only)");
      S->matrix.push_back(desc->matrix[l]);
      S->matrix_dp.push_back(desc->matrix_dp[l]);
      if (l > 0)
        {
          MGX_REQUIRE(desc->transfer[l] && desc->transfer_dp[l], "mgx_solver_create: null transfer");
          S->transfer[l]    = desc->transfer[l];
          S->transfer_dp[l] = desc->transfer_dp[l];
        }
      const size_t n = desc->matrix[l]->d.n_dofs;
      double      *p = nullptr;
      void        *q = nullptr;
      MGX_TRY(S->mem.zeros(&p, n, ctx->stream));
      S->solution.push_back(p);
      if (desc->rhs && desc->rhs[l])
        {
          MGX_TRY(S->mem.upload(&p, desc->rhs[l], n));
          // a rank assembles the rhs over its own cells: complete the interface entries
          // (dst.compress(add) in compute_residual, laplace_operator.h:843)
          MGX_TRY(exchange_add(desc->matrix_dp[l], p));
        }
      else // assembled on the device afterwards: mgx_solver_compute_rhs
        MGX_TRY(S->mem.zeros(&p, n, ctx->stream));
      S->rhs.push_back(p);
      MGX_TRY(S->mem.zeros(&p, n, ctx->stream));
      S->residual.push_back(p);
      const size_t vb = number_size(S->vnumber) * n;
      MGX_TRY(S->mem.zeros(&q, vb, ctx->stream));
      S->defect.push_back(q);
      MGX_TRY(S->mem.zeros(&q, vb, ctx->stream));
      S->t.push_back(q);
      MGX_TRY(S->mem.zeros(&q, vb, ctx->stream));
      S->solution_update.push_back(q);
      // inhomogeneous boundary values (multigrid_solver.h:225-253)
      const uint32_t nb = desc->bc_count[l];
      S->bc_count.push_back(nb);
      uint32_t *bi = nullptr;
      double   *bv = nullptr, *bz = nullptr;
      if (nb)
        {
          MGX_REQUIRE(desc->bc_index && desc->bc_value && desc->bc_index[l] && desc->bc_value[l],
                      "mgx_solver_create: missing boundary lists");
          for (uint32_t i = 0; i < nb; ++i)
            if (desc->bc_index[l][i] >= n)
              return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_solver_create: boundary index out of range");
        }
      MGX_TRY(S->mem.upload(&bi, nb ? desc->bc_index[l] : nullptr, nb, 1));
      MGX_TRY(S->mem.upload(&bv, nb ? desc->bc_value[l] : nullptr, nb, 1));
      MGX_TRY(S->mem.zeros(&bz, (size_t)nb + 1, ctx->stream));
      S->bc_index_dev.push_back(bi);
      S->bc_value_dev.push_back(bv);
      S->bc_zero_dev.push_back(bz);
    }
  // smoothers (multigrid_solver.h:269-289)
  for (int l = 0; l < nl; ++l)
    {
      mgx_smoother_t sm = nullptr;
      MGX_TRY(mgx_compute_diagonal(S->matrix[l])); // :286
      if (l > 0)
        MGX_TRY(mgx_smoother_create(S->matrix[l], 20., S->degree, 15, &sm)); // :274-278
      else
        MGX_TRY(mgx_smoother_create(S->matrix[l], 1e-3, -1, (int)std::max<uint32_t>(3u, S->matrix[l]->d.n_dofs),
                                    &sm)); // :282-284
      S->smooth.push_back(sm);
    }
  if (!ctx->tun.no_graph)
    {
      const uint32_t graph_max = ctx->tun.graph_max_dofs;
      for (int l = 0; l < nl; ++l)
        if (S->matrix[l]->d.n_dofs <= graph_max)
          S->graph_level = l;
    }
  const size_t nmax = S->matrix[nl - 1]->d.n_dofs;
  for (double **v : {&S->cg_r, &S->cg_z, &S->cg_d, &S->cg_h})
    MGX_TRY(S->mem.alloc(v, nmax));
  *out = S.release();
  return MGX_OK;
}

static void set_bc(mgx_solver_t S, int level, double *v, bool zero)
{
  launch_scatter_values(S->ctx->stream, MGX_F64, v, S->bc_index_dev[level],
                        zero ? S->bc_zero_dev[level] : S->bc_value_dev[level], S->bc_count[level]);
}

static int v_cycle_eager(mgx_solver_t S, int level, int my_n_cycles);

static bool graph_usable(mgx_solver_t S, int level)
{
  if (S->graph_level < 0 || level != S->graph_level || S->graph_failed || S->timing || S->ctx->has_comm)
    return false;
  if (S->ctx->profile)
    for (int l = 0; l <= level; ++l)
      if (S->matrix[l]->profiled)
        return false; // HIP-event brackets must stay outside a captured region
  return true;
}

// The V-cycle on levels <= agg_level of a decomposed hierarchy, run on the undecomposed copy of
// those levels every rank holds: the defect is summed over the ranks into the copy's defect vector
// (every DoF contributed by its owner, all others add zero: exact, identical on all ranks), the
// copy's V-cycle runs on its own context (graph replay, no exchanges), and every rank reads the
// correction of its DoFs back.  Replaces one latency-bound exchange per operator application and
// level by one allreduce per V-cycle.
static int v_cycle(mgx_solver_t S, int level, int my_n_cycles);

static int agglomerated_cycle(mgx_solver_t S, int my_n_cycles)
{
  mgx_solver_t  G   = S->agg_solver;
  mgx_context_t ctx = S->ctx;
  const int     L   = S->agg_level, Lg = L + S->agg_offset; // the seam level in the numbering of either solver
  hipStream_t   s = ctx->stream, sg = G->ctx->stream;
  const int     num = S->vnumber;
  const size_t  ng = G->matrix[Lg]->d.n_dofs, nl = S->matrix[L]->d.n_dofs;
  LevelTimer sw = stopwatch(S, L, 5);
  MGX_HIP(hipMemsetAsync(G->defect[Lg], 0, number_size(num) * ng, s));
  launch_scatter_map(s, num, G->defect[Lg], S->defect[L], S->agg_map, S->agg_owned, (uint32_t)nl);
  if (ctx->use_rccl)
    {
      RcclApi &R = rccl_api();
      if (R.AllReduce(G->defect[Lg], G->defect[Lg], ng, num == MGX_F64 ? ncclDouble : ncclFloat, ncclSum, ctx->nccl, s) !=
          ncclSuccess)
        return fail(MGX_ERR_HIP, "ncclAllReduce of the agglomerated defect failed");
    }
  else
    {
      S->agg_host.resize(ng);
      if (num == MGX_F64)
        MGX_HIP(hipMemcpyAsync(S->agg_host.data(), G->defect[Lg], 8 * ng, hipMemcpyDeviceToHost, s));
      else
        {
          std::vector<float> tmp(ng);
          MGX_HIP(hipMemcpyAsync(tmp.data(), G->defect[Lg], 4 * ng, hipMemcpyDeviceToHost, s));
          MGX_HIP(hipStreamSynchronize(s));
          std::copy(tmp.begin(), tmp.end(), S->agg_host.begin());
        }
      MGX_HIP(hipStreamSynchronize(s));
      // (the callback counts in int: pieces of at most 2^30 values, so that no count is ever narrowed)
      if (!ctx->comm.allreduce_sum)
        return fail(MGX_ERR_HIP, "allreduce_sum callback failed");
      for (size_t first = 0; first < (size_t)ng; first += (size_t)1 << 30)
        {
          const size_t piece = std::min<size_t>((size_t)ng - first, (size_t)1 << 30);
          if (ctx->comm.allreduce_sum(ctx->comm.user, S->agg_host.data() + first, (int)piece) != 0)
            return fail(MGX_ERR_HIP, "allreduce_sum callback failed");
        }
      if (num == MGX_F64)
        {
          // pageable staging buffer, rewritten by the next cycle: the copy must have left it before we return
          MGX_HIP(hipMemcpyAsync(G->defect[Lg], S->agg_host.data(), 8 * ng, hipMemcpyHostToDevice, s));
          MGX_HIP(hipStreamSynchronize(s));
        }
      else
        {
          std::vector<float> tmp(S->agg_host.begin(), S->agg_host.end());
          MGX_HIP(hipMemcpyAsync(G->defect[Lg], tmp.data(), 4 * ng, hipMemcpyHostToDevice, s));
          MGX_HIP(hipStreamSynchronize(s));
        }
    }
  if (sg != s)
    {
      MGX_HIP(hipEventRecord(S->agg_in, s));
      MGX_HIP(hipStreamWaitEvent(sg, S->agg_in, 0));
    }
  MGX_TRY(v_cycle(G, Lg, my_n_cycles));
  if (sg != s)
    {
      MGX_HIP(hipEventRecord(S->agg_out, sg));
      MGX_HIP(hipStreamWaitEvent(s, S->agg_out, 0));
    }
  launch_pack(s, num, S->solution_update[L], G->solution_update[Lg], S->agg_map, (uint32_t)nl);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_solver_set_agglomeration(mgx_solver_t S, int level, mgx_solver_t coarse, const uint32_t *local_to_global,
                                 const uint8_t *owned, uint32_t n_local)
{
  MGX_REQUIRE(S && coarse && local_to_global && owned, "mgx_solver_set_agglomeration: null argument");
  MGX_REQUIRE(S->agg_solver == nullptr, "mgx_solver_set_agglomeration: already set");
  MGX_TRY(refuse_2d(S->matrix[0]->d, "mgx_solver_set_agglomeration", "one rank only"));
  MGX_TRY(refuse_2d(coarse->matrix[0]->d, "mgx_solver_set_agglomeration", "one rank only"));
  // (a hierarchy that lacks the coarsest levels of the whole mesh may consist of its finest level alone: the seam is then
  // that level, the only one that exists on both sides)
  MGX_REQUIRE(level >= 0 && (level < S->n_levels - 1 || (level == S->n_levels - 1 && coarse->n_levels > level + 1)),
              "mgx_solver_set_agglomeration: the finest level stays decomposed");
  // (a hierarchy whose level 0 is level k of the whole mesh -- mgx_cube_level_offset -- meets a coarse solver with k more
  // levels: its finest level is the seam either way)
  MGX_REQUIRE(coarse->n_levels >= level + 1, "mgx_solver_set_agglomeration: the coarse solver must end at `level`");
  const int offset = coarse->n_levels - 1 - level;
  MGX_REQUIRE(coarse->vnumber == S->vnumber && coarse->degree == S->degree,
              "mgx_solver_set_agglomeration: number type or smoother degree differ");
  MGX_REQUIRE(coarse->ctx != S->ctx && !coarse->ctx->has_comm,
              "mgx_solver_set_agglomeration: the coarse solver lives on a context of its own without a communicator");
  MGX_REQUIRE(n_local == S->matrix[level]->d.n_dofs, "mgx_solver_set_agglomeration: map length is not the level size");
  const uint32_t ng = coarse->matrix[level + offset]->d.n_dofs;
  for (uint32_t i = 0; i < n_local; ++i)
    if (local_to_global[i] >= ng)
      return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_solver_set_agglomeration: map entry out of range");
  MGX_TRY(S->mem.upload(&S->agg_map, local_to_global, n_local, 1));
  MGX_TRY(S->mem.upload(&S->agg_owned, owned, n_local, 1));
  MGX_HIP(hipEventCreateWithFlags(&S->agg_in, hipEventDisableTiming));
  MGX_HIP(hipEventCreateWithFlags(&S->agg_out, hipEventDisableTiming));
  // the copy runs in line with the decomposed levels: on their stream (no event hops around its graph)
  if (!coarse->ctx->borrowed_stream && coarse->ctx->device == S->ctx->device)
    {
      MGX_HIP(hipStreamSynchronize(coarse->ctx->stream));
      MGX_HIP(hipStreamDestroy(coarse->ctx->stream));
      coarse->ctx->stream          = S->ctx->stream;
      coarse->ctx->borrowed_stream = true;
    }
  S->agg_solver = coarse;
  S->agg_level  = level;
  S->agg_offset = offset;
  return MGX_OK;
}

// MultigridSolver::v_cycle (multigrid_solver.h:641-681), with graph replay of the coarse part
static int v_cycle(mgx_solver_t S, int level, int my_n_cycles)
{
  if (S->agg_solver && level == S->agg_level)
    return agglomerated_cycle(S, my_n_cycles);
  if (my_n_cycles != 1 || !graph_usable(S, level))
    return v_cycle_eager(S, level, my_n_cycles);
  hipStream_t s = S->ctx->stream;
  if (S->graph_exec)
    {
      // (the levels inside the replayed graph cannot be cut by host ranges: one range for the whole coarse part)
      if (S->ctx->tun.roctx)
        {
          char buf[48];
          std::snprintf(buf, sizeof(buf), "v_cycle_graph_levels_0_to_%d", level);
          range_push(S->ctx, buf);
        }
      const hipError_t e = hipGraphLaunch(S->graph_exec, s);
      range_pop(S->ctx);
      MGX_HIP(e);
      return MGX_OK;
    }
  if (S->graph_calls++ == 0)
    return v_cycle_eager(S, level, 1); // first execution eager: lazy allocations happen here
  if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess)
    {
      S->graph_failed = true;
      return v_cycle_eager(S, level, 1);
    }
  const int  status = v_cycle_eager(S, level, 1);
  hipError_t e      = hipStreamEndCapture(s, &S->graph);
  if (status != MGX_OK || e != hipSuccess || !S->graph ||
      hipGraphInstantiate(&S->graph_exec, S->graph, nullptr, nullptr, 0) != hipSuccess)
    {
      S->graph_failed = true;
      S->graph_exec   = nullptr;
      (void)hipGetLastError();
      return v_cycle_eager(S, level, 1); // nothing was executed during the capture
    }
  MGX_TRACE("v_cycle: levels 0..%d captured into a HIP graph", level);
  MGX_HIP(hipGraphLaunch(S->graph_exec, s));
  return MGX_OK;
}

static int v_cycle_eager(mgx_solver_t S, int level, int my_n_cycles)
{
  hipStream_t s = S->ctx->stream;
  if (level == 0)
    {
      LevelTimer sw = stopwatch(S, 0, 0);
      S->timings[1] += 1;
      return smoother_apply(S->smooth[0], S->solution_update[0], S->defect[0], false); // :647 (MGCoarseFromSmoother :72-91)
    }
  const size_t nc = S->matrix[level - 1]->d.n_dofs;
  for (int c = 0; c < my_n_cycles; ++c)
    {
      {
        LevelTimer sw = stopwatch(S, level, 5);
        if (c == 0) // :656-659
          MGX_TRY(smoother_apply(S->smooth[level], S->solution_update[level], S->defect[level], false));
        else
          MGX_TRY(smoother_apply(S->smooth[level], S->solution_update[level], S->defect[level], true));
      }
      // (which of the fused transfer forms run: fused_restrict_blocker / fused_prolong_blocker, which
      // mgx_transfer_create traces)
      if (!fused_restrict_blocker(S->transfer[level], S->ctx->tun))
        {
          // residual and restriction in one pass of the cell loop: t only carries the partial sums
          // of brick-surface DoFs between the colour launches, the residual is never stored
          LevelTimer sw = stopwatch(S, level, 0);
          mgx_operator_t      A = S->matrix[level];
          const TransferData &T = S->transfer[level]->d;
          // scratch form: the bricks store their restricted values block by block (one launch for the level), the
          // coarse defect is assembled from the blocks; otherwise they add into the zeroed coarse defect colour by
          // colour
          void *scratch = (T.coarse_scratch && !A->d.cells_form) ? T.coarse_scratch : nullptr;
          if (!scratch)
            MGX_HIP(hipMemsetAsync(S->defect[level - 1], 0, number_size(S->vnumber) * nc, s)); // :667
          {
            ProfileBracket pb(A, kResidualRestrict);
            BrickLaunch    l;
            l.mode           = kResidualRestrict;
            l.src            = S->solution_update[level];
            l.rhs            = S->defect[level];
            l.out            = S->t[level];
            l.carrier        = A->d.cells_form ? S->t[level] : nullptr; // (only the cell-by-cell form of a cross-check build hands partial sums over)
            l.coarse         = S->defect[level - 1];
            l.coarse_blocks  = T.coarse_blocks;
            l.coarse_scratch = scratch;
            launch_brick_loop(s, A->d, l);
            if (scratch)
              launch_coarse_assemble(s, A->d.number, T, S->defect[level - 1]);
          }
          if (A->plan)
            {
              // decomposed: every rank's bricks restrict their own shares of A x on all their points and b on the
              // points they complete; a DoF on the rank interface is completed by no brick, its b comes from its owner
              // (list kernel); no exchange on the fine level, the coarse defect is summed over the ranks like any
              // restricted vector
              launch_interface_restrict(s, A->d.number, T, S->defect[level - 1], S->defect[level], nullptr);
              MGX_TRY(exchange_add(S->matrix[level - 1], S->defect[level - 1]));
            }
        }
      else
        {
          {
            LevelTimer sw = stopwatch(S, level, 0);
            MGX_TRY(mgx_vmult_residual(S->matrix[level], S->defect[level], S->solution_update[level], S->t[level])); // :663
          }
          {
            LevelTimer sw = stopwatch(S, level, 1);
            MGX_HIP(hipMemsetAsync(S->defect[level - 1], 0, number_size(S->vnumber) * nc, s));         // :667
            MGX_TRY(mgx_restrict_and_add(S->transfer[level], S->defect[level - 1], S->t[level], 1)); // :668
          }
        }
      MGX_TRY(v_cycle(S, level - 1, 1)); // :671
      // :674 + :678.  On one rank with the macro-element brick loop the prolongation is not a kernel of
      // its own: the first post-smoothing iteration forms x + P x_coarse while it gathers x
      if (!fused_prolong_blocker(S->transfer[level], S->ctx->tun, S->smooth[level]->info.degree))
        {
          LevelTimer sw = stopwatch(S, level, 5);
          MGX_TRY(smoother_apply(S->smooth[level], S->solution_update[level], S->defect[level], true,
                                 S->solution_update[level - 1], S->transfer[level]->d.coarse_blocks, &S->transfer[level]->d));
        }
      else
        {
          {
            LevelTimer sw = stopwatch(S, level, 2);
            MGX_TRY(mgx_prolongate(S->transfer[level], S->solution_update[level], S->solution_update[level - 1], 1,
                                   1)); // :674
          }
          {
            LevelTimer sw = stopwatch(S, level, 5);
            MGX_TRY(smoother_apply(S->smooth[level], S->solution_update[level], S->defect[level], true)); // :678
          }
        }
    }
  return MGX_OK;
}

int mgx_solver_compute_rhs(mgx_solver_t S, int level, const double *rhs_q)
{
  MGX_REQUIRE(S && level >= 0 && level < S->n_levels, "mgx_solver_compute_rhs: bad argument");
  MGX_TRY(refuse_2d(S->matrix_dp[level]->d, "mgx_solver_compute_rhs",
                    "right-hand sides of a two-dimensional problem are assembled on the host"));
  // the boundary values in a vector of their own (the level's solution vector is the caller's)
  mgx_operator_t A = S->matrix_dp[level];
  DeviceArena    tmp("mgx_solver_compute_rhs");
  double        *u = nullptr;
  MGX_TRY(tmp.zeros(&u, A->d.n_dofs, S->ctx->stream));
  set_bc(S, level, u, false);
  const int status = mgx_compute_residual(A, S->rhs[level], u, rhs_q);
  (void)hipStreamSynchronize(S->ctx->stream);
  return status;
}

int mgx_solver_compute_rhs_2d(mgx_solver_t S, int level, const double *rhs_q)
{
  MGX_REQUIRE(S && level >= 0 && level < S->n_levels, "mgx_solver_compute_rhs_2d: bad argument");
  mgx_operator_t A = S->matrix_dp[level];
  MGX_TRY(refuse_3d(A, "mgx_solver_compute_rhs_2d", "mgx_solver_compute_rhs"));
  // the boundary values in a vector of their own (the level's solution vector is the caller's)
  DeviceArena tmp("mgx_solver_compute_rhs_2d");
  tmp.drain_before_release(S->ctx->stream);
  double *u = nullptr;
  MGX_TRY(tmp.zeros(&u, A->d.n_dofs, S->ctx->stream));
  set_bc(S, level, u, false);
  return mgx_compute_residual_2d(A, S->rhs[level], u, rhs_q);
}

int mgx_solver_solve(mgx_solver_t S, int do_analyze, double *reduction_rate, double *trace)
{
  return mgx_solver_solve_hooked(S, do_analyze, reduction_rate, trace, nullptr, nullptr);
}

int mgx_solver_solve_hooked(mgx_solver_t S, int do_analyze, double *reduction_rate, double *trace, mgx_level_hook hook,
                            void *user)
{
  MGX_REQUIRE(S, "mgx_solver_solve: null solver");
  hipStream_t s    = S->ctx->stream;
  double      rate = 1.;
  int         first_level = 1;
  if (S->agg_solver && S->agg_offset > 0)
    {
      // The levels of the whole mesh below level 0 of this hierarchy exist on the undecomposed copy only (cells of level
      // 1 dealt out to the ranks, mgx_cube_create_shell_ranks): the copy -- the same problem on every rank -- runs the
      // full multigrid cycle up to the seam, every rank takes the solution of its DoFs from there and goes on above it.
      mgx_solver_t        G  = S->agg_solver;
      const int           L  = S->agg_level, Lg = L + S->agg_offset;
      std::vector<double> gt(2 * (size_t)G->n_levels, 0.);
      MGX_TRY(mgx_solver_solve_hooked(G, do_analyze, &rate, gt.data(), nullptr, nullptr));
      launch_pack(s, MGX_F64, S->solution[L], G->solution[Lg], S->agg_map, (uint32_t)S->matrix[L]->d.n_dofs);
      if (trace)
        for (int l = 0; l <= L; ++l)
          {
            trace[2 * l]     = gt[2 * (size_t)(l + S->agg_offset)];
            trace[2 * l + 1] = gt[2 * (size_t)(l + S->agg_offset) + 1];
          }
      first_level = L + 1;
    }
  else
  {
    // coarse solver invoked twice (multigrid_solver.h:397-402)
    LevelTimer sw = stopwatch(S, 0, 0);
    const size_t n0 = S->matrix[0]->d.n_dofs;
    launch_copy_cast(s, S->defect[0], S->vnumber, S->rhs[0], MGX_F64, n0);
    MGX_TRY(smoother_apply(S->smooth[0], S->t[0], S->defect[0], false));
    MGX_TRY(smoother_apply(S->smooth[0], S->t[0], S->defect[0], true));
    launch_copy_cast(s, S->solution[0], MGX_F64, S->t[0], S->vnumber, n0);
    S->timings[1] += 2;
  }
  for (int level = first_level; level < S->n_levels; ++level)
    {
      const size_t n = S->matrix[level]->d.n_dofs;
      {
        LevelTimer sw = stopwatch(S, level, 3);
        set_bc(S, level - 1, S->solution[level - 1], false); // :408-409
      }
      {
        LevelTimer sw = stopwatch(S, level, 2);
        MGX_TRY(mgx_prolongate(S->transfer_dp[level], S->solution[level], S->solution[level - 1], 0, 0)); // :415
      }
      double init_residual = 1.;
      if (do_analyze && hook) // :420-424 "error start level"
        {
          MGX_HIP(hipStreamSynchronize(s));
          hook(user, level, 0);
        }
      set_bc(S, level, S->solution[level], true); // :427-428
      {
        LevelTimer sw = stopwatch(S, level, 0);
        MGX_TRY(mgx_vmult_residual(S->matrix_dp[level], S->rhs[level], S->solution[level], S->residual[level])); // :432
      }
      {
        LevelTimer sw = stopwatch(S, level, 4);
        launch_copy_cast(s, S->defect[level], S->vnumber, S->residual[level], MGX_F64, n); // :437
      }
      if (do_analyze)
        {
          MGX_TRY(mgx_operator_l2_norm(S->matrix_dp[level], S->residual[level], &init_residual)); // :444
          if (trace)
            trace[2 * level] = init_residual;
        }
      MGX_TRY(v_cycle(S, level, S->n_cycles)); // :451
      {
        LevelTimer sw = stopwatch(S, level, 4);
        launch_add_cast(s, S->solution[level], MGX_F64, S->solution_update[level], S->vnumber, n); // :456
      }
      if (do_analyze)
        {
          set_bc(S, level, S->solution[level], true);                                         // :462-463
          MGX_TRY(mgx_vmult(S->matrix_dp[level], S->residual[level], S->solution[level]));    // :464
          launch_sadd(s, MGX_F64, S->residual[level], -1., 1., S->rhs[level], n);             // :465
          double res_norm = 0;
          MGX_TRY(mgx_operator_l2_norm(S->matrix_dp[level], S->residual[level], &res_norm));        // :466
          rate = std::pow(res_norm / init_residual, 1. / S->n_cycles);                        // :467
          if (trace)
            trace[2 * level + 1] = res_norm;
          if (hook) // :468-472 "error end level"
            {
              MGX_HIP(hipStreamSynchronize(s));
              hook(user, level, 1);
            }
        }
    }
  MGX_HIP(hipGetLastError());
  if (reduction_rate)
    *reduction_rate = rate;
  return MGX_OK;
}

int mgx_solver_vmult(mgx_solver_t S, double *dst, const double *src)
{
  MGX_REQUIRE(S && dst && src, "mgx_solver_vmult: null argument");
  const int    lmax = S->n_levels - 1;
  const size_t n    = S->matrix[lmax]->d.n_dofs;
  hipStream_t  s    = S->ctx->stream;
  if (S->vnumber == MGX_F64 && dst != src && lmax > S->graph_level)
    {
      // same number type: the two precision-converting copies (:503, :507) are plain copies, so
      // the cycle runs on the caller's vectors instead (src is only read on the finest level,
      // every entry of dst is written by the pre-smoother)
      void *defect = S->defect[lmax], *update = S->solution_update[lmax];
      S->defect[lmax]          = const_cast<double *>(src);
      S->solution_update[lmax] = dst;
      const int status         = v_cycle(S, lmax, 1);
      S->defect[lmax]          = defect;
      S->solution_update[lmax] = update;
      return status;
    }
  launch_copy_cast(s, S->defect[lmax], S->vnumber, src, MGX_F64, n); // :503
  MGX_TRY(v_cycle(S, lmax, 1));                                       // :505
  launch_copy_cast(s, dst, MGX_F64, S->solution_update[lmax], S->vnumber, n); // :507
  return MGX_OK;
}

// SolverCG preconditioned by the V-cycle with ReductionControl(max_iterations, abs_tol, reduction)
static int solve_cg_control(mgx_solver_t S, unsigned int max_iterations, double abs_tol, double reduction,
                            unsigned int *iterations, double *reduction_rate, const char *not_converged)
{
  const int      lmax = S->n_levels - 1;
  const size_t   n    = S->matrix[lmax]->d.n_dofs;
  mgx_context_t  ctx  = S->ctx;
  hipStream_t    s    = ctx->stream;
  mgx_operator_t A    = S->matrix_dp[lmax];
  double        *x = S->solution[lmax], *r = S->cg_r, *z = S->cg_z, *d = S->cg_d, *h = S->cg_h;
  MGX_HIP(hipMemsetAsync(x, 0, 8 * n, s)); // :488
  launch_copy_cast(s, r, MGX_F64, S->rhs[lmax], MGX_F64, n);
  double res0 = 0;
  MGX_TRY(mgx_operator_l2_norm(A, r, &res0));
  // Mixed precision on one rank: the precision casts around the V-cycle (:503, :507) are folded into the CG
  // kernels next to them (mgx_vector.hip): the residual update writes the fp32 defect, the r.z product and the
  // direction update read the fp32 result of the cycle.  The values are those the two copies would produce.
  const bool mixed = S->vnumber == MGX_F32 && !ctx->has_comm;
  if (mixed)
    launch_copy_cast(s, S->defect[lmax], MGX_F32, r, MGX_F64, n);
  const float *z32 = mixed ? (const float *)S->solution_update[lmax] : nullptr;
  const auto   v_cycle_dot = [&](double *rz) {
    MGX_TRY(mixed ? v_cycle(S, lmax, 1) : mgx_solver_vmult(S, z, r)); // :505
    if (!mixed)
      return dot(ctx, MGX_F64, r, z, n, rz, A->plan.get());
    launch_dot_f64_f32(s, r, z32, n, ctx->partial_dev, ctx->result_dev);
    return read_result(ctx, rz);
  };
  CGOps<decltype(v_cycle_dot)> ops{A, x, r, z, d, h, v_cycle_dot, mixed ? (float *)S->defect[lmax] : nullptr, z32};
  krylov::SolveResult R;
  MGX_TRY(krylov::solve(ops, res0, max_iterations, abs_tol, reduction, &S->cg_history, R, iterations, reduction_rate));
  if (R.iterations >= max_iterations || R.above_tolerance) // (above: a step that broke down ended the iteration)
    return fail(MGX_ERR_NOT_CONVERGED, not_converged);
  return MGX_OK;
}

int mgx_solver_solve_cg(mgx_solver_t S, unsigned int *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S, "mgx_solver_solve_cg: null solver");
  // SolverCG with ReductionControl(1000, 1e-16, 1e-9) (:486)
  return solve_cg_control(S, 1000, 1e-16, 1e-9, iterations, reduction_rate,
                          "mgx_solver_solve_cg: no convergence in 1000 iterations");
}

/* minimal_surface/program.cc:514-528: the same solver with the caller's ReductionControl */
int mgx_solver_solve_cg_control(mgx_solver_t S, unsigned int max_iterations, double abs_tol, double reduction,
                                unsigned int *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S, "mgx_solver_solve_cg_control: null solver");
  MGX_REQUIRE(max_iterations >= 1 && abs_tol >= 0. && reduction >= 0., "mgx_solver_solve_cg_control: bad control values");
  return solve_cg_control(S, max_iterations, abs_tol, reduction, iterations, reduction_rate,
                          "mgx_solver_solve_cg_control: no convergence within max_iterations");
}

/* MultigridSolver::vmult_with_residual_update (multigrid_solver.h:516-619) */
int mgx_solver_vmult_with_residual_update(mgx_solver_t S, double *residual, double *update, double factor, double out[2])
{
  MGX_REQUIRE(S && residual && update && out && residual != update, "mgx_solver_vmult_with_residual_update: bad argument");
  const int      lmax = S->n_levels - 1;
  mgx_operator_t A    = S->matrix[lmax];
  mgx_context_t  ctx  = S->ctx;
  hipStream_t    s    = ctx->stream;
  const size_t   n    = A->d.n_dofs;
  if (!A->constrained_last)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_vmult_with_residual_update: the constrained DoFs must be numbered last "
                                     "(local_size_without_constraints, multigrid_solver.h:525)");
  if (ctx->has_comm)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_vmult_with_residual_update: single rank only");
  if (!A->cg_partials)
    {
      MGX_TRY(A->mem.alloc(&A->cg_partials, 4 * (size_t)(1u << 16)));
      MGX_TRY(A->mem.alloc(&A->cg_result, 4));
    }
  launch_residual_pre(s, S->vnumber, S->defect[lmax], residual, update, factor, n); // :527-534
  MGX_TRY(v_cycle(S, lmax, 1));                                                      // :538
  return residual_update_finish(s, S->vnumber, S->solution_update[lmax], residual, update, factor, n - A->d.n_constrained, n,
                                A->cg_partials, A->cg_result, out);
}

/* PCG with the matrix-vector product merged with the vector updates (mgx_vmult_with_cg_update):
 *   z = M r (q := z) ; loop: {x += alpha p ; p = beta p + q ; q = A p ; q.p} ; alpha = r.z / p.Ap ;
 *   {r -= alpha q ; r.r} ; {z = M r written into q ; r.z} ; beta = r.z_new / r.z_old
 * The residual update and the preconditioner are what vmult_with_residual_update merges; here the
 * V-cycle runs directly on r and q (no copies into and out of the level vectors in fp64), which
 * moves fewer bytes than the merged form: 3 + 2 instead of 3 + 5 passes next to the V-cycle.
 * Same iterates as mgx_solver_solve_cg up to round-off. */
int mgx_solver_solve_cg_fused(mgx_solver_t S, unsigned int *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S, "mgx_solver_solve_cg_fused: null solver");
  const int      lmax = S->n_levels - 1;
  const size_t   n    = S->matrix[lmax]->d.n_dofs;
  mgx_context_t  ctx  = S->ctx;
  hipStream_t    s    = ctx->stream;
  mgx_operator_t A    = S->matrix_dp[lmax];
  double        *x = S->solution[lmax], *r = S->cg_r, *q = S->cg_z, *p = S->cg_d;
  MGX_REQUIRE(!ctx->has_comm, "mgx_solver_solve_cg_fused: single rank only");
  MGX_HIP(hipMemsetAsync(x, 0, 8 * n, s));
  MGX_HIP(hipMemsetAsync(p, 0, 8 * n, s));
  launch_copy_cast(s, r, MGX_F64, S->rhs[lmax], MGX_F64, n);
  double res0 = 0;
  MGX_TRY(mgx_operator_l2_norm(A, r, &res0));
  MGX_TRY(mgx_solver_vmult(S, q, r)); // q = z_0 = M r_0
  double rz = 0;
  MGX_TRY(dot(ctx, MGX_F64, r, q, n, &rz));
  double       alpha = 0., beta = 0., res = res0;
  unsigned int it = 0;
  S->cg_history.assign(1, res0);
  while (res > 1e-16 && res > 1e-9 * res0 && it < 1000) // ReductionControl(1000, 1e-16, 1e-9), :486
    {
      ++it;
      double sums[4];
      MGX_TRY(mgx_vmult_with_cg_update(A, alpha, beta, r, q, p, x, S->cg_h, sums));
      alpha = rz / sums[0];
      const uint32_t used = launch_axpy_norm(s, MGX_F64, r, q, -alpha, n, A->cg_partials);
      launch_reduce4(s, A->cg_partials, used, nullptr, A->cg_result);
      MGX_TRY(mgx_solver_vmult(S, q, r));
      double h[4], rz_new = 0;
      MGX_HIP(hipMemcpyAsync(h, A->cg_result, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
      MGX_TRY(dot(ctx, MGX_F64, r, q, n, &rz_new)); // synchronises the stream
      res  = std::sqrt(h[2]);
      S->cg_history.push_back(res);
      beta = rz_new / rz;
      rz   = rz_new;
    }
  launch_sadd(s, MGX_F64, x, 1., alpha, p, n); // the update of x that the next step would have made
  if (iterations)
    *iterations = it;
  if (reduction_rate)
    *reduction_rate = it > 0 ? std::pow(res / res0, 1. / it) : 1.;
  MGX_HIP(hipGetLastError());
  if (it >= 1000)
    return fail(MGX_ERR_NOT_CONVERGED, "mgx_solver_solve_cg_fused: no convergence in 1000 iterations");
  return MGX_OK;
}

int mgx_solver_cg_history(mgx_solver_t S, double *history, int capacity, int *count)
{
  MGX_REQUIRE(S && count && (history || capacity == 0), "mgx_solver_cg_history: null argument");
  for (int i = 0; i < capacity && i < (int)S->cg_history.size(); ++i)
    history[i] = S->cg_history[i];
  *count = (int)S->cg_history.size();
  return MGX_OK;
}

int mgx_solver_do_matvec(mgx_solver_t S)
{
  MGX_REQUIRE(S, "mgx_solver_do_matvec: null solver");
  const int lmax = S->n_levels - 1;
  return mgx_vmult(S->matrix_dp[lmax], S->residual[lmax], S->solution[lmax]); // :627
}

int mgx_solver_do_matvec_smoother(mgx_solver_t S)
{
  MGX_REQUIRE(S, "mgx_solver_do_matvec_smoother: null solver");
  const int lmax = S->n_levels - 1;
  return mgx_vmult(S->matrix[lmax], S->solution_update[lmax], S->defect[lmax]); // :636
}

int mgx_solver_get_solution(mgx_solver_t S, int level, int insert_bc, const double **dptr)
{
  MGX_REQUIRE(S && dptr && level >= 0 && level < S->n_levels, "mgx_solver_get_solution: bad argument");
  if (insert_bc)
    set_bc(S, level, S->solution[level], false); // :379-380
  *dptr = S->solution[level];
  return MGX_OK;
}

int mgx_solver_get_vector(mgx_solver_t S, int level, int which, void **dptr)
{
  MGX_REQUIRE(S && dptr && level >= 0 && level < S->n_levels, "mgx_solver_get_vector: bad argument");
  switch (which)
    {
      case 0: *dptr = S->rhs[level]; break;
      case 1: *dptr = S->residual[level]; break;
      case 2: *dptr = S->defect[level]; break;
      case 3: *dptr = S->t[level]; break;
      case 4: *dptr = S->solution_update[level]; break;
      default: return fail(MGX_ERR_INVALID_ARGUMENT, "mgx_solver_get_vector: unknown vector id");
    }
  return MGX_OK;
}

// One V-cycle on the solver's own level vectors: defect[maxlevel] in, solution_update[maxlevel]
// out (mgx_solver_get_vector ids 2 and 4), for a caller that puts another level on top of the
// hierarchy (MultigridSolverDG::dg_v_cycle calls v_cycle(maxlevel, 1), multigrid_solver_dg.h:622)
int mgx_solver_v_cycle(mgx_solver_t S)
{
  MGX_REQUIRE(S, "mgx_solver_v_cycle: null solver");
  return v_cycle(S, S->n_levels - 1, 1);
}

// Re-creates the smoother of one level with other parameters (MultigridSolverDG sets up its FE_Q
// hierarchy with degree_pre - 1 on the finest level and a coarse tolerance of 2e-3,
// multigrid_solver_dg.h:271-291); degree < 0: from the tolerance, as on the coarsest level
int mgx_solver_reset_smoother(mgx_solver_t S, int level, double smoothing_range, int degree, int eig_cg_n_iterations)
{
  MGX_REQUIRE(S && level >= 0 && level < S->n_levels, "mgx_solver_reset_smoother: bad argument");
  MGX_REQUIRE(S->agg_solver == nullptr, "mgx_solver_reset_smoother: not on an agglomerated hierarchy");
  mgx_smoother_t sm = nullptr;
  MGX_TRY(mgx_smoother_create(S->matrix[level], smoothing_range, degree, eig_cg_n_iterations, &sm));
  MGX_TRY(mgx_smoother_destroy(S->smooth[level]));
  S->smooth[level] = sm;
  if (S->graph_exec) // the captured launches belong to the old smoother
    {
      MGX_HIP(hipStreamSynchronize(S->ctx->stream));
      (void)hipGraphExecDestroy(S->graph_exec);
      (void)hipGraphDestroy(S->graph);
      S->graph_exec  = nullptr;
      S->graph       = nullptr;
      S->graph_calls = 0;
    }
  return MGX_OK;
}

/* LaplaceProblem::solve, minimal_surface/program.cc:425-488: the state on every level, the coefficient of every level
 * operator from it, diagonals, smoothers */
int mgx_solver_update_coefficient(mgx_solver_t S, int law, const double *state_fine)
{
  MGX_REQUIRE(S && state_fine, "mgx_solver_update_coefficient: null argument");
  if (S->ctx->has_comm)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_update_coefficient: not on a context with a communicator (single rank only)");
  if (S->agg_solver)
    return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_update_coefficient: not on an agglomerated hierarchy");
  const int nl = S->n_levels, lmax = nl - 1;
  for (int l = 0; l < nl; ++l) // everything that can be refused is refused before the first level changes
    {
      MGX_TRY(require_coefficient_update(S->matrix_dp[l], law, "mgx_solver_update_coefficient"));
      // curved cells: a V-cycle operator of another precision that was told no geometry of its own is written below
      // with the tables, state and geometry of matrix_dp[l]; only its coef_q is needed
      const bool written_from_dp = S->matrix[l] != S->matrix_dp[l] && S->matrix_dp[l]->unit_q && !S->matrix[l]->coef_update;
      if (!written_from_dp)
        MGX_TRY(require_coefficient_update(S->matrix[l], law, "mgx_solver_update_coefficient"));
      else if (!S->matrix[l]->d.coef_q)
        return fail(MGX_ERR_UNSUPPORTED, "mgx_solver_update_coefficient: a V-cycle operator has no per-point coefficient");
    }
  hipStream_t s = S->ctx->stream;
  if (S->nl_state.empty())
    {
      S->nl_state.assign(nl, nullptr);
      for (int l = 0; l < nl; ++l)
        {
          const size_t n = S->matrix_dp[l]->d.n_dofs;
          if (l < lmax)
            MGX_TRY(S->mem.alloc(&S->nl_state[l], n));
        }
    }
  // :425-457 (the reference interpolates in the level number type; here in fp64)
  for (int l = lmax; l > 0; --l)
    MGX_TRY(mgx_interpolate_to_coarse(S->transfer_dp[l], S->nl_state[l - 1], l == lmax ? state_fine : S->nl_state[l]));
  for (int l = 0; l < nl; ++l)
    {
      const double *state = l == lmax ? state_fine : S->nl_state[l];
      MGX_TRY(mgx_evaluate_coefficient(S->matrix_dp[l], law, state)); // :458 / :469
      if (S->matrix[l] != S->matrix_dp[l])
        {
          // The fp32 operator of the level receives the fp64 tensor, rounded: evaluated with the tables of matrix_dp
          // from the fp64 state.  (The reference evaluates in level_number from the state cast to it, :469; the fp32
          // tensor would then sit about 1e-7 from the fp64 one instead of at its rounding, and the level operators of
          // the two precisions would no longer be the same operator up to storage.)
          mgx_operator_t A = S->matrix_dp[l], V = S->matrix[l];
          MGX_REQUIRE(V->d.n_cells == A->d.n_cells && V->d.p == A->d.p, "mgx_solver_update_coefficient: level operators differ");
          launch_evaluate_coefficient(s, A->d, V->d.coef_q, V->d.number, law == MGX_LAW_MINIMAL_SURFACE, A->metric, A->det_jacobian,
                                      A->unit_q, A->jxw_q, state);
          MGX_HIP(hipGetLastError());
          V->has_diag = false;
        }
      // :484, and the smoother with the parameters it was created with (:470-487: a new eigenvalue estimate)
      MGX_TRY(mgx_compute_diagonal(S->matrix[l]));
      mgx_smoother_t old = S->smooth[l], sm = nullptr;
      MGX_TRY(mgx_smoother_create(S->matrix[l], old->req_range, old->req_degree, old->req_eig_its, &sm));
      if (old->fourth_kind)
        MGX_TRY(mgx_smoother_set_polynomial_type(sm, MGX_CHEBYSHEV_FOURTH_KIND));
      MGX_TRY(mgx_smoother_destroy(old));
      S->smooth[l] = sm;
    }
  if (S->graph_exec) // the captured launches carry the old smoothers' buffers and factors
    {
      MGX_HIP(hipStreamSynchronize(s));
      (void)hipGraphExecDestroy(S->graph_exec);
      (void)hipGraphDestroy(S->graph);
      S->graph_exec = nullptr;
      S->graph      = nullptr;
    }
  S->graph_calls = 0;
  return MGX_OK;
}

// level operators of a solver (V-cycle number type / fp64)
int mgx_solver_get_operator(mgx_solver_t S, int level, int fp64, mgx_operator_t *op)
{
  MGX_REQUIRE(S && op && level >= 0 && level < S->n_levels, "mgx_solver_get_operator: bad argument");
  *op = fp64 ? S->matrix_dp[level] : S->matrix[level];
  return MGX_OK;
}

int mgx_solver_n_levels(mgx_solver_t S) { return S ? S->n_levels : 0; }

// device view of an operator's compressed index table (the DG <-> FE_Q transfer of the DG level reads it)
int mgx_operator_device_indices(mgx_operator_t op, const uint32_t **idx27, uint32_t *n_cells, uint32_t *n_dofs, int *degree)
{
  MGX_REQUIRE(op, "mgx_operator_device_indices: null operator");
  if (idx27)
    *idx27 = op->d.idx27;
  if (n_cells)
    *n_cells = op->d.n_cells;
  if (n_dofs)
    *n_dofs = op->d.n_dofs;
  if (degree)
    *degree = op->d.p;
  return MGX_OK;
}

int mgx_solver_get_smoother(mgx_solver_t S, int level, mgx_smoother_t *sm)
{
  MGX_REQUIRE(S && sm && level >= 0 && level < S->n_levels, "mgx_solver_get_smoother: bad argument");
  *sm = S->smooth[level];
  return MGX_OK;
}

int mgx_solver_get_timings(mgx_solver_t S, double *timings)
{
  MGX_REQUIRE(S && timings, "mgx_solver_get_timings: null argument");
  std::copy(S->timings.begin(), S->timings.end(), timings);
  std::fill(S->timings.begin(), S->timings.end(), 0.); // print_wall_times resets :368-370
  return MGX_OK;
}

int mgx_solver_enable_timings(mgx_solver_t S, int enable)
{
  MGX_REQUIRE(S, "mgx_solver_enable_timings: null solver");
  S->timing = enable != 0;
  return MGX_OK;
}

} // extern "C"
