// mgx_internal.hpp -- internal C++ interface between the C ABI (mgx_api.cpp) and the HIP kernels
// (mgx_kernels.hip).  Not installed; the public boundary is include/mgx.h.
#pragma once

#include "../../include/mgx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

struct mgx_context_s;

namespace mgx
{
  constexpr int      kMaxN    = MGX_MAX_DEGREE + 1;
  constexpr uint32_t kInvalid = 0xFFFFFFFFu;

  // Options of a context, carried by the objects built on it (two contexts of one process can differ:
  // the tests compare code paths that way).  The thresholds marked ENV are also read from the
  // environment, ONCE, when a context is created; everything else is set only through
  // mgx_context_set_option(ctx, "<name>", value) before the first object is created on the context.
  // All but rccl_selftest select between numerically equivalent code paths or set thresholds.
  struct Tunables
  {
    bool     trace            = false; // MGX_TRACE            host control flow on stderr
    bool     general_kernel   = false; // MGX_GENERAL_KERNEL   quadrature-point form instead of the separable one
    bool     no_bricks        = false; // MGX_NO_BRICKS        per-cell kernel on every level
    uint32_t brick_min        = 512;   // MGX_BRICK_MIN        bricks per level from which the brick loop is used (measured crossover with the per-cell kernel: between 216 and 512 bricks)
    bool     brick_min_from_env = false;
    uint32_t overlap_min      = 16384; // MGX_OVERLAP_MIN_BRICKS  bricks per rank from which interface bricks run first
    bool     cells_form       = false; // MGX_BRICK_FORM=cells cell-by-cell brick kernel instead of the macro-element one
    uint32_t wide_max         = 1024;  // MGX_BRICK_WIDE_MAX   cell-by-cell form: launches below this use 512 threads
    bool     dg_no_overlap    = false; // MGX_DG_NO_OVERLAP        DG ghost exchange before all cells instead of under the interior ones
    bool     no_restrict_scratch = false; // fused residual + restriction adds into the coarse vector colour by colour instead of through per-brick blocks
    bool     no_fused_residual = false;  // V-cycle: residual and restriction as separate kernels, the prolongation form stays fused
    bool     no_fused_assembly = false;  // per-cell levels: Chebyshev update as a kernel after the assembly kernel
    bool     no_fused_decomposed = false; // decomposed levels: residual / restriction / prolongation as separate kernels
    bool     dg_unmerged_restrict = false; // DG V-cycle: residual and DG -> FE_Q restriction as two kernels instead of the merged action 1
    uint32_t macro_wg_x16     = 0;     // MGX_MACRO_WG_PER_CU_X16  macro kernel grid, in 1/16 workgroups per CU [resident]
    bool     no_diag_table    = false; // MGX_NO_DIAG_TABLE    stream the inverse diagonal in the fused Chebyshev forms
    bool     roctx            = false; // profiler ranges with the reference's LIKWID region names (mgx_range_push/pop, per-level phases of the V-cycle)
    uint32_t fused_prolong_min_bricks = 8192; // p <= 4, levels on a reduced-colour schedule with fewer bricks (per rank): prolongation as a kernel of its own + first post-smoothing step on that schedule (17 M-DoF level of C2: 0.894 against 0.905 ms; emulated rank at 8 GPUs 2.417 against 2.446 ms; a 67 M-DoF rank level, 16 384 bricks, is faster fused: 5.42 against 5.48 ms; 0: fused everywhere)
    bool     no_general_bricks = false; // general tensor branch: per-cell kernel + ordered assembly also where the brick form exists (A/B, tests)
    uint32_t general_brick_min = 2048;  // ... bricks from which vmult of a general operator runs in brick form (one workgroup per brick, 512 resident: below four rounds of workgroups the per-cell kernel with its 16 waves per CU is faster)
    bool     no_macro_v2      = false; // first pipeline of the macro-element kernel (gather after the sweeps) for every form; A/B of mgx_macro2.hip
    bool     no_fused_init    = false; // MGX_NO_FUSED_INIT    store the first Chebyshev iterate
    bool     no_fused_restrict = false; // MGX_NO_FUSED_RESTRICT  separate residual and restriction kernels
    bool     no_fused_prolong = false; // MGX_NO_FUSED_PROLONG prolongation as a kernel of its own
    bool     force_fused_transfers = false; // (no-op since round 4: the fused transfer forms run at every degree)
    bool     transfer_v1      = false; // MGX_TRANSFER_V1      first-version transfer kernels
    bool     restrict_atomic  = false; // MGX_RESTRICT_ATOMIC  one-launch restriction with atomics on every level
    uint32_t restrict_colour_min = 16384; // MGX_RESTRICT_COLOUR_MIN  coarse cells from which restriction runs by colour
    bool     exchange_unfused = false; // MGX_EXCHANGE_UNFUSED one pack / unpack launch per neighbour
    uint32_t cell_colour_min  = 0xFFFFFFFFu; // MGX_CELL_COLOUR_MIN  general-coefficient levels from this many cells run colour by colour; by default only levels whose ordered-assembly tables would not fit do (measured on the shell meshes: one launch + ordered assembly 20 / 56 / 119 / 463 us at 6 k / 25 k / 49 k / 197 k cells against 103 / 136 / 202 / 540 us for the 13 colour launches of the greedy colouring)
    uint32_t free_max_bricks  = 16384; // MGX_FREE_MAX_BRICKS  levels with at most this many bricks run the plain / residual / Chebyshev forms of the brick loop on a reduced-colour schedule (mgx_macro.hip, FREE) instead of eight colour launches
    uint32_t free_one_max     = 1024;  // MGX_FREE_ONE_MAX     ... with one class (one launch) up to this many bricks, two classes beyond
    bool     no_graph         = false; // MGX_NO_GRAPH         no HIP-graph replay of the coarse levels
    uint32_t graph_max_dofs   = 600000; // MGX_GRAPH_MAX_DOFS  largest level inside the replayed graph
    bool     rccl_selftest    = false; // MGX_RCCL_SELFTEST    one-rank communicator may name itself as neighbour
    static Tunables from_environment();
    bool            set(const std::string &name, double value); // false: unknown option
  };

  // 1D data of the element in the operator's number type, resident in device memory and read
  // through wave-uniform (scalar) loads.
  // Even-odd (Appendix B of SURVEY.md, matrix_vector_kernel.h:47-113) form of a symmetric and
  // persymmetric n x n matrix A (A[a][b] = A[b][a] = A[n-1-a][n-1-b]), H = n/2:
  //   ee[a*H+i] = (A[a][i] + A[a][n-1-i])/2, eo[a*H+i] = (A[a][i] - A[a][n-1-i])/2  (a,i < H)
  //   mc[a] = A[a][H] (odd n: middle column = middle row), mhh = A[H][H]
  template <typename T>
  struct EOMat
  {
    T ee[(kMaxN / 2) * (kMaxN / 2)];
    T eo[(kMaxN / 2) * (kMaxN / 2)];
    T mc[kMaxN / 2];
    T mhh;
  };

  template <typename T>
  struct Basis1D
  {
    T S[kMaxN * kMaxN];       // S[q*n+i]   nodal -> quadrature
    T D[kMaxN * kMaxN];       // D[q*n+r]   collocation derivative
    T w[kMaxN];               // quadrature weights
    T P1[2 * kMaxN * kMaxN];  // P1[a*n+i]  prolongation, a in [0,2p]
    // 1D mass and stiffness matrices of the separable (Cartesian, constant coefficient) cell
    // matrix  A_cell = sum_d c_d (M x M x K_d):  M = S^T W S,  K = S^T D^T W D S
    EOMat<T> mass, lapl;
    // P1 in even-odd form for the line products of the fused transfer forms (restrict_half / prolong_line,
    // mgx_brick_device.hpp).  The embedding of a parent into its two children is symmetric under reversal of both
    // indices, P1[2p-a][p-j] = P1[a][j] (checked when the transfer is created).  With nh = (p+1)/2 pairs (j, p-j):
    //   HE[a*nh+j] = (P1[a][j] + P1[a][p-j]) / 2, a <= p;  HO[a*nh+j] = (P1[a][j] - P1[a][p-j]) / 2, a < p;
    //   PC[a] = P1[a][p/2], a <= p (p even: the coarse point in the middle of the parent)
    // at offsets 0, (p+1) nh, (2p+1) nh.
    T P1eo[2 * kMaxN * kMaxN];
  };

  // Reduced-colour schedule of the macro-element kernel (mgx_macro.hip, FREE; built by
  // build_free_schedule, mgx_bricks.cpp): one or two classes of bricks instead of eight colours.  The
  // entities bricks of one class share are PRIVATE: every brick stores their partial sums in a block
  // of its own, priv[brick][n_surf], and launch_surf_finish adds the blocks up per DoF (entries
  // surf_pos[surf_start[i] .. surf_start[i+1]) for DoF surf_dof[i], ascending) and applies the
  // post-operation.  The first n_surf_shared DoFs of that list are shared with other ranks: their
  // sum goes to the carrier vector and is completed after the exchange.
  struct FreeSchedule
  {
    int       n_classes = 0;                    // 1 or 2
    int       n_groups = 0, n_iface_groups = 0; // launch groups (classes, interface bricks first if split)
    uint32_t  group_start[9] = {0};
    uint32_t *ent         = nullptr; // device [n_bricks * entities]: entity table in group order, flags of this schedule
    uint32_t *surf_off    = nullptr; // device [entities per brick]: offset of a private entity in a block, kInvalid: not private
    uint32_t  n_surf      = 0;       // values per block
    void     *priv        = nullptr; // device, number type
    uint32_t *surf_dof    = nullptr, *surf_start = nullptr, *surf_pos = nullptr;
    uint32_t  n_surf_dofs = 0, n_surf_shared = 0;
    bool      available() const { return ent != nullptr; }
  };

  // Brick schedule of a level (mgx_brick.hip): 64-cell bricks sorted by colour, one launch per
  // colour; per brick the first DoF of each of its 9^3 mesh entities and the FIRST/LAST flags.
  struct BrickData
  {
    uint32_t  n_bricks  = 0;
    int       n_colours = 0;       // launch groups
    int       n_iface_groups = 0;  // leading groups = bricks on the rank interface (0: not split)
    uint32_t  colour_start[33] = {0};
    uint32_t *ent_base  = nullptr; // device [n_bricks * 729]
    uint8_t  *ent_flags = nullptr; // device [n_bricks * 729]  bit0 FIRST, bit1 LAST
    uint32_t *item_map  = nullptr; // device [(NB p + 1)^3]: write-out order of the macro-element kernel
    uint32_t *item_map2 = nullptr; // device: the same items, interior of the brick first (second pipeline, mgx_macro2.hip)
    std::vector<uint32_t> order; // host: colour-sorted position -> brick index in cell order
    uint32_t *order_dev = nullptr; // device copy (general operator: brick_general_kernel finds its cells through it)
    bool      available() const { return n_bricks > 0; }
    FreeSchedule fr; // reduced-colour schedule of the plain / residual / Chebyshev forms (may be absent)
  };
  constexpr int kBrickEntities = 729;
  constexpr int kMaxColours    = 32;

  // The cells of the launches of a per-cell kernel: list k is cells[start[k] .. start[k + 1]), and the cells of one list
  // share no DoF (plain adds).  cells: device; start: host, n + 1 offsets; n == 0: one launch over all cells.
  struct CellLists
  {
    const uint32_t *cells = nullptr;
    const uint32_t *start = nullptr;
    int             n     = 0;
    CellLists() = default;
    CellLists(const uint32_t *cells_, const uint32_t *start_, int n_) : cells(cells_), start(start_), n(n_) {}
  };
  // Cells sorted by colour, at most 32 colours (CellColouring of mgx_index_tables.hpp with the order on the device):
  // colour k is order[start[k] .. start[k + 1]).  order == nullptr: not coloured.
  struct ColourLists
  {
    uint32_t *order     = nullptr; // device [n_cells]
    int       n         = 0;
    uint32_t  start[33] = {0};
    CellLists lists() const { return CellLists(order, start, n); }
  };

  // Device-side view of a LaplaceOperator level (laplace_operator.h:126-163)
  struct OperatorData
  {
    int       p        = 0;
    int       number   = 1; // MGX_F64
    // 3: hexahedra.  2: quadrilaterals (mgx_kernels_2d.hip) -- idx27 / idx27_plain hold 9 entries per cell, coef is
    // [xx,yy,xy], coef_q [n_cells][3][n^2], cell_scratch and asm_pos count n^2 local values per cell, and there is no
    // brick schedule: ordered assembly or cell colours, for the separable form too
    int       dim      = 3;
    uint32_t  n_cells  = 0;
    uint32_t  n_dofs   = 0;
    uint32_t  n_constrained = 0;
    uint32_t *idx27         = nullptr; // device
    uint32_t *idx27_plain   = nullptr; // device (may be null)
    uint32_t *constrained   = nullptr; // device
    void     *basis         = nullptr; // device Basis1D<T>
    void     *inv_diag      = nullptr; // device, number type
    double    coef[6]       = {0, 0, 0, 0, 0, 0};
    bool      full_tensor   = false;   // affine cells with off-diagonal coefficient entries (:473-486)
    void     *coef_q        = nullptr; // device [n_cells][6][n^3], number type: general branch (:493-522)
    void     *grad_1d       = nullptr; // device [n*n], number type: G = D S, nodal derivative at the quadrature points
    // general branch on levels with many cells: cells sorted by colour (cells of one colour share
    // no DoF), one launch per colour without atomics; nullptr: one launch with atomic adds
    ColourLists cell_colours;
    // Ordered assembly of the per-cell kernels (levels without a brick schedule and without cell
    // colours): the kernels store each cell's (p+1)^3 local results in cell_scratch and
    // assemble_kernel adds, for every DoF d, the entries asm_pos[asm_start[d] .. asm_start[d+1]) in
    // ascending cell order -- no atomics, bitwise reproducible.  nullptr: not built.
    uint32_t *asm_start     = nullptr; // device [n_dofs + 1]
    uint32_t *asm_pos       = nullptr; // device: cell (p+1)^3 + local index (k n + j) n + i
    void     *cell_scratch  = nullptr; // device [n_cells (p+1)^3], number type
    BrickData bricks;
    BrickData gbricks; // general tensor branch, p = 4, one rank: one-launch schedule of brick_general_kernel (fr, item_map)
    bool      cells_form    = false; // Tunables::cells_form of the context the operator was created on
    uint32_t  wide_max      = 1024;  // Tunables::wide_max
    uint32_t  macro_wg_x16  = 0;     // Tunables::macro_wg_x16
    uint32_t  n_cus         = 256;   // compute units of the device of the operator's context
    bool      separable     = true; // Cartesian constant-coefficient fast path of the brick loop
    // inverse diagonal per brick item ((NB p + 1)^3 values in item order) if it is the same for
    // every brick (uniform mesh), else nullptr: the macro-element kernel then reads it from
    // registers instead of streaming inv_diag (mgx_macro.hip, DTAB)
    void     *diag_items    = nullptr;
    void     *diag_items2   = nullptr; // ... in the order of bricks.item_map2 (second pipeline)
    bool      macro_v2      = true;    // !Tunables::no_macro_v2
  };

  struct TransferData
  {
    const OperatorData *coarse = nullptr, *fine = nullptr;
    uint32_t           *children = nullptr;    // device [n_coarse_cells*8]
    uint8_t            *weight_shift = nullptr; // device [n_coarse_cells*27]: weight = 2^-shift
    uint32_t           *own27 = nullptr;        // device [n_fine_cells]: bit e set iff the fine cell is
                                                // the first (in cell order) containing its entity e
    // pipelined transfers (mgx_transfer.hip): 125 words per parent for the 5^3 mesh entities of its
    // children patch: first fine DoF | log2(multiplicity) << 29 | owned-by-this-parent << 31;
    // nullptr if the fine level has 2^29 DoFs or more (first-version kernels are used then)
    uint32_t           *patch = nullptr;
    // fused residual + restriction (BrickMode kResidualRestrict): per fine brick, in the fine level's
    // colour-sorted brick order, the first coarse DoF (constrained: invalid) of the (2 PB + 1)^3 mesh
    // entities of the PB^3 parents the brick's cells belong to (PB = 2 for p <= 4, 1 for p >= 5)
    uint32_t           *coarse_blocks = nullptr;
    // ... restricted values per brick, [n_bricks][(PB p + 1)^3] in the number type, and the ordered assembly of the
    // coarse vector from them: coarse[d] = sum of coarse_scratch[cs_pos[k]], k in [cs_start[d], cs_start[d + 1]),
    // in ascending brick order (launch_coarse_assemble).  The bricks of a level then write disjoint addresses and the
    // fused residual + restriction is ONE launch per level.
    void               *coarse_scratch = nullptr;
    uint32_t           *cs_start = nullptr, *cs_pos = nullptr;
    // ... on a decomposed mesh: the DoFs on the rank interface, which no brick completes, are transferred by two
    // list kernels after the exchange.  Restriction (CSR by coarse DoF over the interface DoFs this rank owns):
    // coarse[ifr_cdof[i]] += sum_k ifr_w[k] r[ifr_fdof[k]], k in [ifr_start[i], ifr_start[i+1]).  Prolongation (CSR by
    // entry i of the fine plan's list of shared DoFs): (P e)[shared[i]] = sum_k ifp_w[k] e[ifp_cdof[k]]
    uint32_t           *ifr_cdof = nullptr, *ifr_start = nullptr, *ifr_fdof = nullptr;
    void               *ifr_w = nullptr;
    uint32_t            n_ifr = 0;
    uint32_t           *ifp_start = nullptr, *ifp_cdof = nullptr;
    void               *ifp_w = nullptr;
    uint32_t            n_ifp = 0;
    mutable uint32_t    pipe_grid[4] = {0, 0, 0, 0}; // persistent grid of prolongate(add), prolongate, restrict x2
    bool                owner_weights = false;   // restriction: weight 1 for the parent that owns a fine entity, 0 for the others (multi-block meshes)
    bool                coarse_coloured = false; // coarse cells c and c' with c % 8 == c' % 8 share no DoF
    // two dimensions (mgx_kernels_2d.hip): children [n_coarse_cells*4], weight_shift [n_coarse_cells*9], own27 the
    // ownership bits of the 9 entities of a fine cell; the restriction runs over the parents colour by colour
    // (parents of one colour share no DoF: plain adds)
    ColourLists         parent_colours;
    uint32_t            n_cus = 256;
    uint32_t            colour_min = 16384; // Tunables::restrict_colour_min
  };

  // transport of the context (mgx_api.cpp) for other translation units: exchange of packed device
  // buffers (counts[k] entries of `number` type with rank ranks[k], both directions), sum of a few
  // host doubles over the ranks (no-op on a single rank)
  int  exchange_buffers(struct ::mgx_context_s *ctx, int plan_id, int number, int n_neighbors, const int *ranks,
                        const uint32_t *counts, void *const *send, void *const *recv, hipStream_t stream = nullptr);
  // Overlap of an exchange with work on the context's stream: side_stream_begin returns the context's side stream, ordered
  // behind everything enqueued on the main stream so far (nullptr: no side stream, run in order);
  // side_stream_end orders the main stream behind the side stream again.
  hipStream_t side_stream_begin(struct ::mgx_context_s *ctx);
  int         side_stream_end(struct ::mgx_context_s *ctx);
  int  allreduce_sum(struct ::mgx_context_s *ctx, double *values, int count);
  int  dot_owned_prefix(struct ::mgx_context_s *ctx, int number, const void *x, const void *y, size_t n, double *out);
  bool context_has_comm(struct ::mgx_context_s *ctx);
  int  operator_dim(struct ::mgx_operator_s *op); // 3 or 2 (mgx_operator_desc::dim)
  const Tunables &context_tunables(struct ::mgx_context_s *ctx);
  // One part of a V-cycle of a multigrid solver, timed into times[part] of its level when `timed` (print_wall_times of
  // the reference: host timers around synchronised parts -- for diagnosis, the parts no longer overlap their launches);
  // ranges: a roctx range named after the part and the level around it, where the context's options ask for ranges
  struct LevelTimer
  {
    struct ::mgx_context_s               *ctx;
    double                               *slot; // null: not timed
    bool                                  ranges;
    std::chrono::steady_clock::time_point t0;
    LevelTimer(struct ::mgx_context_s *ctx, bool timed, double *times, int level, int part, bool with_ranges = false);
    ~LevelTimer();
    LevelTimer(const LevelTimer &) = delete;
  };
  // the part of vmult_with_residual_update after the V-cycle (multigrid_solver.h:543-619): the post kernel on the cycle's
  // result, the block sums added in a fixed order, and the first two of the four sums on the host
  int residual_update_finish(hipStream_t s, int number, const void *cycle_result, double *residual, double *update, double factor,
                             size_t n_free, size_t n, double *partials, double *sums_dev, double out[2]);

  // records the message mgx_last_error() returns on the calling thread; returns `code` (used by the
  // translation units that implement parts of the C ABI outside mgx_api.cpp)
  int report_error(int code, const char *message);
  inline int report_error(int code, const std::string &message) { return report_error(code, message.c_str()); }

// status plumbing of the host code behind the C ABI (the codes are those of include/mgx.h): a failed HIP call, a failed
// callee, a refused argument -- each returns from the calling function with the status
#define MGX_HIP(call)                                                                                                \
  do                                                                                                                 \
    {                                                                                                                \
      hipError_t e_ = (call);                                                                                        \
      if (e_ != hipSuccess)                                                                                          \
        return mgx::report_error(MGX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                                                std::to_string(__LINE__) + ")");                                     \
    }                                                                                                                \
  while (0)

#define MGX_TRY(call)     \
  do                      \
    {                     \
      int s_ = (call);    \
      if (s_ != MGX_OK)   \
        return s_;        \
    }                     \
  while (0)

#define MGX_REQUIRE(cond, msg)                                      \
  do                                                                \
    {                                                               \
      if (!(cond))                                                  \
        return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, (msg));  \
    }                                                               \
  while (0)

  void launch_prolongate_pipe(hipStream_t s, const TransferData &t, void *fine, const void *coarse, bool add,
                              bool with_constraints);
  void launch_restrict_add_pipe(hipStream_t s, const TransferData &t, void *coarse, const void *fine,
                                bool with_constraints);

  // ---- cell loops (mgx_kernels.hip, mgx_kernels_2d.hip, mgx_nonlinear_2d.hip) ----
  // The list loop of the per-cell kernels: launch(list, count, scratch) once per non-empty list of cells that share no
  // DoF (plain adds); with no lists once over all cells, into the scratch array of the ordered assembly if `ordered`
  // (the caller assembles), else with atomic adds.  Returns the scratch array the launch wrote, or nullptr.
  template <typename T, typename F>
  static T *for_each_cell_list(const OperatorData &op, const CellLists &lists, bool ordered, F &&launch)
  {
    T *scratch = (lists.n == 0 && ordered) ? (T *)op.cell_scratch : nullptr;
    if (lists.n == 0 && op.n_cells > 0)
      launch((const uint32_t *)nullptr, op.n_cells, scratch);
    for (int k = 0; k < lists.n; ++k)
      if (const uint32_t count = lists.start[k + 1] - lists.start[k])
        launch(lists.cells + lists.start[k], count, scratch);
    return scratch;
  }
  // The symmetric tensor [xx,yy,zz,xy,xz,yz] a general kernel applies (PERQ decides which it reads): one per cell and
  // quadrature point, device [n_cells][6][n^3] in the kernel's number type, or one per mesh; the other is null / zero.
  struct CellTensor
  {
    const void *per_point = nullptr;
    double      c[6]      = {0, 0, 0, 0, 0, 0};
    static CellTensor at_points(const void *q)
    {
      CellTensor t;
      t.per_point = q;
      return t;
    }
    static CellTensor per_mesh(const double *m)
    {
      CellTensor t;
      std::copy(m, m + 6, t.c);
      return t;
    }
    // the coefficient of an operator of the general branch
    static CellTensor of(const OperatorData &op) { return op.coef_q ? at_points(op.coef_q) : per_mesh(op.coef); }
  };
  // dst += A_cells * src  (MatrixFree::cell_loop(local_apply), laplace_operator.h:527-558)
  // op.asm_start (ordered assembly): dst is WRITTEN (no zeroing by the caller), and dst[d] = tail_src[d] for
  // d >= n_head if tail_src is given; otherwise dst must be zero on entry
  // post (ordered assembly only): the Chebyshev update of PreconditionChebyshev inside the assembly kernel instead of
  // a kernel of its own -- src is the iterate x, updated in place after every cell has read it:
  //   x_new = x + f2 dinv (b - A x) [+ f1 (x - x_old), three_term];  x_old = x;  rows >= n_head: A x = x (identity rows)
  struct ChebPost
  {
    void       *x_old;
    const void *b, *dinv;
    double      f1, f2;
    bool        three_term;
  };
  void launch_cell_loop(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *tail_src = nullptr,
                        uint32_t n_head = 0,
                        const ChebPost *post = nullptr);
  // general operator, brick form (p = 4, OperatorData::gbricks; mgx_kernels.hip brick_general_kernel)
  void launch_general_bricks(hipStream_t s, const OperatorData &op, void *dst, const void *src);
  // mode 0: dst = ordered sums of op.cell_scratch (tail as above), mode 1: dst += them
  void launch_assemble(hipStream_t s, const OperatorData &op, int mode, void *dst, const void *tail_src, uint32_t n_head);
  // the same assembly with the Chebyshev update as its post-operation (ChebPost): x is the iterate, updated in place
  void launch_assemble_cheb(hipStream_t s, const OperatorData &op, void *x, uint32_t n_head, const ChebPost &post);
  // ---- brick loop (mgx_macro.hip, mgx_macro2.hip; cross-check builds: mgx_brick.hip) ----
  // fused post-operations (what the reference passes as operation_after_loop).  The values are public: they are the
  // form numbers of mgx_profile_read
  enum BrickMode
  {
    kPlain    = 0, // out = A src                                   (vmult, laplace_operator.h:573)
    kResidual = 1, // out = a - A src                               (vmult_residual, :605)
    kCheb     = 2, // out = x + f1 (x - out) + f2 b (a - A x)       (PreconditionChebyshev update)
    kChebFirst = 3, // out = x + f2 b (a - A x)                     (first step: no x_old term)
    kChebZeroOld = 4, // out = x + f1 x + f2 b (a - A x)             (x_old known to be zero)
    // start of PreconditionChebyshev::vmult (zero initial guess): the first iterate x_1 = f0 b a is
    // never stored -- the first loop iteration computes it while gathering (kChebInit, x_old = 0),
    // the second one recomputes it as its x_old (kChebOldInit); separable kernel only
    kChebInit    = 5, // x := f0 b a ; out = x + f1 x + f2 b (a - A x)
    kChebOldInit = 6, // out = x + f1 (x - f0 b a) + f2 b (a - A x)
    // V-cycle: the residual a - A x is only needed restricted to the next coarser level
    // (multigrid_solver.h:663-668).  Every brick restricts the residual values it completes (its
    // LAST points, everything else masked to zero) with the transposed embedding and adds the
    // (PB p + 1)^3 coarse values to the coarse vector; the residual itself is never stored.
    kResidualRestrict = 7,
    // fused PCG step (vmult_with_cg_update, laplace_operator.h:638-719; macro-element kernel only):
    // the gather forms p_new = f2 p + q (f1 == 0: p_new = q); at completion x += f1 p_old,
    // p = p_new, q = A p_new, and q.p, r.r, q.r, q.q are accumulated per workgroup
    kCgUpdate = 8,
    // first post-smoothing iteration of the V-cycle with the coarse-grid correction formed on the
    // fly (multigrid_solver.h:674-678; macro-element kernel only): the gather adds the prolongated
    // coarse values to x (prolong_brick), the iteration is kChebFirst on the corrected x, which is
    // also written back at completion (it is x_old of the next iteration).  coarse / coarse_blocks
    // as for kResidualRestrict.
    kChebFirstProlong = 9
  };
  // the fused Chebyshev forms (they use the inverse diagonal and keep the source value)
  __host__ __device__ constexpr bool is_cheb_mode(int mode)
  {
    return (mode >= kCheb && mode <= kChebOldInit) || mode == kChebFirstProlong;
  }
  // the forms that run on the reduced-colour schedules (FreeSchedule) where a level has one
  constexpr bool on_free_schedule(int mode) { return mode >= kPlain && mode <= kChebOldInit; }

  // One launch of the brick loop over the launch groups [group_begin, group_end) of a level, and the operands of the
  // list kernels that complete it (launch_surf_finish, launch_unpack_ordered_cheb).  In the notation of BrickMode:
  // a = rhs, b = dinv, x = src.
  struct BrickLaunch
  {
    BrickMode       mode    = kPlain;
    const void     *src     = nullptr; // vector the loop gathers (kChebInit: not read)
    const void     *rhs     = nullptr; // residual forms: right-hand side; Chebyshev forms: rhs of the smoother
    const void     *dinv    = nullptr; // Chebyshev forms: inverse diagonal
    const void     *old     = nullptr; // kCheb: previous iterate (nullptr: it is `out`, which is then read before written)
    void           *out     = nullptr; // result vector
    void           *carrier = nullptr; // partial sums of brick-surface DoFs between the launches of a level (may be `out`)
    double          f0 = 0., f1 = 0., f2 = 0.;
    void           *coarse         = nullptr; // kResidualRestrict / kChebFirstProlong: vector of the next coarser level
    const uint32_t *coarse_blocks  = nullptr; // ... TransferData::coarse_blocks
    void           *coarse_scratch = nullptr; // kResidualRestrict: TransferData::coarse_scratch (nullptr: added into `coarse` colour by colour)
    int             group_begin = 0, group_end = -1; // default: all groups of the eight-colour schedule (the interface /
                                                     // interior halves of a split schedule are launched separately)
    // on_free_schedule(mode), op.bricks.fr.available(): the launch groups are those of the reduced-colour schedule; the
    // caller completes the private DoFs with launch_surf_finish
    bool            free_schedule = false;

    BrickLaunch groups(int g0, int g1) const
    {
      BrickLaunch l = *this;
      l.group_begin = g0;
      l.group_end   = g1;
      return l;
    }
    // what the launchers work with: every pointer a kernel may form an address from is valid
    BrickLaunch resolved(int n_groups = 0) const
    {
      BrickLaunch l = *this;
      if (l.group_end < 0)
        l.group_end = n_groups;
      if (!l.old)
        l.old = l.out;
      if (!l.src)
        l.src = l.rhs; // kChebInit: never dereferenced
      return l;
    }
  };
  void launch_brick_loop(hipStream_t s, const OperatorData &op, const BrickLaunch &launch);

  // f(std::integral_constant<int, P>()) for P = p; false: no kernel is built for this degree.  (MGX_MACRO_ONLY_P: A/B
  // builds of the macro-element translation units with one degree.)
  template <typename F>
  static bool dispatch_degree(int p, F &&f)
  {
    switch (p)
      {
#define MGX_DEGREE_CASE(P) \
  case P: f(std::integral_constant<int, P>()); return true;
#ifdef MGX_MACRO_ONLY_P
        MGX_DEGREE_CASE(MGX_MACRO_ONLY_P)
#else
        MGX_DEGREE_CASE(1)
        MGX_DEGREE_CASE(2)
        MGX_DEGREE_CASE(3)
        MGX_DEGREE_CASE(4)
        MGX_DEGREE_CASE(5)
        MGX_DEGREE_CASE(6)
        MGX_DEGREE_CASE(7)
        MGX_DEGREE_CASE(8)
        MGX_DEGREE_CASE(9)
#endif
#undef MGX_DEGREE_CASE
        default: return false;
      }
  }
  // f(std::integral_constant<int, MODE>()) for the one of MODES that equals mode; false: none does
  template <int... MODES, typename F>
  static bool dispatch_mode(int mode, F &&f)
  {
    return ((mode == MODES ? (f(std::integral_constant<int, MODES>()), true) : false) || ...);
  }
  // f(T()) with T the number type: double for MGX_F64, float otherwise
  template <typename F>
  static void dispatch_number(int number, F &&f)
  {
    if (number == MGX_F64)
      f(double());
    else
      f(float());
  }
  // f(T(), std::integral_constant<int, P>()) for the number type and P = p; false: no kernel is built for this degree
  template <typename F>
  static bool dispatch_number_degree(int number, int p, F &&f)
  {
    bool found = false;
    dispatch_number(number, [&](auto t) { found = dispatch_degree(p, [&](auto P) { f(t, P); }); });
    return found;
  }
  // workgroups of a persistent launch over `count` bricks: as many as are resident at once (wgs_per_cu on every CU of
  // the operator's device); Tunables::macro_wg_x16 sets the number per CU instead (tuning aid)
  inline uint32_t persistent_grid(const OperatorData &op, int wgs_per_cu, uint32_t count)
  {
    const uint32_t resident = op.macro_wg_x16 ? std::max<uint32_t>(1u, op.n_cus * op.macro_wg_x16 / 16u) : (uint32_t)wgs_per_cu * op.n_cus;
    return std::min(count, resident);
  }
  // LaplaceOperator::compute_residual (laplace_operator.h:804-845) through the general per-cell kernel:
  // dst += sum over the cells of  S^T [ rhs_q - D^T (K D S (-src)) ], src read through idx27_plain; assembly as in
  // launch_cell_diagonal (lists of cells that share no DoF / ordered assembly / atomics).  dst zeroed by the caller.
  void launch_cell_residual(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *rhs_q,
                            const CellLists &lists);
  // MinimalSurfaceOperator::compute_residual (minimal_surface/program.cc:169-197) on affine cells with the metric
  // M = J^-1 J^-T [xx,yy,zz,xy,xz,yz] and det J: dst = - sum over the cells of grad phi_i . a JxW M grad u, a = 1 or
  // 1 / sqrt(1 + |grad u|^2); src through idx27_plain, dst through idx27.  lists.n > 0: launches over cell lists that share
  // no DoF (dst zeroed by the caller); lists.n == 0: the operator's ordered assembly (required then, dst written)
  // unit_q / jxw_q (device, number type of op; nullptr: affine cells): per-point geometry of curved cells as in
  // launch_evaluate_coefficient -- the flux of a point is a U g, a = 1 or 1 / sqrt(1 + g . U g / JxW_q)
  void launch_cell_nl_residual(hipStream_t s, const OperatorData &op, bool minimal_surface, const double *metric, double det,
                               const void *unit_q, const void *jxw_q, void *dst, const void *src, const CellLists &lists);
  // ---- solution-dependent coefficients (mgx_nonlinear.hip) ----
  // MinimalSurfaceOperator::evaluate_coefficient (minimal_surface/program.cc:120-165) on affine cells: op.coef_q =
  // JxW_q M (first_time) or JxW_q (M - (M g)(M g)^T / (1 + s)) / sqrt(1 + s), s = g^T M g, g the reference-space
  // gradient of `state` (operator's number type, read through idx27_plain) at the quadrature points.
  // op: index table, 1D tables and number type of the state and of the arithmetic; coef_q / coef_number: the tensor
  // array written and its number type (that of op, or fp32 from an fp64 op: the rounded fp64 tensor).
  // unit_q / jxw_q: per-point geometry of curved cells, device [n_cells][6][n^3] = JxW_q J^-1 J^-T and [n_cells][n^3] = JxW_q
  // in the number type of op (metric and det are not read then); nullptr: affine cells.
  void launch_evaluate_coefficient(hipStream_t s, const OperatorData &op, void *coef_q, int coef_number, bool minimal_surface,
                                   const double *metric, double det, const void *unit_q, const void *jxw_q, const void *state);
  // state interpolation to the coarser level (minimal_surface/program.cc:425-457): every coarse DoF = the polynomial of
  // the child that contains the coarse node, evaluated there.  r1d: device [(2p+1)(p+1)], r1d[a (p+1) + i] = weight of
  // fine patch point a for coarse node i; own_c: device [n_coarse_cells], bit e set iff the cell is the first (in cell
  // order) that contains its entity e -- the one writer of the entity's DoFs
  void launch_interpolate_to_coarse(hipStream_t s, const TransferData &t, const void *r1d, const uint32_t *own_c, void *coarse,
                                    const void *fine);
  // completes the private DoFs of a launch on a reduced-colour schedule: DoFs [first, first + count) of
  // op.bricks.fr.surf_dof; those below n_surf_shared: carrier[d] = sum only
  // constrained / n_constrained (Chebyshev forms): rows where A x = x, updated by the same launch
  void launch_surf_finish(hipStream_t s, const OperatorData &op, const BrickLaunch &launch, uint32_t first, uint32_t count,
                          const uint32_t *constrained = nullptr, uint32_t n_constrained = 0,
                          const FreeSchedule *schedule = nullptr); // schedule: another one than op.bricks.fr
  // macro-element form of the separable brick loop (mgx_macro.hip), one translation unit per number
  // type; false: mode / degree not covered (the caller falls back to the cell-by-cell form)
  bool launch_macro_loop_f64(hipStream_t s, const OperatorData &op, const BrickLaunch &launch);
  bool launch_macro_loop_f32(hipStream_t s, const OperatorData &op, const BrickLaunch &launch);
  // fused PCG step on a brick-scheduled level (mgx_macro.hip, kCgUpdate)
  bool launch_macro_cg_update_f64(hipStream_t s, const OperatorData &op, double alpha, double beta, const void *r, void *q,
                                  void *p, void *x, void *carrier, double *partials, uint32_t capacity,
                                  uint32_t *n_partials);
  bool launch_macro_cg_update_f32(hipStream_t s, const OperatorData &op, double alpha, double beta, const void *r, void *q,
                                  void *p, void *x, void *carrier, double *partials, uint32_t capacity,
                                  uint32_t *n_partials);
  void launch_reduce4(hipStream_t s, const double *partials, uint32_t n, const double *extra, double *sums);
  void macro_diag_table_f64(hipStream_t s, const OperatorData &op, const uint32_t *item_map, void *table, uint32_t *flag_dev);
  void macro_diag_table_f32(hipStream_t s, const OperatorData &op, const uint32_t *item_map, void *table, uint32_t *flag_dev);
  // second pipeline (mgx_macro2.hip, macro2_covers); false: form / degree not covered, use the first
  bool launch_macro2_loop_f64(hipStream_t s, const OperatorData &op, const BrickLaunch &launch);
  bool launch_macro2_loop_f32(hipStream_t s, const OperatorData &op, const BrickLaunch &launch);
  // true: the brick loop evaluates the separable form (7 sweeps); false: the general
  // quadrature-point form of laplace_operator.h:436-523 (12 sweeps)
  // diag += diagonal of the cell matrices (local_compute_diagonal, laplace_operator.h:770-800)
  // a1d[i] = sum_q w_q (dphi_i(x_q))^2, m1d[i] = sum_q w_q phi_i(x_q)^2 (host arrays, n entries)
  // lists: launches whose cells share no DoF (plain adds); lists.n == 0: ordered assembly if op.asm_start, else one
  // launch with atomic adds
  void launch_cell_diagonal(hipStream_t s, const OperatorData &op, void *diag, const double *a1d, const double *m1d,
                            const CellLists &lists);
  // transfers
  void launch_prolongate(hipStream_t s, const TransferData &t, void *fine, const void *coarse, bool add,
                         bool with_constraints);
  void launch_restrict_add(hipStream_t s, const TransferData &t, void *coarse, const void *fine,
                           bool with_constraints);
  // ---- quadrilaterals (mgx_kernels_2d.hip): what the four launchers above hand over to when op.dim == 2 ----
  // the cell loop with launch_cell_loop's arguments; the cells are added up by the ordered assembly (op.asm_start: dst
  // is written) or colour by colour with plain adds (op.cell_colours: dst zeroed by the caller) -- never atomics
  void launch_cell_loop_2d(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *tail_src,
                           uint32_t n_head, const ChebPost *post);
  void launch_cell_diagonal_2d(hipStream_t s, const OperatorData &op, void *diag, const double *a1d, const double *m1d);
  void launch_prolongate_2d(hipStream_t s, const TransferData &t, void *fine, const void *coarse, bool add,
                            bool with_constraints);
  void launch_restrict_add_2d(hipStream_t s, const TransferData &t, void *coarse, const void *fine, bool with_constraints);
  // ---- solution-dependent coefficients on quadrilaterals (mgx_nonlinear_2d.hip) ----
  // what launch_evaluate_coefficient, launch_cell_nl_residual (whose `lists` are not looked at: the 2D residual derives
  // them) and launch_interpolate_to_coarse hand over to when op.dim == 2: metric is [xx,yy,xy], coef_q and unit_q are [n_cells][3][n^2], jxw_q is [n_cells][n^2], own_c holds 9 bits per coarse cell.
  // The residual adds the cells up as launch_cell_loop_2d does: the ordered assembly where the level has the tables (dst
  // is written), else colour by colour (dst zeroed by the caller); the caller has checked that one of the two exists.
  void launch_evaluate_coefficient_2d(hipStream_t s, const OperatorData &op, void *coef_q, int coef_number, bool minimal_surface,
                                      const double *metric, double det, const void *unit_q, const void *jxw_q, const void *state);
  void launch_cell_nl_residual_2d(hipStream_t s, const OperatorData &op, bool minimal_surface, const double *metric, double det,
                                  const void *unit_q, const void *jxw_q, void *dst, const void *state);
  void launch_interpolate_to_coarse_2d(hipStream_t s, const TransferData &t, const void *r1d, const uint32_t *own_c, void *coarse,
                                       const void *fine);
  // ---- linear problems on quadrilaterals (mgx_rhs_2d.hip) ----
  // launch_cell_residual in two dimensions: dst = sum over the cells of S^T [ rhs_q - D^T (C D S src) ], src through
  // idx27_plain, rows through idx27; rhs_q [n_cells][n^2] in the number type or nullptr.  The cells are added up as
  // launch_cell_loop_2d does: the ordered assembly (dst is written) or colour by colour (dst zeroed by the caller).
  void launch_cell_residual_2d(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *rhs_q);
  // partials [l2_error_grid_2d][4]: block sums {sum (u_h - u_q)^2 JxW_q, sum JxW_q, 0, 0} in fp64, to be added by
  // launch_reduce4; vec (through idx27_plain), u_q and jxw_q [n_cells][n^2] in the number type
  void     launch_l2_error_2d(hipStream_t s, const OperatorData &op, const void *vec, const void *u_q, const void *jxw_q,
                              double *partials);
  uint32_t l2_error_grid_2d(int p, uint32_t n_cells);

  // ---- vector kernels (mgx_vector.hip) ----
  void launch_copy_cast(hipStream_t s, void *dst, int dn, const void *src, int sn, size_t n);
  void launch_add_cast(hipStream_t s, void *dst, int dn, const void *src, int sn, size_t n);
  void launch_sadd(hipStream_t s, int number, void *x, double sx, double a, const void *v, size_t n);
  // res = rhs - res over [0,n)
  void launch_rhs_minus(hipStream_t s, int number, void *res, const void *rhs, size_t n);
  // dst[c] = src[c] for constrained c  /  res[c] = rhs[c] - lhs[c]
  void launch_constrained_copy(hipStream_t s, int number, void *dst, const void *src, const uint32_t *list,
                               uint32_t count);
  void launch_constrained_residual(hipStream_t s, int number, void *res, const void *rhs, const void *lhs,
                                   const uint32_t *list, uint32_t count);
  void launch_constrained_set(hipStream_t s, int number, void *v, double value, const uint32_t *list,
                              uint32_t count);
  void launch_invert(hipStream_t s, int number, void *v, size_t n);
  void launch_scatter_values(hipStream_t s, int number, void *v, const uint32_t *idx_dev, const double *val_dev,
                             uint32_t count);
  // Chebyshev updates (PreconditionChebyshev internal::vector_updates); not the numbering of BrickMode
  enum ChebUpdate
  {
    kUpdateStart     = 0, // x = f2 * dinv * b, x_old = 0
    kUpdateFirst     = 1, // x_new = x + f2 * dinv * (b - t)                       (x_old <- x)
    kUpdateThreeTerm = 2  // x_new = x + f1 * (x - x_old) + f2 * dinv * (b - t)     (x_old <- x)
  };
  void launch_cheb_update(hipStream_t s, int number, ChebUpdate mode, void *x, void *x_old, const void *b,
                          const void *t, const void *dinv, double f1, double f2, size_t n);
  void launch_cheb_init(hipStream_t s, int number, void *x, const void *b, const void *dinv, double f2, size_t n);
  // ax == nullptr: (A x)_c = x_c (constrained rows); otherwise the product is read from ax
  void launch_cheb_constrained(hipStream_t s, int number, BrickMode mode, const void *x, void *out, const void *b,
                               const void *dinv, double f1, double f2, const uint32_t *list, uint32_t count,
                               const void *ax = nullptr, const void *old = nullptr, double f0 = 0.);
  // interface exchange helpers
  void launch_pack(hipStream_t s, int number, void *buf, const void *v, const uint32_t *list, uint32_t count);
  // Launches of a sum over cells in which no two cells share an FE_Q DoF (plain read-modify-writes): the classes of cells
  // k, k + stride, ... (forest order: the same child of every parent; 8 in three dimensions, 4 in two), or, where the
  // caller coloured the cells itself, the lists of `lists`.  stride 1 and no list: one launch over all cells.
  struct DisjointCells
  {
    uint32_t  stride = 1;
    CellLists lists;
  };
  // DG <-> FE_Q transfer on one mesh of dimension dim: to_dg: dg += P cg, else cg += P^T dg (the restriction), launch by
  // launch of `launches`.  Three dimensions (mgx_kernels.hip): stride 8, or one launch with atomics.  Two
  // (mgx_kernels_2d.hip, through the 9-entry table): stride 4 or lists -- there is no atomic route, the caller has
  // checked that the cells of a launch share no DoF.
  void launch_dg_cg_transfer(hipStream_t s, int number, int p, int dim, bool to_dg, void *dst, const void *src,
                             const uint32_t *idx27, uint32_t n_cells, const void *P1, const DisjointCells &launches = DisjointCells());
  void launch_dg_cg_transfer_2d(hipStream_t s, int number, int p, bool to_dg, void *dst, const void *src, const uint32_t *idx9,
                                uint32_t n_cells, const void *P1, const DisjointCells &launches);
  // DG <-> DG transfer over one step of a level hierarchy (mgx_dg_transfer.hip): prolong: fine += P coarse, else
  // coarse += P^T fine, group by group; dim == 2 or 3.  false: no kernel for this pair of degrees
  //   coarse_degree == fine_degree = p: a mesh step, a group is a coarse cell and its 2^dim children.  n_groups coarse
  //   cells; children [n_groups][2^dim] names every fine cell exactly once (the caller has checked it); identity:
  //   children[c][k] == 2^dim c + k, the table is not read; m1d [2][(p+1)^2] in the number type
  //   coarse_degree < fine_degree: a degree step on one mesh, a group is a cell.  n_groups cells; m1d [(pf+1)][(pc+1)]
  //   in the number type; children and identity are not looked at
  bool launch_dg_transfer(hipStream_t s, int number, int fine_degree, int coarse_degree, bool prolong, void *dst, const void *src,
                          uint32_t n_groups, const void *m1d, int dim, const uint32_t *children, bool identity);
  // ---- DG cell kernel (mgx_dg_kernels.hip): what it offers the host code of mgx_dg_api.cpp ----
  namespace dg
  {
    struct Host1D;   // mgx_dg_host.hpp
    struct Geometry;

    enum Action
    {
      kVmult     = 0,
      kRestrict  = 1, // residual, changed to the FE_Q basis and added into the FE_Q vector
      kCgSums    = 2, // product stored, the four sums of the merged CG iteration
      kChebyshev = 3, // numbering of laplace_operator_dg.h:957-962
      kResidual  = 4,
      kJacobi    = 5, // P^-1 only (scaled by f2)
      kPcgSums   = 6  // product stored, the four sums of the merged CG iteration weighted by the inverse lumped mass
    };

    // what every launch of one operator shares (device pointers; consts: a copy of const_block)
    struct CellOperands
    {
      int            number = 0, degree = 0, basis = 0;
      const int32_t *neigh    = nullptr;
      const void    *consts   = nullptr;
      // [4^dim][(p+1)^dim], row: bit f set for a Dirichlet face; has_neumann: [9^dim][(p+1)^dim], row: face_kind_code
      const void    *inv_diag = nullptr;
      uint32_t       n_owned  = 0;       // owned cells of the operator: neighbour entries >= n_owned are ghosts
      bool           has_ghosts = false;
      int            dim        = 3;     // 2: quadrilaterals, neigh [n_cells][4] (mgx_dg_kernels_2d.hip)
      bool           has_neumann = false; // a neighbour entry is MGX_DG_NEUMANN: the variant kernels run
    };

    // one launch of the cell kernel; vectors and P1 in the operator's number type
    struct DGLaunch
    {
      DGLaunch(int action_, void *dst_, const void *rhs_, const void *src_) : action(action_), dst(dst_), rhs(rhs_), src(src_) {}
      int             action;
      void           *dst;
      const void     *rhs, *src;
      double          f1 = 0, f2 = 0;
      int             iteration_index = 0;
      const uint32_t *cell_list       = nullptr; // cells of this launch (nullptr: cell_first + cell_stride * i)
      uint32_t        cell_first = 0, cell_stride = 1, n_cells = 0;
      // kCgSums: [workgroups][4] block sums.  kRestrict: the FE_Q vector the transformed residual is added into, the
      // compressed index table of the FE_Q cells (in the order of the DG cells), the 1D change of basis [n][n] and
      // whether the cells of the launch share no FE_Q DoF (plain adds instead of atomics)
      double         *partials = nullptr;
      void           *cg       = nullptr;
      const uint32_t *idx27    = nullptr;
      const void     *P1       = nullptr;
      int             plain    = 0;
      // kPcgSums: the inverse lumped mass of a cell, [(p+1)^dim] in the number type (device); block sums in `partials`
      const void     *lumped   = nullptr;
    };
    // a status of include/mgx.h: MGX_ERR_UNSUPPORTED for a degree, basis or action no kernel is built for
    // (two dimensions: every action but kCgSums; kRestrict there adds without atomics whatever `plain` says -- the
    // cells of a launch must share no FE_Q DoF -- and idx27 is the 9-entry table)
    int      launch_dg_cells(hipStream_t s, const CellOperands &op, const DGLaunch &launch);
    uint32_t cell_grid(int number, int p, uint32_t n_cells, int dim); // workgroups of a launch over n_cells cells
    // the constant block of the cell kernel in the number type, from the host data
    std::vector<char> const_block(int number, const Host1D &h, const Geometry &g);
    // ghost exchange: whole cells / (Hermite-like basis) value and normal derivative on face faces[c] of cells[c]
    void launch_pack_cells(hipStream_t s, int number, void *buf, const void *vec, const uint32_t *cells, uint32_t count,
                           uint32_t n3);
    void launch_pack_faces(hipStream_t s, int number, void *buf, const void *vec, const uint32_t *cells, const uint8_t *faces,
                           uint32_t count, int N, double hderiv);
    // v[i] = (global index of i mod 11) - mean over n_cells cells of n3 entries; cell_id: global cell numbers or null
    void launch_start_vector(hipStream_t s, int number, void *v, const uint32_t *cell_id, uint32_t n_cells, uint32_t n3,
                             double mean);

    // ---- right-hand side and L2 error on the device (mgx_dg_rhs.hip) ----
    // a function as the kernels take it: kind MGX_DG_FN_NONE (zero), _SINE_PRODUCT or _SAMPLED (include/mgx_dg.h)
    struct DGFunctionArgs
    {
      int           kind = 0;
      double        amplitude = 0, wave[3] = {0, 0, 0}, phase[3] = {0, 0, 0};
      const double *cell_values = nullptr, *face_values = nullptr;
    };
    // the doubles of the operator's host data the kernels compute with: the Jacobian ([d * 3 + a], whatever the
    // dimension) and the origin of x = origin + J (pos + xi), the Gauss rule, |det J| and the face factors of Geometry
    struct DGRhsGeometry
    {
      double jac[9], origin[3], xq[kMaxN], wq[kMaxN], det, sigma[3], fw[3], cn[3][3];
      double normal[3][3]; // normal[d]: the unit normal towards +xi_d in real coordinates
    };
    struct DGRhsOperands
    {
      int            number = 0, degree = 0, dim = 3;
      const int32_t *neigh    = nullptr;
      const void    *consts   = nullptr; // the constant block of the cell kernel: S, D and the end values b, g
      const int32_t *cell_pos = nullptr; // device [n_cells][dim]; needed by sine products only
      uint32_t       n_cells  = 0;       // owned cells
      bool           has_neumann = false; // a neighbour entry is MGX_DG_NEUMANN: the MIXED kernel runs
      DGRhsGeometry  geo;
    };
    // dst (number type) = int f phi_i + sum over the Dirichlet faces of int g (sigma_F phi_i - d_n phi_i) + sum over
    // the Neumann faces of int h phi_i on the owned cells (h sampled: the flux in face_values; h a sine product: the
    // potential u of h = n . grad u); false: no kernel for this degree or dimension
    bool launch_dg_rhs(hipStream_t s, const DGRhsOperands &op, const DGFunctionArgs &f, const DGFunctionArgs &g,
                       const DGFunctionArgs &h, void *dst);
    // partials [rhs_grid][4]: block sums {sum (u_h - u)^2 JxW, sum JxW, 0, 0}, to be added by launch_reduce4
    bool     launch_dg_l2_error(hipStream_t s, const DGRhsOperands &op, const DGFunctionArgs &u, const void *vec, double *partials);
    uint32_t rhs_grid(int p, uint32_t n_cells, int dim); // workgroups of either launch
  } // namespace dg
  void launch_zero_head_copy_tail(hipStream_t s, int number, void *dst, const void *src, uint32_t n_head, uint32_t n);
  void launch_scatter_map(hipStream_t s, int number, void *dst, const void *src, const uint32_t *map,
                          const uint8_t *mask, uint32_t n);
  void launch_pack_all(hipStream_t s, int number, void *const *send, const uint32_t *start, int n_neighbors,
                       const void *v, const uint32_t *index, const uint8_t *seg, uint32_t total);
  void launch_unpack_ordered(hipStream_t s, int number, void *const *recv, int n_neighbors, void *v,
                             const uint32_t *shared, const uint32_t *csr_start, const uint8_t *csr_k,
                             const uint32_t *csr_pos, uint32_t n_shared);
  // Chebyshev post-operation of the interface DoFs folded into the ordered unpack (one launch instead of two, and the
  // constrained rows -- A x = x -- ride along): what launch_cheb_constrained would do with ax = the completed sums
  // (post: the operands of the brick launch the exchange completes)
  void launch_unpack_ordered_cheb(hipStream_t s, int number, void *const *recv, int n_neighbors, void *v,
                                  const uint32_t *shared, const uint32_t *csr_start, const uint8_t *csr_k,
                                  const uint32_t *csr_pos, uint32_t n_shared, const BrickLaunch &post,
                                  const uint32_t *constrained, uint32_t n_constrained);
  void launch_unpack_add(hipStream_t s, int number, void *v, const void *buf, const uint32_t *list, uint32_t count);
  void launch_list_residual(hipStream_t s, int number, void *res, const void *rhs, const uint32_t *list,
                            uint32_t count); // res[i] = rhs[i] - res[i]
  void launch_dot_list(hipStream_t s, int number, const void *x, const void *y, const uint32_t *list,
                       uint32_t count, double *partial_dev, double *result_dev);
  void launch_index_mod11(hipStream_t s, int number, void *v, const uint32_t *global_index_dev, double mean,
                          size_t n); // v[i] = (gid(i) % 11) - mean  (gid = i if the index array is null)
  // partial[0..n_blocks) block sums of x.y, then reduced into *result_dev (double)
  void launch_dot(hipStream_t s, int number, const void *x, const void *y, size_t n, double *partial_dev,
                  double *result_dev);
  constexpr int kDotBlocks = 1024;
  // CG vector updates with fused reductions
  //   x += alpha d ; r -= alpha h ; result = r.r
  void launch_cg_update(hipStream_t s, int number, void *x, void *r, const void *d, const void *h, double alpha,
                        size_t n, double *partial_dev, double *result_dev);
  //   d = z + beta d
  void launch_xpby(hipStream_t s, int number, void *d, const void *z, double beta, size_t n);
  // mixed-precision PCG: the same with the fp32 copy of the new residual written along / the fp32 vector read directly
  void launch_cg_update_f32copy(hipStream_t s, double *x, double *r, const double *d, const double *h, double alpha, size_t n,
                                float *r32, double *partial_dev, double *result_dev);
  void launch_dot_f64_f32(hipStream_t s, const double *x, const float *y, size_t n, double *partial_dev, double *result_dev);
  void launch_xpby_f64_f32(hipStream_t s, double *d, const float *z, double beta, size_t n);
  // z = dinv .* r ; result = r.z
  void launch_jacobi_dot(hipStream_t s, int number, void *z, const void *dinv, const void *r, size_t n,
                         double *partial_dev, double *result_dev);
  // fused PCG helpers (mgx_vector.hip); the uint32_t results are the numbers of sum quadruples the
  // kernels appended at `partials` (added up by launch_reduce4)
  uint32_t launch_cg_list_update(hipStream_t s, int number, const uint32_t *list, uint32_t count, double alpha,
                                 double beta, const void *r, void *q, void *p, void *x, double *partials);
  // fused transfers on a decomposed level (TransferData::ifr_* / ifp_*, mgx_vector.hip):
  // coarse += R (b - ax) over the owned interface DoFs;  xi = x + P e, out = xi + f2 dinv (b - ax), x = xi on the shared DoFs
  // coarse[d] = ordered sum of the bricks' restricted values (TransferData::coarse_scratch), every coarse DoF written
  void launch_coarse_assemble(hipStream_t s, int number, const TransferData &tr, void *coarse);
  void launch_interface_restrict(hipStream_t s, int number, const TransferData &tr, void *coarse, const void *b, const void *ax);
  void launch_interface_prolong_cheb(hipStream_t s, int number, const TransferData &tr, const uint32_t *shared, const void *e,
                                     void *x, void *out, const void *b, const void *dinv, double f2, const void *ax);
  uint32_t launch_axpy_norm(hipStream_t s, int number, void *r, const void *q, double factor, size_t n, double *partials);
  void     launch_cg_pre(hipStream_t s, int number, void *x, void *p, void *q, double alpha, double beta, size_t n);
  uint32_t launch_dot4(hipStream_t s, int number, const void *q, const void *p, const void *r, size_t n, double *partials);
  // ---- lumped-mass PCG on the DG operator (mgx_dg_pcg_solver_*, solver_dg/program.cc:134-148, 222-263) ----
  // `table`: the inverse lumped mass of a cell, n3 <= kPcgTableMax entries in the number type (device); entry i of a
  // vector belongs to local index i mod n3.
  // Device scalars of the merged form, written by launch_pcg_scalars and read by launch_pcg_update:
  //   scalars[0] = alpha, [1] = beta, [2] = stalled_at (-1: no breakdown so far), [3] unused
  constexpr uint32_t kPcgTableMax = 1000; // (MGX_MAX_DEGREE + 1)^3
  //   x = 0 ; r = b ; p = m r
  void launch_pcg_start(hipStream_t s, int number, void *x, void *r, void *p, const void *b, const void *table, uint32_t n3,
                        size_t n);
  // the block sums {q.p, r.mr, q.mr, q.mq} of iteration k added in a fixed order, then
  //   alpha = s1 / s0 ; rho_next = s1 - 2 alpha s2 + alpha^2 s3 ; beta = rho_next / s1 ; rho_hist[k] = s1 ; rho_hist[k + 1] = rho_next
  // unless s0 or s1 is not a positive finite number, rho_next is not finite, or a breakdown is on record: then
  // alpha = beta = 0, rho_hist[k + 1] = rho_hist[k] (k == 0: s1 if it is finite and not negative, else 0) and
  // stalled_at = k, once.  rho_next finite but not positive: the step is taken, beta = 0, rho_hist[k + 1] = 0 and
  // stalled_at = k + 1 (the steps taken, either way)
  // More than kPcgPresumFrom block sums: kPcgPresums workgroups add a contiguous share each into presums
  // [kPcgPresums][4] first (a fourth launch; the order of the additions stays fixed), the one workgroup adds those.
  constexpr uint32_t kPcgPresumFrom = 4096, kPcgPresums = 256;
  void launch_pcg_scalars(hipStream_t s, const double *partials, uint32_t n_partials, uint32_t k, double *scalars, double *rho_hist,
                          double *presums);
  //   x += alpha p ; r -= alpha q ; p = m r + beta p      (alpha, beta from `scalars`)
  void launch_pcg_update(hipStream_t s, int number, void *x, void *r, void *p, const void *q, const void *table, uint32_t n3,
                         const double *scalars, size_t n);
  //   v[i] = table[i mod n3]  (the separate form's diagonal vector)
  void launch_tile_table(hipStream_t s, int number, void *v, const void *table, uint32_t n3, size_t n);
  void     launch_residual_pre(hipStream_t s, int defect_number, void *defect, const double *residual, const double *update,
                               double factor, size_t n);
  uint32_t launch_residual_post(hipStream_t s, int z_number, const void *z, double *residual, double *update, double factor,
                                size_t n_free, size_t n, double *partials);
} // namespace mgx
