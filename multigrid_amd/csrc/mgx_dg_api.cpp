// mgx_dg_api.cpp -- host side of the DG objects of include/mgx_dg.h: the operator (set-up, ghost exchange, the
// applications of the cell kernel), MultigridSolverDG on top of an FE_Q hierarchy, the DG-to-DG level transfer
// objects (between two meshes, between two degrees: one object behind two handles) and MultigridSolverDGPlain on
// h-only and mixed h/p level sequences.  No kernel lives here: the cell kernel and its launch are mgx_dg_kernels.hip
// (DG section of mgx_internal.hpp), the level transfer kernel mgx_dg_transfer.hip, the kernels of the right-hand side
// with boundary data and of the L2 error mgx_dg_rhs.hip, the fp64 numerics of the set-up mgx_dg_host.cpp.
#include "mgx_device_memory.hpp"
#include "mgx_dg_host.hpp"
#include "mgx_internal.hpp"
#include "mgx_krylov.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

using namespace mgx::dg;

struct mgx_dg_operator_s
{
  mgx_context_t    ctx = nullptr;
  mgx::DeviceArena mem{"mgx_dg_operator"};
  int           degree = 0, basis = 0, number = MGX_F32;
  int           dim = 3; // 2: quadrilaterals -- 4 faces, (p+1)^2 entries per cell, one rank
  uint32_t      n_cells = 0;
  int32_t      *neigh   = nullptr; // device [n_cells][2 dim]
  void         *consts  = nullptr; // device DGConst<T>
  void         *inv_diag = nullptr; // device [4^dim][(p+1)^dim]; has_neumann: [9^dim][(p+1)^dim] (build_inverse_diagonal)
  // inverse of the lumped mass matrix of a cell (solver_dg/program.cc:134-148): host fp64 and device in the number type,
  // [(p+1)^dim]; an entry is not positive and finite where the lumped mass is not (mgx_dg_pcg_solver_create refuses)
  std::vector<double> lumped_inv_host;
  void               *lumped_inv = nullptr;
  Host1D        h;
  Geometry      g;
  // decomposed mesh: ghost cells behind the owned ones, filled from their owners before every
  // application (mgx_dg_update_ghost_values)
  uint32_t                n_ghost = 0;
  int                     plan_id = 0;
  std::vector<int>        nb_rank;
  std::vector<uint32_t>   nb_count, nb_recv_first, nb_entries;
  std::vector<uint32_t *> nb_cells_dev;
  std::vector<void *>     nb_send;
  // cells without / with a ghost neighbour: the former run while the ghost exchange is in flight
  // (the reference completes its exchange, laplace_operator_dg.h:986-1057, before the cell loop)
  uint32_t *interior_cells = nullptr, *boundary_cells = nullptr; // device
  uint32_t  n_interior = 0, n_boundary = 0;
  bool      interior_is_prefix = false; // the interior cells are cells 0 ... n_interior - 1
  // entries per ghost: a whole cell, or for the Hermite-like basis two values per face point
  // (data_per_face of laplace_operator_dg.h:565)
  uint32_t               ghost_stride = 0;
  std::vector<uint8_t *> nb_faces_dev; // Hermite-like basis: face of every sent cell towards the neighbour rank
  // block sums of the merged CG iteration (action 2) and their total, allocated at the first use
  double  *cg_partials = nullptr, *cg_sums = nullptr;
  uint32_t cg_capacity = 0;
  // right-hand side and L2 error (mgx_dg_compute_rhs, mgx_dg_compute_l2_error): the Jacobian as [d * 3 + a], whether a
  // cell has a Dirichlet face, and the cell positions of mgx_dg_operator_set_cell_positions (device [n_cells][dim])
  double   jac[9]        = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool     has_dirichlet = false;
  bool     has_neumann   = false; // a face is MGX_DG_NEUMANN: the variant kernels run, the diagonals are coded in base 3
  int32_t *cell_pos      = nullptr;
  double   origin[3]     = {0, 0, 0};
};

// one step of a DG level hierarchy (mgx_dg_transfer.hip).  A mesh step (MGTransferMatrixFree between two DG levels):
// coarse_degree == fine_degree, a group is a coarse cell with its 2^dim children.  A degree step on one mesh:
// coarse_degree < fine_degree, a group is a cell, no children
struct DGLevelStep
{
  explicit DGLevelStep(const char *owner)
    : mem{owner}
  {}
  mgx_context_t       ctx = nullptr;
  mgx::DeviceArena    mem;
  int                 fine_degree = 0, coarse_degree = 0, basis = 0, number = MGX_F32;
  int                 dim = 3;
  uint32_t            n_groups = 0;
  uint32_t           *children = nullptr; // mesh step: device [n_groups][2^dim]
  bool                identity = false;   // children[c][k] == 2^dim c + k (checked at creation): the table is not read
  void               *m1d      = nullptr; // device, number type: [2][(p+1)^2], or [(pf+1)][(pc+1)]
  std::vector<double> m1d_host;
};

// a DG level of either multigrid solver: operator, smoother and the vectors of the V-cycle
struct DGLevel
{
  mgx_dg_operator_t  A = nullptr;
  const DGLevelStep *step = nullptr; // plain solver: from the level below (null on level 0), a mesh refinement or a degree raise
  size_t             n = 0;          // owned DoFs
  size_t             n_vec = 0;      // entries of a vector: owned cells, then the ghost cells of a decomposed mesh
  mgx_smoother_info  info{};
  void              *defect = nullptr, *t = nullptr, *update = nullptr, *old = nullptr; // V-cycle number type
  double            *r = nullptr, *z = nullptr, *d = nullptr, *h = nullptr;             // finest level: the outer CG, fp64
  double             times[6] = {0, 0, 0, 0, 0, 0};                                     // timings[level] of the reference
};

// MultigridSolverDG (common/multigrid_solver_dg.h:55-747): the DG level on top of an FE_Q hierarchy
struct mgx_dg_solver_s
{
  mgx_context_t     ctx = nullptr;
  mgx::DeviceArena  mem{"mgx_dg_solver"};
  DGLevel           level;
  mgx_dg_operator_t A_dp = nullptr;
  mgx_solver_t      cfe = nullptr;
  int               degree = 0, number = MGX_F32;
  mgx_operator_t    fe = nullptr; // finest FE_Q operator (interface sum of the restricted defect)
  bool              decomposed = false;
  void             *P1 = nullptr; // device, V-cycle number type
  const uint32_t   *idx27 = nullptr;
  uint32_t          n_cells = 0, n_cg = 0;
  bool              cg_eight_colours = false; // cells c, c + 8, ... of the FE_Q level share no DoF
  void             *cg_defect = nullptr, *cg_update = nullptr; // the FE_Q solver's finest-level vectors
  // Two dimensions (dim == 2: quadrilaterals, idx27 is the 9-entry table): the restriction never uses atomics.  Cells c,
  // c + 4, ... share no DoF (cg_four_colours, checked), or the cells are coloured here (cg_colours)
  int              dim = 3;
  bool             cg_four_colours = false;
  mgx::ColourLists cg_colours; // order == nullptr: no lists
  // the launches of a restriction: 3D stride 8 or one launch (atomics); 2D stride 4 or the colour lists
  mgx::DisjointCells restriction_launches() const
  {
    mgx::DisjointCells d;
    d.stride = cg_eight_colours ? 8u : (cg_four_colours ? 4u : 1u);
    d.lists  = cg_colours.lists();
    return d;
  }
};

// the two public handles of a step
struct mgx_dg_transfer_s : DGLevelStep
{
  mgx_dg_transfer_s()
    : DGLevelStep("mgx_dg_transfer")
  {}
};

struct mgx_dg_degree_transfer_s : DGLevelStep
{
  mgx_dg_degree_transfer_s()
    : DGLevelStep("mgx_dg_degree_transfer")
  {}
};

// MultigridSolverDGPlain (common/multigrid_solver_dg_plain.h:55-595)
struct mgx_dg_plain_solver_s
{
  mgx_context_t        ctx = nullptr;
  mgx::DeviceArena     mem{"mgx_dg_plain_solver"};
  std::vector<DGLevel> level;
  mgx_dg_operator_t    A_dp = nullptr;
  int                  number = MGX_F32;
  double              *partials = nullptr, *sums = nullptr; // vmult_with_residual_update
  bool                 timed = false;
};

// conjugate gradients on the DG operator alone, preconditioned by the inverse lumped mass (solver_dg/program.cc:134-148,
// 177-178, 222-263)
struct mgx_dg_pcg_solver_s
{
  mgx_context_t     ctx = nullptr;
  mgx::DeviceArena  mem{"mgx_dg_pcg_solver"};
  mgx_dg_operator_t A = nullptr;
  int               form = MGX_DG_PCG_MERGED;
  unsigned          max_iterations = 0, check_every = 1;
  double            tolerance = 0;
  size_t            n = 0;
  uint32_t          n3 = 0, blocks = 0;
  void             *r = nullptr, *p = nullptr, *q = nullptr; // the operator's number type
  void             *z = nullptr, *dinv = nullptr;            // separate form: M^-1 r and the diagonal as a vector
  double           *partials = nullptr;                      // merged: [blocks][4]; separate: kDotBlocks
  double           *presums  = nullptr;                      // merged: [kPcgPresums][4], the first stage of many block sums
  double           *scalars = nullptr, *rho_dev = nullptr;   // merged: alpha, beta, stalled_at, - ; [max_iterations + 1]
  double           *result  = nullptr;                       // separate: a dot product
  std::vector<double> rho;                                   // history of the last solve
};

namespace
{
  int dg_fail(int code, const std::string &msg) { return mgx::report_error(code, msg.c_str()); }

  size_t dg_nsz(int number) { return number == MGX_F64 ? 8 : 4; }

  // entries of a cell: (p+1)^dim
  uint64_t dg_cell_entries(int degree, int dim) { return dim == 2 ? (uint64_t)(degree + 1) * (degree + 1) : (uint64_t)(degree + 1) * (degree + 1) * (degree + 1); }

  // the `dim` field of the descriptors: 0 and 3 mean three dimensions; -1: neither 0, 2 nor 3
  int dg_desc_dim(int dim) { return dim == 0 || dim == 3 ? 3 : (dim == 2 ? 2 : -1); }

  // pack kernels on the context's stream; `overlap`: the exchange itself on the side stream, begun
  // behind the pack kernels -- the caller enqueues independent work and then calls ghosts_finish
  int ghosts_pack(mgx_dg_operator_t op, const void *vec)
  {
    hipStream_t    s   = (hipStream_t)mgx_context_stream(op->ctx);
    const uint32_t n3  = (uint32_t)dg_cell_entries(op->degree, op->dim);
    const int      nnb = (int)op->nb_rank.size();
    for (int k = 0; k < nnb; ++k)
      {
        if (op->basis == MGX_DG_HERMITE)
          launch_pack_faces(s, op->number, op->nb_send[k], vec, op->nb_cells_dev[k], op->nb_faces_dev[k], op->nb_count[k],
                            op->degree + 1, op->h.hderiv);
        else
          launch_pack_cells(s, op->number, op->nb_send[k], vec, op->nb_cells_dev[k], op->nb_count[k], n3);
      }
    MGX_HIP(hipGetLastError());
    return MGX_OK;
  }

  int ghosts_exchange(mgx_dg_operator_t op, void *vec, hipStream_t stream)
  {
    const uint32_t n3  = (uint32_t)dg_cell_entries(op->degree, op->dim);
    const size_t   es  = dg_nsz(op->number);
    const int      nnb = (int)op->nb_rank.size();
    std::vector<void *> recv(nnb);
    for (int k = 0; k < nnb; ++k)
      recv[k] = (char *)vec + ((size_t)op->n_cells * n3 + (size_t)(op->nb_recv_first[k] - op->n_cells) * op->ghost_stride) *
                                es; // straight into the ghosts
    return mgx::exchange_buffers(op->ctx, op->plan_id, op->number, nnb, op->nb_rank.data(), op->nb_entries.data(),
                                 op->nb_send.data(), recv.data(), stream);
  }

  int update_ghosts(mgx_dg_operator_t op, void *vec)
  {
    if (op->n_ghost == 0)
      return MGX_OK;
    MGX_TRY(ghosts_pack(op, vec));
    return ghosts_exchange(op, vec, nullptr);
  }

  int launch_cells(mgx_dg_operator_t op, const DGLaunch &launch, hipStream_t stream = nullptr)
  {
    const CellOperands o{op->number, op->degree, op->basis, op->neigh, op->consts, op->inv_diag, op->n_cells, op->n_ghost > 0, op->dim, op->has_neumann};
    return launch_dg_cells(stream ? stream : (hipStream_t)mgx_context_stream(op->ctx), o, launch);
  }

  // One application over all cells of the operator (the launch names none).  with_ghosts: the action reads neighbour
  // cells, so the ghost cells of src are refreshed first; the cells without a ghost neighbour run while that exchange
  // is in flight on the context's side stream (with the blocking callback transport: while the host waits in it).
  int run(mgx_dg_operator_t op, DGLaunch all, bool with_ghosts = false)
  {
    all.n_cells = op->n_cells;
    if (!with_ghosts || op->n_ghost == 0)
      return launch_cells(op, all);
    void *ghosted = const_cast<void *>(all.src);
    MGX_TRY(ghosts_pack(op, all.src));
    hipStream_t side = (op->n_interior > 0 && !mgx::context_tunables(op->ctx).dg_no_overlap) ? mgx::side_stream_begin(op->ctx)
                                                                                               : nullptr;
    if (!side)
      {
        MGX_TRY(ghosts_exchange(op, ghosted, nullptr));
        return launch_cells(op, all);
      }
    // main stream: interior cells; side stream: exchange, then the cells next to a ghost cell (they
    // write other cells of dst than the interior launch and share its read-only operands)
    // (interior cells first in the caller's order: two contiguous ranges, no index lists)
    DGLaunch interior = all, boundary = all;
    interior.cell_list = op->interior_is_prefix ? nullptr : op->interior_cells;
    interior.n_cells   = op->n_interior;
    boundary.cell_list  = op->interior_is_prefix ? nullptr : op->boundary_cells;
    boundary.cell_first = op->interior_is_prefix ? op->n_interior : 0;
    boundary.n_cells    = op->n_boundary;
    if (all.partials) // the block sums of the second launch behind those of the first
      boundary.partials += 4 * (size_t)cell_grid(op->number, op->degree, op->n_interior, op->dim);
    // whatever fails below, the main stream is ordered behind the side stream again before returning:
    // nothing of this application may still be in flight when the caller reuses src / dst
    int status = launch_cells(op, interior);
    if (status == MGX_OK)
      status = ghosts_exchange(op, ghosted, side);
    if (status == MGX_OK)
      status = launch_cells(op, boundary, side);
    const int joined = mgx::side_stream_end(op->ctx);
    return status != MGX_OK ? status : joined;
  }

  // room for the four sums of `blocks` workgroups (cg_partials) and for their total (cg_sums)
  int reserve_block_sums(mgx_dg_operator_t op, uint32_t blocks)
  {
    if (blocks > op->cg_capacity)
      {
        op->mem.release(op->cg_partials);
        op->cg_partials = nullptr;
        op->cg_capacity = 0;
        MGX_TRY(op->mem.alloc(&op->cg_partials, 4 * (size_t)blocks));
        op->cg_capacity = blocks;
      }
    if (!op->cg_sums)
      MGX_TRY(op->mem.alloc(&op->cg_sums, 4));
    return MGX_OK;
  }

  // ---- stages of mgx_dg_operator_create ----
  int validate_dg_operator_desc(mgx_context_t ctx, const mgx_dg_operator_desc *desc, mgx_dg_operator_t *out)
  {
    MGX_REQUIRE(ctx && desc && out, "mgx_dg_operator_create: null argument");
    if (desc->degree < 1 || desc->degree > MGX_MAX_DEGREE)
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: degree must be in 1.." + std::to_string(MGX_MAX_DEGREE));
    if (desc->basis < MGX_DG_HERMITE || desc->basis > MGX_DG_GAUSS)
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: basis must be MGX_DG_HERMITE, _GAUSS_LOBATTO or _GAUSS");
    if (desc->number != MGX_F32 && desc->number != MGX_F64)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: number must be MGX_F32 or MGX_F64");
    MGX_REQUIRE(desc->n_cells != 0 && desc->neighbours, "mgx_dg_operator_create: empty mesh");
    const int dim = dg_desc_dim(desc->dim);
    if (dim < 0)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: dim must be 0 or 3 (three dimensions) or 2");
    if (dim == 2 && desc->n_ghost_cells > 0)
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: 2D DG operator on one rank only");
    const uint64_t n3 = dg_cell_entries(desc->degree, dim);
    if ((uint64_t)desc->n_cells * n3 * dg_nsz(desc->number) >= (1ull << 40))
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: vector larger than 1 TiB");
    const uint64_t n_all = (uint64_t)desc->n_cells + desc->n_ghost_cells;
    if (n_all * n3 >= (1ull << 32))
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: more than 2^32 vector entries per rank");
    for (uint64_t i = 0; i < (uint64_t)desc->n_cells * 2 * dim; ++i)
      if (desc->neighbours[i] != MGX_DG_BOUNDARY && desc->neighbours[i] != MGX_DG_NEUMANN &&
          (desc->neighbours[i] < 0 || (uint64_t)desc->neighbours[i] >= n_all))
        return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: neighbour entry " + std::to_string(i) +
                                                   " is neither a cell (of the mesh or a ghost cell), MGX_DG_BOUNDARY nor MGX_DG_NEUMANN");
    if (desc->n_ghost_cells > 0)
      {
        if (!desc->exchange || !mgx::context_has_comm(ctx))
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: ghost cells need an exchange plan and a "
                                                   "communicator on the context");
        const mgx_dg_exchange_desc &e = *desc->exchange;
        if (e.n_neighbors < 1 || !e.neighbor_rank || !e.count || !e.send_cells || !e.recv_first)
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: incomplete exchange plan");
        uint64_t                    covered = 0;
        for (int k = 0; k < e.n_neighbors; ++k)
          {
            if (k > 0 && e.neighbor_rank[k] <= e.neighbor_rank[k - 1])
              return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: neighbour ranks must be ascending");
            if (e.recv_first[k] < desc->n_cells || (uint64_t)e.recv_first[k] + e.count[k] > n_all)
              return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: ghost range outside the ghost cells");
            if (e.count[k] > 0 && !e.send_cells[k])
              return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: incomplete exchange plan");
            for (uint32_t i = 0; i < e.count[k]; ++i)
              if (e.send_cells[k][i] >= desc->n_cells)
                return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: only owned cells can be sent");
            covered += e.count[k];
          }
        if (covered != desc->n_ghost_cells)
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_operator_create: the exchange plan does not fill every ghost cell "
                                                   "exactly once");
      }
    return MGX_OK;
  }

  // 1D data and geometry factors; the symmetries the cell kernel rests on are checked, not assumed
  int build_basis_and_geometry(mgx_dg_operator_s &op, const mgx_dg_operator_desc *desc)
  {
    std::string why;
    int         status = build_1d(desc->degree, desc->basis, op.h, why);
    if (status == MGX_OK)
      status = op.dim == 2 ? build_geometry_2d(desc->jacobian, desc->degree, op.g, why) // laplace_operator_dg.h:749-771, dim == 2
                           : build_geometry(desc->jacobian, desc->degree, op.g, why);
    if (status != MGX_OK)
      return dg_fail(status, "mgx_dg_operator_create: " + why);
    // the even-odd line products of the cell kernel (mul_eo) rest on the reversal symmetry of the 1D
    // matrices: S[q][i] = S[n-1-q][n-1-i], D[q][r] = -D[n-1-q][n-1-r].  All three bases have it.
    const int n = op.h.n;
    double    dev = 0, scale = 0;
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i)
        {
          dev   = std::max(dev, std::fabs(op.h.S[q * n + i] - op.h.S[(n - 1 - q) * n + n - 1 - i]));
          dev   = std::max(dev, std::fabs(op.h.D[q * n + i] + op.h.D[(n - 1 - q) * n + n - 1 - i]));
          scale = std::max(scale, std::max(std::fabs(op.h.S[q * n + i]), std::fabs(op.h.D[q * n + i])));
        }
    if (dev > 1e-11 * scale)
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: the 1D basis is not symmetric under x -> 1 - x");
    if (!op.h.e_parity)
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: the eigenvectors of the 1D problem have no definite parity "
                                          "(degenerate eigenvalues)");
    return MGX_OK;
  }

  // table[cat][(p+1)^dim]: inverse of the transformed diagonal for every combination of Dirichlet faces (host);
  // 64 combinations of 6 faces, 16 of the 4 faces of a quadrilateral (JacobiTransformed, laplace_operator_dg.h:2162).
  // An operator with Neumann faces: 3^(2 dim) rows, one per combination of face kinds in base 3 (face_kind_code of the
  // cell kernels); the rows of the combinations its cells have are built and must be positive, the others stay zero.
  int build_inverse_diagonal(const mgx_dg_operator_s &op, const int32_t *neighbours, uint64_t n3, std::vector<double> &table)
  {
    std::vector<double> diag;
    const int           nf = 2 * op.dim;
    int                 kind[6];
    if (op.has_neumann)
      {
        unsigned n_cat = 1;
        for (int f = 0; f < nf; ++f)
          n_cat *= 3u;
        std::vector<bool> occurs(n_cat, false);
        for (uint32_t c = 0; c < op.n_cells; ++c)
          {
            unsigned code = 0, weight = 1;
            for (int f = 0; f < nf; ++f, weight *= 3u)
              code += weight * (unsigned)kind_of_entry(neighbours[(size_t)c * nf + f]);
            occurs[code] = true;
          }
        // A cell whose faces are all Neumann faces (a one-cell pure-Neumann mesh) has a singular block: the constants.
        // Its transformed diagonal shows that at p = 1 only -- the eigenvector basis does not hold the constant
        // otherwise -- so the combination itself is refused.
        if (occurs[n_cat - 1])
          return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: transformed cell block is not positive definite: every face "
                                              "of a cell is a Neumann face");
        table.assign(n_cat * n3, 0.0);
        for (unsigned cat = 0; cat < n_cat; ++cat)
          {
            if (!occurs[cat])
              continue;
            for (unsigned f = 0, rest = cat; f < (unsigned)nf; ++f, rest /= 3u)
              kind[f] = (int)(rest % 3u);
            transformed_diagonal(op.h, op.g, kind, diag);
            for (uint64_t i = 0; i < n3; ++i)
              {
                if (!(diag[i] > 0))
                  return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: transformed cell block is not positive");
                table[cat * n3 + i] = 1.0 / diag[i];
              }
          }
        return MGX_OK;
      }
    const unsigned      n_cat = 1u << nf;
    table.resize(n_cat * n3);
    for (unsigned cat = 0; cat < n_cat; ++cat)
      {
        for (int f = 0; f < nf; ++f)
          kind[f] = (cat >> f) & 1u ? kDirichlet : kInterior;
        transformed_diagonal(op.h, op.g, kind, diag);
        for (uint64_t i = 0; i < n3; ++i)
          {
            if (!(diag[i] > 0))
              return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: transformed cell block is not positive");
            table[cat * n3 + i] = 1.0 / diag[i];
          }
      }
    return MGX_OK;
  }

  // lumped[i] = |det J| prod_d sum_q w_q phi_{i_d}(x_q) on the (p+1)-point Gauss rule, x fastest; the table holds 1 / lumped
  void build_lumped_mass_inverse(const mgx_dg_operator_s &op, const double *J, std::vector<double> &table)
  {
    const int    n   = op.h.n;
    const double det = op.dim == 2 ? J[0] * J[3] - J[1] * J[2]
                                   : J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) +
                                       J[2] * (J[3] * J[7] - J[4] * J[6]);
    std::vector<double> sum(n, 0.0), line(n);
    for (int i = 0; i < n; ++i)
      for (int q = 0; q < n; ++q)
        sum[i] += op.h.wq[q] * op.h.S[q * n + i];
    // the basis is symmetric under x -> 1 - x (build_basis_and_geometry has checked it): the mean of the two mirror
    // entries keeps the table exactly symmetric and sheds the part of the rounding error that is not.  The sums cancel
    // from terms of 0.1 to 0.011 at p = 9 (Gauss-Lobatto): against numpy 6.0e-14 becomes 2.7e-14 there, 8.0e-14 in 3D
    for (int i = 0; i < n; ++i)
      line[i] = 0.5 * (sum[i] + sum[n - 1 - i]);
    const int nz = op.dim == 2 ? 1 : n;
    table.resize((size_t)n * n * nz);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          table[((size_t)k * n + j) * n + i] = 1.0 / (std::fabs(det) * line[i] * line[j] * (op.dim == 2 ? 1.0 : line[k]));
  }

  // neighbour ranks, their send lists and buffers, and (Hermite-like basis) the face every sent cell is sent for
  int upload_exchange_plan(mgx_dg_operator_s &op, const mgx_dg_operator_desc *desc)
  {
    const size_t                nsz = dg_nsz(op.number);
    const mgx_dg_exchange_desc &e = *desc->exchange;
    op.plan_id                    = e.plan_id;
    for (int k = 0; k < e.n_neighbors; ++k)
      {
        op.nb_rank.push_back(e.neighbor_rank[k]);
        op.nb_count.push_back(e.count[k]);
        op.nb_entries.push_back((uint32_t)((uint64_t)e.count[k] * op.ghost_stride));
        op.nb_recv_first.push_back(e.recv_first[k]);
        uint32_t *cells = nullptr;
        void     *buf   = nullptr;
        MGX_TRY(op.mem.upload(&cells, e.send_cells[k], e.count[k], 1));
        op.nb_cells_dev.push_back(cells);
        MGX_TRY(op.mem.alloc(&buf, nsz * ((size_t)e.count[k] * op.ghost_stride + 1)));
        op.nb_send.push_back(buf);
        if (op.basis == MGX_DG_HERMITE)
          {
            // the face of every sent cell that looks at this neighbour's cells
            std::vector<uint8_t> face(e.count[k]);
            for (uint32_t i = 0; i < e.count[k]; ++i)
              {
                int found = -1, n_found = 0;
                for (int f = 0; f < 6; ++f)
                  {
                    const int32_t nbr = desc->neighbours[(size_t)e.send_cells[k][i] * 6 + f];
                    if (nbr >= 0 && (uint32_t)nbr >= e.recv_first[k] && (uint32_t)nbr < e.recv_first[k] + e.count[k])
                      {
                        found = f;
                        ++n_found;
                      }
                  }
                if (n_found != 1)
                  return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_operator_create: a sent cell must touch the cells of the "
                                                      "receiving rank through exactly one face");
                face[i] = (uint8_t)found;
              }
            uint8_t *fd = nullptr;
            MGX_TRY(op.mem.upload(&fd, face, 1));
            op.nb_faces_dev.push_back(fd);
          }
      }
    return MGX_OK;
  }

  // cells without / with a ghost neighbour
  int split_interior_and_boundary(mgx_dg_operator_s &op, const mgx_dg_operator_desc *desc)
  {
    std::vector<uint32_t> interior, boundary;
    for (uint32_t c = 0; c < desc->n_cells; ++c)
      {
        bool ghost = false;
        for (int f = 0; f < 6; ++f)
          ghost = ghost || (desc->neighbours[(size_t)c * 6 + f] >= 0 && (uint32_t)desc->neighbours[(size_t)c * 6 + f] >= desc->n_cells);
        (ghost ? boundary : interior).push_back(c);
      }
    op.n_interior = (uint32_t)interior.size();
    op.n_boundary = (uint32_t)boundary.size();
    op.interior_is_prefix = interior.empty() || interior.back() + 1 == interior.size();
    MGX_TRY(op.mem.upload(&op.interior_cells, interior, 1));
    MGX_TRY(op.mem.upload(&op.boundary_cells, boundary, 1));
    return MGX_OK;
  }

  int upload_constants(mgx_dg_operator_s &op)
  {
    const std::vector<char> block = const_block(op.number, op.h, op.g);
    return op.mem.upload_bytes(&op.consts, block.data(), block.size());
  }
} // namespace

extern "C" {

int mgx_dg_operator_create(mgx_context_t ctx, const mgx_dg_operator_desc *desc, mgx_dg_operator_t *out)
{
  MGX_TRY(validate_dg_operator_desc(ctx, desc, out));
  const int      dim = dg_desc_dim(desc->dim);
  const uint64_t n3  = dg_cell_entries(desc->degree, dim);
  // failures below return through the destroy function, which frees what the operator's arena holds by then
  std::unique_ptr<mgx_dg_operator_s, int (*)(mgx_dg_operator_t)> op(new mgx_dg_operator_s, mgx_dg_operator_destroy);
  op->ctx     = ctx;
  op->dim     = dim;
  op->degree  = desc->degree;
  op->basis   = desc->basis;
  op->number  = desc->number;
  op->n_cells = desc->n_cells;
  op->n_ghost = desc->n_ghost_cells;
  op->ghost_stride = desc->basis == MGX_DG_HERMITE ? 2u * (desc->degree + 1) * (desc->degree + 1) : (uint32_t)n3;
  MGX_TRY(build_basis_and_geometry(*op, desc));
  {
    const int32_t *end = desc->neighbours + 2 * (size_t)dim * desc->n_cells;
    op->has_neumann    = std::find(desc->neighbours, end, MGX_DG_NEUMANN) != end;
  }
  std::vector<double> table;
  MGX_TRY(build_inverse_diagonal(*op, desc->neighbours, n3, table));
  MGX_TRY(op->mem.upload(&op->neigh, desc->neighbours, 2 * (size_t)dim * desc->n_cells));
  for (int d = 0; d < dim; ++d)
    for (int a = 0; a < dim; ++a)
      op->jac[d * 3 + a] = desc->jacobian[d * dim + a];
  op->has_dirichlet = std::find(desc->neighbours, desc->neighbours + 2 * (size_t)dim * desc->n_cells, MGX_DG_BOUNDARY) !=
                      desc->neighbours + 2 * (size_t)dim * desc->n_cells;
  if (op->n_ghost > 0)
    {
      MGX_TRY(upload_exchange_plan(*op, desc));
      MGX_TRY(split_interior_and_boundary(*op, desc));
    }
  MGX_TRY(op->mem.upload_as(desc->number, &op->inv_diag, table.data(), table.size()));
  build_lumped_mass_inverse(*op, desc->jacobian, op->lumped_inv_host);
  MGX_TRY(op->mem.upload_as(desc->number, &op->lumped_inv, op->lumped_inv_host.data(), op->lumped_inv_host.size()));
  MGX_TRY(upload_constants(*op));
  *out = op.release();
  return MGX_OK;
}

int mgx_dg_operator_destroy(mgx_dg_operator_t op)
{
  if (!op)
    return MGX_OK;
  (void)hipStreamSynchronize((hipStream_t)mgx_context_stream(op->ctx));
  delete op;
  return MGX_OK;
}

uint64_t mgx_dg_operator_vector_size(mgx_dg_operator_t op)
{
  return op ? mgx_dg_operator_n_dofs(op) + (uint64_t)op->n_ghost * op->ghost_stride : 0;
}

int mgx_dg_update_ghost_values(mgx_dg_operator_t op, void *vec)
{
  MGX_REQUIRE(op && vec, "mgx_dg_update_ghost_values: null argument");
  if (op->dim == 2)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_update_ghost_values: 2D DG operator on one rank only, there are no ghost cells");
  return update_ghosts(op, vec);
}

uint64_t mgx_dg_operator_n_dofs(mgx_dg_operator_t op)
{
  return op ? (uint64_t)op->n_cells * dg_cell_entries(op->degree, op->dim) : 0;
}

int mgx_dg_vmult(mgx_dg_operator_t op, void *dst, const void *src)
{
  MGX_REQUIRE(op && dst && src && dst != src, "mgx_dg_vmult: null or aliased vectors");
  return run(op, DGLaunch(kVmult, dst, nullptr, src), true);
}

int mgx_dg_vmult_residual(mgx_dg_operator_t op, void *dst, const void *rhs, const void *src)
{
  MGX_REQUIRE(op && dst && src && rhs && dst != src, "mgx_dg_vmult_residual: null or aliased vectors");
  return run(op, DGLaunch(kResidual, dst, rhs, src), true);
}

int mgx_dg_jacobi_vmult(mgx_dg_operator_t op, void *dst, const void *src)
{
  MGX_REQUIRE(op && dst && src, "mgx_dg_jacobi_vmult: null vector");
  DGLaunch l(kJacobi, dst, nullptr, src);
  l.f2 = 1.0;
  return run(op, l);
}

int mgx_dg_vmult_with_chebyshev_update(mgx_dg_operator_t op, const void *rhs, unsigned iteration_index, double factor1,
                                       double factor2, void *solution, void *solution_old)
{
  MGX_REQUIRE(op && rhs && solution, "mgx_dg_vmult_with_chebyshev_update: null vector");
  if (iteration_index == 0)
    {
      DGLaunch l(kJacobi, solution, nullptr, rhs);
      l.f2 = factor2;
      return run(op, l);
    }
  MGX_REQUIRE(solution_old && solution_old != solution, "mgx_dg_vmult_with_chebyshev_update: solution_old is null or aliases solution");
  DGLaunch l(kChebyshev, solution_old, rhs, solution);
  l.f1              = factor1;
  l.f2              = factor2;
  l.iteration_index = (int)iteration_index;
  return run(op, l, true);
}

int mgx_dg_vmult_with_cg_update(mgx_dg_operator_t op, double alpha, double beta, const void *r, void *q, void *p, void *x,
                                double sums[4])
{
  MGX_REQUIRE(op && r && q && p && x && sums && q != p, "mgx_dg_vmult_with_cg_update: null or aliased vectors");
  if (op->dim == 2)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_vmult_with_cg_update: the merged CG iteration is not built for 2D DG operators "
                                        "(the 2D cell kernel has no epilogue with the four sums)");
  hipStream_t    s      = (hipStream_t)mgx_context_stream(op->ctx);
  const bool     split  = op->n_ghost > 0 && op->n_interior > 0;
  const uint32_t blocks = split ? cell_grid(op->number, op->degree, op->n_interior, op->dim) +
                                    cell_grid(op->number, op->degree, op->n_boundary, op->dim)
                                : cell_grid(op->number, op->degree, op->n_cells, op->dim);
  MGX_TRY(reserve_block_sums(op, blocks));
  // laplace_operator_dg.h:871-902: x += alpha p ; p = beta p + q (alpha == 0: p = q) on the owned entries
  mgx::launch_cg_pre(s, op->number, x, p, q, alpha, beta, (size_t)mgx_dg_operator_n_dofs(op));
  // :903 q = A p with the sums of the next iteration
  if (op->n_cells == 0)
    MGX_HIP(hipMemsetAsync(op->cg_sums, 0, sizeof(double) * 4, s));
  else
    {
      // without the overlap of the ghost exchange the cells run in one launch: its blocks are not the split's
      MGX_HIP(hipMemsetAsync(op->cg_partials, 0, sizeof(double) * 4 * (size_t)blocks, s));
      DGLaunch l(kCgSums, q, r, p);
      l.partials = op->cg_partials;
      MGX_TRY(run(op, l, true));
      mgx::launch_reduce4(s, op->cg_partials, blocks, nullptr, op->cg_sums);
    }
  MGX_HIP(hipMemcpyAsync(sums, op->cg_sums, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  MGX_HIP(hipStreamSynchronize(s));
  return mgx::allreduce_sum(op->ctx, sums, 4); // :904-906
}

int mgx_dg_operator_lumped_mass_inverse(mgx_dg_operator_t op, double *table)
{
  MGX_REQUIRE(op && table, "mgx_dg_operator_lumped_mass_inverse: null argument");
  std::copy(op->lumped_inv_host.begin(), op->lumped_inv_host.end(), table);
  return MGX_OK;
}

int mgx_dg_vmult_with_pcg_sums(mgx_dg_operator_t op, const void *r, void *q, const void *p, double sums[4])
{
  MGX_REQUIRE(op && r && q && p && sums && q != p && q != r, "mgx_dg_vmult_with_pcg_sums: null or aliased vectors");
  hipStream_t    s      = (hipStream_t)mgx_context_stream(op->ctx);
  const bool     split  = op->n_ghost > 0 && op->n_interior > 0;
  const uint32_t blocks = split ? cell_grid(op->number, op->degree, op->n_interior, op->dim) +
                                    cell_grid(op->number, op->degree, op->n_boundary, op->dim)
                                : cell_grid(op->number, op->degree, op->n_cells, op->dim);
  MGX_TRY(reserve_block_sums(op, blocks));
  // without the overlap of the ghost exchange the cells run in one launch: its blocks are not the split's
  MGX_HIP(hipMemsetAsync(op->cg_partials, 0, sizeof(double) * 4 * (size_t)blocks, s));
  DGLaunch l(kPcgSums, q, r, p);
  l.partials = op->cg_partials;
  l.lumped   = op->lumped_inv;
  MGX_TRY(run(op, l, true));
  mgx::launch_reduce4(s, op->cg_partials, blocks, nullptr, op->cg_sums);
  MGX_HIP(hipMemcpyAsync(sums, op->cg_sums, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  MGX_HIP(hipStreamSynchronize(s));
  return mgx::allreduce_sum(op->ctx, sums, 4);
}

int mgx_dg_operator_info(mgx_dg_operator_t op, double *hderiv, double penalty[3], double eigenvalues_1d[MGX_MAX_DEGREE + 1])
{
  MGX_REQUIRE(op, "mgx_dg_operator_info: null operator");
  if (hderiv)
    *hderiv = op->h.hderiv;
  if (penalty)
    for (int d = 0; d < op->dim; ++d)
      penalty[d] = op->g.sigma[d];
  if (eigenvalues_1d)
    {
      std::vector<double> sorted(op->h.lambda.begin(), op->h.lambda.begin() + op->h.n);
      std::sort(sorted.begin(), sorted.end()); // (held parity by parity internally)
      for (int i = 0; i <= MGX_MAX_DEGREE; ++i)
        eigenvalues_1d[i] = i < op->h.n ? sorted[i] : 0.0;
    }
  return MGX_OK;
}

int mgx_dg_operator_basis(mgx_dg_operator_t op, double *shape_values, double *quadrature_points,
                          double *quadrature_weights)
{
  MGX_REQUIRE(op, "mgx_dg_operator_basis: null operator");
  const int n = op->h.n;
  if (shape_values)
    std::copy(op->h.S.begin(), op->h.S.begin() + n * n, shape_values);
  if (quadrature_points)
    std::copy(op->h.xq.begin(), op->h.xq.begin() + n, quadrature_points);
  if (quadrature_weights)
    std::copy(op->h.wq.begin(), op->h.wq.begin() + n, quadrature_weights);
  return MGX_OK;
}

} // extern "C"

/* ---------------------------------------------------------------------------------------------
 * right-hand side with boundary data, L2 error (kernels: mgx_dg_rhs.hip)
 * --------------------------------------------------------------------------------------------- */
namespace
{
  DGRhsOperands rhs_operands(mgx_dg_operator_t op)
  {
    DGRhsOperands o;
    o.number = op->number, o.degree = op->degree, o.dim = op->dim;
    o.neigh = op->neigh, o.consts = op->consts, o.cell_pos = op->cell_pos, o.n_cells = op->n_cells;
    o.has_neumann = op->has_neumann;
    DGRhsGeometry &g = o.geo;
    std::copy(op->jac, op->jac + 9, g.jac);
    std::copy(op->origin, op->origin + 3, g.origin);
    for (int q = 0; q < kMaxN; ++q)
      {
        g.xq[q] = q < op->h.n ? op->h.xq[q] : 0.0;
        g.wq[q] = q < op->h.n ? op->h.wq[q] : 0.0;
      }
    const double *J = op->jac;
    g.det           = std::fabs(op->dim == 2 ? J[0] * J[4] - J[1] * J[3]
                                             : J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) +
                                       J[2] * (J[3] * J[7] - J[4] * J[6]));
    for (int d = 0; d < 3; ++d)
      {
        g.sigma[d] = op->g.sigma[d];
        g.fw[d]    = op->g.fw[d];
        for (int a = 0; a < 3; ++a)
          g.cn[d][a] = op->g.cn[d][a];
      }
    // unit normals towards +xi_d: the rows of J^-1, normalised (cofactors of J; the third row and column of a 2D
    // Jacobian stand for the identity)
    {
      double M[9];
      std::copy(J, J + 9, M);
      if (op->dim == 2)
        M[2] = M[5] = M[6] = M[7] = 0., M[8] = 1.;
      const double cof[3][3] = {{M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4]},
                                {M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5]},
                                {M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]}};
      const double det = M[0] * cof[0][0] + M[1] * cof[1][0] + M[2] * cof[2][0];
      for (int d = 0; d < 3; ++d)
        {
          const double len = std::sqrt(cof[d][0] * cof[d][0] + cof[d][1] * cof[d][1] + cof[d][2] * cof[d][2]);
          for (int i = 0; i < 3; ++i)
            g.normal[d][i] = (det < 0 ? -1.0 : 1.0) * cof[d][i] / len;
        }
    }
    return o;
  }

  // a function of the C ABI as the kernels take it.  role: "f", "g", "h" or "u" -- g reads the face values on the
  // Dirichlet faces, h on the Neumann faces, the others the cell values.  NULL: zero.
  int function_args(mgx_dg_operator_t op, const char *entry, const char *role, const mgx_dg_function *fn, DGFunctionArgs &out)
  {
    out = DGFunctionArgs{};
    if (!fn)
      return MGX_OK;
    const std::string who = std::string(entry) + ": function " + role;
    if (fn->kind == MGX_DG_FN_SINE_PRODUCT)
      {
        if (dg_desc_dim(fn->dim) != op->dim)
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + " is a sine product of dim " + std::to_string(fn->dim) + ", the operator has " +
                                                     std::to_string(op->dim) + " dimensions");
        if (!op->cell_pos)
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + " is a sine product and needs coordinates: call "
                                                         "mgx_dg_operator_set_cell_positions first");
        out.kind      = MGX_DG_FN_SINE_PRODUCT;
        out.amplitude = fn->amplitude;
        for (int d = 0; d < op->dim; ++d)
          {
            if (!std::isfinite(fn->wave[d]) || !std::isfinite(fn->phase[d]))
              return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + ": wave and phase must be finite");
            out.wave[d]  = fn->wave[d];
            out.phase[d] = fn->phase[d];
          }
        return MGX_OK;
      }
    if (fn->kind != MGX_DG_FN_SAMPLED)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + ": kind must be MGX_DG_FN_SINE_PRODUCT or MGX_DG_FN_SAMPLED");
    const bool on_faces = role[0] == 'g' || role[0] == 'h';
    if (on_faces && !fn->face_values)
      {
        if (role[0] == 'g' ? op->has_dirichlet : op->has_neumann)
          return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + " is sampled without face_values, but the mesh has " +
                                                     (role[0] == 'g' ? "Dirichlet" : "Neumann") + " faces");
        return MGX_OK; // no face reads it: as good as none
      }
    if (!on_faces && !fn->cell_values)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, who + " is sampled without cell_values");
    out.kind        = MGX_DG_FN_SAMPLED;
    out.cell_values = fn->cell_values;
    out.face_values = fn->face_values;
    return MGX_OK;
  }
} // namespace

extern "C" {

int mgx_dg_operator_set_cell_positions(mgx_dg_operator_t op, const double origin[3], const int32_t *cell_pos)
{
  MGX_REQUIRE(op && origin && cell_pos, "mgx_dg_operator_set_cell_positions: null argument");
  for (int d = 0; d < op->dim; ++d)
    MGX_REQUIRE(std::isfinite(origin[d]), "mgx_dg_operator_set_cell_positions: origin must be finite");
  // a launch in flight may still read the old table
  MGX_HIP(hipStreamSynchronize((hipStream_t)mgx_context_stream(op->ctx)));
  op->mem.release(op->cell_pos);
  op->cell_pos = nullptr;
  MGX_TRY(op->mem.upload(&op->cell_pos, cell_pos, (size_t)op->dim * op->n_cells));
  for (int d = 0; d < 3; ++d)
    op->origin[d] = d < op->dim ? origin[d] : 0.0;
  return MGX_OK;
}

int mgx_dg_compute_rhs(mgx_dg_operator_t op, const mgx_dg_function *f, const mgx_dg_function *g, void *dst)
{
  MGX_REQUIRE(op, "mgx_dg_compute_rhs: null operator");
  MGX_REQUIRE(dst, "mgx_dg_compute_rhs: dst is null");
  DGFunctionArgs fa, ga;
  MGX_TRY(function_args(op, "mgx_dg_compute_rhs", "f", f, fa));
  MGX_TRY(function_args(op, "mgx_dg_compute_rhs", "g", g, ga));
  if (!launch_dg_rhs((hipStream_t)mgx_context_stream(op->ctx), rhs_operands(op), fa, ga, DGFunctionArgs{}, dst))
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_compute_rhs: no kernel for this degree and dimension");
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_dg_compute_rhs_mixed(mgx_dg_operator_t op, const mgx_dg_function *f, const mgx_dg_function *g, const mgx_dg_function *h,
                             void *dst)
{
  MGX_REQUIRE(op, "mgx_dg_compute_rhs_mixed: null operator");
  MGX_REQUIRE(dst, "mgx_dg_compute_rhs_mixed: dst is null");
  DGFunctionArgs fa, ga, ha;
  MGX_TRY(function_args(op, "mgx_dg_compute_rhs_mixed", "f", f, fa));
  MGX_TRY(function_args(op, "mgx_dg_compute_rhs_mixed", "g", g, ga));
  MGX_TRY(function_args(op, "mgx_dg_compute_rhs_mixed", "h", h, ha));
  if (!launch_dg_rhs((hipStream_t)mgx_context_stream(op->ctx), rhs_operands(op), fa, ga, ha, dst))
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_compute_rhs_mixed: no kernel for this degree and dimension");
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_dg_compute_l2_error(mgx_dg_operator_t op, const void *vec, const mgx_dg_function *u, double sums[2])
{
  MGX_REQUIRE(op, "mgx_dg_compute_l2_error: null operator");
  MGX_REQUIRE(vec && sums, "mgx_dg_compute_l2_error: vec or sums is null");
  MGX_REQUIRE(u, "mgx_dg_compute_l2_error: the function u is null");
  DGFunctionArgs ua;
  MGX_TRY(function_args(op, "mgx_dg_compute_l2_error", "u", u, ua));
  hipStream_t    s      = (hipStream_t)mgx_context_stream(op->ctx);
  const uint32_t blocks = rhs_grid(op->degree, op->n_cells, op->dim);
  MGX_TRY(reserve_block_sums(op, blocks));
  if (!launch_dg_l2_error(s, rhs_operands(op), ua, vec, op->cg_partials))
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_compute_l2_error: no kernel for this degree and dimension");
  MGX_HIP(hipGetLastError());
  mgx::launch_reduce4(s, op->cg_partials, blocks, nullptr, op->cg_sums);
  double all[4];
  MGX_HIP(hipMemcpyAsync(all, op->cg_sums, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  MGX_HIP(hipStreamSynchronize(s));
  sums[0] = all[0];
  sums[1] = all[1];
  return MGX_OK;
}

} // extern "C"

/* ---------------------------------------------------------------------------------------------
 * MultigridSolverDG
 * --------------------------------------------------------------------------------------------- */
namespace
{
  // over the first n (owned) entries
  int dg_norm(mgx_context_t ctx, size_t n, int number, const void *x, double *out)
  {
    MGX_TRY(mgx::dot_owned_prefix(ctx, number, x, x, n, out));
    *out = std::sqrt(*out);
    return MGX_OK;
  }

  // The four steps of a CG iteration (mgx_krylov.hpp) on a DG operator, over its n owned entries: x (null: none), r, z,
  // d, h vectors of A's number type, precondition(z, r): z = M^-1 r
  template <typename Preconditioner>
  struct DGCGOps
  {
    mgx_context_t     ctx;
    mgx_dg_operator_t A;
    size_t            n;
    void             *x, *r, *z, *d, *h;
    Preconditioner    precondition;
    int precondition_dot(double *rz)
    {
      MGX_TRY(precondition(z, r));
      return mgx::dot_owned_prefix(ctx, A->number, r, z, n, rz);
    }
    int direction(double beta, bool first) { return first ? mgx_copy_cast(ctx, d, A->number, z, A->number, n) : mgx_sadd(ctx, A->number, d, beta, 1.0, z, n); }
    int vmult_dot(double *dh)
    {
      MGX_TRY(mgx_dg_vmult(A, h, d));
      return mgx::dot_owned_prefix(ctx, A->number, d, h, n, dh);
    }
    int update(double alpha, double *res)
    {
      if (x)
        MGX_TRY(mgx_sadd(ctx, A->number, x, 1.0, alpha, d, n));
      MGX_TRY(mgx_sadd(ctx, A->number, r, 1.0, -alpha, h, n));
      return dg_norm(ctx, n, A->number, r, res);
    }
  };

  // SolverCG with ReductionControl(100, 1e-16, tolerance) and zero start on the fp64 operator A_dp, on the fp64 vectors of a
  // solver's finest level v; precondition(z, r): z = M^-1 r; `name` heads the message when the residual stays above the tolerance
  template <typename Preconditioner>
  int dg_solve_cg(mgx_context_t ctx, mgx_dg_operator_t A_dp, const DGLevel &v, Preconditioner precondition, double tolerance,
                  const double *rhs, double *solution, unsigned *iterations, double *reduction_rate, const char *name)
  {
    MGX_HIP(hipMemsetAsync(solution, 0, 8 * v.n_vec, (hipStream_t)mgx_context_stream(ctx)));
    MGX_TRY(mgx_copy_cast(ctx, v.r, MGX_F64, rhs, MGX_F64, v.n));
    double res0 = 0;
    MGX_TRY(dg_norm(ctx, v.n, MGX_F64, v.r, &res0));
    DGCGOps<Preconditioner>  ops{ctx, A_dp, v.n, solution, v.r, v.z, v.d, v.h, precondition};
    mgx::krylov::SolveResult R;
    MGX_TRY(mgx::krylov::solve(ops, res0, 100, 1e-16, tolerance, nullptr, R, iterations, reduction_rate));
    return R.above_tolerance ? dg_fail(MGX_ERR_NOT_CONVERGED, std::string(name) + ": 100 iterations") : MGX_OK;
  }

  // PreconditionChebyshev<LaplaceOperatorCompactCombine, Vector, JacobiTransformed>: vmult (zero start) and
  // step, through the merged operation (deal.II hands iteration index 0 / 1, then k + 1 / k + 2)
  // (update and old trade places with every step, as the reference swaps its two vectors)
  int dg_smoother_apply(DGLevel &L, bool is_step)
  {
    const mgx_smoother_info      &I = L.info;
    mgx::krylov::ChebyshevFactors F(I);
    int                           index = is_step ? 2 : 1;
    MGX_TRY(mgx_dg_vmult_with_chebyshev_update(L.A, L.defect, is_step ? 1 : 0, 0., F.first(), L.update, L.old));
    if (is_step)
      std::swap(L.update, L.old);
    if (I.degree < 2 || std::fabs(I.delta) < 1e-40)
      return MGX_OK;
    for (int k = 0; k < I.degree - 1; ++k, ++index)
      {
        double f1, f2;
        F.next(k, f1, f2);
        MGX_TRY(mgx_dg_vmult_with_chebyshev_update(L.A, L.defect, (unsigned)index, f1, f2, L.update, L.old));
        std::swap(L.update, L.old);
      }
    return MGX_OK;
  }

  // PreconditionChebyshev::initialize -> estimate_eigenvalues for a DG operator with JacobiTransformed
  // (multigrid_solver_dg.h:293-303, multigrid_solver_dg_plain.h:192-213): at most max_its iterations of CG
  // preconditioned with JacobiTransformed on v_i = (global index of i mod 11) - mean, as mgx_krylov.hpp runs them
  // (lanczos_estimate with the dense solver up to 64 rows; chebyshev_interval for smoothing_range and degree).  The
  // level's own vectors carry the iteration -- they are free until the first cycle -- and are zero again afterwards;
  // cell_global_id: host, may be null.
  int dg_smoother_initialize(mgx_context_t ctx, DGLevel &L, const uint32_t *cell_global_id, int max_its, double smoothing_range,
                             int degree)
  {
    mgx_dg_operator_t A      = L.A;
    void             *r      = L.t;
    hipStream_t       s      = (hipStream_t)mgx_context_stream(ctx);
    const size_t      n      = L.n;
    const int         number = A->number;
    double       ng     = (double)n; // global number of DoFs
    MGX_TRY(mgx::allreduce_sum(ctx, &ng, 1));
    const uint64_t ngl  = (uint64_t)(ng + 0.5);
    const uint64_t full = ngl / 11, rem = ngl % 11;
    const double   mean = (full * 55.0 + rem * (rem - 1) / 2.0) / (double)ngl;
    {
      mgx::DeviceArena tmp("DG smoother set-up");
      uint32_t        *cell_id = nullptr;
      if (cell_global_id)
        MGX_TRY(tmp.upload(&cell_id, cell_global_id, A->n_cells));
      launch_start_vector(s, number, r, cell_id, A->n_cells, (uint32_t)(n / A->n_cells), mean);
      MGX_HIP(hipStreamSynchronize(s));
    }
    double res = 0;
    MGX_TRY(dg_norm(ctx, n, number, r, &res));
    const auto jacobi = [A](void *z, const void *r) { return mgx_dg_jacobi_vmult(A, z, r); };
    DGCGOps<decltype(jacobi)> ops{ctx, A, n, nullptr, r, L.update, L.old, L.defect, jacobi};
    MGX_TRY(mgx::krylov::lanczos_estimate(ops, res, max_its, mgx::krylov::RitzRule{sym_eig}, L.info));
    mgx::krylov::chebyshev_interval(smoothing_range, degree, L.info);
    for (void *v : {L.defect, L.t, L.update, L.old})
      MGX_HIP(hipMemsetAsync(v, 0, dg_nsz(number) * L.n_vec, s));
    return MGX_OK;
  }

  // operator, lengths and the zeroed vectors of a level; finest: those of the outer CG too
  int dg_level_allocate(mgx::DeviceArena &mem, DGLevel &L, mgx_dg_operator_t A, bool finest, hipStream_t s)
  {
    L.A     = A;
    L.n     = (size_t)mgx_dg_operator_n_dofs(A);
    L.n_vec = (size_t)mgx_dg_operator_vector_size(A);
    for (void **v : {&L.defect, &L.t, &L.update, &L.old})
      MGX_TRY(mem.zeros(v, dg_nsz(A->number) * L.n_vec, s));
    if (finest)
      for (double **v : {&L.r, &L.z, &L.d, &L.h})
        MGX_TRY(mem.zeros(v, L.n_vec, s));
    return MGX_OK;
  }

  // vmult of a solver (multigrid_solver_dg.h:433-436, _dg_plain.h:327-331): cast the source in, one cycle, cast the update out
  template <typename Cycle>
  int dg_level_vmult(mgx_context_t ctx, DGLevel &top, Cycle cycle, double *dst, const double *src)
  {
    MGX_TRY(mgx_copy_cast(ctx, top.defect, top.A->number, src, MGX_F64, top.n));
    MGX_TRY(cycle());
    return mgx_copy_cast(ctx, dst, MGX_F64, top.update, top.A->number, top.n);
  }

  // vmult_residual_and_restrict_to_cg (laplace_operator_dg.h:853-861, action 1 :1798-1819): cg = sum over the cells of
  // P^T (rhs - A lhs), inside the cell kernel.  Cells c, c + 8, ... share no FE_Q DoF when the mesh is in forest order:
  // eight launches with plain adds (the sum is then the same in every run); one launch with atomics otherwise.  Two
  // dimensions: four launches (cells c, c + 4, ...), or one per colour of the solver's own colouring; never atomics.
  int dg_residual_and_restrict(mgx_dg_solver_t S, void *cg, const void *rhs, const void *lhs)
  {
    hipStream_t       s  = (hipStream_t)mgx_context_stream(S->ctx);
    mgx_dg_operator_t op = S->level.A;
    MGX_HIP(hipMemsetAsync(cg, 0, dg_nsz(S->number) * S->n_cg, s));
    if (op->n_ghost > 0)
      MGX_TRY(update_ghosts(op, const_cast<void *>(lhs)));
    DGLaunch l(kRestrict, nullptr, rhs, lhs);
    l.cg      = cg;
    l.idx27   = S->idx27;
    l.P1      = S->P1;
    l.n_cells = op->n_cells;
    const mgx::DisjointCells launches = S->restriction_launches();
    if (launches.lists.n > 0)
      {
        l.plain = 1;
        for (int k = 0; k < launches.lists.n; ++k)
          {
            l.cell_list = launches.lists.cells + launches.lists.start[k];
            l.n_cells   = launches.lists.start[k + 1] - launches.lists.start[k]; // of this launch: the length of its list
            MGX_TRY(launch_cells(op, l));
          }
      }
    else if (launches.stride == 1)
      MGX_TRY(launch_cells(op, l));
    else
      {
        l.plain       = 1;
        l.cell_stride = launches.stride;
        for (uint32_t k = 0; k < launches.stride && k < op->n_cells; ++k)
          {
            l.cell_first = k;
            l.n_cells    = (op->n_cells - k + launches.stride - 1) / launches.stride;
            MGX_TRY(launch_cells(op, l));
          }
      }
    if (S->decomposed) // FE_Q DoFs on a rank interface collect the contributions of all sharers
      MGX_TRY(mgx_exchange_add(S->fe, cg));
    return MGX_OK;
  }

  // dg_v_cycle(1) (multigrid_solver_dg.h:605-633): defect in, update out
  int dg_v_cycle(mgx_dg_solver_t S)
  {
    hipStream_t s = (hipStream_t)mgx_context_stream(S->ctx);
    DGLevel    &L = S->level;
    MGX_TRY(dg_smoother_apply(L, false));
    // vmult_residual_and_restrict_to_cg (:616-618)
    if (!mgx::context_tunables(S->ctx).dg_unmerged_restrict)
      MGX_TRY(dg_residual_and_restrict(S, S->cg_defect, L.defect, L.update));
    else
      {
        MGX_TRY(mgx_dg_vmult_residual(L.A, L.t, L.defect, L.update));
        MGX_HIP(hipMemsetAsync(S->cg_defect, 0, dg_nsz(S->number) * S->n_cg, s));
        mgx::launch_dg_cg_transfer(s, S->number, S->degree, S->dim, false, S->cg_defect, L.t, S->idx27, S->n_cells, S->P1,
                                   S->restriction_launches());
        if (S->decomposed) // FE_Q DoFs on a rank interface collect the contributions of all sharers
          MGX_TRY(mgx_exchange_add(S->fe, S->cg_defect));
      }
    MGX_TRY(mgx_solver_v_cycle(S->cfe)); // :622
    // prolongate_add_cg_to_dg (:625; laplace_operator_dg.h:1863-1894)
    mgx::launch_dg_cg_transfer(s, S->number, S->degree, S->dim, true, L.update, S->cg_update, S->idx27, S->n_cells, S->P1);
    MGX_HIP(hipGetLastError());
    return dg_smoother_apply(L, true); // :629
  }
} // namespace

extern "C" {

int mgx_dg_solver_create(mgx_context_t ctx, const mgx_dg_solver_desc *desc, mgx_dg_solver_t *out)
{
  MGX_REQUIRE(ctx && desc && out && desc->matrix_dg && desc->matrix_dg_dp, "mgx_dg_solver_create: null argument");
  mgx_dg_operator_t A = desc->matrix_dg, Ad = desc->matrix_dg_dp;
  if ((A->dim == 2 || Ad->dim == 2) && !desc->cfe) // (before the null check of cfe: a refusal, not an invalid argument)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_solver_create: 2D DG operators, but the descriptor names no FE_Q hierarchy in two "
                                        "dimensions (cfe: a solver made from an mgx_square); without one use "
                                        "mgx_dg_plain_solver_create");
  if (A->dim != Ad->dim)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_solver_create: matrix_dg and matrix_dg_dp differ in their dimension");
  if (A->has_neumann || Ad->has_neumann)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_solver_create: DG operator with Neumann faces -- the FE_Q levels of the hierarchy "
                                        "constrain every boundary DoF; use mgx_dg_plain_solver_create");
  MGX_REQUIRE(desc->cfe, "mgx_dg_solver_create: null argument");
  if (Ad->number != MGX_F64 || A->n_cells != Ad->n_cells || A->degree != Ad->degree || A->basis != Ad->basis)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_solver_create: matrix_dg_dp must be the fp64 twin of matrix_dg");
  if (desc->degree_pre < 1)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_solver_create: degree_pre must be at least 1");
  const int      lmax = mgx_solver_n_levels(desc->cfe) - 1;
  mgx_operator_t fe   = nullptr;
  MGX_TRY(mgx_solver_get_operator(desc->cfe, lmax, 0, &fe));
  const int dim = A->dim == 2 ? 2 : 3;
  if (mgx::operator_dim(fe) != dim) // (before cells and degree are compared: they cannot agree)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_solver_create: the DG operators are " + std::to_string(dim) + "D, the FE_Q hierarchy is " +
                                          std::to_string(mgx::operator_dim(fe)) + "D -- a DG level sits on the FE_Q hierarchy of its own mesh");
  const int       ne    = dim == 2 ? 9 : 27; // entries of a cell in the compressed index table
  const uint32_t *idx27 = nullptr;
  uint32_t        nc = 0, ncg = 0;
  int             p = 0;
  MGX_TRY(mgx_operator_device_indices(fe, &idx27, &nc, &ncg, &p));
  if (nc != A->n_cells || p != A->degree || mgx_operator_number(fe) != A->number)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_solver_create: the FE_Q hierarchy's finest level must have the DG "
                                             "operator's cells, degree and number type");
  std::unique_ptr<mgx_dg_solver_s, int (*)(mgx_dg_solver_t)> S(new mgx_dg_solver_s, mgx_dg_solver_destroy);
  S->ctx = ctx;
  S->A_dp = Ad;
  S->cfe = desc->cfe;
  S->degree = A->degree;
  S->number = A->number;
  S->fe = fe;
  S->decomposed = A->n_ghost > 0;
  if (A->n_ghost != Ad->n_ghost)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_solver_create: the two DG operators must share the partition");
  S->idx27 = idx27;
  S->n_cells = nc;
  S->n_cg = ncg;
  S->dim = dim;
  {
    // forest order (the same child of every parent in one class: 8 classes of cells c, c + 8, ... in three dimensions,
    // 4 in two): checked, not assumed
    const uint32_t        classes = dim == 2 ? 4u : 8u;
    std::vector<uint32_t> h27(ne * (size_t)nc), stamp(ncg, 0xFFFFFFFFu);
    MGX_HIP(hipMemcpy(h27.data(), idx27, sizeof(uint32_t) * h27.size(), hipMemcpyDeviceToHost));
    // an entity's first DoF identifies it; p = 1: the entry of an entity without DoFs (inside a line, quad or hex) is
    // no address
    const auto key = [&](uint32_t c, int e) {
      const uint32_t v = h27[ne * (size_t)c + e];
      return mgx::entity_size(e, S->degree) != 0 && v < ncg ? v : 0xFFFFFFFFu;
    };
    bool ok = nc >= classes * classes;
    for (uint32_t k = 0; k < classes && ok; ++k)
      for (uint32_t c = k; c < nc && ok; c += classes)
        for (int e = 0; e < ne && ok; ++e)
          {
            const uint32_t v = key(c, e);
            if (v == 0xFFFFFFFFu)
              continue;
            // stamp = class * nc + cell would overflow: class and cell apart
            const uint32_t mark = k * 0x10000000u + c / classes;
            ok                  = stamp[v] == 0xFFFFFFFFu || (stamp[v] >> 28) != k || stamp[v] == mark;
            stamp[v]            = mark;
          }
    ok = ok && nc / classes < 0x10000000u;
    (dim == 2 ? S->cg_four_colours : S->cg_eight_colours) = ok;
    if (dim == 2 && !ok)
      {
        // fewer than 16 cells or another cell order: the greedy colours of the FE_Q operator's own cell colouring
        // (mgx_index_tables.hpp).  There is no launch with atomics to fall back to in two dimensions.
        const mgx::CellColouring colours = mgx::colour_cells_greedy(h27.data(), ne, nc, ncg, S->degree);
        if (colours.more_than_32)
          return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_solver_create: the cells of the FE_Q level need more than 32 colours for a "
                                              "DG -> FE_Q restriction without atomics");
        MGX_TRY(mgx::upload_colours(S->mem, S->cg_colours, colours));
      }
  }
  hipStream_t s = (hipStream_t)mgx_context_stream(ctx);
  MGX_TRY(dg_level_allocate(S->mem, S->level, A, true, s));
  {
    const int n1 = S->degree + 1;
    MGX_TRY(S->mem.upload_as(S->number, &S->P1, A->h.P1.data(), (size_t)n1 * n1));
  }
  // the FE_Q hierarchy under a DG level smooths with degree_pre - 1 on its finest level and solves
  // the coarsest one to 2e-3 (multigrid_solver_dg.h:271-291)
  if (lmax > 0)
    MGX_TRY(mgx_solver_reset_smoother(desc->cfe, lmax, 20., std::max(1, desc->degree_pre - 1), 15));
  {
    uint32_t n0 = 0;
    mgx_operator_t f0 = nullptr;
    MGX_TRY(mgx_solver_get_operator(desc->cfe, 0, 0, &f0));
    MGX_TRY(mgx_operator_device_indices(f0, nullptr, nullptr, &n0, nullptr));
    MGX_TRY(mgx_solver_reset_smoother(desc->cfe, 0, 2e-3, -1, (int)std::max<uint32_t>(3u, n0)));
  }
  MGX_TRY(mgx_solver_get_vector(desc->cfe, lmax, 2, &S->cg_defect));
  MGX_TRY(mgx_solver_get_vector(desc->cfe, lmax, 4, &S->cg_update));

  // smooth_dg.initialize (multigrid_solver_dg.h:293-303): eigenvalue estimate by 15 iterations of
  // CG preconditioned with JacobiTransformed on v_i = (i mod 11) - mean, lambda_max = 1.2 x the
  // largest Ritz value, range 20
  MGX_TRY(dg_smoother_initialize(ctx, S->level, desc->cell_global_id, 15, 20., desc->degree_pre));
  MGX_HIP(hipStreamSynchronize(s));
  *out = S.release();
  return MGX_OK;
}

int mgx_dg_solver_destroy(mgx_dg_solver_t S)
{
  if (!S)
    return MGX_OK;
  if (S->ctx)
    (void)hipStreamSynchronize((hipStream_t)mgx_context_stream(S->ctx));
  delete S;
  return MGX_OK;
}

int mgx_dg_solver_smoother_info(mgx_dg_solver_t S, mgx_smoother_info *info)
{
  MGX_REQUIRE(S && info, "mgx_dg_solver_smoother_info: null argument");
  *info = S->level.info;
  return MGX_OK;
}

int mgx_dg_restrict_to_cg(mgx_dg_solver_t S, void *cg_dst, const void *dg_src)
{
  MGX_REQUIRE(S && cg_dst && dg_src, "mgx_dg_restrict_to_cg: null argument");
  hipStream_t s = (hipStream_t)mgx_context_stream(S->ctx);
  MGX_HIP(hipMemsetAsync(cg_dst, 0, dg_nsz(S->number) * S->n_cg, s));
  mgx::launch_dg_cg_transfer(s, S->number, S->degree, S->dim, false, cg_dst, dg_src, S->idx27, S->n_cells, S->P1,
                             S->restriction_launches());
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_dg_vmult_residual_and_restrict_to_cg(mgx_dg_solver_t S, void *cg_dst, const void *rhs, const void *lhs)
{
  MGX_REQUIRE(S && cg_dst && rhs && lhs, "mgx_dg_vmult_residual_and_restrict_to_cg: null argument");
  return dg_residual_and_restrict(S, cg_dst, rhs, lhs);
}

int mgx_dg_prolongate_add_cg_to_dg(mgx_dg_solver_t S, void *dg_dst, const void *cg_src)
{
  MGX_REQUIRE(S && dg_dst && cg_src, "mgx_dg_prolongate_add_cg_to_dg: null argument");
  hipStream_t s = (hipStream_t)mgx_context_stream(S->ctx);
  mgx::launch_dg_cg_transfer(s, S->number, S->degree, S->dim, true, dg_dst, cg_src, S->idx27, S->n_cells, S->P1);
  MGX_HIP(hipGetLastError());
  return MGX_OK;
}

int mgx_dg_solver_vmult(mgx_dg_solver_t S, double *dst, const double *src)
{
  MGX_REQUIRE(S && dst && src, "mgx_dg_solver_vmult: null argument");
  return dg_level_vmult(S->ctx, S->level, [S] { return dg_v_cycle(S); }, dst, src);
}

int mgx_dg_solver_solve_cg(mgx_dg_solver_t S, double tolerance, const double *rhs, double *solution,
                           unsigned *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S && rhs && solution, "mgx_dg_solver_solve_cg: null argument");
  // preconditioner = one DG V-cycle (multigrid_solver_dg.h:410-424)
  const auto v_cycle = [S](void *z, const void *r) { return mgx_dg_solver_vmult(S, (double *)z, (const double *)r); };
  return dg_solve_cg(S->ctx, S->A_dp, S->level, v_cycle, tolerance, rhs, solution, iterations, reduction_rate,
                     "mgx_dg_solver_solve_cg");
}

} // extern "C"

/* ---------------------------------------------------------------------------------------------
 * DG-to-DG level transfer and MultigridSolverDGPlain
 * --------------------------------------------------------------------------------------------- */
namespace
{
  // a step in one direction: fine += P coarse (prolong) or coarse += P^T fine; `entry` names the caller in the messages
  int step_apply(const DGLevelStep *T, bool prolong, void *dst, const void *src, const char *entry)
  {
    if (!T || !dst || !src || dst == src)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, std::string(entry) + ": null or aliased vectors");
    if (!mgx::launch_dg_transfer((hipStream_t)mgx_context_stream(T->ctx), T->number, T->fine_degree, T->coarse_degree, prolong, dst, src,
                                 T->n_groups, T->m1d, T->dim, T->children, T->identity))
      return dg_fail(MGX_ERR_UNSUPPORTED, std::string(entry) + ": no kernel for this pair of degrees");
    MGX_HIP(hipGetLastError());
    return MGX_OK;
  }

  // what both kinds of step hold, and the 1D matrix on the device in the number type
  int step_fill(DGLevelStep &T, mgx_context_t ctx, int dim, int basis, int number, uint32_t n_groups, const std::vector<double> &m1d)
  {
    T.ctx      = ctx;
    T.dim      = dim;
    T.basis    = basis;
    T.number   = number;
    T.n_groups = n_groups;
    T.m1d_host = m1d;
    return T.mem.upload_as(number, &T.m1d, m1d.data(), m1d.size());
  }

  int step_matrix(const DGLevelStep *T, double *m1d, const char *entry)
  {
    if (!T || !m1d)
      return dg_fail(MGX_ERR_INVALID_ARGUMENT, std::string(entry) + ": null argument");
    std::copy(T->m1d_host.begin(), T->m1d_host.end(), m1d);
    return MGX_OK;
  }

  template <typename Step> // the handle's own type: what was created is what is deleted
  int step_destroy(Step *T)
  {
    if (!T)
      return MGX_OK;
    if (T->ctx)
      (void)hipStreamSynchronize((hipStream_t)mgx_context_stream(T->ctx));
    delete T;
    return MGX_OK;
  }

  // v_cycle(level, 1) (multigrid_solver_dg_plain.h:456-496): defect[level] in, update[level] out
  int plain_v_cycle(mgx_dg_plain_solver_t S, int l)
  {
    hipStream_t s = (hipStream_t)mgx_context_stream(S->ctx);
    DGLevel    &L = S->level[l];
    if (l == 0) // coarse = the level-0 smoother's vmult (:462)
      {
        mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 0);
        L.times[1] += 1;
        return dg_smoother_apply(L, false);
      }
    DGLevel &C = S->level[l - 1];
    {
      mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 5);
      MGX_TRY(dg_smoother_apply(L, false)); // :472
    }
    {
      mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 0);
      MGX_TRY(mgx_dg_vmult_residual(L.A, L.t, L.defect, L.update)); // :478
    }
    {
      mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 1);
      MGX_HIP(hipMemsetAsync(C.defect, 0, dg_nsz(S->number) * C.n, s)); // :482
      MGX_TRY(step_apply(L.step, false, C.defect, L.t, "mgx_dg_plain_solver: restriction")); // :483
    }
    MGX_TRY(plain_v_cycle(S, l - 1));
    {
      mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 2);
      MGX_TRY(step_apply(L.step, true, L.update, C.update, "mgx_dg_plain_solver: prolongation")); // :489
    }
    mgx::LevelTimer timer(S->ctx, S->timed, L.times, l, 5);
    return dg_smoother_apply(L, true); // :493
  }

  // the step from level l - 1 to level l: whichever of desc->transfer[l - 1] and desc->degree_transfer[l - 1] is set
  // (either array may be null); null if neither is
  const DGLevelStep *step_of(const mgx_dg_hp_solver_desc *desc, int l)
  {
    if (desc->transfer && desc->transfer[l - 1])
      return desc->transfer[l - 1];
    return desc->degree_transfer ? desc->degree_transfer[l - 1] : nullptr;
  }

  // the solver object of a checked level sequence: level vectors and smooth[level].initialize
  int plain_solver_build(mgx_context_t ctx, const mgx_dg_hp_solver_desc *desc, mgx_dg_plain_solver_t *out)
  {
    const int         L   = desc->n_levels - 1;
    mgx_dg_operator_t top = desc->matrix[L];
    std::unique_ptr<mgx_dg_plain_solver_s, int (*)(mgx_dg_plain_solver_t)> S(new mgx_dg_plain_solver_s, mgx_dg_plain_solver_destroy);
    S->ctx    = ctx;
    S->A_dp   = desc->matrix_dg_dp;
    S->number = top->number;
    S->level.resize(L + 1);
    hipStream_t s = (hipStream_t)mgx_context_stream(ctx);
    for (int l = 0; l <= L; ++l)
      {
        MGX_TRY(dg_level_allocate(S->mem, S->level[l], desc->matrix[l], l == L, s));
        S->level[l].step = l > 0 ? step_of(desc, l) : nullptr;
      }
    MGX_TRY(S->mem.alloc(&S->partials, 4 * (size_t)mgx::kDotBlocks));
    MGX_TRY(S->mem.alloc(&S->sums, 4));
    // smooth[level].initialize (:192-213)
    for (int l = 0; l <= L; ++l)
      {
        DGLevel        &lv  = S->level[l];
        const uint32_t *ids = desc->cell_global_id ? desc->cell_global_id[l] : nullptr;
        if (l > 0)
          MGX_TRY(dg_smoother_initialize(ctx, lv, ids, 15, 20., l < L ? desc->degree_pre : std::max(1, desc->degree_pre - 1)));
        else
          MGX_TRY(dg_smoother_initialize(ctx, lv, ids, (int)std::min<size_t>(lv.n, 0x7FFFFFFF), 1e-5, -1));
      }
    MGX_HIP(hipStreamSynchronize(s));
    *out = S.release();
    return MGX_OK;
  }

  // what both entry points of the plain solver ask of a level sequence: the operators level by level, the step between
  // two levels, the fp64 twin; then the solver.  degree_raises: mgx_dg_hp_solver_create; without them
  // (mgx_dg_plain_solver_create) all levels have one degree, every step is a mesh refinement, and a problem without a
  // Dirichlet face is called unsupported, not an invalid argument
  int plain_solver_create(const std::string &name, bool degree_raises, mgx_context_t ctx, const mgx_dg_hp_solver_desc *desc,
                          mgx_dg_plain_solver_t *out)
  {
    const auto refuse = [&](const std::string &why) { return dg_fail(MGX_ERR_INVALID_ARGUMENT, name + why); };
    const auto str    = [](uint64_t v) { return std::to_string(v); };
    if (!ctx || !out || !desc->matrix || !desc->matrix_dg_dp || (!degree_raises && desc->n_levels > 1 && !desc->transfer))
      return refuse("null argument");
    if (desc->n_levels < 1 || desc->n_levels > 32)
      return refuse("n_levels must be in 1..32");
    if (desc->degree_pre < 1)
      return refuse("degree_pre must be at least 1");
    const int         L   = desc->n_levels - 1;
    mgx_dg_operator_t top = desc->matrix[L], Ad = desc->matrix_dg_dp;
    if (!top)
      return refuse("matrix[" + str(L) + "] is null");
    const int         singular   = degree_raises ? MGX_ERR_INVALID_ARGUMENT : MGX_ERR_UNSUPPORTED;
    const std::string no_dirichlet = " has no Dirichlet face: the problem is singular (pure Neumann problems are not solved)";
    for (int l = 0; l <= L; ++l)
      {
        mgx_dg_operator_t A     = desc->matrix[l];
        const std::string level = "level " + str(l) + ": matrix[" + str(l) + "]";
        if (!A)
          return refuse(level + " is null");
        if (A->ctx != ctx)
          return refuse(level + " belongs to another context");
        if (A->n_ghost > 0)
          return refuse(level + " has ghost cells; the plain DG multigrid runs on one rank");
        if (A->basis != top->basis || A->number != top->number || (!degree_raises && A->degree != top->degree))
          return refuse(level + " differs from the finest level in " + (degree_raises ? "" : "degree, ") + "basis or number type");
        if (A->dim != top->dim)
          return refuse(level + " has dimension " + str(A->dim) + ", the finest level " + str(top->dim));
        if (!A->has_dirichlet)
          return dg_fail(singular, name + level + no_dirichlet);
        if (l == 0)
          continue;
        mgx_dg_operator_t  C = desc->matrix[l - 1];
        const DGLevelStep *H = desc->transfer ? desc->transfer[l - 1] : nullptr;
        const DGLevelStep *P = desc->degree_transfer ? desc->degree_transfer[l - 1] : nullptr;
        const std::string  step = "the step from level " + str(l - 1) + " to level " + str(l), at = "[" + str(l - 1) + "]";
        if (!degree_raises && !H)
          return refuse("transfer" + at + " is null");
        if ((H != nullptr) == (P != nullptr))
          return refuse(step + " needs exactly one of transfer" + at + " (a mesh refinement) and degree_transfer" + at +
                        " (a degree raise), it has " + (H ? "both" : "neither"));
        const DGLevelStep *S     = H ? H : P;
        const std::string  which = (H ? "transfer" : "degree_transfer") + at;
        if (S->basis != top->basis || S->number != top->number || S->ctx != ctx)
          return refuse(step + ": " + which + " differs from the operators in basis, number type or context");
        if (S->dim != top->dim)
          return refuse(step + ": " + which + " has dimension " + str(S->dim) + ", the operators " + str(top->dim));
        if (H)
          {
            if (C->degree != A->degree || H->fine_degree != A->degree)
              return refuse(step + " is a mesh refinement: the levels have degrees " + str(C->degree) + " and " + str(A->degree) +
                            ", the transfer " + str(H->fine_degree) + " (all equal required)");
            if (H->n_groups != C->n_cells || ((uint64_t)C->n_cells << top->dim) != A->n_cells)
              return refuse(step + " is a mesh refinement: level " + str(l) + " has " + str(A->n_cells) + " cells, level " + str(l - 1) +
                            " " + str(C->n_cells) + " and the transfer " + str(H->n_groups) + " coarse cells (" + str(1 << top->dim) +
                            " x coarse = fine required)");
          }
        else
          {
            if (C->n_cells != A->n_cells || P->n_groups != A->n_cells)
              return refuse(step + " is a degree raise: the levels have " + str(C->n_cells) + " and " + str(A->n_cells) +
                            " cells, the degree transfer " + str(P->n_groups) + " (all equal required)");
            if (C->degree >= A->degree)
              return refuse(step + " is a degree raise: the coarse degree " + str(C->degree) + " must be below the fine degree " +
                            str(A->degree));
            if (P->coarse_degree != C->degree || P->fine_degree != A->degree)
              return refuse(step + ": the degree transfer is between degrees " + str(P->coarse_degree) + " and " + str(P->fine_degree) +
                            ", its operators have " + str(C->degree) + " and " + str(A->degree));
          }
      }
    if (Ad->number != MGX_F64 || Ad->n_cells != top->n_cells || Ad->degree != top->degree || Ad->basis != top->basis || Ad->n_ghost > 0 ||
        Ad->ctx != ctx || Ad->dim != top->dim)
      return refuse("matrix_dg_dp must be the fp64 twin of the operator of level " + str(L) + ", the finest");
    if (!Ad->has_dirichlet)
      return dg_fail(singular, name + "matrix_dg_dp" + no_dirichlet);
    return plain_solver_build(ctx, desc, out);
  }
} // namespace

extern "C" {

int mgx_dg_transfer_create(mgx_context_t ctx, const mgx_dg_transfer_desc *desc, mgx_dg_transfer_t *out)
{
  MGX_REQUIRE(ctx && desc && out && desc->children, "mgx_dg_transfer_create: null argument");
  if (desc->degree < 1 || desc->degree > MGX_MAX_DEGREE)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_transfer_create: degree must be in 1.." + std::to_string(MGX_MAX_DEGREE));
  if (desc->basis < MGX_DG_HERMITE || desc->basis > MGX_DG_GAUSS)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_transfer_create: basis must be MGX_DG_HERMITE, _GAUSS_LOBATTO or _GAUSS");
  if (desc->number != MGX_F32 && desc->number != MGX_F64)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_transfer_create: number must be MGX_F32 or MGX_F64");
  if (desc->n_coarse_cells == 0 || desc->n_coarse_cells >= (1u << 28))
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_transfer_create: n_coarse_cells must be in 1 .. 2^28 - 1");
  const int dim = dg_desc_dim(desc->dim);
  if (dim < 0)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_transfer_create: dim must be 0 or 3 (three dimensions) or 2");
  // every fine cell is the child of exactly one coarse cell: what lets the kernels write without atomics, and what
  // keeps every access inside the fine vector
  const size_t      n_kids = (size_t)1 << dim;
  const size_t      n_fine = n_kids * (size_t)desc->n_coarse_cells;
  std::vector<bool> seen(n_fine, false);
  bool              identity = true;
  for (size_t i = 0; i < n_fine; ++i)
    {
      const uint32_t f = desc->children[i];
      if (f >= n_fine || seen[f])
        return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_transfer_create: children must name every fine cell 0 .. " +
                                                   std::to_string(n_kids) + " n_coarse_cells - 1 exactly once (entry " +
                                                   std::to_string(i) + " = " + std::to_string(f) + ")");
      seen[f]  = true;
      identity = identity && f == i;
    }
  Host1D      h;
  std::string why;
  const int   status = build_1d(desc->degree, desc->basis, h, why);
  if (status != MGX_OK)
    return dg_fail(status, "mgx_dg_transfer_create: " + why);
  std::unique_ptr<mgx_dg_transfer_s, int (*)(mgx_dg_transfer_t)> T(new mgx_dg_transfer_s, mgx_dg_transfer_destroy);
  T->fine_degree = T->coarse_degree = desc->degree;
  T->identity                       = identity;
  MGX_TRY(T->mem.upload(&T->children, desc->children, n_fine));
  MGX_TRY(step_fill(*T, ctx, dim, desc->basis, desc->number, desc->n_coarse_cells, h.embed));
  *out = T.release();
  return MGX_OK;
}

int mgx_dg_degree_transfer_create(mgx_context_t ctx, const mgx_dg_degree_transfer_desc *desc, mgx_dg_degree_transfer_t *out)
{
  MGX_REQUIRE(ctx && desc && out, "mgx_dg_degree_transfer_create: null argument");
  if (desc->number != MGX_F32 && desc->number != MGX_F64)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_degree_transfer_create: number must be MGX_F32 or MGX_F64");
  if (desc->n_cells == 0 || desc->n_cells >= (1u << 31))
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_degree_transfer_create: n_cells must be in 1 .. 2^31 - 1");
  const int dim = dg_desc_dim(desc->dim);
  if (dim < 0)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_degree_transfer_create: dim must be 0 or 3 (three dimensions) or 2");
  // degrees and basis: checked by the host function, which names what it refuses
  std::vector<double> e1d((size_t)(MGX_MAX_DEGREE + 1) * (MGX_MAX_DEGREE + 1));
  MGX_TRY(mgx_dg_degree_embedding(desc->fine_degree, desc->coarse_degree, desc->basis, e1d.data()));
  e1d.resize((size_t)(desc->fine_degree + 1) * (desc->coarse_degree + 1));
  std::unique_ptr<mgx_dg_degree_transfer_s, int (*)(mgx_dg_degree_transfer_t)> T(new mgx_dg_degree_transfer_s,
                                                                                 mgx_dg_degree_transfer_destroy);
  T->fine_degree   = desc->fine_degree;
  T->coarse_degree = desc->coarse_degree;
  MGX_TRY(step_fill(*T, ctx, dim, desc->basis, desc->number, desc->n_cells, e1d));
  *out = T.release();
  return MGX_OK;
}

int mgx_dg_transfer_destroy(mgx_dg_transfer_t T) { return step_destroy(T); }
int mgx_dg_degree_transfer_destroy(mgx_dg_degree_transfer_t T) { return step_destroy(T); }

int mgx_dg_transfer_prolongate_and_add(mgx_dg_transfer_t T, void *fine_dst, const void *coarse_src)
{
  return step_apply(T, true, fine_dst, coarse_src, "mgx_dg_transfer_prolongate_and_add");
}

int mgx_dg_transfer_restrict_and_add(mgx_dg_transfer_t T, void *coarse_dst, const void *fine_src)
{
  return step_apply(T, false, coarse_dst, fine_src, "mgx_dg_transfer_restrict_and_add");
}

int mgx_dg_degree_transfer_prolongate_and_add(mgx_dg_degree_transfer_t T, void *fine_dst, const void *coarse_src)
{
  return step_apply(T, true, fine_dst, coarse_src, "mgx_dg_degree_transfer_prolongate_and_add");
}

int mgx_dg_degree_transfer_restrict_and_add(mgx_dg_degree_transfer_t T, void *coarse_dst, const void *fine_src)
{
  return step_apply(T, false, coarse_dst, fine_src, "mgx_dg_degree_transfer_restrict_and_add");
}

int mgx_dg_transfer_matrix(mgx_dg_transfer_t T, double *p1d) { return step_matrix(T, p1d, "mgx_dg_transfer_matrix"); }
int mgx_dg_degree_transfer_matrix(mgx_dg_degree_transfer_t T, double *e1d) { return step_matrix(T, e1d, "mgx_dg_degree_transfer_matrix"); }

int mgx_dg_hp_solver_create(mgx_context_t ctx, const mgx_dg_hp_solver_desc *desc, mgx_dg_plain_solver_t *out)
{
  if (!desc)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_hp_solver_create: null argument");
  return plain_solver_create("mgx_dg_hp_solver_create: ", true, ctx, desc, out);
}

int mgx_dg_plain_solver_create(mgx_context_t ctx, const mgx_dg_plain_solver_desc *desc, mgx_dg_plain_solver_t *out)
{
  if (!desc)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_plain_solver_create: null argument");
  const mgx_dg_hp_solver_desc levels{desc->n_levels, desc->matrix, desc->matrix_dg_dp, desc->transfer, nullptr, desc->degree_pre,
                                     desc->cell_global_id};
  return plain_solver_create("mgx_dg_plain_solver_create: ", false, ctx, &levels, out);
}

int mgx_dg_plain_solver_destroy(mgx_dg_plain_solver_t S)
{
  if (!S)
    return MGX_OK;
  if (S->ctx)
    (void)hipStreamSynchronize((hipStream_t)mgx_context_stream(S->ctx));
  delete S;
  return MGX_OK;
}

int mgx_dg_plain_solver_smoother_info(mgx_dg_plain_solver_t S, int level, mgx_smoother_info *info)
{
  if (!S || !info || level < 0 || level >= (int)S->level.size())
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_plain_solver_smoother_info: null argument or no such level");
  *info = S->level[level].info;
  return MGX_OK;
}

int mgx_dg_plain_solver_vmult(mgx_dg_plain_solver_t S, double *dst, const double *src)
{
  MGX_REQUIRE(S && dst && src, "mgx_dg_plain_solver_vmult: null argument");
  return dg_level_vmult(S->ctx, S->level.back(), [S] { return plain_v_cycle(S, (int)S->level.size() - 1); }, dst, src);
}

int mgx_dg_plain_solver_solve_cg(mgx_dg_plain_solver_t S, double tolerance, const double *rhs, double *solution,
                                 unsigned *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S && rhs && solution, "mgx_dg_plain_solver_solve_cg: null argument");
  // preconditioner = one V-cycle (multigrid_solver_dg_plain.h:303-317)
  const auto v_cycle = [S](void *z, const void *r) { return mgx_dg_plain_solver_vmult(S, (double *)z, (const double *)r); };
  return dg_solve_cg(S->ctx, S->A_dp, S->level.back(), v_cycle, tolerance, rhs, solution, iterations, reduction_rate,
                     "mgx_dg_plain_solver_solve_cg");
}

int mgx_dg_plain_solver_vmult_with_residual_update(mgx_dg_plain_solver_t S, double *residual, double *update, double factor,
                                                   double sums[2])
{
  MGX_REQUIRE(S && residual && update && sums && residual != update, "mgx_dg_plain_solver_vmult_with_residual_update: null or aliased argument");
  hipStream_t s   = (hipStream_t)mgx_context_stream(S->ctx);
  DGLevel    &top = S->level.back();
  mgx::launch_residual_pre(s, S->number, top.defect, residual, update, factor, top.n); // :353-358
  MGX_TRY(plain_v_cycle(S, (int)S->level.size() - 1));                                 // :362
  // :365-413 (no constrained rows in DG: every entry takes the V-cycle's value); block sums added in a fixed order
  return mgx::residual_update_finish(s, S->number, top.update, residual, update, factor, top.n, top.n, S->partials, S->sums, sums);
}

int mgx_dg_plain_solver_enable_timings(mgx_dg_plain_solver_t S, int on)
{
  MGX_REQUIRE(S, "mgx_dg_plain_solver_enable_timings: null solver");
  S->timed = on != 0;
  return MGX_OK;
}

int mgx_dg_plain_solver_get_timings(mgx_dg_plain_solver_t S, double *times)
{
  MGX_REQUIRE(S && times, "mgx_dg_plain_solver_get_timings: null argument");
  for (size_t l = 0; l < S->level.size(); ++l)
    for (int j = 0; j < 6; ++j)
      {
        times[6 * l + j]       = S->level[l].times[j];
        S->level[l].times[j] = 0.;
      }
  return MGX_OK;
}

int mgx_dg_plain_solver_do_matvec(mgx_dg_plain_solver_t S)
{
  MGX_REQUIRE(S, "mgx_dg_plain_solver_do_matvec: null solver");
  return mgx_dg_vmult(S->A_dp, S->level.back().h, S->level.back().d); // matrix_dg_dp.vmult(residual, solution), :435
}

int mgx_dg_plain_solver_do_matvec_smoother(mgx_dg_plain_solver_t S)
{
  MGX_REQUIRE(S, "mgx_dg_plain_solver_do_matvec_smoother: null solver");
  DGLevel &top = S->level.back();
  return mgx_dg_vmult(top.A, top.t, top.defect); // matrix[maxlevel].vmult, :444
}

} // extern "C"

/* ---------------------------------------------------------------------------------------------
 * lumped-mass PCG on the DG operator (solver_dg/program.cc:134-148, 177-178, 222-263)
 * --------------------------------------------------------------------------------------------- */
namespace
{
  bool pcg_positive_finite(double v) { return v > 0. && std::isfinite(v); }

  // what both forms report from the history rho[0 .. k]
  void pcg_report(const std::vector<double> &rho, unsigned k, unsigned *iterations, double *reduction_rate)
  {
    if (iterations)
      *iterations = k;
    if (reduction_rate)
      *reduction_rate = k > 0 && rho[0] > 0. ? std::pow(std::sqrt(rho[k] / rho[0]), 1.0 / k) : 0.;
  }

  // The merged form: per iteration the cell kernel (q = A p and the block sums), one workgroup that adds them and writes
  // alpha, beta and the history, and the update kernel.  Nothing returns to the host inside the loop; the host looks at
  // the history every check_every iterations if there is a tolerance, once at the end otherwise.
  int pcg_solve_merged(mgx_dg_pcg_solver_t S, const void *rhs, void *x, unsigned *k_stop)
  {
    hipStream_t       s  = (hipStream_t)mgx_context_stream(S->ctx);
    mgx_dg_operator_t A  = S->A;
    const unsigned    nk = S->max_iterations;
    mgx::launch_pcg_start(s, A->number, x, S->r, S->p, rhs, A->lumped_inv, S->n3, S->n);
    DGLaunch l(kPcgSums, S->q, S->r, S->p);
    l.partials = S->partials;
    l.lumped   = A->lumped_inv;
    l.n_cells  = A->n_cells;
    double   head[4]; // scalars
    unsigned done = 0;
    *k_stop       = nk;
    while (done < nk)
      {
        MGX_TRY(launch_cells(A, l));
        mgx::launch_pcg_scalars(s, S->partials, S->blocks, done, S->scalars, S->rho_dev, S->presums);
        mgx::launch_pcg_update(s, A->number, x, S->r, S->p, S->q, A->lumped_inv, S->n3, S->scalars, S->n);
        ++done;
        if (S->tolerance > 0. && (done % S->check_every == 0 || done == nk))
          {
            MGX_HIP(hipMemcpyAsync(head, S->scalars, sizeof(head), hipMemcpyDeviceToHost, s));
            MGX_HIP(hipMemcpyAsync(S->rho.data(), S->rho_dev, sizeof(double) * (done + 1), hipMemcpyDeviceToHost, s));
            MGX_HIP(hipStreamSynchronize(s));
            if (head[2] >= 0.)
              {
                *k_stop = (unsigned)head[2];
                break;
              }
            if (std::sqrt(S->rho[done] / S->rho[0]) <= S->tolerance)
              {
                *k_stop = done;
                break;
              }
          }
      }
    MGX_HIP(hipGetLastError());
    if (S->tolerance > 0.)
      {
        S->rho.resize(done + 1);
        return MGX_OK;
      }
    MGX_HIP(hipMemcpyAsync(head, S->scalars, sizeof(head), hipMemcpyDeviceToHost, s));
    MGX_HIP(hipMemcpyAsync(S->rho.data(), S->rho_dev, sizeof(double) * (nk + 1), hipMemcpyDeviceToHost, s));
    MGX_HIP(hipStreamSynchronize(s));
    if (head[2] >= 0.)
      *k_stop = (unsigned)head[2];
    return MGX_OK;
  }

  // The separate form, the yardstick: textbook PCG (deal.II's SolverCG around the cell-based operator, :222-241) from
  // mgx_dg_vmult and the dot / update kernels of the FE_Q solver, the scalars on the host.  Same history, same stopping
  // rule, same breakdown rule as the merged form.
  int pcg_solve_separate(mgx_dg_pcg_solver_t S, const void *rhs, void *x, unsigned *k_stop)
  {
    hipStream_t       s   = (hipStream_t)mgx_context_stream(S->ctx);
    mgx_dg_operator_t A   = S->A;
    const int         num = A->number;
    const unsigned    nk  = S->max_iterations;
    auto              fetch = [&](double *v) {
      MGX_HIP(hipMemcpyAsync(v, S->result, sizeof(double), hipMemcpyDeviceToHost, s));
      MGX_HIP(hipStreamSynchronize(s));
      return (int)MGX_OK;
    };
    MGX_HIP(hipMemsetAsync(x, 0, dg_nsz(num) * S->n, s));
    MGX_HIP(hipMemcpyAsync(S->r, rhs, dg_nsz(num) * S->n, hipMemcpyDeviceToDevice, s));
    mgx::launch_jacobi_dot(s, num, S->z, S->dinv, S->r, S->n, S->partials, S->result); // z = M^-1 r ; r.z
    MGX_HIP(hipMemcpyAsync(S->p, S->z, dg_nsz(num) * S->n, hipMemcpyDeviceToDevice, s));
    double rho = 0, pq = 0;
    MGX_TRY(fetch(&rho));
    S->rho[0] = rho >= 0. && std::isfinite(rho) ? rho : 0.;
    unsigned done = 0;
    *k_stop       = nk;
    bool stalled  = false;
    while (done < nk)
      {
        if (!stalled)
          {
            MGX_TRY(mgx_dg_vmult(A, S->q, S->p));
            mgx::launch_dot(s, num, S->p, S->q, S->n, S->partials, S->result);
            MGX_TRY(fetch(&pq));
            stalled = !(pcg_positive_finite(pq) && pcg_positive_finite(rho));
          }
        double rho_next = S->rho[done];
        if (!stalled)
          {
            const double alpha = rho / pq;
            mgx::launch_cg_update(s, num, x, S->r, S->p, S->q, alpha, S->n, S->partials, S->result); // x += alpha p ; r -= alpha q
            mgx::launch_jacobi_dot(s, num, S->z, S->dinv, S->r, S->n, S->partials, S->result);
            MGX_TRY(fetch(&rho_next));
            // (a residual that has reached zero is a breakdown of the next iteration, not of this one)
            if (!(rho_next >= 0.) || !std::isfinite(rho_next))
              return dg_fail(MGX_ERR_NOT_CONVERGED, "mgx_dg_pcg_solver_solve: r.M^-1 r is not a number");
            mgx::launch_xpby(s, num, S->p, S->z, rho_next / rho, S->n);
            rho = rho_next;
          }
        else if (*k_stop == nk)
          *k_stop = done;
        ++done;
        S->rho[done] = rho_next;
        if (S->tolerance > 0. && (done % S->check_every == 0 || done == nk))
          {
            if (stalled)
              break;
            if (std::sqrt(S->rho[done] / S->rho[0]) <= S->tolerance)
              {
                *k_stop = done;
                break;
              }
          }
      }
    MGX_HIP(hipGetLastError());
    S->rho.resize(done + 1);
    return MGX_OK;
  }
} // namespace

extern "C" {

int mgx_dg_pcg_solver_create(mgx_context_t ctx, const mgx_dg_pcg_solver_desc *desc, mgx_dg_pcg_solver_t *out)
{
  MGX_REQUIRE(ctx && desc && out && desc->matrix, "mgx_dg_pcg_solver_create: null argument");
  mgx_dg_operator_t A = desc->matrix;
  if (A->ctx != ctx)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_pcg_solver_create: operator of another context");
  if (desc->form != MGX_DG_PCG_MERGED && desc->form != MGX_DG_PCG_SEPARATE)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_pcg_solver_create: form must be MGX_DG_PCG_MERGED or MGX_DG_PCG_SEPARATE");
  if (!(desc->tolerance >= 0.) || !std::isfinite(desc->tolerance))
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_pcg_solver_create: tolerance must be a finite number >= 0");
  if (desc->check_every < 1)
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_pcg_solver_create: check_every must be at least 1");
  if (desc->max_iterations >= (1u << 24))
    return dg_fail(MGX_ERR_INVALID_ARGUMENT, "mgx_dg_pcg_solver_create: max_iterations must be below 2^24");
  if (A->n_ghost > 0)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_pcg_solver_create: the operator has ghost cells; the lumped-mass PCG runs on one "
                                        "rank (its scalars stay on the device, there is no allreduce)");
  if (!A->has_dirichlet)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_pcg_solver_create: the operator has no Dirichlet face: the problem is singular (pure "
                                        "Neumann problems are not solved)");
  for (size_t i = 0; i < A->lumped_inv_host.size(); ++i)
    if (!pcg_positive_finite(A->lumped_inv_host[i]))
      return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_pcg_solver_create: the lumped mass of local index " + std::to_string(i) +
                                            " is not positive: no preconditioner for this basis");
  std::unique_ptr<mgx_dg_pcg_solver_s, int (*)(mgx_dg_pcg_solver_t)> S(new mgx_dg_pcg_solver_s, mgx_dg_pcg_solver_destroy);
  S->ctx            = ctx;
  S->A              = A;
  S->form           = desc->form;
  S->max_iterations = desc->max_iterations;
  S->check_every    = desc->check_every;
  S->tolerance      = desc->tolerance;
  S->n              = (size_t)mgx_dg_operator_n_dofs(A);
  S->n3             = (uint32_t)dg_cell_entries(A->degree, A->dim);
  if (S->n3 > mgx::kPcgTableMax)
    return dg_fail(MGX_ERR_UNSUPPORTED, "mgx_dg_pcg_solver_create: more entries per cell than the update kernel's table holds");
  S->rho.assign((size_t)S->max_iterations + 1, 0.);
  hipStream_t  s   = (hipStream_t)mgx_context_stream(ctx);
  const size_t vec = dg_nsz(A->number) * S->n;
  for (void **v : {&S->r, &S->p, &S->q})
    {
      MGX_TRY(S->mem.zeros(v, vec, s));
    }
  if (S->form == MGX_DG_PCG_MERGED)
    {
      S->blocks = cell_grid(A->number, A->degree, A->n_cells, A->dim);
      MGX_TRY(S->mem.zeros(&S->partials, 4 * (size_t)S->blocks, s));
      MGX_TRY(S->mem.zeros(&S->presums, 4 * (size_t)mgx::kPcgPresums, s));
      MGX_TRY(S->mem.zeros(&S->scalars, 4, s));
      MGX_TRY(S->mem.zeros(&S->rho_dev, (size_t)S->max_iterations + 1, s));
    }
  else
    {
      MGX_TRY(S->mem.zeros(&S->z, vec, s));
      MGX_TRY(S->mem.alloc(&S->dinv, vec));
      mgx::launch_tile_table(s, A->number, S->dinv, A->lumped_inv, S->n3, S->n);
      MGX_TRY(S->mem.zeros(&S->partials, (size_t)mgx::kDotBlocks, s));
      MGX_TRY(S->mem.zeros(&S->result, 1, s));
    }
  MGX_HIP(hipGetLastError());
  MGX_HIP(hipStreamSynchronize(s));
  *out = S.release();
  return MGX_OK;
}

int mgx_dg_pcg_solver_destroy(mgx_dg_pcg_solver_t S)
{
  if (!S)
    return MGX_OK;
  if (S->ctx)
    (void)hipStreamSynchronize((hipStream_t)mgx_context_stream(S->ctx));
  delete S;
  return MGX_OK;
}

int mgx_dg_pcg_solver_solve(mgx_dg_pcg_solver_t S, const void *rhs, void *solution, unsigned *iterations, double *reduction_rate)
{
  MGX_REQUIRE(S && rhs && solution && rhs != solution, "mgx_dg_pcg_solver_solve: null or aliased vectors");
  S->rho.assign((size_t)S->max_iterations + 1, 0.);
  unsigned k = 0;
  if (S->max_iterations == 0)
    {
      hipStream_t s = (hipStream_t)mgx_context_stream(S->ctx);
      MGX_HIP(hipMemsetAsync(solution, 0, dg_nsz(S->A->number) * S->n, s)); // :225 output = 0
      MGX_HIP(hipStreamSynchronize(s));
    }
  else
    MGX_TRY(S->form == MGX_DG_PCG_MERGED ? pcg_solve_merged(S, rhs, solution, &k) : pcg_solve_separate(S, rhs, solution, &k));
  pcg_report(S->rho, k, iterations, reduction_rate);
  return MGX_OK;
}

int mgx_dg_pcg_solver_history(mgx_dg_pcg_solver_t S, double *rho, unsigned *count)
{
  MGX_REQUIRE(S && count, "mgx_dg_pcg_solver_history: null argument");
  *count = (unsigned)S->rho.size();
  if (rho)
    std::copy(S->rho.begin(), S->rho.end(), rho);
  return MGX_OK;
}

} // extern "C"
