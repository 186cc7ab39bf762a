/*
 * mgx_dg.h -- C ABI of the MI355X-native DG (symmetric interior penalty) Laplace operator with the
 * merged Chebyshev update (libmgx.so); BASELINE config 5, first slice: one GPU, affine mesh.
 *
 * Reference interface replaced (paths relative to the reference root):
 *     multigrid::LaplaceOperatorCompactCombine<3,p,Number,type>  common/laplace_operator_dg.h:350-2024
 *     multigrid::JacobiTransformed<3,p,Number,type>              common/laplace_operator_dg.h:2028-2256
 * as driven by matvec_dg_cheby/program.cc:40-200.  Conventions as in mgx.h (status codes, device
 * pointers, the context's stream, no CPU fallback).
 *
 * Vector layout: the reference's DG numbering -- (p+1)^3 contiguous coefficients per cell, x
 * fastest (laplace_operator_dg.h:1141-1146 reads a cell as one contiguous block) -- cells in the
 * order of the neighbour table handed to mgx_dg_operator_create.
 */
#ifndef MGX_DG_H
#define MGX_DG_H

#include "mgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `type` template parameter of LaplaceOperatorCompactCombine (laplace_operator_dg.h:343-348) */
#define MGX_DG_HERMITE 0       /* FE_DGQHermite: neighbour access of two node layers only */
#define MGX_DG_GAUSS_LOBATTO 1 /* FE_DGQ */
#define MGX_DG_GAUSS 2         /* FE_DGQArbitraryNodes(QGauss): collocation, no basis change */

#define MGX_DG_BOUNDARY (-1)   /* neighbour entry of a (homogeneous Dirichlet) boundary face */
/* neighbour entry of a boundary face with the natural (Neumann) condition: the face contributes nothing to the bilinear
 * form of the face-based SIP formulation (laplace_operator_dg_face.h:66-160, which integrates Dirichlet faces only); its
 * datum h = d_n u enters the right-hand side as int_F h phi_i (mgx_dg_compute_rhs_mixed).  Every action of the operator
 * (vmult, residual, the merged Chebyshev and CG forms, block Jacobi), 3D and 2D, every basis, degree and number type,
 * decomposed or not.  An operator whose faces are all interior or Neumann faces is singular (constants); it can be
 * created and applied but the solvers below refuse it. */
#define MGX_DG_NEUMANN (-2)

typedef struct mgx_dg_operator_s *mgx_dg_operator_t;

/* Ghost-cell exchange of a decomposed DG mesh (replaces the MPI_Isend / MPI_Irecv of face data,
 * laplace_operator_dg.h:986-1057, and the send lists built at :607-723).  A rank stores its owned
 * cells first and, behind them, one ghost for every cell of another rank that shares a face with an
 * owned cell; neighbour-table entries >= n_cells address them.  A ghost holds the reference's
 * data_per_face (:565): the whole cell for the two Lagrange bases; for the Hermite-like basis two
 * values per face point, the trace and the normal derivative as the owner computes them from its two
 * node layers (:1015-1039), [face point][2], 2 (p+1)^2 entries.  Ghosts of one rank are contiguous.  Both sides of a pair exchange the same number of cells (true for block
 * decompositions; checked).  An operator application runs the cells without a ghost neighbour while
 * the exchange is in flight on a second stream, the others behind it (the reference waits for the
 * exchange, :1057, before its cell loop); owned cells ordered interior-first make both parts
 * contiguous launches. */
typedef struct
{
  int                    plan_id;
  int                    n_neighbors;
  const int             *neighbor_rank; /* ascending */
  const uint32_t        *count;         /* cells sent to = received from neighbour k */
  const uint32_t *const *send_cells;    /* owned cells to send, in the order the neighbour stores them */
  const uint32_t        *recv_first;    /* first ghost cell (>= n_cells) filled by neighbour k */
} mgx_dg_exchange_desc;

typedef struct
{
  int      degree;             /* 1 .. MGX_MAX_DEGREE */
  int      basis;              /* MGX_DG_* */
  int      number;             /* MGX_F32 (matvec_dg_cheby/program.cc:88) or MGX_F64 */
  uint32_t n_cells;
  /* [n_cells][6] cell behind face 2d+s (direction d, lower s = 0 / upper s = 1 side),
   * MGX_DG_BOUNDARY or MGX_DG_NEUMANN; replaces start_indices_on_neighbor / dirichlet_faces
   * (laplace_operator_dg.h:453-459, 480-560).  Host memory, copied. */
  const int32_t *neighbours;
  /* the one cell Jacobian dx/dxi, row-major [real][reference]; the reference asserts a single
   * Jacobian for the whole mesh as well (laplace_operator_dg.h:749-750) */
  double jacobian[9];
  /* decomposed mesh (one rank per GPU; the context carries the communicator, mgx.h): number of
   * ghost cells and their exchange; 0 / NULL on a single rank.  Vectors then hold
   * mgx_dg_operator_vector_size() entries, owned cells first, like deal.II's owned | ghost layout */
  uint32_t                    n_ghost_cells;
  const mgx_dg_exchange_desc *exchange;
  /* space dimension of the cells: 0 or 3: three (everything above), 2: two -- LaplaceOperatorCompactCombine<2,...>
   * (the dim == 2 branches, laplace_operator_dg.h:418, 1028, 1147, 1675) as poisson_dg_plain/program.cc:65 sets it.
   * Then neighbours is [n_cells][4] (face 2d+s, d = 0, 1), jacobian holds a row-major 2 x 2 in its first four entries
   * (the rest is ignored), vectors hold (p+1)^2 coefficients per cell, x fastest, and n_ghost_cells must be 0 (one
   * rank only).  Any other value: MGX_ERR_INVALID_ARGUMENT. */
  int dim;
} mgx_dg_operator_desc;

/* LaplaceOperatorCompactCombine::reinit (:361-771) + JacobiTransformed::JacobiTransformed
 * (:2031-2038, local_compute_diagonals :2099-2233): 1D basis data, penalty and normal factors,
 * eigenvector basis and the inverse transformed diagonals (one set per combination of Dirichlet
 * faces -- at most 64 -- instead of one per cell; with Neumann faces one set per combination of face kinds that occurs
 * in the mesh, of 3^6).  Refused with MGX_ERR_UNSUPPORTED if a transformed diagonal is not positive.  An operator with a
 * cell whose faces are all Neumann faces (a one-cell pure-Neumann mesh) is refused with the same status: the block of
 * that cell is singular, the constants are in its null space, and block Jacobi cannot invert it. */
/* desc->dim == 2: the same with the dim == 2 branches (:418 data per face, :749-771 geometry; JacobiTransformed
 * :2162): 16 combinations of Dirichlet faces. */
int mgx_dg_operator_create(mgx_context_t ctx, const mgx_dg_operator_desc *desc, mgx_dg_operator_t *op);
int mgx_dg_operator_destroy(mgx_dg_operator_t op);

/* LaplaceOperatorCompactCombine::m (:796-800): n_cells (p+1)^dim */
uint64_t mgx_dg_operator_n_dofs(mgx_dg_operator_t op);

/* entries of a vector including the ghost cells (== mgx_dg_operator_n_dofs on a single rank) */
uint64_t mgx_dg_operator_vector_size(mgx_dg_operator_t op);
/* Vector::update_ghost_values (the import of laplace_operator_dg.h:986-1057): fills the ghost cells
 * of vec from their owners.  Every operator application below does this for its source vector
 * (whose ghost part is therefore written although the argument is const). */
/* A 2D operator lives on one rank (the exchange of :1028 is not built): MGX_ERR_UNSUPPORTED. */
int mgx_dg_update_ghost_values(mgx_dg_operator_t op, void *vec);

/* LaplaceOperatorCompactCombine::vmult (:802-806, action 0).  dst must not alias src.  2D operators: the cell loop
 * of :1147 with the dim == 2 cell term (:1675) and faces (:1418), as the three entry points below. */
int mgx_dg_vmult(mgx_dg_operator_t op, void *dst, const void *src);

/* vmult_with_merged_ops<4> (:962-966, epilogue :1812-1818): dst = rhs - A src */
int mgx_dg_vmult_residual(mgx_dg_operator_t op, void *dst, const void *rhs, const void *src);

/* JacobiTransformed::vmult (:2046-2084): dst = T D^-1 T^T src per cell.  dst may alias src. */
int mgx_dg_jacobi_vmult(mgx_dg_operator_t op, void *dst, const void *src);

/* LaplaceOperatorCompactCombine::vmult_with_chebyshev_update (:910-955, epilogue :1839-1860).
 *   iteration_index == 0:  solution = factor2 P^-1 rhs
 *   iteration_index == 1:  new = factor2 P^-1 (rhs - A solution) + (1 + factor1) solution
 *   iteration_index >= 2:  new = ... - factor1 solution_old
 * For iteration_index >= 1 `new` is written over solution_old; the reference then swaps the two
 * vectors (:931) -- with raw pointers that swap is the caller's (the Python binding and
 * tools/matvec_dg_cheby.py do it).  solution and solution_old must not alias. */
int mgx_dg_vmult_with_chebyshev_update(mgx_dg_operator_t op, const void *rhs, unsigned iteration_index,
                                       double factor1, double factor2, void *solution, void *solution_old);

/* LaplaceOperatorCompactCombine::vmult_with_cg_update (:863-908; action 2, epilogue :1827-1838): one iteration of
 * the merged conjugate-gradient loop around the operator,
 *   alpha != 0:  x += alpha p ;  p = beta p + q      alpha == 0:  p = q
 *   q = A p ;  sums = { q.p, r.r, q.r, q.q }  summed over all ranks (host array)
 * The four sums come out of the cell kernel's epilogue (block sums added in a fixed order). */
/* Not built for 2D operators (the plain solver does not run it): MGX_ERR_UNSUPPORTED. */
int mgx_dg_vmult_with_cg_update(mgx_dg_operator_t op, double alpha, double beta, const void *r, void *q, void *p, void *x,
                                double sums[4]);

/* The preconditioner of solver_dg/program.cc:134-148, the inverse of the lumped mass matrix: the mesh has one cell
 * Jacobian, so it is one table of (p+1)^dim numbers,
 *   1 / lumped[i],  lumped[i] = |det J| prod_d sum_q w_q phi_{i_d}(x_q)   ((p+1)-point Gauss rule, x fastest),
 * computed in double when the operator is created and kept on the device in the operator's number type.  `table`: host
 * array of (p+1)^dim entries.  An entry is not positive and finite where the lumped mass is not (none of the three
 * bases at p = 1 .. 9); mgx_dg_pcg_solver_create then refuses the operator.  Works in 3D and 2D. */
int mgx_dg_operator_lumped_mass_inverse(mgx_dg_operator_t op, double *table);

/* The operator's part of one merged iteration of that preconditioned CG (solver_dg/program.cc:222-263; action
 * kPcgSums of both cell kernels):
 *   q = A p ;  sums = { q.p, r.(m r), q.(m r), q.(m q) }  summed over all ranks (host array)
 * with m the table above at every entry's local index.  The sums are formed in double in the cell kernel's epilogue
 * and added in a fixed order: the same bits in every run.  r and p are not written (but for p's ghost part, as in
 * every application); q must alias neither.  3D, decomposed or not, and 2D. */
int mgx_dg_vmult_with_pcg_sums(mgx_dg_operator_t op, const void *r, void *q, const void *p, double sums[4]);

/* 1D data of the operator for inspection: hermite_derivative_on_face (:408-409), the penalty
 * parameters get_penalty(face 2d) (:789-793) and the 1D generalised eigenvalues (:207-208).
 * Any pointer may be NULL.  A 2D operator fills penalty[0..1] and leaves penalty[2] untouched. */
int mgx_dg_operator_info(mgx_dg_operator_t op, double *hermite_derivative_on_face, double penalty[3],
                         double eigenvalues_1d[MGX_MAX_DEGREE + 1]);

/* 1D element data a harness needs for right-hand sides and error norms (what FEEvaluation hands the
 * reference's drivers): shape_values[q*(p+1)+i] = phi_i at Gauss point q of [0,1], the points and
 * weights of the (p+1)-point Gauss rule.  Any pointer may be NULL. */
int mgx_dg_operator_basis(mgx_dg_operator_t op, double *shape_values, double *quadrature_points,
                          double *quadrature_weights);

/* ---- right-hand side with Dirichlet boundary data and the L2 error, on the device ----
 * The reference's DG solvers integrate the volume term of the right-hand side only (common/multigrid_solver_dg_plain.h:
 * 163-185, multigrid_solver_dg.h:243-262) although their solution does not vanish on the boundary.  The face-based form
 * (laplace_operator_dg_face.h:146-157), a_F(u, v) = int_F (sigma_F u v - d_n u v - u d_n v) on a Dirichlet face F, says what
 * boundary values g add:  b_i += int_F g (sigma_F phi_i - d_n phi_i).  The operator stays linear (homogeneous mirror
 * values); the right-hand side carries the data.  3D and 2D, all bases, degrees and number types. */

/* Integer position of every owned cell -- the cell_ijk / cell_ij of mgx_dg_box_neighbours[_2d] -- host [n_cells][dim],
 * copied; real coordinates are x = origin + J (pos + xi), J the operator's Jacobian, xi in [0,1]^dim (origin[2] is not
 * read in 2D).  May be called again.  Without it a request that needs coordinates (a sine product) returns
 * MGX_ERR_INVALID_ARGUMENT. */
int mgx_dg_operator_set_cell_positions(mgx_dg_operator_t op, const double origin[3], const int32_t *cell_pos);

#define MGX_DG_FN_SINE_PRODUCT 1 /* amplitude prod_d sin(wave[d] x_d + phase[d]), evaluated in the kernel (in double) */
#define MGX_DG_FN_SAMPLED 2      /* values in the quadrature points, device arrays of doubles */
#define MGX_DG_FN_NONE 0         /* (internal: what a NULL function stands for) */
typedef struct
{
  int kind; /* MGX_DG_FN_SINE_PRODUCT or MGX_DG_FN_SAMPLED */
  /* sine product: the number of directions, 0 or 3: three, 2: two; it must be the operator's.  Sampled: not read. */
  int    dim;
  double amplitude, wave[3], phase[3];
  /* sampled, device, cells in the operator's order: cell_values [n_cells][(p+1)^dim], the values in the Gauss points, x
   * fastest (read where the function is f or u); face_values [n_cells][2 dim][(p+1)^(dim-1)], face 2d+s, the Gauss
   * points of the face with the lower remaining direction fastest (read where the function is g; only the entries of
   * Dirichlet faces are).  Whichever is not read may be NULL.  A sampled function needs no cell positions. */
  const double *cell_values, *face_values;
} mgx_dg_function;

/* For every owned cell  dst_i = int_K f phi_i + sum over the Dirichlet faces F of K  int_F g (sigma_F phi_i - d_n phi_i)
 * on the (p+1)-point Gauss rule, sigma_F, the face weight and the normal from the operator's own geometry.  f == NULL:
 * f = 0; g == NULL: the reference's volume-only vector.  dst (device, the operator's number type) is overwritten; the
 * arithmetic, function evaluation included, is in double and only the store converts.  One writer per entry, no
 * atomics: the same bits in every run.  Decomposed operators: owned cells only, the ghost part of dst is left alone;
 * no communication (a face to another rank is not a Dirichlet face). */
/* Neumann faces of the operator are treated as such, with zero flux (mgx_dg_compute_rhs_mixed with h == NULL). */
int mgx_dg_compute_rhs(mgx_dg_operator_t op, const mgx_dg_function *f, const mgx_dg_function *g, void *dst);

/* The same plus the Neumann term: dst_i += sum over the Neumann faces F of K  int_F h phi_i, h the outward normal
 * derivative d_n u prescribed on F.  h == NULL: zero flux.  h sampled: face_values ([n_cells][2 dim][(p+1)^(dim-1)], as
 * for g) holds h in the Gauss points of the faces; only the entries of Neumann faces are read.  h a sine product: the
 * struct describes a potential u, and the kernel forms h = n . grad u with the outward unit normal of the operator's own
 * geometry -- on a sheared mesh the flux of a sine product is not one itself.  In double, one writer per entry. */
int mgx_dg_compute_rhs_mixed(mgx_dg_operator_t op, const mgx_dg_function *f, const mgx_dg_function *g, const mgx_dg_function *h,
                             void *dst);

/* sums = { sum_K sum_q (u_h(x_q) - u(x_q))^2 JxW_q,  sum_K sum_q JxW_q } over this rank's owned cells, u_h the function
 * of vec (device, the operator's number type): the two numbers of compute_l2_error (multigrid_solver_dg_plain.h:219-259)
 * before the sum over the ranks and the square root -- no communication here; the caller adds over the ranks and takes
 * sqrt(sums[0] / sums[1]).  Block sums in double, added in a fixed order: the same bits in every run. */
int mgx_dg_compute_l2_error(mgx_dg_operator_t op, const void *vec, const mgx_dg_function *u, double sums[2]);

/* ---- MultigridSolverDG<dim,p,Number,double> (common/multigrid_solver_dg.h:55-747): the DG level on top
 * of the FE_Q(p) multigrid hierarchy of the same mesh.  Every mgx_dg_solver_* and the three transfer entry points
 * below serve dim = 3 (one or several ranks) and dim = 2 (one rank: 2D DG operators over the FE_Q solver of an
 * mgx_square).  In 2D every result is bitwise reproducible: the DG -> FE_Q restriction, stand-alone or inside the cell
 * kernel, adds without atomics in launches over cells that share no FE_Q DoF. ---- */
typedef struct mgx_dg_solver_s *mgx_dg_solver_t;
typedef struct
{
  mgx_dg_operator_t matrix_dg;    /* V-cycle number type (multigrid_solver_dg.h:700) */
  mgx_dg_operator_t matrix_dg_dp; /* its fp64 twin for the outer iteration (:703) */
  /* MultigridSolver of the FE_Q(p) hierarchy (include/mgx.h) in the V-cycle number type, built on
   * the same context; the cells of its finest level in the order of the DG operators' cells.  The
   * DG solver re-configures its smoothers as the reference does (:271-291: degree_pre - 1 on the
   * finest FE_Q level, coarse tolerance 2e-3) and runs its V-cycle in place. */
  mgx_solver_t      cfe;
  int               degree_pre;   /* Chebyshev degree of the DG smoother (:300) */
  /* optional, host [n_cells]: a decomposition-independent id of every owned cell (e.g. its
   * lexicographic position in the whole mesh); the start vector of the eigenvalue estimate is
   * ((id (p+1)^3 + local index) mod 11) - mean, deal.II's (global DoF index mod 11) - mean.
   * NULL: the cell's index on this rank.  Decomposed meshes: matrix_dg / matrix_dg_dp carry ghost
   * cells (all device vectors of the solver interface then have mgx_dg_operator_vector_size
   * entries), cfe is the decomposed FE_Q solver of the same partition, not agglomerated. */
  const uint32_t   *cell_global_id;
} mgx_dg_solver_desc;
/* ctor (:58-323), incl. smooth_dg.initialize: eigenvalue estimate with JacobiTransformed.  Refused with
 * MGX_ERR_UNSUPPORTED: 2D operators with cfe == NULL; DG operators and an FE_Q hierarchy of different dimensions;
 * operators with Neumann faces (the FE_Q levels constrain every boundary DoF, their coarse correction would be that of
 * another problem); in 2D, cells whose restriction would need more than 32 launches (cells c, c + 4, ... of an
 * mgx_square share no DoF: 4 launches; any other cell order is coloured here).  A refused call leaves nothing behind. */
int mgx_dg_solver_create(mgx_context_t ctx, const mgx_dg_solver_desc *desc, mgx_dg_solver_t *solver);
int mgx_dg_solver_destroy(mgx_dg_solver_t solver);
int mgx_dg_solver_smoother_info(mgx_dg_solver_t solver, mgx_smoother_info *info);
/* MultigridSolverDG::vmult (:429-440): one DG V-cycle = smoother, residual restricted to FE_Q
 * (laplace_operator_dg.h:1798-1819), FE_Q V-cycle, correction embedded back (:1863-1894), smoother;
 * fp64 device vectors in the DG layout */
int mgx_dg_solver_vmult(mgx_dg_solver_t solver, double *dst, const double *src);
/* MultigridSolverDG::solve_cg(tolerance) (:410-424) on a given right-hand side: zero start, at
 * most 100 iterations; iterations = last_step, reduction_rate = (res/res0)^(1/its) */
int mgx_dg_solver_solve_cg(mgx_dg_solver_t solver, double tolerance, const double *rhs, double *solution,
                           unsigned *iterations, double *reduction_rate);
/* the two transfers of the DG level on their own (V-cycle number type): cg = P^T dg (cg is
 * zeroed first; constrained rows stay zero) and dg += P cg */
int mgx_dg_restrict_to_cg(mgx_dg_solver_t solver, void *cg_dst, const void *dg_src);
int mgx_dg_prolongate_add_cg_to_dg(mgx_dg_solver_t solver, void *dg_dst, const void *cg_src);
/* LaplaceOperatorCompactCombine::vmult_residual_and_restrict_to_cg (:852-861; action 1, epilogue :1798-1819) of the
 * solver's V-cycle operator: cg = P^T (rhs - A lhs), the residual changed to the FE_Q basis and added into the FE_Q
 * vector inside the cell kernel (cg zeroed first, summed over the rank interfaces of a decomposed mesh).  The V-cycle
 * runs this form unless the context option "dg_unmerged_restrict" is set. */
int mgx_dg_vmult_residual_and_restrict_to_cg(mgx_dg_solver_t solver, void *cg_dst, const void *rhs, const void *lhs);

/* ---- level transfer between two DG spaces: MGTransferMatrixFree<3,Number> on FE_DGQ* level vectors, as
 * MultigridSolverDGPlain uses it (common/multigrid_solver_dg_plain.h:150-159 build, :483 restrict_and_add, :489
 * prolongate_and_add).  Same degree and basis on both levels; every coarse cell has eight children. ---- */
typedef struct mgx_dg_transfer_s *mgx_dg_transfer_t;
typedef struct
{
  int      degree; /* 1 .. MGX_MAX_DEGREE */
  int      basis;  /* MGX_DG_* */
  int      number; /* MGX_F32 or MGX_F64: the type of the vectors */
  uint32_t n_coarse_cells;
  /* host [n_coarse_cells][8], copied: fine cell that is child kx + 2 ky + 4 kz of a coarse cell; every fine cell
   * 0 .. 8 n_coarse_cells - 1 exactly once (checked) */
  const uint32_t *children;
  /* 0 or 3: as above; 2: MGTransferMatrixFree<2,Number> -- children is [n_coarse_cells][4], child kx + 2 ky, every
   * fine cell 0 .. 4 n_coarse_cells - 1 exactly once (checked).  Any other value: MGX_ERR_INVALID_ARGUMENT. */
  int dim;
} mgx_dg_transfer_desc;
/* MGTransferMatrixFree::build: the 1D embedding of the parent's basis into the two children's, computed in double
 * from the operator's own 1D polynomials (the same matrix in two and three dimensions) */
int mgx_dg_transfer_create(mgx_context_t ctx, const mgx_dg_transfer_desc *desc, mgx_dg_transfer_t *transfer);
int mgx_dg_transfer_destroy(mgx_dg_transfer_t transfer);
/* MGTransferMatrixFree::prolongate_and_add: fine[children[c][k]] += (P_kz (x) P_ky (x) P_kx) coarse[c]; dim == 2:
 * (P_ky (x) P_kx), here and below */
int mgx_dg_transfer_prolongate_and_add(mgx_dg_transfer_t transfer, void *fine_dst, const void *coarse_src);
/* MGTransferMatrixFree::restrict_and_add: coarse[c] += sum_k (P_kz (x) P_ky (x) P_kx)^T fine[children[c][k]]; DG has
 * neither weights nor constrained rows.  Both operations give the same bits in every run. */
int mgx_dg_transfer_restrict_and_add(mgx_dg_transfer_t transfer, void *coarse_dst, const void *fine_src);
/* the 1D embedding for inspection (MGTransferMatrixFree's prolongation_matrix_1d, one half at a time):
 * p1d[h (p+1)^2 + i (p+1) + j] = coefficient i, in the child's basis on [0,1], of phi_j((x + h) / 2) */
int mgx_dg_transfer_matrix(mgx_dg_transfer_t transfer, double *p1d);

/* ---- level transfer between two DG spaces of different degree on the same mesh (p-coarsening; no counterpart in the
 * reference, whose plain DG multigrid coarsens the mesh only).  Same basis kind and the same cells in the same order on
 * both levels: cell c is the run of (pc+1)^dim entries in the coarse vector and of (pf+1)^dim in the fine one. ---- */

/* The 1D embedding of the space of degree coarse_degree into that of fine_degree, 1 <= coarse_degree < fine_degree <=
 * MGX_MAX_DEGREE, both in the basis MGX_DG_*: e1d[i (pc+1) + j] = coefficient i, in the basis of degree pf, of the function
 * j of the basis of degree pc on the same cell ((pf+1)(pc+1) doubles).  Host only, needs neither a context nor a device;
 * computed in double from the 1D polynomials of the operator (interpolation in the Gauss points of the fine space: the
 * spaces are nested, any unisolvent set of points gives the same matrix).  coarse_degree >= fine_degree or a null
 * pointer: MGX_ERR_INVALID_ARGUMENT; a degree outside 1 .. MGX_MAX_DEGREE or an unknown basis: MGX_ERR_UNSUPPORTED. */
int mgx_dg_degree_embedding(int fine_degree, int coarse_degree, int basis, double *e1d);

typedef struct mgx_dg_degree_transfer_s *mgx_dg_degree_transfer_t;
typedef struct
{
  int      fine_degree, coarse_degree; /* 1 <= coarse_degree < fine_degree <= MGX_MAX_DEGREE */
  int      basis;                      /* MGX_DG_* */
  int      number;                     /* MGX_F32 or MGX_F64: the type of the vectors */
  uint32_t n_cells;                    /* of either level, >= 1 */
  int      dim;                        /* 0 or 3: three dimensions, 2: two.  Any other value: MGX_ERR_INVALID_ARGUMENT. */
} mgx_dg_degree_transfer_desc;
/* uploads mgx_dg_degree_embedding in the number type; refuses what that function refuses, with its status */
int mgx_dg_degree_transfer_create(mgx_context_t ctx, const mgx_dg_degree_transfer_desc *desc, mgx_dg_degree_transfer_t *transfer);
int mgx_dg_degree_transfer_destroy(mgx_dg_degree_transfer_t transfer);
/* fine[c] += (E (x) E (x) E) coarse[c]; dim == 2: (E (x) E), here and below.  The vectors must not alias. */
int mgx_dg_degree_transfer_prolongate_and_add(mgx_dg_degree_transfer_t transfer, void *fine_dst, const void *coarse_src);
/* coarse[c] += (E (x) E (x) E)^T fine[c].  One writer per entry in both operations: the same bits in every run. */
int mgx_dg_degree_transfer_restrict_and_add(mgx_dg_degree_transfer_t transfer, void *coarse_dst, const void *fine_src);
/* the 1D embedding the object was created with, (pf+1)(pc+1) doubles as mgx_dg_degree_embedding gives them */
int mgx_dg_degree_transfer_matrix(mgx_dg_degree_transfer_t transfer, double *e1d);

/* ---- MultigridSolverDGPlain<3,p,Number,double> (common/multigrid_solver_dg_plain.h:55-595): the DG-SIP operator on
 * every level of a globally refined mesh, Chebyshev / JacobiTransformed smoothers, DG-to-DG transfers, level 0 solved
 * by its Chebyshev iteration; one rank ---- */
typedef struct mgx_dg_plain_solver_s *mgx_dg_plain_solver_t;
typedef struct
{
  int                      n_levels;
  const mgx_dg_operator_t *matrix;       /* [n_levels], V-cycle number type (:95-122) */
  mgx_dg_operator_t        matrix_dg_dp; /* fp64 twin of matrix[n_levels - 1] (:126-146) */
  const mgx_dg_transfer_t *transfer;     /* [n_levels - 1], transfer[l - 1] between levels l - 1 and l (:150-159) */
  int                      degree_pre;   /* Chebyshev degree of levels 0 < l < L; max(1, degree_pre - 1) on level L (:195-202) */
  /* optional [n_levels] (entries may be NULL), host [n_cells of the level]: as in mgx_dg_solver_desc */
  const uint32_t *const *cell_global_id;
} mgx_dg_plain_solver_desc;
/* ctor (:58-215): level vectors and smooth[level].initialize -- levels l > 0: range 20, 15 CG iterations; level 0:
 * range 1e-5, degree by Varga's rule, at most m() CG iterations (:204-209).  The dimension is that of the operators
 * (poisson_dg_plain/program.cc:65 runs dimension 2): all operators and transfers must share it, and a level has 2^dim
 * times the cells of the one below.  Operators with Neumann faces are accepted (every level should mark the same sides);
 * a level or matrix_dg_dp without any Dirichlet face is refused with MGX_ERR_UNSUPPORTED: the problem is singular. */
int mgx_dg_plain_solver_create(mgx_context_t ctx, const mgx_dg_plain_solver_desc *desc, mgx_dg_plain_solver_t *solver);
/* The same solver on a level sequence in which every step is either a mesh refinement (same degree, 2^dim times the
 * cells) or a degree raise (same cells, coarse degree < fine degree): h- and p-coarsening mixed at will.  The levels
 * below the finest are rediscretisations, each with the penalty (p+1)^2 of its own degree -- not Galerkin products. */
typedef struct
{
  int                      n_levels;
  const mgx_dg_operator_t *matrix;       /* [n_levels], V-cycle number type, coarsest first */
  mgx_dg_operator_t        matrix_dg_dp; /* fp64 twin of matrix[n_levels - 1] */
  /* [n_levels - 1] each (an array without any entry may be NULL); of transfer[l - 1] and degree_transfer[l - 1]
   * exactly one is non-NULL: the step from level l - 1 to level l is a mesh refinement or a degree raise */
  const mgx_dg_transfer_t        *transfer;
  const mgx_dg_degree_transfer_t *degree_transfer;
  int                             degree_pre; /* as in mgx_dg_plain_solver_desc, whatever the kind of step */
  const uint32_t *const          *cell_global_id; /* as in mgx_dg_plain_solver_desc */
} mgx_dg_hp_solver_desc;
/* Returns the handle type of mgx_dg_plain_solver_create: every entry point below works on it unchanged, and with
 * mesh refinements only the solver is the one mgx_dg_plain_solver_create builds.  Smoothers as there (levels 0 < l < L:
 * degree_pre; level L: max(1, degree_pre - 1); level 0: range 1e-5, Varga's rule).  Refused with
 * MGX_ERR_INVALID_ARGUMENT and a message that names the level: a step with both or neither transfer; operators that
 * differ in basis, number type, dimension or context, have ghost cells or no Dirichlet face; a mesh refinement with
 * unequal degrees, other than 2^dim times the cells, or a transfer of another degree or n_coarse_cells; a degree raise
 * with unequal cell counts, coarse degree >= fine degree, or a degree transfer whose degrees or n_cells are not those
 * of its two operators; a matrix_dg_dp that is not the fp64 twin of the last level. */
int mgx_dg_hp_solver_create(mgx_context_t ctx, const mgx_dg_hp_solver_desc *desc, mgx_dg_plain_solver_t *solver);
int mgx_dg_plain_solver_destroy(mgx_dg_plain_solver_t solver);
int mgx_dg_plain_solver_smoother_info(mgx_dg_plain_solver_t solver, int level, mgx_smoother_info *info);
/* MultigridSolverDGPlain::vmult (:322-334): one V-cycle (:456-496); fp64 device vectors of the finest level */
int mgx_dg_plain_solver_vmult(mgx_dg_plain_solver_t solver, double *dst, const double *src);
/* MultigridSolverDGPlain::solve_cg(tolerance) (:303-317) on a given right-hand side: zero start, at most 100
 * iterations; iterations = last_step, reduction_rate = (res/res0)^(1/its) */
int mgx_dg_plain_solver_solve_cg(mgx_dg_plain_solver_t solver, double tolerance, const double *rhs, double *solution,
                                 unsigned *iterations, double *reduction_rate);
/* MultigridSolverDGPlain::vmult_with_residual_update (:340-427): defect = residual + factor update; V-cycle -> mg;
 * residual += factor update; sums = {mg.residual, mg.(factor update)} (factor == 0: both mg.residual); update = mg.
 * The sums are added in a fixed order. */
int mgx_dg_plain_solver_vmult_with_residual_update(mgx_dg_plain_solver_t solver, double *residual, double *update,
                                                   double factor, double sums[2]);
/* wall time per level of the V-cycles since the last call (print_wall_times, :264-287), seconds, for diagnosis: the
 * stream is synchronised around every part while enabled.  times [n_levels][6]: level 0 {coarse solve, calls, 0...},
 * level l > 0 {mg_mv, restrict, prolongate, 0, 0, smoother} (the columns of `timings[level]`). */
int mgx_dg_plain_solver_enable_timings(mgx_dg_plain_solver_t solver, int on);
int mgx_dg_plain_solver_get_timings(mgx_dg_plain_solver_t solver, double *times);
/* do_matvec / do_matvec_smoother (:432-445): one product with the finest fp64 / V-cycle operator on the solver's
 * own vectors (timing aids) */
int mgx_dg_plain_solver_do_matvec(mgx_dg_plain_solver_t solver);
int mgx_dg_plain_solver_do_matvec_smoother(mgx_dg_plain_solver_t solver);

/* ---- conjugate gradients on the DG operator alone, preconditioned by the inverse lumped mass matrix: the solver of
 * solver_dg/program.cc (SolverCG with IterationNumberControl, :177-178; DiagonalMatrix of the lumped mass, :134-148),
 * in the program's two forms, "cell-based loops" (:222-241) and "interleaved loops" (:243-263); 3D and 2D, one rank ----
 *
 * MGX_DG_PCG_MERGED: the whole iteration stays on the device.  Per iteration three plain launches on the context's
 * stream -- the cell kernel (q = A p with the four block sums of mgx_dg_vmult_with_pcg_sums), one workgroup that adds
 * them and writes
 *   alpha = s1 / s0 ;  rho_next = s1 - 2 alpha s2 + alpha^2 s3 ;  beta = rho_next / s1 ;  rho[k] = s1, rho[k+1] = rho_next
 * and one pass  x += alpha p ; r -= alpha q ; p = m r + beta p  that loads alpha and beta from device memory.  If s0 or s1
 * is not a positive finite number or rho_next is not finite, alpha = beta = 0 and the iteration index k is recorded
 * once: x and r stay as they are from then on, the history stays flat, no NaN is produced.  If only rho_next fails,
 * finite but not positive -- the residual has reached rounding level, where the recurrence cancels -- the step is still
 * taken, beta = 0, rho[k+1] = 0 and k + 1 is recorded: the number of steps taken, either way.
 * MGX_DG_PCG_SEPARATE: the yardstick, textbook PCG from mgx_dg_vmult, separate dot-product and update kernels and
 * scalars on the host (two to three host round trips per iteration); same interface, history and stopping rule. */
#define MGX_DG_PCG_MERGED 0
#define MGX_DG_PCG_SEPARATE 1
typedef struct mgx_dg_pcg_solver_s *mgx_dg_pcg_solver_t;
typedef struct
{
  mgx_dg_operator_t matrix;         /* without ghost cells (else MGX_ERR_UNSUPPORTED); vectors are in its number type */
  int               form;           /* MGX_DG_PCG_* */
  unsigned          max_iterations; /* n_tests of IterationNumberControl (:177) */
  double            tolerance;      /* 0: run max_iterations (the reference's 1e-20); > 0: stop at sqrt(rho_k / rho_0) <= tolerance */
  unsigned          check_every;    /* >= 1: with a tolerance, the host looks at the history every so many iterations */
} mgx_dg_pcg_solver_desc;
/* solver_dg/program.cc:134-148, 177-178: owns r, p, q, the block sums, the scalars and the history.  Refused with
 * MGX_ERR_UNSUPPORTED (and a reason) if an entry of the preconditioner table is not positive and finite, or if the
 * operator has no Dirichlet face at all (Neumann faces only: the problem is singular). */
int mgx_dg_pcg_solver_create(mgx_context_t ctx, const mgx_dg_pcg_solver_desc *desc, mgx_dg_pcg_solver_t *solver);
int mgx_dg_pcg_solver_destroy(mgx_dg_pcg_solver_t solver);
/* solver.solve(laplace_operator, output, input, diagonal) (solver_dg/program.cc:222-263): zero start, `solution` is
 * overwritten (:225 output = 0) and must not alias rhs; device vectors of mgx_dg_operator_n_dofs entries.  The operator
 * and the update are applied k times each, so x_k and r_k are formed.  With a tolerance the solve stops at the first
 * checked k (multiples of check_every, and max_iterations) with sqrt(rho_k / rho_0) <= tolerance.  iterations = that k,
 * max_iterations if the tolerance was not met, or the iteration of the breakdown if one came first;
 * reduction_rate = sqrt(rho_k / rho_0)^(1/k).  max_iterations == 0 or rhs == 0: x = 0, 0 iterations, rate 0.
 * iterations and reduction_rate may be NULL. */
int mgx_dg_pcg_solver_solve(mgx_dg_pcg_solver_t solver, const void *rhs, void *solution, unsigned *iterations,
                            double *reduction_rate);
/* the history rho_k = r_k . M^-1 r_k of the last solve (solver_dg/program.cc:134-148 the preconditioner, :222-263 the
 * loops): rho[0] at the start, rho[k] after iteration k, for every iteration that ran; *count = their number (at most
 * max_iterations + 1).  rho may be NULL to ask for the count only. */
int mgx_dg_pcg_solver_history(mgx_dg_pcg_solver_t solver, double *rho, unsigned *count);

/* ---- mesh helpers (stand in for GridGenerator + DoFHandler of the harness) ---- */

/* matvec_dg_cheby/program.cc:55-77: cells per direction and the cell Jacobian of the sheared box
 * after n_cell_steps refinement steps */
int mgx_dg_cheby_mesh(int n_cell_steps, int cells[3], double jacobian[9]);

/* neighbour table of a box of cells[0] x cells[1] x cells[2] cells, all outer faces Dirichlet.
 * ordering 0: lexicographic, x fastest; 1: z-order (space-filling curve, as p4est gives the
 * reference).  cell_ijk (optional) receives the (i, j, k) position of every cell. */
int mgx_dg_box_neighbours(const int cells[3], int ordering, int32_t *neighbours, int32_t *cell_ijk);

/* child table between a box of coarse_cells and its global refinement (2 coarse_cells per direction), the cells of
 * either numbered as mgx_dg_box_neighbours numbers them in the given ordering (Triangulation::refine_global):
 * children[c * 8 + kx + 2 ky + 4 kz] = fine cell at position 2 ijk(c) + (kx, ky, kz) */
int mgx_dg_box_children(const int coarse_cells[3], int coarse_ordering, int fine_ordering, uint32_t *children);

/* the same two tables for a box of cells[0] x cells[1] quadrilaterals: neighbours [n][4] (face 2d+s, d = 0, 1),
 * cell_ij [n][2] (optional); ordering 0: lexicographic, 1: z-order over the two coordinates;
 * children[c * 4 + kx + 2 ky] = fine cell at position 2 ij(c) + (kx, ky) */
int mgx_dg_box_neighbours_2d(const int cells[2], int ordering, int32_t *neighbours, int32_t *cell_ij);
int mgx_dg_box_children_2d(const int coarse_cells[2], int coarse_ordering, int fine_ordering, uint32_t *children);

/* marks whole sides of a box in a table made by mgx_dg_box_neighbours[_2d] (dim 3 / 2): every boundary entry of face
 * 2d+s becomes side_kind[2d+s], MGX_DG_BOUNDARY or MGX_DG_NEUMANN.  cells: the box, [dim]; cell_pos: [n_cells][dim], the
 * positions the table was made with (the owned cells of a rank with their positions in the whole box will do: entries
 * of rank faces are cells).  The table is checked against the positions first and left alone if it does not fit. */
int mgx_dg_box_set_sides(int dim, const int *cells, uint32_t n_cells, const int32_t *cell_pos, const int *side_kind, int32_t *neighbours);

#ifdef __cplusplus
}
#endif
#endif
