/*
 * mgx_square.h -- host-side discretisation provider for poisson_cube with dimension = 2: what deal.II's
 * Triangulation<2> / DoFHandler<2> / MatrixFree<2> / FE_Q<2> would hand to LaplaceOperator<2,p,number> and
 * MultigridSolver<2,p,...>.  The two-dimensional counterpart of mgx_cube.h, one rank only; it feeds the descriptors
 * of mgx.h with dim = 2.
 *
 *   mesh            a box of roots[0] x roots[1] square coarse cells of size h0 from (origin, origin), refined
 *                   n_refine times: level l has roots[d] 2^l cells per direction
 *   cell order      coarse cells lexicographic (x fastest), Morton order inside a coarse cell: the children of cell
 *                   c are 4c .. 4c+3 with child = x + 2y
 *   DoF numbering   first touch, entity by entity in cell order (contiguous per entity, x fastest inside the quad
 *                   interior: the contract of the 9-entry compressed index table), Dirichlet DoFs last
 *   problem         u = sin(3 pi x) sin(3 pi y), f = 2 (3 pi)^2 u, coefficient 1, Dirichlet values on all four sides
 *                   (poisson_cube/program.cc with dimension = 2)
 *   jacobian        optional constant 2 x 2 matrix A of an affine map x = (origin, origin) + A X of the whole box
 *                   (sheared or anisotropic box): the cells of level l have the Jacobian h_l A, the operator the one
 *                   tensor det(A) (A^T A)^-1 = [xx, yy, xy] per mesh -- the full-tensor form when xy != 0 -- and u, f
 *                   are those of the physical coordinates
 */
#ifndef MGX_SQUARE_H
#define MGX_SQUARE_H

#include "mgx.h"
#include "mgx_cube.h" /* mgx_cube_solver: the hierarchy objects of a solver */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgx_square_s *mgx_square_t;

typedef struct
{
  int           degree, n_refine;
  int           roots[2];
  double        origin, h0;
  const double *jacobian; /* 2 x 2 row-major, NULL: identity */
} mgx_square_box_desc;

/* the square [-0.9, 1]^2 of poisson_cube with n_subdiv coarse cells per direction */
int mgx_square_create(int degree, int n_subdiv, int n_refine, mgx_square_t *square);
int mgx_square_create_box(const mgx_square_box_desc *desc, mgx_square_t *square);
/* A mesh with curved cells (what a Triangulation<2> with a PolarManifold and MappingQ(p) hands to MatrixFree<2>): the
 * box of desc, normalised to the unit square (X, Y), is mapped to the quarter annulus r = 0.5 + 0.5 X, theta = (pi/2) Y,
 * (x, y) = r (cos theta, sin theta).  Every cell of every level places its (p+1)^2 Gauss-Lobatto nodes by the exact
 * map -- the isoparametric degree p, the rule of the 3D shell sector.  desc->jacobian must be NULL and desc->origin is
 * not read.  mgx_square_operator_desc hands out the per-point unit-law tensor (mgx_square_unit_q) as coef_q.  The
 * Poisson problem of the box does not exist here: mgx_square_rhs, mgx_square_bc_index / _value and
 * mgx_square_solver_create are refused (NULL / MGX_ERR_UNSUPPORTED), mgx_square_bc_count is 0, mgx_square_l2_error is
 * NaN; the hierarchy is that of mgx_square_solver_create_general.  A linear problem on such a square is stated through
 * mgx_square_problem (below) and solved by mgx_square_solver_create_problem. */
#define MGX_SQUARE_GEOMETRY_ANNULUS_SECTOR 1
int mgx_square_create_mapped(const mgx_square_box_desc *desc, int geometry, mgx_square_t *square);
/* The unit disc of minimal_surface/program.cc (GridGenerator::hyper_ball in two dimensions, centre 0, radius 1, a
 * SphericalManifold on the boundary, MappingQGeneric(p)): five coarse cells -- a centre square with the corners
 * (+-i, +-i), i = 1 - 1/sqrt 2, and four blocks between it and the circle, whose corners there are (+-o, +-o),
 * o = 1/sqrt 2 -- refined n_refine times; level l has 5 4^l cells, block b holds the cells b 4^l ..., Morton order
 * inside a block (children of c: 4c .. 4c+3).  Three cells meet at the four corners of the centre square on every
 * level.  New vertices: the midpoint of an edge (on the circle: of the arc), the transfinite centre of a cell; cell nodes:
 * linear on straight edges, by angle on the arcs of the boundary, transfinite inside.  Everything of a mapped square
 * holds (per-point unit-law tensor as coef_q, no Poisson problem, mgx_square_solver_create_general), and further:
 * mgx_square_weight_shift is NULL (mgx_transfer_create derives owner weights); there is no lattice of cells and no grid
 * of DoFs -- mgx_square_cells_per_dim2 gives zeros, mgx_square_cell_coords and mgx_square_dof_grid NULL, with the reason
 * in mgx_last_error(), mgx_square_cell_size is 0 -- and mgx_square_seeded_vector keys its generator by the DoF index. */
#define MGX_SQUARE_GEOMETRY_BALL 2
int mgx_square_create_ball(int degree, int n_refine, mgx_square_t *square);
int mgx_square_destroy(mgx_square_t square);

int      mgx_square_n_levels(mgx_square_t square);
int      mgx_square_degree(mgx_square_t square);
uint32_t mgx_square_n_cells(mgx_square_t square, int level);
uint32_t mgx_square_n_dofs(mgx_square_t square, int level);
uint32_t mgx_square_n_constrained(mgx_square_t square, int level);
void     mgx_square_cells_per_dim2(mgx_square_t square, int level, uint32_t cells[2]);
double   mgx_square_cell_size(mgx_square_t square, int level);

/* tables (host memory owned by the square) */
const uint32_t *mgx_square_idx9(mgx_square_t square, int level);       /* [n_cells][9], constrained entities invalid */
const uint32_t *mgx_square_idx9_plain(mgx_square_t square, int level); /* [n_cells][9] */
const uint32_t *mgx_square_constrained(mgx_square_t square, int level);
const uint32_t *mgx_square_children(mgx_square_t square, int level);     /* level >= 1: [n_cells(level-1)][4] */
const uint8_t  *mgx_square_weight_shift(mgx_square_t square, int level); /* level >= 1: [n_cells(level-1)][9]; the disc: NULL */
const uint32_t *mgx_square_cell_coords(mgx_square_t square, int level);  /* [n_cells][2] */
/* dof -> lexicographic grid id gy Gx + gx, G_d = N_d p + 1 */
const uint32_t *mgx_square_dof_grid(mgx_square_t square, int level);
const double   *mgx_square_shape_values(mgx_square_t square);
const double   *mgx_square_colloc_grad(mgx_square_t square);
const double   *mgx_square_qweights(mgx_square_t square);
const double   *mgx_square_qpoints(mgx_square_t square);
const double   *mgx_square_gll(mgx_square_t square);
const double   *mgx_square_prolong_1d(mgx_square_t square);

/* rhs = int f phi - int grad u_bc . K grad phi, assembled on the host at the first call; boundary values */
const double   *mgx_square_rhs(mgx_square_t square, int level);
uint32_t        mgx_square_bc_count(mgx_square_t square, int level);
const uint32_t *mgx_square_bc_index(mgx_square_t square, int level);
const double   *mgx_square_bc_value(mgx_square_t square, int level);
/* L2 error of a host copy of solution[level] (boundary values inserted), with the Gauss rule of the operator */
double mgx_square_l2_error(mgx_square_t square, int level, const double *solution_host);
/* the generator of mgx_cube_seeded_vector, keyed by the grid id */
int mgx_square_seeded_vector(mgx_square_t square, int level, uint64_t seed, double *out_host);

/* fills desc for LaplaceOperator<2,p,number> on `level` (dim = 2; pointers stay owned by the square) */
int mgx_square_operator_desc(mgx_square_t square, int level, int number, mgx_operator_desc *desc);
/* the per-(cell, q) tensor equivalent to the descriptor's coef: out[n_cells][3][(p+1)^2] = coef[c] w_qx w_qy */
int mgx_square_coef_q(mgx_square_t square, int level, double *out);
/* everything MultigridSolver's constructor builds, on the device (mgx_cube_solver_create in two dimensions);
 * per_point != 0: the level operators in the per-(cell, q) form with mgx_square_coef_q.  Released with
 * mgx_cube_solver_destroy. */
int mgx_square_solver_create(mgx_context_t ctx, mgx_square_t square, int vcycle_number, int degree_pre, int n_cycles,
                             int per_point, mgx_cube_solver *out);

/* ---- geometry for the solution-dependent coefficients (minimal_surface/program.cc with dimension = 2) ---- */
/* affine cells of level `level` of a box: metric = J^-1 J^-T as [xx, yy, xy] and det J with J = h_level A (A the
 * box's jacobian) -- the arguments of mgx_operator_enable_coefficient_update_2d.  Refused on a mapped square. */
int mgx_square_affine_metric(mgx_square_t square, int level, double metric[3], double *det_jacobian);
/* out[n_dofs][2]: physical coordinates of the Gauss-Lobatto node of every DoF (where the boundary function of
 * LaplaceProblem<2>::interpolate_boundary_values is evaluated) */
int mgx_square_dof_coordinates(mgx_square_t square, int level, double *out);
/* out[n_cells][(p+1)^2][2]: the nodes of every cell, x fastest */
int mgx_square_cell_nodes(mgx_square_t square, int level, double *out);
/* the per-point geometry from the cell nodes (isoparametric): out[n_cells][3][(p+1)^2] = JxW_q J^-1 J^-T as
 * [xx, yy, xy] and out[n_cells][(p+1)^2] = JxW_q -- the arguments of mgx_operator_enable_coefficient_update_q_2d.  On a
 * box they equal the affine geometry up to rounding. */
int mgx_square_unit_q(mgx_square_t square, int level, double *out);
int mgx_square_jxw_q(mgx_square_t square, int level, double *out);
/* mgx_cube_solver_create_general in two dimensions: the hierarchy of LaplaceProblem<2>::solve for a solution-dependent
 * coefficient (minimal_surface/program.cc:425-488).  Operators in the per-point form with coef_q_per_level[l]
 * ([n_cells][3][(p+1)^2]; NULL or a NULL entry: the unit-law tensor), zero right-hand sides, homogeneous boundary
 * values, every level enabled (a box: mgx_operator_enable_coefficient_update_2d on the operators of both precisions; a
 * mapped square: mgx_operator_enable_coefficient_update_q_2d on the fp64 operators, an fp32 V-cycle operator receives the
 * rounded fp64 tensor).  One rank.  Released with mgx_cube_solver_destroy. */
int mgx_square_solver_create_general(mgx_context_t ctx, mgx_square_t square, int vcycle_number, int degree_pre, int n_cycles,
                                     const double *const *coef_q_per_level, mgx_cube_solver *out);

/* ---- a linear problem -div(a grad u) = f with Dirichlet values on every square: box, sheared box, annulus sector, disc ---- */
#define MGX_SQUARE_PROBLEM_CUBE  0  /* u = sin(3 pi x) sin(3 pi y), a = 1: the box's own problem */
#define MGX_SQUARE_PROBLEM_SHELL 1  /* u = sin(2 pi (x+y)), a = 1 + contrast prod_{e<2} cos^2(2 pi x_e + 0.1 e),
                                       f = -(a lap u + grad a . grad u): poisson_shell/program.cc:97-225, dim = 2 */
typedef struct
{
  int    kind;
  double contrast; /* the program's 1e6; read by MGX_SQUARE_PROBLEM_SHELL only: finite, >= 0 */
} mgx_square_problem;
/* The geometry of a problem, on every square: a cell is the isoparametric interpolant (degree p) of its nodes
 * (mgx_square_cell_nodes); the quadrature points x_q are that interpolant at the Gauss points, and unit_q / JxW_q
 * (mgx_square_unit_q, mgx_square_jxw_q) come from its Jacobian.  On a box this is the affine geometry up to rounding.
 *   coef_q          out[n_cells][3][(p+1)^2] = a(x_q) unit_q (unit_q: mgx_square_coef_q, the operator's own tensor)
 *   rhs_quadrature  out[n_cells][(p+1)^2]    = f(x_q) JxW_q, the rhs_q of mgx_compute_residual_2d
 *   solution_q      out[n_cells][(p+1)^2]    = u(x_q), the u_q of mgx_compute_l2_error_2d
 *   bc_value        out[n_constrained]       = u at the node of every constrained DoF, in the order of mgx_square_constrained
 * A NULL problem, an unknown kind or a bad contrast: MGX_ERR_INVALID_ARGUMENT. */
int mgx_square_problem_coef_q(mgx_square_t square, int level, const mgx_square_problem *problem, double *out);
int mgx_square_problem_rhs_quadrature(mgx_square_t square, int level, const mgx_square_problem *problem, double *out);
int mgx_square_problem_solution_q(mgx_square_t square, int level, const mgx_square_problem *problem, double *out);
int mgx_square_problem_bc_value(mgx_square_t square, int level, const mgx_square_problem *problem, double *out);
/* MultigridSolver<2,p,...> for the problem: the level operators in the per-point form with mgx_square_problem_coef_q (an
 * fp32 V-cycle operator receives it rounded), the boundary values of the problem, and every level's right-hand side
 * assembled on the device (mgx_solver_desc::rhs NULL, then mgx_solver_compute_rhs_2d with mgx_square_problem_rhs_quadrature).
 * One rank.  Released with mgx_cube_solver_destroy.  mgx_square_solver_create, mgx_square_rhs, mgx_square_bc_* and
 * mgx_square_l2_error are what they were: the box's host-assembled problem, refused on a mapped square.  (deal.II's
 * two-dimensional hyper_shell, the closed ring, is not built: the curved meshes are the annulus sector and the disc.) */
int mgx_square_solver_create_problem(mgx_context_t ctx, mgx_square_t square, int vcycle_number, int degree_pre, int n_cycles,
                                     const mgx_square_problem *problem, mgx_cube_solver *out);

#ifdef __cplusplus
}
#endif
#endif
