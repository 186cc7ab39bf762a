// mgx_dg_host.hpp -- host numerics of the DG (symmetric interior penalty) operator, in fp64 and without the device:
// the 1D data of an element basis (quadrature, shape values, the generalised eigenproblem of the block-Jacobi
// preconditioner, the embedding into the two halves of a cell), the geometry factors of an affine cell and the
// transformed diagonal.  Implemented in mgx_dg_host.cpp; read by mgx_dg_api.cpp (set-up of the objects) and
// mgx_dg_kernels.hip (which turns them into the constant block of the cell kernel).
#pragma once

#include "../../include/mgx_dg.h"

#include <string>
#include <vector>

namespace mgx::dg
{
  constexpr int kMaxN = MGX_MAX_DEGREE + 1;

  // eigenvalues (ascending) and eigenvectors (columns of V) of a symmetric matrix, cyclic Jacobi
  void sym_eig(int n, std::vector<double> A, std::vector<double> &lambda, std::vector<double> &V);

  struct Host1D
  {
    int                 n = 0;
    std::vector<double> xq, wq, S, SD, D, E, lambda;
    bool                e_parity = false; // eigenvectors sorted even first / odd behind (see build_1d)
    double              b[2][kMaxN], g[2][kMaxN], fb[2][kMaxN], fg[2][kMaxN];
    double              hderiv = 0;
    std::vector<double> P1; // [i*n+q]: values in the Gauss-Lobatto nodes -> coefficients of the element basis
    // [h*n*n + i*n+j], h = 0, 1: coefficient i, in this basis on [0,1], of phi_j((x + h) / 2) -- the embedding of a
    // cell's space into the spaces of its two halves (level transfer between DG spaces)
    std::vector<double> embed;
    // eigenfunctions: Laplace form, first-derivative form, values and derivatives at the two ends
    std::vector<double> lt, ct, beta[2], gamma[2];
  };

  // 1D data of degree p in the basis MGX_DG_*; a status of include/mgx.h, with the reason in `why` on failure
  int build_1d(int p, int basis, Host1D &h, std::string &why);

  // K = det J * J^-1 J^-T (dim 3: xx yy zz xy xz yz; dim 2: xx yy xy), cn[d][a] = n_d . grad xi_a with n_d the unit
  // normal towards +xi_d, fw[d] the face JxW without the quadrature weight, sigma[d] the penalty; entries of
  // directions >= dim are zero
  struct Geometry
  {
    double K[6], cn[3][3], fw[3], sigma[3];
    int    dim = 3;
  };

  int build_geometry(const double J[9], int p, Geometry &g, std::string &why);
  // the same for a cell of two dimensions, J row-major 2 x 2 (laplace_operator_dg.h:749-771 with dim == 2); refused
  // unless every entry is finite and the determinant positive
  int build_geometry_2d(const double J[4], int p, Geometry &g, std::string &why);

  // what lies behind a face of a cell, from its neighbour entry: a cell (owned or ghost), a homogeneous Dirichlet
  // face (MGX_DG_BOUNDARY) or a Neumann face (MGX_DG_NEUMANN), which contributes nothing to the bilinear form
  enum FaceKind
  {
    kInterior  = 0,
    kDirichlet = 1,
    kNeumann   = 2
  };
  constexpr int kind_of_entry(int32_t entry) { return entry >= 0 ? kInterior : (entry == MGX_DG_NEUMANN ? kNeumann : kDirichlet); }

  // diagonal of T^T A_KK T for one combination of face kinds (kind[f], a FaceKind, of the 2 dim faces): Kronecker
  // products of 1D forms in the eigenvector basis, in which the mass matrix is the identity.  An interior face gives
  // half of what a Dirichlet face gives, a Neumann face nothing.
  // g.dim == 2: (p+1)^2 entries (JacobiTransformed, laplace_operator_dg.h:2162)
  void transformed_diagonal(const Host1D &h, const Geometry &g, const int *kind, std::vector<double> &diag);
} // namespace mgx::dg
