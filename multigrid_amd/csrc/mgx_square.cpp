// mgx_square.cpp -- host-side structured discretisation on quadrilaterals (see include/mgx_square.h): the
// two-dimensional counterpart of mgx_cube.cpp, one rank.  Pure host code; the device work is behind mgx.h.  The 1D
// element data (Gauss-Lobatto nodes, Gauss rule, shape values, collocation derivative, embedding) are those of
// mgx_cube.cpp (mgx_element.hpp).
#include "../../include/mgx_square.h"
#include "mgx_element.hpp"
#include "mgx_hierarchy.hpp"
#include "mgx_index_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace
{
  constexpr double kPi = 3.14159265358979323846264338327950288;

  struct Level
  {
    uint32_t              N[2] = {0, 0}; // cells per direction
    uint32_t              n_cells = 0, n_dofs = 0;
    double                h = 0;
    std::vector<uint32_t> idx9, idx9_plain, constrained, children, coords, dof_grid;
    std::vector<uint8_t>  weight_shift;
    std::vector<double>   bc_value, rhs;
    std::vector<double>   unit_q, jxw_q; // mapped square: [n_cells][3][n^2], [n_cells][n^2]
    // the disc: the vertices v00, v10, v01, v11 of every cell, the positions of the vertices, which lie on the circle
    std::vector<uint32_t> cell_vertices;
    std::vector<double>   vertex_xy;
    std::vector<uint8_t>  on_circle;
  };
} // namespace

struct mgx_square_s
{
  int                p = 0, roots[2] = {1, 1};
  double             origin = -0.9, h0 = 1.9;
  double             A[4] = {1, 0, 0, 1}, detA = 1, coef[3] = {1, 1, 0};
  int                geometry = 0; // 0: the box; MGX_SQUARE_GEOMETRY_ANNULUS_SECTOR, MGX_SQUARE_GEOMETRY_BALL
  mgx::Basis         basis;
  std::vector<Level> levels;

  void   map(double X, double Y, double &x, double &y) const
  {
    x = origin + A[0] * X + A[1] * Y;
    y = origin + A[2] * X + A[3] * Y;
  }
  // physical position of the point (X, Y) of the box (coordinates from its lower corner)
  void   point(double X, double Y, double &x, double &y) const
  {
    if (geometry == 0)
      return map(X, Y, x, y);
    const double r = 0.5 + 0.5 * X / (roots[0] * h0), theta = 0.5 * 3.14159265358979323846264338327950288 * Y / (roots[1] * h0);
    x = r * std::cos(theta);
    y = r * std::sin(theta);
  }
  static double u(double x, double y) { return std::sin(3 * kPi * x) * std::sin(3 * kPi * y); }
  static double f(double x, double y) { return 2 * (3 * kPi) * (3 * kPi) * u(x, y); }
};

namespace
{
  using mgx::entity_size; // (of the 9 entities of a cell, e = cy 3 + cx)
  inline uint32_t compact_bits(uint32_t m) // the even bits of m
  {
    uint32_t r = 0;
    for (int b = 0; b < 16; ++b)
      r |= ((m >> (2 * b)) & 1u) << b;
    return r;
  }

  void build_level(const mgx_square_s &Q, Level &L, int level)
  {
    const int p = Q.p;
    L.N[0]      = (uint32_t)Q.roots[0] << level;
    L.N[1]      = (uint32_t)Q.roots[1] << level;
    L.n_cells   = L.N[0] * L.N[1];
    L.h         = Q.h0 / (double)(1u << level);
    L.coords.resize(2 * (size_t)L.n_cells);
    const uint32_t per_root = 1u << (2 * level);
    for (uint32_t c = 0; c < L.n_cells; ++c)
      {
        const uint32_t root = c >> (2 * level), m = c & (per_root - 1);
        L.coords[2 * (size_t)c]     = ((root % (uint32_t)Q.roots[0]) << level) | compact_bits(m);
        L.coords[2 * (size_t)c + 1] = ((root / (uint32_t)Q.roots[0]) << level) | compact_bits(m >> 1);
      }
    // entities on the lattice (2 Nx + 1) x (2 Ny + 1): key (2 cx + ex, 2 cy + ey); first touch in cell order, the
    // entities on the boundary (all four sides Dirichlet) after all others
    const uint32_t        Ex = 2 * L.N[0] + 1, Ey = 2 * L.N[1] + 1;
    std::vector<uint32_t> base((size_t)Ex * Ey, MGX_INVALID_INDEX);
    auto key = [&](uint32_t c, int e) { return (size_t)(2 * L.coords[2 * (size_t)c + 1] + e / 3) * Ex + 2 * L.coords[2 * (size_t)c] + e % 3; };
    auto on_boundary = [&](size_t k) { return k % Ex == 0 || k % Ex == Ex - 1 || k / Ex == 0 || k / Ex == Ey - 1; };
    uint32_t counter = 0;
    for (int pass = 0; pass < 2; ++pass)
      {
        for (uint32_t c = 0; c < L.n_cells; ++c)
          for (int e = 0; e < 9; ++e)
            {
              const size_t k = key(c, e);
              if (base[k] != MGX_INVALID_INDEX || on_boundary(k) != (pass == 1))
                continue;
              base[k] = counter;
              if (pass == 1)
                for (int d = 0; d < entity_size(e, p); ++d)
                  L.constrained.push_back(counter + (uint32_t)d);
              counter += (uint32_t)entity_size(e, p);
            }
      }
    L.n_dofs = counter;
    L.idx9.resize(9 * (size_t)L.n_cells);
    L.idx9_plain.resize(9 * (size_t)L.n_cells);
    for (uint32_t c = 0; c < L.n_cells; ++c)
      for (int e = 0; e < 9; ++e)
        {
          const size_t k                  = key(c, e);
          L.idx9_plain[9 * (size_t)c + e] = base[k];
          L.idx9[9 * (size_t)c + e]       = on_boundary(k) ? MGX_INVALID_INDEX : base[k];
        }
    const uint32_t Gx = L.N[0] * (uint32_t)p + 1;
    L.dof_grid.resize(L.n_dofs);
    for (uint32_t c = 0; c < L.n_cells; ++c)
      for (int j = 0; j <= p; ++j)
        for (int i = 0; i <= p; ++i)
          L.dof_grid[mgx::cell_dof(&L.idx9_plain[9 * (size_t)c], 2, p, i, j)] =
            (L.coords[2 * (size_t)c + 1] * (uint32_t)p + (uint32_t)j) * Gx + L.coords[2 * (size_t)c] * (uint32_t)p + (uint32_t)i;
    // boundary values at the nodes (the Poisson problem of the box; a mapped square has none)
    L.bc_value.resize(Q.geometry == 0 ? L.constrained.size() : 0);
    for (size_t i = 0; i < L.bc_value.size(); ++i)
      {
        const uint32_t g  = L.dof_grid[L.constrained[i]], gx = g % Gx, gy = g / Gx;
        const uint32_t cx = std::min(gx / (uint32_t)p, L.N[0] - 1), cy = std::min(gy / (uint32_t)p, L.N[1] - 1);
        double         x, y;
        Q.map(L.h * (cx + Q.basis.gll[gx - cx * p]), L.h * (cy + Q.basis.gll[gy - cy * p]), x, y);
        L.bc_value[i] = mgx_square_s::u(x, y);
      }
    if (level > 0)
      {
        // the children of cell c are 4c .. 4c+3 (Morton order); multiplicity of the patch entities: a patch side is
        // shared with the neighbouring parent if there is one
        const uint32_t npar = L.n_cells / 4, Nx = L.N[0] / 2, Ny = L.N[1] / 2;
        L.children.resize(4 * (size_t)npar);
        L.weight_shift.resize(9 * (size_t)npar);
        for (uint32_t pc = 0; pc < npar; ++pc)
          {
            for (int ch = 0; ch < 4; ++ch)
              L.children[4 * (size_t)pc + ch] = 4 * pc + (uint32_t)ch;
            const uint32_t px = L.coords[2 * (size_t)(4 * pc)] / 2, py = L.coords[2 * (size_t)(4 * pc) + 1] / 2;
            for (int e = 0; e < 9; ++e)
              {
                const int ca = e % 3, cb = e / 3;
                const int sx = (ca == 0 && px > 0) || (ca == 2 && px + 1 < Nx), sy = (cb == 0 && py > 0) || (cb == 2 && py + 1 < Ny);
                L.weight_shift[9 * (size_t)pc + e] = (uint8_t)(sx + sy);
              }
          }
      }
  }

  // the cell matrix of the operator (the same on every cell and level: det(J) J^-1 J^-T does not depend on h in two
  // dimensions): K[a][b] = sum_q w_q grad phi_a . C grad phi_b, a = j n + i
  std::vector<double> cell_matrix(const mgx_square_s &Q)
  {
    const int           p = Q.p, n = p + 1, n2 = n * n;
    std::vector<double> G((size_t)n * n), gx((size_t)n2 * n2), gy((size_t)n2 * n2), K((size_t)n2 * n2, 0.);
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i)
        {
          double g = 0;
          for (int r = 0; r < n; ++r)
            g += Q.basis.D[q * n + r] * Q.basis.S[r * n + i];
          G[q * n + i] = g;
        }
    for (int qy = 0; qy < n; ++qy)
      for (int qx = 0; qx < n; ++qx)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i)
            {
              gx[(size_t)(qy * n + qx) * n2 + j * n + i] = G[qx * n + i] * Q.basis.S[qy * n + j];
              gy[(size_t)(qy * n + qx) * n2 + j * n + i] = Q.basis.S[qx * n + i] * G[qy * n + j];
            }
    for (int q = 0; q < n2; ++q)
      {
        const double w = Q.basis.gw[q % n] * Q.basis.gw[q / n], t0 = Q.coef[0] * w, t1 = Q.coef[1] * w, t2 = Q.coef[2] * w;
        const double *dx = &gx[(size_t)q * n2], *dy = &gy[(size_t)q * n2];
        for (int a = 0; a < n2; ++a)
          {
            const double fa = t0 * dx[a] + t2 * dy[a], fb = t2 * dx[a] + t1 * dy[a];
            for (int b = 0; b < n2; ++b)
              K[(size_t)a * n2 + b] += fa * dx[b] + fb * dy[b];
          }
      }
    return K;
  }

  // rhs = int f phi - int grad u_bc . C grad phi (multigrid_solver.h:225-261), rows of constrained DoFs zero
  void build_rhs(const mgx_square_s &Q, Level &L)
  {
    const int                 p = Q.p, n = p + 1, n2 = n * n;
    const std::vector<double> K = cell_matrix(Q);
    std::vector<double>       ubc(L.n_dofs, 0.), ul(n2), F(n2);
    for (size_t i = 0; i < L.constrained.size(); ++i)
      ubc[L.constrained[i]] = L.bc_value[i];
    L.rhs.assign(L.n_dofs, 0.);
    const double jxw = L.h * L.h * Q.detA;
    for (uint32_t c = 0; c < L.n_cells; ++c)
      {
        const uint32_t *ixp = &L.idx9_plain[9 * (size_t)c], *ix = &L.idx9[9 * (size_t)c];
        std::fill(F.begin(), F.end(), 0.);
        for (int qy = 0; qy < n; ++qy)
          for (int qx = 0; qx < n; ++qx)
            {
              double x, y;
              Q.map(L.h * (L.coords[2 * (size_t)c] + Q.basis.gq[qx]), L.h * (L.coords[2 * (size_t)c + 1] + Q.basis.gq[qy]), x, y);
              const double fq = mgx_square_s::f(x, y) * Q.basis.gw[qx] * Q.basis.gw[qy] * jxw;
              for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i)
                  F[j * n + i] += fq * Q.basis.S[qx * n + i] * Q.basis.S[qy * n + j];
            }
        bool any = false;
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i)
            {
              ul[j * n + i] = ubc[mgx::cell_dof(ixp, 2, p, i, j)];
              any           = any || ul[j * n + i] != 0.;
            }
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i)
            {
              const uint32_t d = mgx::cell_dof(ix, 2, p, i, j);
              if (d == MGX_INVALID_INDEX)
                continue;
              double v = F[j * n + i];
              if (any)
                for (int b = 0; b < n2; ++b)
                  v -= K[(size_t)(j * n + i) * n2 + b] * ul[b];
              L.rhs[d] += v;
            }
      }
  }

  // ---- the disc (MGX_SQUARE_GEOMETRY_BALL): five blocks, no lattice ----
  // Coarse mesh: the vertices C(s, t) = (s i, t i) and O(s, t) = (s o, t o), o = 1 / sqrt 2, i = 1 - o, numbered
  // C(-1,-1), C(1,-1), C(-1,1), C(1,1), then O likewise; the blocks centre, right, top, left, bottom with right-handed
  // frames in which every shared edge runs the same way in both of its cells (the index table knows no edge flip).
  void ball_coarse_level(Level &L)
  {
    const double o = std::sqrt(0.5), i = 1. - o;
    for (int k = 0; k < 8; ++k)
      {
        const double r = k < 4 ? i : o;
        L.vertex_xy.push_back((k & 1) ? r : -r);
        L.vertex_xy.push_back((k & 2) ? r : -r);
        L.on_circle.push_back(k >= 4);
      }
    static const uint32_t blocks[5][4] = {{0, 1, 2, 3}, {1, 5, 3, 7}, {2, 3, 6, 7}, {0, 2, 4, 6}, {0, 4, 1, 5}};
    L.cell_vertices.assign(&blocks[0][0], &blocks[0][0] + 20);
  }

  inline uint64_t vertex_pair(uint32_t a, uint32_t b) { return ((uint64_t)std::min(a, b) << 32) | std::max(a, b); }

  // Refinement: a new vertex on an edge is the straight midpoint, projected to the circle if both ends lie on it (the
  // midpoint of the arc); the new vertex of a cell is 1/2 (sum of its four edge midpoints) - 1/4 (sum of its four
  // vertices), the centre of the transfinite interpolation.  The children of cell c are 4c .. 4c+3, child = x + 2y.
  void ball_refine(const Level &C, Level &L)
  {
    L.vertex_xy = C.vertex_xy;
    L.on_circle = C.on_circle;
    std::unordered_map<uint64_t, uint32_t> mid;
    mid.reserve(2 * C.cell_vertices.size());
    const auto add_vertex = [&](double x, double y, bool circle) {
      L.vertex_xy.push_back(x);
      L.vertex_xy.push_back(y);
      L.on_circle.push_back(circle);
      return (uint32_t)L.on_circle.size() - 1;
    };
    const auto midpoint = [&](uint32_t a, uint32_t b) {
      const auto at = mid.find(vertex_pair(a, b));
      if (at != mid.end())
        return at->second;
      double     x = 0.5 * (L.vertex_xy[2 * (size_t)a] + L.vertex_xy[2 * (size_t)b]), y = 0.5 * (L.vertex_xy[2 * (size_t)a + 1] + L.vertex_xy[2 * (size_t)b + 1]);
      const bool circle = L.on_circle[a] && L.on_circle[b];
      if (circle)
        {
          const double r = std::hypot(x, y);
          x /= r, y /= r;
        }
      return mid[vertex_pair(a, b)] = add_vertex(x, y, circle);
    };
    const size_t nc = C.cell_vertices.size() / 4;
    L.cell_vertices.resize(16 * nc);
    for (size_t c = 0; c < nc; ++c)
      {
        const uint32_t *v = &C.cell_vertices[4 * c];
        const uint32_t  mb = midpoint(v[0], v[1]), mt = midpoint(v[2], v[3]), ml = midpoint(v[0], v[2]), mr = midpoint(v[1], v[3]);
        double          xy[2];
        for (int d = 0; d < 2; ++d)
          {
            const double *X = L.vertex_xy.data() + d;
            xy[d] = 0.5 * (X[2 * (size_t)mb] + X[2 * (size_t)mt] + X[2 * (size_t)ml] + X[2 * (size_t)mr]) -
                    0.25 * (X[2 * (size_t)v[0]] + X[2 * (size_t)v[1]] + X[2 * (size_t)v[2]] + X[2 * (size_t)v[3]]);
          }
        const uint32_t ctr         = add_vertex(xy[0], xy[1], false);
        const uint32_t child[4][4] = {{v[0], mb, ml, ctr}, {mb, v[1], ctr, mr}, {ml, ctr, v[2], mt}, {ctr, mr, mt, v[3]}};
        std::copy(&child[0][0], &child[0][0] + 16, &L.cell_vertices[16 * c]);
      }
  }

  // Tables of a level of the disc from its cells' vertices: an entity is a vertex, an edge (its pair of vertices) or a
  // cell; first touch in cell order, the entities on the circle (all Dirichlet) after all others, as in build_level.
  // false: a shared edge runs in opposite directions in its two cells
  bool build_ball_level(const mgx_square_s &Q, Level &L, int level)
  {
    const int p = Q.p;
    L.n_cells   = (uint32_t)(L.cell_vertices.size() / 4);
    const uint32_t nv = (uint32_t)L.on_circle.size();
    // edges in the order of their first touch; entity e of a cell runs from vertex from[e] to vertex to[e]
    static const int                       from[9] = {0, 0, 1, 0, 0, 1, 2, 2, 3}, to[9] = {0, 1, 1, 2, 0, 3, 2, 3, 3};
    std::unordered_map<uint64_t, uint32_t> edge;
    std::vector<uint32_t>                  edge_first; // the vertex an edge starts from
    std::vector<uint8_t>                   edge_on_circle;
    std::vector<uint32_t>                  key(9 * (size_t)L.n_cells);
    edge.reserve(3 * (size_t)L.n_cells);
    for (uint32_t c = 0; c < L.n_cells; ++c)
      for (int e = 0; e < 9; ++e)
        {
          const uint32_t a = L.cell_vertices[4 * (size_t)c + from[e]], b = L.cell_vertices[4 * (size_t)c + to[e]];
          if (e == 4)
            continue;
          if (a == b)
            {
              key[9 * (size_t)c + e] = a;
              continue;
            }
          const auto at = edge.find(vertex_pair(a, b));
          uint32_t   id;
          if (at == edge.end())
            {
              id = edge[vertex_pair(a, b)] = (uint32_t)edge_first.size();
              edge_first.push_back(a);
              edge_on_circle.push_back(L.on_circle[a] && L.on_circle[b]);
            }
          else if (edge_first[id = at->second] != a)
            return false;
          key[9 * (size_t)c + e] = nv + id;
        }
    const uint32_t ned = (uint32_t)edge_first.size();
    for (uint32_t c = 0; c < L.n_cells; ++c)
      key[9 * (size_t)c + 4] = nv + ned + c;
    auto on_boundary = [&](uint32_t k) { return k < nv ? L.on_circle[k] != 0 : (k < nv + ned && edge_on_circle[k - nv] != 0); };
    std::vector<uint32_t> base((size_t)nv + ned + L.n_cells, MGX_INVALID_INDEX);
    uint32_t              counter = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (uint32_t c = 0; c < L.n_cells; ++c)
        for (int e = 0; e < 9; ++e)
          {
            const uint32_t k = key[9 * (size_t)c + e];
            if (base[k] != MGX_INVALID_INDEX || on_boundary(k) != (pass == 1))
              continue;
            base[k] = counter;
            if (pass == 1)
              for (int d = 0; d < entity_size(e, p); ++d)
                L.constrained.push_back(counter + (uint32_t)d);
            counter += (uint32_t)entity_size(e, p);
          }
    L.n_dofs = counter;
    L.idx9.resize(9 * (size_t)L.n_cells);
    L.idx9_plain.resize(9 * (size_t)L.n_cells);
    for (size_t i = 0; i < key.size(); ++i)
      {
        L.idx9_plain[i] = base[key[i]];
        L.idx9[i]       = on_boundary(key[i]) ? MGX_INVALID_INDEX : base[key[i]];
      }
    L.dof_grid.resize(L.n_dofs); // (no grid: the generators are keyed by the DoF index)
    for (uint32_t d = 0; d < L.n_dofs; ++d)
      L.dof_grid[d] = d;
    if (level > 0)
      {
        L.children.resize(L.n_cells);
        for (uint32_t c = 0; c < L.n_cells; ++c)
          L.children[c] = c;
      }
    return true;
  }

  // Nodes of a cell of the disc (isoparametric degree p): on a straight edge the Gauss-Lobatto nodes are placed linearly,
  // on an edge of the boundary on the arc at angles linear in the node parameter; the nodes inside by transfinite
  // interpolation of the four edges, X(s, u) = (1-u) B(s) + u T(s) + (1-s) L(u) + s R(u) - the bilinear map of the
  // corners -- the bilinear map itself wherever all four edges are straight.
  void ball_cell_nodes(const mgx_square_s &Q, const Level &L, uint32_t c, double *xy)
  {
    const int       p = Q.p, n = p + 1;
    const uint32_t *v = &L.cell_vertices[4 * (size_t)c];
    const double   *g = Q.basis.gll;
    const auto      X = [&](int k, int d) { return L.vertex_xy[2 * (size_t)v[k] + d]; };
    const auto      edge = [&](int a, int b, int first, int stride) {
      double      *out = xy + 2 * first;
      const double xa = X(a, 0), ya = X(a, 1), xb = X(b, 0), yb = X(b, 1);
      if (L.on_circle[v[a]] && L.on_circle[v[b]])
        {
          const double ta = std::atan2(ya, xa);
          double       dt = std::atan2(yb, xb) - ta;
          dt -= 2 * kPi * std::round(dt / (2 * kPi));
          for (int i = 1; i < p; ++i)
            out[2 * stride * i] = std::cos(ta + g[i] * dt), out[2 * stride * i + 1] = std::sin(ta + g[i] * dt);
        }
      else
        for (int i = 1; i < p; ++i)
          out[2 * stride * i] = xa + g[i] * (xb - xa), out[2 * stride * i + 1] = ya + g[i] * (yb - ya);
      out[0] = xa, out[1] = ya;
      out[2 * stride * p] = xb, out[2 * stride * p + 1] = yb;
    };
    edge(0, 1, 0, 1);     // B
    edge(2, 3, p * n, 1); // T
    edge(0, 2, 0, n);     // L
    edge(1, 3, p, n);     // R
    for (int j = 1; j < p; ++j)
      for (int i = 1; i < p; ++i)
        for (int d = 0; d < 2; ++d)
          {
            const double s = g[i], u = g[j];
            xy[2 * (j * n + i) + d] = (1 - u) * xy[2 * i + d] + u * xy[2 * (p * n + i) + d] + (1 - s) * xy[2 * (j * n) + d] +
                                      s * xy[2 * (j * n + p) + d] -
                                      ((1 - s) * (1 - u) * X(0, d) + s * (1 - u) * X(1, d) + (1 - s) * u * X(2, d) + s * u * X(3, d));
          }
  }

  bool valid(mgx_square_t q, int l) { return q && l >= 0 && l < (int)q->levels.size(); }

  // the (p+1)^2 Gauss-Lobatto nodes of cell c, x fastest: xy[2 (j n + i)], placed by the exact map
  void cell_nodes(const mgx_square_s &Q, const Level &L, uint32_t c, double *xy)
  {
    const int n = Q.p + 1;
    if (Q.geometry == MGX_SQUARE_GEOMETRY_BALL)
      return ball_cell_nodes(Q, L, c, xy);
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i)
        Q.point(L.h * (L.coords[2 * (size_t)c] + Q.basis.gll[i]), L.h * (L.coords[2 * (size_t)c + 1] + Q.basis.gll[j]), xy[2 * (j * n + i)],
                xy[2 * (j * n + i) + 1]);
  }

  // Per-point geometry of the isoparametric cells: with J the Jacobian of the degree-p interpolant of the cell nodes at a
  // Gauss point, G = J^T J = [[a, b], [b, c]] and det J = sqrt(a c - b^2):  JxW J^-1 J^-T = (w / det J) [c, a, -b].
  // unit [n_cells][3][n^2] and jxw [n_cells][n^2]; false: a cell with det J <= 0
  bool point_geometry(const mgx_square_s &Q, const Level &L, double *unit, double *jxw)
  {
    const int           p = Q.p, n = p + 1, n2 = n * n;
    std::vector<double> G((size_t)n * n), xy(2 * (size_t)n2);
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i)
        {
          double g = 0;
          for (int r = 0; r < n; ++r)
            g += Q.basis.D[q * n + r] * Q.basis.S[r * n + i];
          G[q * n + i] = g;
        }
    for (uint32_t cell = 0; cell < L.n_cells; ++cell)
      {
        cell_nodes(Q, L, cell, xy.data());
        for (int qy = 0; qy < n; ++qy)
          for (int qx = 0; qx < n; ++qx)
            {
              double xa = 0, xb = 0, ya = 0, yb = 0; // d(x, y) / d(xi, eta)
              for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i)
                  {
                    const double da = G[qx * n + i] * Q.basis.S[qy * n + j], db = Q.basis.S[qx * n + i] * G[qy * n + j];
                    xa += da * xy[2 * (j * n + i)];
                    xb += db * xy[2 * (j * n + i)];
                    ya += da * xy[2 * (j * n + i) + 1];
                    yb += db * xy[2 * (j * n + i) + 1];
                  }
              const double det = xa * yb - xb * ya;
              if (!(det > 0.))
                return false;
              const double w = Q.basis.gw[qx] * Q.basis.gw[qy], a = xa * xa + ya * ya, b = xa * xb + ya * yb, c = xb * xb + yb * yb;
              const size_t q = (size_t)qy * n + qx;
              if (unit)
                {
                  double *u = unit + (size_t)cell * 3 * n2 + q;
                  u[0] = w * c / det, u[n2] = w * a / det, u[2 * n2] = -w * b / det;
                }
              if (jxw)
                jxw[(size_t)cell * n2 + q] = w * det;
            }
      }
    return true;
  }

  // curved cells: the unit-law tensor is the operator's coefficient, kept with JxW on the level
  bool store_point_geometry(const mgx_square_s &Q, Level &L)
  {
    const size_t n2 = (size_t)(Q.p + 1) * (Q.p + 1);
    L.unit_q.resize((size_t)L.n_cells * 3 * n2);
    L.jxw_q.resize((size_t)L.n_cells * n2);
    return point_geometry(Q, L, L.unit_q.data(), L.jxw_q.data());
  }

  // ---- linear problems on every square (mgx_square_problem) ----
  // The geometry of a problem is that of point_geometry, stated once: a cell is the degree-p interpolant of its nodes
  // (cell_nodes), x(xi, eta) = sum_ij phi_i(xi) phi_j(eta) X_ij.  Its quadrature points are therefore
  // x_q = sum_ij S[qx][i] S[qy][j] X_ij, and unit_q / jxw_q come from the Jacobian of the same interpolant.
  // xq[2 (qy n + qx)] from the nodes xy[2 (j n + i)] of a cell
  void quadrature_points(const mgx_square_s &Q, const double *xy, double *xq)
  {
    const int     n = Q.p + 1;
    const double *S = Q.basis.S;
    for (int qy = 0; qy < n; ++qy)
      for (int qx = 0; qx < n; ++qx)
        {
          double x = 0, y = 0;
          for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i)
              {
                const double s = S[qx * n + i] * S[qy * n + j];
                x += s * xy[2 * (j * n + i)];
                y += s * xy[2 * (j * n + i) + 1];
              }
          xq[2 * (qy * n + qx)] = x, xq[2 * (qy * n + qx) + 1] = y;
        }
  }

  // u, a and f = -(a lap u + grad a . grad u) of a problem at a point
  struct ProblemFunctions
  {
    int    kind;
    double contrast;
    double u(double x, double y) const
    {
      return kind == MGX_SQUARE_PROBLEM_CUBE ? mgx_square_s::u(x, y) : std::sin(2 * kPi * (x + y));
    }
    // c_e = cos(2 pi x_e + 0.1 e), e = 0, 1 (poisson_shell/program.cc:157-169 with dim = 2)
    double a(double x, double y) const
    {
      if (kind == MGX_SQUARE_PROBLEM_CUBE)
        return 1.;
      const double c0 = std::cos(2 * kPi * x), c1 = std::cos(2 * kPi * y + 0.1);
      return 1. + contrast * (c0 * c0) * (c1 * c1);
    }
    double f(double x, double y) const
    {
      if (kind == MGX_SQUARE_PROBLEM_CUBE)
        return mgx_square_s::f(x, y);
      const double c0 = std::cos(2 * kPi * x), c1 = std::cos(2 * kPi * y + 0.1);
      const double s0 = std::sin(2 * kPi * x), s1 = std::sin(2 * kPi * y + 0.1);
      const double lap = -2 * (2 * kPi) * (2 * kPi) * std::sin(2 * kPi * (x + y)), du = 2 * kPi * std::cos(2 * kPi * (x + y));
      const double ax = contrast * (-4 * kPi * c0 * s0) * (c1 * c1), ay = contrast * (c0 * c0) * (-4 * kPi * c1 * s1);
      return -(lap * a(x, y) + (ax + ay) * du);
    }
  };

  // the checked arguments of a problem accessor; the status is reported
  int problem_arguments(mgx_square_t q, int l, const mgx_square_problem *problem, const void *out, const char *who, ProblemFunctions &F)
  {
    const auto refuse = [&](const char *why) { return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, (std::string(who) + why).c_str()); };
    if (!valid(q, l) || !out)
      return refuse(": bad argument");
    if (!problem)
      return refuse(": null problem");
    if (problem->kind != MGX_SQUARE_PROBLEM_CUBE && problem->kind != MGX_SQUARE_PROBLEM_SHELL)
      return refuse(": unknown problem kind");
    if (problem->kind == MGX_SQUARE_PROBLEM_SHELL && !(problem->contrast >= 0. && std::isfinite(problem->contrast)))
      return refuse(": the contrast must be finite and not negative");
    F.kind     = problem->kind;
    F.contrast = problem->contrast;
    return MGX_OK;
  }

  // visit(cell, q, x, y) at every quadrature point of the level, cells and points in order
  template <typename Visit>
  void for_each_quadrature_point(const mgx_square_s &Q, const Level &L, Visit &&visit)
  {
    const size_t        n2 = (size_t)(Q.p + 1) * (Q.p + 1);
    std::vector<double> xy(2 * n2), xq(2 * n2);
    for (uint32_t c = 0; c < L.n_cells; ++c)
      {
        cell_nodes(Q, L, c, xy.data());
        quadrature_points(Q, xy.data(), xq.data());
        for (size_t k = 0; k < n2; ++k)
          visit(c, k, xq[2 * k], xq[2 * k + 1]);
      }
  }
} // namespace

static int square_create(const mgx_square_box_desc *bd, int geometry, mgx_square_t *out);

extern "C" {

int mgx_square_create_box(const mgx_square_box_desc *bd, mgx_square_t *out) { return square_create(bd, 0, out); }

int mgx_square_create_mapped(const mgx_square_box_desc *bd, int geometry, mgx_square_t *out)
{
  if (geometry != MGX_SQUARE_GEOMETRY_ANNULUS_SECTOR)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_mapped: unknown geometry");
  if (bd && bd->jacobian)
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_square_create_mapped: a jacobian on a mapped square (its geometry is that "
                                                  "of its own map; jacobian must be NULL)");
  return square_create(bd, geometry, out);
}

} // extern "C"

static int square_create(const mgx_square_box_desc *bd, int geometry, mgx_square_t *out)
{
  if (!bd || !out || bd->degree < 1 || bd->degree > MGX_MAX_DEGREE || bd->n_refine < 0 || bd->n_refine > 14 || bd->roots[0] < 1 ||
      bd->roots[1] < 1 || !(bd->h0 > 0))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_box: bad argument");
  if (((uint64_t)bd->roots[0] << bd->n_refine) * ((uint64_t)bd->roots[1] << bd->n_refine) * (uint64_t)(bd->degree * bd->degree) >= 0xFFFFFFF0ull)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_box: the finest level does not fit 32-bit indices");
  mgx_square_s *Q = new mgx_square_s;
  Q->p            = bd->degree;
  Q->roots[0]     = bd->roots[0];
  Q->roots[1]     = bd->roots[1];
  Q->origin       = bd->origin;
  Q->h0           = bd->h0;
  if (bd->jacobian)
    std::copy(bd->jacobian, bd->jacobian + 4, Q->A);
  Q->detA = Q->A[0] * Q->A[3] - Q->A[1] * Q->A[2];
  if (!(Q->detA > 0))
    {
      delete Q;
      return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_box: the jacobian must have a positive determinant");
    }
  // det(J) J^-1 J^-T = det(A) (A^T A)^-1
  const double g00 = Q->A[0] * Q->A[0] + Q->A[2] * Q->A[2], g11 = Q->A[1] * Q->A[1] + Q->A[3] * Q->A[3],
               g01 = Q->A[0] * Q->A[1] + Q->A[2] * Q->A[3], dg = g00 * g11 - g01 * g01;
  Q->coef[0] = Q->detA * g11 / dg;
  Q->coef[1] = Q->detA * g00 / dg;
  Q->coef[2] = g01 == 0. ? 0. : -Q->detA * g01 / dg;
  mgx::make_basis(Q->basis, Q->p);
  Q->geometry = geometry;
  Q->levels.resize((size_t)bd->n_refine + 1);
  for (int l = 0; l <= bd->n_refine; ++l)
    {
      Level &L = Q->levels[l];
      build_level(*Q, L, l);
      if (geometry != 0 && !store_point_geometry(*Q, L))
        {
          mgx_square_destroy(Q);
          return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_mapped: a cell with det J <= 0");
        }
    }
  *out = Q;
  return MGX_OK;
}

extern "C" int mgx_square_create_ball(int degree, int n_refine, mgx_square_t *out)
{
  if (!out || degree < 1 || degree > MGX_MAX_DEGREE || n_refine < 0 || n_refine > 14)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_ball: bad argument");
  if ((5ull << (2 * n_refine)) * (uint64_t)(degree * degree) >= 0xFFFFFFF0ull)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create_ball: the finest level does not fit 32-bit indices");
  mgx_square_s *Q = new mgx_square_s;
  Q->p            = degree;
  Q->roots[0] = Q->roots[1] = 0; // (no lattice)
  Q->geometry               = MGX_SQUARE_GEOMETRY_BALL;
  mgx::make_basis(Q->basis, Q->p);
  Q->levels.resize((size_t)n_refine + 1);
  for (int l = 0; l <= n_refine; ++l)
    {
      Level &L = Q->levels[l];
      if (l == 0)
        ball_coarse_level(L);
      else
        ball_refine(Q->levels[l - 1], L);
      const char *why = !build_ball_level(*Q, L, l)   ? "mgx_square_create_ball: a shared edge runs in opposite directions in its cells"
                        : !store_point_geometry(*Q, L) ? "mgx_square_create_ball: a cell with det J <= 0"
                                                       : nullptr;
      if (why)
        {
          mgx_square_destroy(Q);
          return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, why);
        }
    }
  *out = Q;
  return MGX_OK;
}

extern "C" {

int mgx_square_create(int degree, int n_subdiv, int n_refine, mgx_square_t *out)
{
  if (n_subdiv < 1)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_create: bad argument");
  mgx_square_box_desc bd;
  bd.degree   = degree;
  bd.n_refine = n_refine;
  bd.roots[0] = bd.roots[1] = n_subdiv;
  bd.origin   = -0.9;
  bd.h0       = 1.9 / n_subdiv;
  bd.jacobian = nullptr;
  return mgx_square_create_box(&bd, out);
}

int mgx_square_destroy(mgx_square_t q)
{
  delete q;
  return MGX_OK;
}

int      mgx_square_n_levels(mgx_square_t q) { return (int)q->levels.size(); }
int      mgx_square_degree(mgx_square_t q) { return q->p; }
uint32_t mgx_square_n_cells(mgx_square_t q, int l) { return q->levels[l].n_cells; }
uint32_t mgx_square_n_dofs(mgx_square_t q, int l) { return q->levels[l].n_dofs; }
uint32_t mgx_square_n_constrained(mgx_square_t q, int l) { return (uint32_t)q->levels[l].constrained.size(); }
// the disc has no lattice of cells and no grid of DoFs
static bool refuse_ball(mgx_square_t q, const char *who)
{
  if (q->geometry != MGX_SQUARE_GEOMETRY_BALL)
    return false;
  mgx::report_error(MGX_ERR_UNSUPPORTED, (std::string(who) + ": not on the disc (five blocks: no lattice of cells, no grid of DoFs)").c_str());
  return true;
}
void mgx_square_cells_per_dim2(mgx_square_t q, int l, uint32_t cells[2])
{
  (void)refuse_ball(q, "mgx_square_cells_per_dim2");
  cells[0] = q->levels[l].N[0];
  cells[1] = q->levels[l].N[1];
}
double          mgx_square_cell_size(mgx_square_t q, int l) { return q->levels[l].h; }
const uint32_t *mgx_square_idx9(mgx_square_t q, int l) { return q->levels[l].idx9.data(); }
const uint32_t *mgx_square_idx9_plain(mgx_square_t q, int l) { return q->levels[l].idx9_plain.data(); }
const uint32_t *mgx_square_constrained(mgx_square_t q, int l) { return q->levels[l].constrained.data(); }
const uint32_t *mgx_square_children(mgx_square_t q, int l) { return l > 0 ? q->levels[l].children.data() : nullptr; }
// (the disc: NULL -- three cells meet at four of its vertices, the transfer derives owner weights itself)
const uint8_t  *mgx_square_weight_shift(mgx_square_t q, int l) { return l > 0 && !q->levels[l].weight_shift.empty() ? q->levels[l].weight_shift.data() : nullptr; }
const uint32_t *mgx_square_cell_coords(mgx_square_t q, int l) { return refuse_ball(q, "mgx_square_cell_coords") ? nullptr : q->levels[l].coords.data(); }
const uint32_t *mgx_square_dof_grid(mgx_square_t q, int l) { return refuse_ball(q, "mgx_square_dof_grid") ? nullptr : q->levels[l].dof_grid.data(); }
const double   *mgx_square_shape_values(mgx_square_t q) { return q->basis.S; }
const double   *mgx_square_colloc_grad(mgx_square_t q) { return q->basis.D; }
const double   *mgx_square_qweights(mgx_square_t q) { return q->basis.gw; }
const double   *mgx_square_qpoints(mgx_square_t q) { return q->basis.gq; }
const double   *mgx_square_gll(mgx_square_t q) { return q->basis.gll; }
const double   *mgx_square_prolong_1d(mgx_square_t q) { return q->basis.P1; }

// the Poisson problem exists on the box only
static bool refuse_mapped(mgx_square_t q, const char *who)
{
  if (q->geometry == 0)
    return false;
  mgx::report_error(MGX_ERR_UNSUPPORTED, (std::string(who) + ": not on a mapped square (no Poisson problem there)").c_str());
  return true;
}

const double *mgx_square_rhs(mgx_square_t q, int l)
{
  if (refuse_mapped(q, "mgx_square_rhs"))
    return nullptr;
  Level &L = q->levels[l];
  if (L.rhs.empty())
    build_rhs(*q, L);
  return L.rhs.data();
}
uint32_t        mgx_square_bc_count(mgx_square_t q, int l) { return q->geometry == 0 ? (uint32_t)q->levels[l].constrained.size() : 0u; }
const uint32_t *mgx_square_bc_index(mgx_square_t q, int l)
{
  return refuse_mapped(q, "mgx_square_bc_index") ? nullptr : q->levels[l].constrained.data();
}
const double *mgx_square_bc_value(mgx_square_t q, int l)
{
  return refuse_mapped(q, "mgx_square_bc_value") ? nullptr : q->levels[l].bc_value.data();
}

double mgx_square_l2_error(mgx_square_t q, int l, const double *sol)
{
  if (refuse_mapped(q, "mgx_square_l2_error"))
    return std::nan("");
  const Level        &L = q->levels[l];
  const int           p = q->p, n = p + 1;
  std::vector<double> ul((size_t)n * n), t((size_t)n * n);
  const double        jxw = L.h * L.h * q->detA;
  double              err = 0, vol = 0;
  for (uint32_t c = 0; c < L.n_cells; ++c)
    {
      const uint32_t *ix = &L.idx9_plain[9 * (size_t)c];
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          ul[j * n + i] = sol[mgx::cell_dof(ix, 2, p, i, j)];
      for (int j = 0; j < n; ++j) // along x
        for (int qx = 0; qx < n; ++qx)
          {
            double s = 0;
            for (int i = 0; i < n; ++i)
              s += q->basis.S[qx * n + i] * ul[j * n + i];
            t[j * n + qx] = s;
          }
      for (int qy = 0; qy < n; ++qy)
        for (int qx = 0; qx < n; ++qx)
          {
            double s = 0, x, y;
            for (int j = 0; j < n; ++j)
              s += q->basis.S[qy * n + j] * t[j * n + qx];
            q->map(L.h * (L.coords[2 * (size_t)c] + q->basis.gq[qx]), L.h * (L.coords[2 * (size_t)c + 1] + q->basis.gq[qy]), x, y);
            const double w = q->basis.gw[qx] * q->basis.gw[qy] * jxw, d = s - mgx_square_s::u(x, y);
            err += d * d * w;
            vol += w;
          }
    }
  return std::sqrt(err / vol);
}

int mgx_square_seeded_vector(mgx_square_t q, int l, uint64_t seed, double *out)
{
  if (!valid(q, l) || !out)
    return MGX_ERR_INVALID_ARGUMENT;
  mgx::seeded_fill(seed, q->levels[l].dof_grid.data(), q->levels[l].n_dofs, out);
  return MGX_OK;
}

int mgx_square_operator_desc(mgx_square_t q, int l, int number, mgx_operator_desc *d)
{
  if (!valid(q, l) || !d)
    return MGX_ERR_INVALID_ARGUMENT;
  const Level &L = q->levels[l];
  std::memset(d, 0, sizeof(*d));
  d->degree        = q->p;
  d->number        = number;
  d->n_cells       = L.n_cells;
  d->n_dofs        = L.n_dofs;
  d->idx27         = L.idx9.data();
  d->idx27_plain   = L.idx9_plain.data();
  d->constrained   = L.constrained.data();
  d->n_constrained = (uint32_t)L.constrained.size();
  d->coef[0]       = q->coef[0];
  d->coef[1]       = q->coef[1];
  d->coef[2]       = q->coef[2];
  d->shape_values  = q->basis.S;
  d->colloc_grad   = q->basis.D;
  d->qweights      = q->basis.gw;
  d->global_index  = L.dof_grid.data();
  d->dim           = 2;
  if (q->geometry != 0) // curved cells: JxW_q J^-1 J^-T of every point (coef is not read then)
    d->coef_q = L.unit_q.data();
  return MGX_OK;
}

int mgx_square_affine_metric(mgx_square_t q, int l, double metric[3], double *det_jacobian)
{
  if (!valid(q, l) || !metric || !det_jacobian)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_affine_metric: bad argument");
  if (q->geometry != 0)
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_square_affine_metric: not on a mapped square (curved cells: "
                                                  "mgx_square_unit_q, mgx_square_jxw_q)");
  // J = h A:  J^-1 J^-T = (A^T A)^-1 / h^2 = coef / (det(A) h^2)
  const double h = q->levels[l].h, s = 1. / (q->detA * h * h);
  metric[0] = q->coef[0] * s, metric[1] = q->coef[1] * s, metric[2] = q->coef[2] * s;
  *det_jacobian = q->detA * h * h;
  return MGX_OK;
}

int mgx_square_cell_nodes(mgx_square_t q, int l, double *out)
{
  if (!valid(q, l) || !out)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_cell_nodes: bad argument");
  const size_t n2 = (size_t)(q->p + 1) * (q->p + 1);
  for (uint32_t c = 0; c < q->levels[l].n_cells; ++c)
    cell_nodes(*q, q->levels[l], c, out + 2 * n2 * c);
  return MGX_OK;
}

int mgx_square_dof_coordinates(mgx_square_t q, int l, double *out)
{
  if (!valid(q, l) || !out)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_dof_coordinates: bad argument");
  const Level        &L = q->levels[l];
  const int           p = q->p, n = p + 1;
  std::vector<double> xy(2 * (size_t)n * n);
  for (uint32_t c = 0; c < L.n_cells; ++c)
    {
      cell_nodes(*q, L, c, xy.data());
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          {
            const uint32_t d = mgx::cell_dof(&L.idx9_plain[9 * (size_t)c], 2, p, i, j);
            out[2 * (size_t)d]     = xy[2 * (j * n + i)];
            out[2 * (size_t)d + 1] = xy[2 * (j * n + i) + 1];
          }
    }
  return MGX_OK;
}

int mgx_square_unit_q(mgx_square_t q, int l, double *out)
{
  if (!valid(q, l) || !out)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_unit_q: bad argument");
  const Level &L = q->levels[l];
  if (!L.unit_q.empty())
    std::copy(L.unit_q.begin(), L.unit_q.end(), out);
  else if (!point_geometry(*q, L, out, nullptr))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_unit_q: a cell with det J <= 0");
  return MGX_OK;
}

int mgx_square_jxw_q(mgx_square_t q, int l, double *out)
{
  if (!valid(q, l) || !out)
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_jxw_q: bad argument");
  const Level &L = q->levels[l];
  if (!L.jxw_q.empty())
    std::copy(L.jxw_q.begin(), L.jxw_q.end(), out);
  else if (!point_geometry(*q, L, nullptr, out))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_jxw_q: a cell with det J <= 0");
  return MGX_OK;
}

int mgx_square_coef_q(mgx_square_t q, int l, double *out)
{
  if (!valid(q, l) || !out)
    return MGX_ERR_INVALID_ARGUMENT;
  const int    n  = q->p + 1;
  const size_t n2 = (size_t)n * n;
  if (q->geometry != 0) // (the descriptor's coefficient is this tensor already)
    return mgx_square_unit_q(q, l, out);
  for (size_t c = 0; c < q->levels[l].n_cells; ++c)
    for (int k = 0; k < 3; ++k)
      for (size_t p = 0; p < n2; ++p)
        out[(c * 3 + k) * n2 + p] = q->coef[k] * q->basis.gw[p % n] * q->basis.gw[p / n];
  return MGX_OK;
}

int mgx_square_problem_coef_q(mgx_square_t q, int l, const mgx_square_problem *problem, double *out)
{
  ProblemFunctions F;
  if (const int status = problem_arguments(q, l, problem, out, "mgx_square_problem_coef_q", F); status != MGX_OK)
    return status;
  if (const int status = mgx_square_coef_q(q, l, out); status != MGX_OK) // the unit-law tensor of the level's geometry
    return status;
  const size_t n2 = (size_t)(q->p + 1) * (q->p + 1);
  for_each_quadrature_point(*q, q->levels[l], [&](uint32_t c, size_t k, double x, double y) {
    const double a = F.a(x, y);
    for (int e = 0; e < 3; ++e)
      out[((size_t)c * 3 + e) * n2 + k] *= a;
  });
  return MGX_OK;
}

int mgx_square_problem_rhs_quadrature(mgx_square_t q, int l, const mgx_square_problem *problem, double *out)
{
  ProblemFunctions F;
  if (const int status = problem_arguments(q, l, problem, out, "mgx_square_problem_rhs_quadrature", F); status != MGX_OK)
    return status;
  if (const int status = mgx_square_jxw_q(q, l, out); status != MGX_OK)
    return status;
  const size_t n2 = (size_t)(q->p + 1) * (q->p + 1);
  for_each_quadrature_point(*q, q->levels[l], [&](uint32_t c, size_t k, double x, double y) { out[(size_t)c * n2 + k] *= F.f(x, y); });
  return MGX_OK;
}

int mgx_square_problem_solution_q(mgx_square_t q, int l, const mgx_square_problem *problem, double *out)
{
  ProblemFunctions F;
  if (const int status = problem_arguments(q, l, problem, out, "mgx_square_problem_solution_q", F); status != MGX_OK)
    return status;
  const size_t n2 = (size_t)(q->p + 1) * (q->p + 1);
  for_each_quadrature_point(*q, q->levels[l], [&](uint32_t c, size_t k, double x, double y) { out[(size_t)c * n2 + k] = F.u(x, y); });
  return MGX_OK;
}

int mgx_square_problem_bc_value(mgx_square_t q, int l, const mgx_square_problem *problem, double *out)
{
  ProblemFunctions F;
  if (const int status = problem_arguments(q, l, problem, out, "mgx_square_problem_bc_value", F); status != MGX_OK)
    return status;
  const Level          &L = q->levels[l];
  const int             p = q->p, n = p + 1;
  std::vector<uint32_t> at(L.n_dofs, MGX_INVALID_INDEX); // DoF -> position in the list of constrained DoFs
  for (size_t i = 0; i < L.constrained.size(); ++i)
    at[L.constrained[i]] = (uint32_t)i;
  std::vector<double> xy(2 * (size_t)n * n);
  for (uint32_t c = 0; c < L.n_cells; ++c)
    {
      cell_nodes(*q, L, c, xy.data());
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          {
            const uint32_t k = at[mgx::cell_dof(&L.idx9_plain[9 * (size_t)c], 2, p, i, j)];
            if (k != MGX_INVALID_INDEX)
              out[k] = F.u(xy[2 * (j * n + i)], xy[2 * (j * n + i) + 1]);
          }
    }
  return MGX_OK;
}

// general: the hierarchy of mgx_square_solver_create_general with the tensors coef_q[l] (nullptr: the unit law)
static int square_solver_create(mgx_context_t ctx, mgx_square_t q, int vnumber, int degree_pre, int n_cycles, int per_point,
                                bool general, const double *const *coef_q, mgx_cube_solver *out);

int mgx_square_solver_create(mgx_context_t ctx, mgx_square_t q, int vnumber, int degree_pre, int n_cycles, int per_point,
                             mgx_cube_solver *out)
{
  if (!ctx || !q || !out || (vnumber != MGX_F32 && vnumber != MGX_F64))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_solver_create: bad argument");
  if (q->geometry != 0)
    return mgx::report_error(MGX_ERR_UNSUPPORTED, "mgx_square_solver_create: not on a mapped square (no Poisson problem there; "
                                                  "mgx_square_solver_create_general)");
  return square_solver_create(ctx, q, vnumber, degree_pre, n_cycles, per_point, false, nullptr, out);
}

int mgx_square_solver_create_general(mgx_context_t ctx, mgx_square_t q, int vnumber, int degree_pre, int n_cycles,
                                     const double *const *coef_q, mgx_cube_solver *out)
{
  if (!ctx || !q || !out || (vnumber != MGX_F32 && vnumber != MGX_F64))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_solver_create_general: bad argument");
  return square_solver_create(ctx, q, vnumber, degree_pre, n_cycles, 1, true, coef_q, out);
}

int mgx_square_solver_create_problem(mgx_context_t ctx, mgx_square_t q, int vnumber, int degree_pre, int n_cycles,
                                     const mgx_square_problem *problem, mgx_cube_solver *out)
{
  if (!ctx || !q || !out || (vnumber != MGX_F32 && vnumber != MGX_F64))
    return mgx::report_error(MGX_ERR_INVALID_ARGUMENT, "mgx_square_solver_create_problem: bad argument");
  const int                        nl = (int)q->levels.size();
  const size_t                     n2 = (size_t)(q->p + 1) * (q->p + 1);
  std::vector<std::vector<double>> bc_value(nl); // (read by mgx_solver_create, after every level was described)
  for (int l = 0; l < nl; ++l)
    {
      bc_value[l].resize(std::max<size_t>(q->levels[l].constrained.size(), 1));
      // (checks the problem as well, before anything exists on the device)
      if (const int status = mgx_square_problem_bc_value(q, l, problem, bc_value[l].data()); status != MGX_OK)
        return status;
    }
  const auto describe = [&](int l, mgx::LevelDesc &d) {
    const Level &L = q->levels[l];
    mgx_square_operator_desc(q, l, MGX_F64, &d.op);
    d.scratch.resize((size_t)L.n_cells * 3 * n2);
    if (const int status = mgx_square_problem_coef_q(q, l, problem, d.scratch.data()); status != MGX_OK)
      return status;
    d.op.coef_q             = d.scratch.data(); // (an fp32 V-cycle operator receives it rounded)
    d.transfer.children     = L.children.data();
    d.transfer.prolong_1d   = q->basis.P1;
    d.transfer.weight_shift = L.weight_shift.empty() ? nullptr : L.weight_shift.data();
    d.rhs                   = nullptr; // assembled on the device below
    d.bc_index              = L.constrained.data();
    d.bc_value              = bc_value[l].data();
    d.bc_count              = (uint32_t)L.constrained.size();
    return (int)MGX_OK;
  };
  int status = mgx::build_hierarchy(ctx, nl, vnumber, degree_pre, n_cycles, describe, out);
  if (status != MGX_OK)
    return status;
  // the right-hand sides on the device (laplace_operator.h:804-845): the host only evaluates f JxW at the quadrature
  // points (the loop of mgx_cube_solver_create_opt)
  for (int l = 0; l < nl && status == MGX_OK; ++l)
    {
      const size_t        count = n2 * q->levels[l].n_cells;
      std::vector<double> fq(count);
      void               *fq_dev = nullptr;
      status                     = mgx_square_problem_rhs_quadrature(q, l, problem, fq.data());
      if (status == MGX_OK)
        status = mgx_malloc(ctx, &fq_dev, sizeof(double) * count);
      if (status == MGX_OK)
        status = mgx_upload(ctx, fq_dev, fq.data(), sizeof(double) * count);
      if (status == MGX_OK)
        status = mgx_solver_compute_rhs_2d(out->solver, l, (const double *)fq_dev);
      if (fq_dev)
        {
          const std::string keep = status != MGX_OK ? mgx_last_error() : "";
          (void)mgx_sync(ctx);
          (void)mgx_free(ctx, fq_dev);
          if (status != MGX_OK)
            mgx::report_error(status, keep.c_str());
        }
    }
  return status == MGX_OK ? MGX_OK : mgx::abandon_hierarchy(status, out);
}

} // extern "C"

static int square_solver_create(mgx_context_t ctx, mgx_square_t q, int vnumber, int degree_pre, int n_cycles, int per_point,
                                bool general, const double *const *coef_q, mgx_cube_solver *out)
{
  // (general hierarchy: the Newton update has a zero right-hand side until the caller writes one, and homogeneous
  // boundary values)
  const std::vector<double> zero(general ? q->levels.back().n_dofs : 0, 0.);
  const auto describe = [&](int l, mgx::LevelDesc &d) {
    const Level &L = q->levels[l];
    mgx_square_operator_desc(q, l, MGX_F64, &d.op);
    if (general && coef_q && coef_q[l])
      d.op.coef_q = coef_q[l];
    else if (per_point && !d.op.coef_q) // (a mapped square: the descriptor carries its per-point tensor)
      {
        d.scratch.resize((size_t)d.op.n_cells * 3 * (q->p + 1) * (q->p + 1));
        mgx_square_coef_q(q, l, d.scratch.data());
        d.op.coef_q = d.scratch.data();
      }
    if (general && q->geometry != 0) // curved cells
      {
        d.geometry = mgx::LevelDesc::per_point;
        d.unit_q   = L.unit_q.data();
        d.jxw_q    = L.jxw_q.data();
      }
    else if (general)
      {
        d.geometry = mgx::LevelDesc::affine;
        mgx_square_affine_metric(q, l, d.metric, &d.det);
      }
    d.transfer.children     = L.children.data();
    d.transfer.prolong_1d   = q->basis.P1;
    d.transfer.weight_shift = L.weight_shift.empty() ? nullptr : L.weight_shift.data();
    d.rhs                   = general ? zero.data() : mgx_square_rhs(q, l);
    d.bc_index              = L.constrained.data();
    d.bc_value              = L.bc_value.data();
    d.bc_count              = general ? 0u : (uint32_t)L.constrained.size();
    return (int)MGX_OK;
  };
  return mgx::build_hierarchy(ctx, (int)q->levels.size(), vnumber, degree_pre, n_cycles, describe, out);
}
