// Runs the functions of multigrid_amd/csrc/mgx_index_tables.hpp on small tables built here and prints tables and
// results as lines "<case> <key> <numbers>" for tests/test_index_tables_host.py, which restates the rules in numpy.
// Built with AddressSanitizer and UBSan; no device, no library.
//
// A mesh is a list of cells with 2^dim integer corner points (multilinear cells); an entity is identified by its
// midpoint, so any conforming mesh gets a consistent table: structured boxes, three cells around a vertex or an edge.
#include "../multigrid_amd/csrc/mgx_index_tables.hpp"

#include <array>
#include <cstdio>
#include <map>
#include <string>

using namespace mgx;
using Point = std::array<long, 3>;
using Cell  = std::array<Point, 8>; // corner k at reference point (k & 1, k >> 1 & 1, k >> 2)
struct Mesh
{
  int               dim;
  std::vector<Cell> cells;
};
constexpr long kScale = 64; // corner coordinates are multiples of it: midpoints of the entities of children stay integers

// the point of a cell at reference coordinates r / 4 per direction
Point point_at(const Mesh &m, const Cell &c, const int r[3])
{
  Point x = {0, 0, 0};
  for (int k = 0; k < (1 << m.dim); ++k)
    {
      long w = 1;
      for (int d = 0; d < m.dim; ++d)
        w *= (k >> d & 1) ? r[d] : 4 - r[d];
      for (int d = 0; d < 3; ++d)
        x[d] += w * c[k][d];
    }
  for (int d = 0; d < 3; ++d)
    x[d] /= (m.dim == 2 ? 16 : 64);
  return x;
}

Mesh box(int dim, const int n[3])
{
  Mesh m{dim, {}};
  for (int z = 0; z < (dim == 3 ? n[2] : 1); ++z)
    for (int y = 0; y < n[1]; ++y)
      for (int x = 0; x < n[0]; ++x)
        {
          Cell c{};
          for (int k = 0; k < (1 << dim); ++k)
            c[k] = {kScale * (x + (k & 1)), kScale * (y + (k >> 1 & 1)), dim == 3 ? kScale * (z + (k >> 2)) : 0};
          m.cells.push_back(c);
        }
  return m;
}

// the cells sorted by the interleaved bits of their low corner
Mesh morton(const Mesh &m)
{
  std::map<unsigned long, Cell> sorted;
  for (const Cell &c : m.cells)
    {
      unsigned long key = 0;
      for (int b = 0; b < 8; ++b)
        for (int d = 0; d < m.dim; ++d)
          key |= (unsigned long)((c[0][d] / kScale) >> b & 1) << (m.dim * b + d);
      sorted[key] = c;
    }
  Mesh out{m.dim, {}};
  for (const auto &kc : sorted)
    out.cells.push_back(kc.second);
  return out;
}

// one refinement: child k of parent c is fine cell position(2^dim c + k); children[2^dim c + k] names it
Mesh refine(const Mesh &m, std::vector<uint32_t> &children, bool reversed)
{
  const int      nch = 1 << m.dim;
  const uint32_t nf  = (uint32_t)m.cells.size() * nch;
  Mesh           fine{m.dim, std::vector<Cell>(nf)};
  children.resize(nf);
  for (uint32_t c = 0; c < m.cells.size(); ++c)
    for (int k = 0; k < nch; ++k)
      {
        Cell child{};
        for (int v = 0; v < nch; ++v)
          {
            const int r[3] = {2 * ((k & 1) + (v & 1)), 2 * ((k >> 1 & 1) + (v >> 1 & 1)), 2 * ((k >> 2) + (v >> 2))};
            child[v]       = point_at(m, m.cells[c], r);
          }
        const uint32_t at = reversed ? nf - 1 - (nch * c + k) : nch * c + k;
        fine.cells[at]    = child;
        children[nch * c + k] = at;
      }
  return fine;
}

// The table of a mesh at degree p.  numbering: first DoF by entity midpoint, filled in the order of the first mesh it
// sees and shared by the meshes that follow (the same numbering under another cell order).  Entities without DoFs
// (p = 1) get garbage that looks like an index.
struct Numbering
{
  std::map<Point, uint32_t> base;
  uint32_t                  n_dofs = 0;
};
std::vector<uint32_t> table(const Mesh &m, int p, Numbering &num)
{
  const int             ne = n_entities(m.dim);
  std::vector<uint32_t> idx(ne * m.cells.size());
  for (size_t c = 0; c < m.cells.size(); ++c)
    for (int e = 0; e < ne; ++e)
      {
        const int  r[3] = {2 * (e % 3), 2 * (e / 3 % 3), 2 * (e / 9)};
        const auto it   = num.base.find(point_at(m, m.cells[c], r));
        if (entity_size(e, p) == 0)
          idx[ne * c + e] = (uint32_t)(7 * c + e);
        else if (it != num.base.end())
          idx[ne * c + e] = it->second;
        else
          {
            idx[ne * c + e] = num.base[point_at(m, m.cells[c], r)] = num.n_dofs;
            num.n_dofs += (uint32_t)entity_size(e, p);
          }
      }
  if (p == 1)
    for (uint32_t &v : idx)
      v = v < num.n_dofs ? v : v % num.n_dofs;
  return idx;
}

template <typename V>
void print(const std::string &name, const char *key, const V &v)
{
  std::printf("%s %s", name.c_str(), key);
  for (const auto a : v)
    std::printf(" %lu", (unsigned long)a);
  std::printf("\n");
}

// owner masks and colours of a table
void report(const std::string &name, int dim, const std::vector<uint32_t> &idx, uint32_t n_cells, uint32_t n_dofs, int p)
{
  const int ne = n_entities(dim);
  print(name, "meta", std::vector<uint32_t>{(uint32_t)dim, (uint32_t)ne, n_cells, n_dofs, (uint32_t)p});
  print(name, "idx", idx);
  bool out_of_range = false;
  print(name, "masks", first_owner_masks(idx.data(), ne, n_cells, n_dofs, p, &out_of_range));
  print(name, "out_of_range", std::vector<int>{out_of_range});
  const CellColouring col = colour_cells_greedy(idx.data(), ne, n_cells, n_dofs, p);
  print(name, "colours", std::vector<int>{col.more_than_32, col.n});
  print(name, "start", std::vector<uint32_t>(col.start, col.start + 33));
  print(name, "order", col.order);
}

// shifts of the children patches of `coarse` after one refinement
void report_shifts(const std::string &name, const Mesh &coarse, int p, bool reversed)
{
  std::vector<uint32_t> children;
  const Mesh            fine = refine(coarse, children, reversed);
  Numbering             num;
  const auto            idx = table(fine, p, num);
  print(name, "meta", std::vector<uint32_t>{(uint32_t)coarse.dim, (uint32_t)n_entities(coarse.dim), (uint32_t)fine.cells.size(),
                                            num.n_dofs, (uint32_t)p, (uint32_t)coarse.cells.size()});
  print(name, "idx", idx);
  print(name, "children", children);
  const PatchShifts s = patch_multiplicity_shifts(coarse.dim, children.data(), idx.data(), (uint32_t)coarse.cells.size(), num.n_dofs);
  print(name, "shift", s.shift);
  print(name, "irregular", std::vector<int>{s.irregular});
}

// n quadrilaterals around the vertex with DoF 0, p = 1: neighbours share a spoke
void report_fan(const std::string &name, uint32_t n)
{
  std::vector<uint32_t> idx(9 * n);
  const uint32_t        n_dofs = 1 + 2 * n;
  for (uint32_t c = 0; c < n; ++c)
    for (int e = 0; e < 9; ++e)
      idx[9 * c + e] = e == 0 ? 0u : e == 2 ? 1 + c : e == 6 ? 1 + (c + 1) % n : e == 8 ? 1 + n + c : (5 * c + e) % n_dofs;
  report(name, 2, idx, n, n_dofs, 1);
}

// three cells around the vertex (2D) or the edge (3D) at the origin, spokes at 0, 120 and 240 degrees in a lattice
Mesh three_around(int dim)
{
  const long spoke[3][2] = {{2, 0}, {-1, 2}, {-1, -2}}, corner[3][2] = {{1, 2}, {-2, 0}, {1, -2}};
  Mesh       m{dim, {}};
  for (int i = 0; i < 3; ++i)
    {
      const int j = (i + 1) % 3;
      Cell      c{};
      for (int z = 0; z < (dim == 3 ? 2 : 1); ++z)
        {
          c[4 * z + 0] = {0, 0, kScale * z};
          c[4 * z + 1] = {kScale * spoke[i][0], kScale * spoke[i][1], kScale * z};
          c[4 * z + 2] = {kScale * spoke[j][0], kScale * spoke[j][1], kScale * z};
          c[4 * z + 3] = {kScale * corner[i][0], kScale * corner[i][1], kScale * z};
        }
      m.cells.push_back(c);
    }
  return m;
}

int main()
{
  const int boxes[6][4] = {{2, 1, 1, 1}, {2, 3, 2, 1}, {2, 4, 4, 1}, {3, 1, 1, 1}, {3, 3, 2, 1}, {3, 2, 2, 2}};
  for (const auto &b : boxes)
    for (int p = 1; p <= 3; ++p)
      {
        const int   dim = b[0];
        const Mesh  lex = box(dim, b + 1), mor = morton(lex);
        Numbering   num;
        const auto  idx_lex = table(lex, p, num), idx_mor = table(mor, p, num);
        std::string name = "box" + std::to_string(dim) + "d-" + std::to_string(b[1]) + "x" + std::to_string(b[2]) +
                           (dim == 3 ? "x" + std::to_string(b[3]) : "") + "-p" + std::to_string(p);
        report(name + "-lex", dim, idx_lex, (uint32_t)lex.cells.size(), num.n_dofs, p);
        report(name + "-morton", dim, idx_mor, (uint32_t)mor.cells.size(), num.n_dofs, p);
        if (p == 2 && (b[1] == 4 || b[3] == 2)) // as idx27 carries them: the entities on the boundary of the box constrained
          {
            std::vector<uint32_t> con = idx_mor;
            const int             ne  = n_entities(dim);
            for (size_t c = 0; c < mor.cells.size(); ++c)
              for (int e = 0; e < ne; ++e)
                {
                  const int   r[3] = {2 * (e % 3), 2 * (e / 3 % 3), 2 * (e / 9)};
                  const Point x    = point_at(mor, mor.cells[c], r);
                  for (int d = 0; d < dim; ++d)
                    if (x[d] == 0 || x[d] == kScale * b[1 + d])
                      con[ne * c + e] = 0xFFFFFFFFu;
                }
            report(name + "-constrained", dim, con, (uint32_t)mor.cells.size(), num.n_dofs, p);
          }
      }
  report_fan("fan-32", 32);
  report_fan("fan-33", 33);
  for (int dim = 2; dim <= 3; ++dim)
    {
      const int n[3] = {3, 2, 1};
      for (int p = 1; p <= 3; ++p)
        {
          report_shifts("refined-box" + std::to_string(dim) + "d-p" + std::to_string(p), box(dim, n), p, false);
          report_shifts("refined-box" + std::to_string(dim) + "d-reversed-p" + std::to_string(p), box(dim, n), p, true);
        }
      report_shifts("three-around-" + std::to_string(dim) + "d", three_around(dim), 2, false);
    }
  std::printf("done done 1\n");
  return 0;
}
