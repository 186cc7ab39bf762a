// Runs the functions of multigrid_amd/csrc/mgx_index_tables.hpp and mgx_transfer_tables.hpp on small tables built here and
// prints tables and results as lines "<case> <key> <numbers>" for tests/test_index_tables_host.py, which restates the
// rules in numpy.  Built with AddressSanitizer and UBSan; no device, no library.
//
// A mesh is a list of cells with 2^dim integer corner points (multilinear cells); an entity is identified by its
// midpoint, so any conforming mesh gets a consistent table: structured boxes, three cells around a vertex or an edge.
#include "../multigrid_amd/csrc/mgx_transfer_tables.hpp"

#include <array>
#include <cstdio>
#include <cstring>
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
// (p = 1) get garbage that looks like an index, or (garbage = false) the number of the next entity: one per entity.
struct Numbering
{
  std::map<Point, uint32_t> base;
  uint32_t                  n_dofs = 0;
};
std::vector<uint32_t> table(const Mesh &m, int p, Numbering &num, bool garbage = true)
{
  const int             ne = n_entities(m.dim);
  std::vector<uint32_t> idx(ne * m.cells.size());
  for (size_t c = 0; c < m.cells.size(); ++c)
    for (int e = 0; e < ne; ++e)
      {
        const int  r[3] = {2 * (e % 3), 2 * (e / 3 % 3), 2 * (e / 9)};
        const auto it   = num.base.find(point_at(m, m.cells[c], r));
        if (entity_size(e, p) == 0 && garbage)
          idx[ne * c + e] = (uint32_t)(7 * c + e);
        else if (it != num.base.end())
          idx[ne * c + e] = it->second;
        else
          {
            idx[ne * c + e] = num.base[point_at(m, m.cells[c], r)] = num.n_dofs;
            num.n_dofs += (uint32_t)entity_size(e, p);
          }
      }
  if (p == 1 && garbage)
    for (uint32_t &v : idx)
      v = v < num.n_dofs ? v : v % num.n_dofs;
  return idx;
}

// as idx27 carries them: the entities on the boundary of the box [0, n]^dim constrained
std::vector<uint32_t> constrain_boundary(const Mesh &m, std::vector<uint32_t> idx, const int n[3])
{
  const int ne = n_entities(m.dim);
  for (size_t c = 0; c < m.cells.size(); ++c)
    for (int e = 0; e < ne; ++e)
      {
        const int   r[3] = {2 * (e % 3), 2 * (e / 3 % 3), 2 * (e / 9)};
        const Point x    = point_at(m, m.cells[c], r);
        for (int d = 0; d < m.dim; ++d)
          if (x[d] == 0 || x[d] == kScale * n[d])
            idx[ne * c + e] = 0xFFFFFFFFu;
      }
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
  const IndexRows a = ordered_assembly(idx.data(), dim, n_cells, n_dofs, p);
  print(name, "asm_start", a.start);
  print(name, "asm_pos", a.pos);
}

// doubles as their bit patterns
void print_bits(const std::string &name, const char *key, const std::vector<double> &v)
{
  std::printf("%s %s", name.c_str(), key);
  for (const double a : v)
    {
      long bits;
      std::memcpy(&bits, &a, sizeof bits);
      std::printf(" %ld", bits);
    }
  std::printf("\n");
}

// the node rule at degree p: entity of every node of a line, every node of a cell through a table with entry 1000 e
// (both ways to ask), in two and three dimensions; the row rule for m = 1, 2 cells
void report_rules(int p)
{
  const std::string name = "rules-p" + std::to_string(p);
  std::vector<int>  ent;
  for (int a = 0; a <= p; ++a)
    for (int v : {node_entity(a, p).code, node_entity(a, p).off, node_entity(a, p).len})
      ent.push_back(v);
  print(name, "entity", ent);
  uint32_t ix[27];
  for (int e = 0; e < 27; ++e)
    ix[e] = 1000u * e;
  ix[5] = ix[23] = kInvalidIndex;
  for (int dim = 2; dim <= 3; ++dim)
    {
      std::vector<uint32_t> asked, walked(n_local_values(dim, p));
      for (int k = 0; k < (dim == 3 ? p + 1 : 1); ++k)
        for (int j = 0; j <= p; ++j)
          for (int i = 0; i <= p; ++i)
            asked.push_back(dim == 3 ? cell_dof(ix, 3, p, i, j, k) : cell_dof(ix, 2, p, i, j));
      for_each_cell_dof(ix, dim, p, [&](int l, uint32_t dof) { walked.at(l) = dof; });
      print(name, dim == 3 ? "asked3" : "asked2", asked);
      print(name, dim == 3 ? "walked3" : "walked2", walked);
    }
  for (int m = 1; m <= 2; ++m)
    {
      std::vector<int> views, points;
      for (int l = 0; l <= 2 * m; ++l)
        {
          const RowViews v = row_layer_views(l, m);
          for (int x : {v.n, v.cell[0], v.code[0], v.cell[1], v.code[1], row_layer_size(l, p)})
            views.push_back(x);
        }
      for (int a = 0; a <= m * p; ++a)
        for (int x : {row_point_layer(a, p).code, row_point_layer(a, p).off, row_point_layer(a, p).len})
          points.push_back(x);
      print(name, m == 1 ? "views1" : "views2", views);
      print(name, m == 1 ? "points1" : "points2", points);
    }
}

// patch table of one refinement of `coarse`; tamper: child 1 of parent 0 names its interior where its face in the parent's
// mid plane should stand
void report_patch(const std::string &name, const Mesh &coarse, int p, bool reversed, bool owner_weights, bool tamper)
{
  std::vector<uint32_t> children;
  const Mesh            fine = refine(coarse, children, reversed);
  Numbering             num;
  auto                  idx = table(fine, p, num, false);
  const uint32_t        npar = (uint32_t)coarse.cells.size(), nf = (uint32_t)fine.cells.size();
  if (tamper)
    idx[27 * (size_t)children[1] + 12] = idx[27 * (size_t)children[1] + 13];
  const PatchShifts     s   = patch_multiplicity_shifts(3, children.data(), idx.data(), npar, num.n_dofs);
  const auto            own = first_owner_masks(idx.data(), 27, nf, num.n_dofs, p);
  std::vector<uint8_t>  foreign;
  if (owner_weights)
    for (uint32_t d = 0; d < num.n_dofs; ++d)
      foreign.push_back(d % 3 == 0);
  const PatchTable t = patch_table(children.data(), idx.data(), own.data(), s.shift.data(), npar, p, owner_weights,
                                   owner_weights ? foreign.data() : nullptr);
  print(name, "meta", std::vector<uint32_t>{3, 27, nf, num.n_dofs, (uint32_t)p, npar, owner_weights});
  print(name, "idx", idx);
  print(name, "children", children);
  print(name, "shift", s.shift);
  print(name, "own", own);
  print(name, "foreign", foreign);
  print(name, "patch", t.words);
  print(name, "consistent", std::vector<int>{t.consistent});
}

// 8 bricks of PB^3 parents (cb fine cells each) in a cube of 2 PB parents per direction, everything in Morton order: block
// table, its scratch CSR, the cell lists of the fine level (8 brick colours of one brick)
void report_bricks(const std::string &name, int p, int PB, const std::vector<uint32_t> &order)
{
  const int      n[3] = {2 * PB, 2 * PB, 2 * PB};
  const Mesh     coarse = morton(box(3, n));
  Numbering      num, num_fine;
  const auto     plain = table(coarse, p, num), idx = constrain_boundary(coarse, plain, n);
  const uint32_t nb = 8, cb = 8 * PB * PB * PB;
  std::vector<uint32_t> children;
  const Mesh     fine = refine(coarse, children, false);
  const auto     idx_fine = table(fine, p, num_fine);
  print(name, "meta", std::vector<uint32_t>{3, 27, (uint32_t)fine.cells.size(), num_fine.n_dofs, (uint32_t)p, (uint32_t)PB, nb,
                                            num.n_dofs, (uint32_t)coarse.cells.size()});
  print(name, "idx", idx_fine);
  print(name, "idx_coarse", idx);
  print(name, "idx_coarse_plain", plain);
  print(name, "brick_order", order);
  print(name, "forest", std::vector<int>{children_in_forest_order(children.data(), children.size())});
  const auto tab = coarse_block_table(idx.data(), plain.data(), order.data(), nb, PB);
  print(name, "blocks", tab);
  const IndexRows a = block_assembly(tab.data(), nb, PB, p, num.n_dofs);
  print(name, "cs_start", a.start);
  print(name, "cs_pos", a.pos);
  const uint32_t       colour_start[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
  const IndexRows l = brick_cell_lists(order.data(), colour_start, 8, cb);
  print(name, "lists", l.pos);
  print(name, "list_start", l.start);
}

// interface rows of a 2 x 1 x 1 mesh refined once: the shared DoFs are those of the plane between the two parents
void report_interface(const std::string &name, int p, bool constrained, bool half_foreign, bool lost_dof)
{
  const int             n[3] = {2, 1, 1};
  const Mesh            coarse = box(3, n);
  std::vector<uint32_t> children;
  const Mesh            fine = refine(coarse, children, false);
  Numbering             num, num_fine;
  auto                  idxc = table(coarse, p, num, false), idxf = table(fine, p, num_fine, false);
  std::vector<uint32_t> shared, not_owned;
  std::vector<uint8_t>  on_plane(num_fine.n_dofs + 1, 0);
  if (constrained) // (both meshes fill the same box)
    {
      idxc = constrain_boundary(coarse, idxc, n);
      idxf = constrain_boundary(fine, idxf, n);
    }
  for (size_t c = 0; c < fine.cells.size(); ++c)
    for (int e = 0; e < 27; ++e)
      {
        const int r[3] = {2 * (e % 3), 2 * (e / 3 % 3), 2 * (e / 9)};
        if (point_at(fine, fine.cells[c], r)[0] == kScale && idxf[27 * c + e] != kInvalidIndex)
          for (int t = 0; t < entity_size(e, p); ++t)
            on_plane[idxf[27 * c + e] + t] = 1;
      }
  on_plane[num_fine.n_dofs] = lost_dof; // a DoF that no cell holds
  for (uint32_t d = 0; d <= num_fine.n_dofs; ++d)
    if (on_plane[d])
      shared.push_back(d);
  if (half_foreign)
    {
      for (size_t i = 0; i < shared.size(); i += 2)
        not_owned.push_back(shared[i]);
      not_owned.push_back(0); // (not shared: a foreign DoF elsewhere changes nothing)
    }
  std::vector<double> P1((2 * p + 1) * (p + 1)); // Lagrange basis on the nodes j / p at the points a / 2p
  for (int a = 0; a <= 2 * p; ++a)
    for (int j = 0; j <= p; ++j)
      {
        double v = 1;
        for (int k = 0; k <= p; ++k)
          if (k != j)
            v *= ((double)a / (2 * p) - (double)k / p) / ((double)j / p - (double)k / p);
        P1[a * (p + 1) + j] = v;
      }
  const InterfaceRows rows = interface_rows(children.data(), idxf.data(), idxc.data(), 2, num_fine.n_dofs + 1, shared.data(),
                                            (uint32_t)shared.size(), not_owned.data(), not_owned.size(), P1.data(), p);
  print(name, "meta", std::vector<uint32_t>{3, 27, (uint32_t)fine.cells.size(), num_fine.n_dofs + 1, (uint32_t)p, 2, num.n_dofs});
  print(name, "idx", idxf);
  print(name, "idx_coarse", idxc);
  print(name, "children", children);
  print(name, "shared", shared);
  print(name, "not_owned", not_owned);
  print_bits(name, "P1", P1);
  print(name, "verdict", std::vector<size_t>{rows.uncovered, rows.n_entries});
  print(name, "p_start", rows.p_start);
  print(name, "p_cdof", rows.p_cdof);
  print_bits(name, "p_w", rows.p_w);
  print(name, "r_cdof", rows.r_cdof);
  print(name, "r_start", rows.r_start);
  print(name, "r_fdof", rows.r_fdof);
  print_bits(name, "r_w", rows.r_w);
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
        if (p == 2 && (b[1] == 4 || b[3] == 2))
          report(name + "-constrained", dim, constrain_boundary(mor, idx_mor, b + 1), (uint32_t)mor.cells.size(), num.n_dofs, p);
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
  for (int p = 1; p <= 9; ++p)
    report_rules(p);
  {
    const int n321[3] = {3, 2, 1}, n222[3] = {2, 2, 2}, n444[3] = {4, 4, 4};
    for (int p = 1; p <= 3; ++p)
      for (int variant = 0; variant < 4; ++variant) // children reversed (1), owner weights and a foreign mask (2)
        {
          const std::string tag = std::string(variant & 1 ? "-reversed" : "") + (variant & 2 ? "-owner" : "") + "-p" + std::to_string(p);
          report_patch("patch-3x2x1" + tag, box(3, n321), p, variant & 1, variant & 2, false);
          report_patch("patch-2x2x2" + tag, box(3, n222), p, variant & 1, variant & 2, false);
        }
    report_patch("patch-2x2x2-tampered-p2", box(3, n222), 2, false, false, true);
    // parents coloured by index mod 8: the parity classes in Morton order, neighbours in z in lexicographic order
    for (int p = 1; p <= 2; ++p)
      {
        const Mesh lex = box(3, n444), mor = morton(lex);
        Numbering  num;
        const auto idx_lex = table(lex, p, num), idx_mor = table(mor, p, num);
        for (const auto *idx : {&idx_lex, &idx_mor})
          {
            const std::string name = std::string("mod8-") + (idx == &idx_lex ? "lex" : "morton") + "-p" + std::to_string(p);
            print(name, "meta", std::vector<uint32_t>{3, 27, 64, num.n_dofs, (uint32_t)p});
            print(name, "idx", *idx);
            print(name, "coloured", std::vector<int>{coloured_by_index_mod_8(idx->data(), 64, num.n_dofs, p)});
          }
      }
  }
  for (int permuted = 0; permuted < 2; ++permuted)
    {
      const std::vector<uint32_t> order = permuted ? std::vector<uint32_t>{3, 0, 7, 1, 6, 2, 5, 4} : std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6, 7};
      report_bricks(std::string("bricks-4x4x4-p2") + (permuted ? "-permuted" : ""), 2, 2, order);
      report_bricks(std::string("bricks-2x2x2-p5") + (permuted ? "-permuted" : ""), 5, 1, order);
    }
  for (int p = 1; p <= 3; ++p)
    for (int variant = 0; variant < 4; ++variant) // boundary constrained (1), every other shared DoF foreign (2)
      report_interface(std::string("interface") + (variant & 1 ? "-constrained" : "") + (variant & 2 ? "-half" : "") + "-p" + std::to_string(p),
                       p, variant & 1, variant & 2, false);
  report_interface("interface-lost-p2", 2, false, false, true);
  std::printf("done done 1\n");
  return 0;
}
