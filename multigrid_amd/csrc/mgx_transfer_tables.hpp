// mgx_transfer_tables.hpp -- the assembly and transfer tables of a hexahedral FE_Q level pair (the ordered assembly also
// for quadrilaterals), from host arrays to std::vectors: what mgx_operator_create and mgx_transfer_create (mgx_api.cpp)
// upload after they have downloaded the tables, and before they decide what a verdict means.  Host only, standard C++,
// addressed through the node and row rules of mgx_index_tables.hpp; tests/index_tables_check.cpp runs these on their own.
#pragma once

#include "mgx_index_tables.hpp"

#include <cmath>

namespace mgx
{
  // rows of numbers: row r is pos[start[r] .. start[r + 1])
  struct IndexRows
  {
    std::vector<uint32_t> start, pos;
  };

  // Ordered assembly: for every DoF the positions (cell (p+1)^dim + local index) of its contributions in ascending cell
  // order; constrained entities contribute nothing.  pos carries one entry of padding.
  inline IndexRows ordered_assembly(const uint32_t *idx, int dim, uint32_t n_cells, uint32_t n_dofs, int p)
  {
    const int      ne = n_entities(dim);
    const uint32_t nl = (uint32_t)n_local_values(dim, p);
    auto           for_each_local = [&](auto &&f) {
      for (uint32_t c = 0; c < n_cells; ++c)
        for_each_cell_dof(idx + ne * (size_t)c, dim, p, [&](int l, uint32_t dof) {
          if (dof != kInvalidIndex)
            f(dof, c * nl + (uint32_t)l);
        });
    };
    IndexRows out;
    out.start.assign((size_t)n_dofs + 1, 0);
    for_each_local([&](uint32_t dof, uint32_t) { ++out.start[dof + 1]; });
    for (size_t i = 0; i < n_dofs; ++i)
      out.start[i + 1] += out.start[i];
    out.pos.resize(out.start.back() + 1);
    std::vector<uint32_t> fill(out.start.begin(), out.start.end() - 1);
    for_each_local([&](uint32_t dof, uint32_t l) { out.pos[fill[dof]++] = l; });
    return out;
  }

  // Cells of a brick level in lists whose cells share no DoF: brick colour by brick colour (order[colour_start[g] ..
  // colour_start[g + 1]) are the bricks of colour g, which share no DoF); inside a brick the cells with the same position
  // m mod 8 in Morton order -- the same child of every parent -- do not touch.  8 lists per colour, their cells in pos.
  inline IndexRows brick_cell_lists(const uint32_t *order, const uint32_t *colour_start, int n_colours, uint32_t cells_per_brick)
  {
    IndexRows out;
    out.start.assign(1, 0);
    out.pos.reserve((size_t)colour_start[n_colours] * cells_per_brick);
    for (int g = 0; g < n_colours; ++g)
      for (uint32_t q = 0; q < 8; ++q)
        {
          for (uint32_t pos = colour_start[g]; pos < colour_start[g + 1]; ++pos)
            for (uint32_t m = q; m < cells_per_brick; m += 8)
              out.pos.push_back(order[pos] * cells_per_brick + m);
          out.start.push_back((uint32_t)out.pos.size());
        }
    return out;
  }

  // The (2 m + 1)^3 entities of a block of m^3 cells by the row rule: f(cell, entity of that cell, first) for every view
  // of entity e, z slowest, the cell as the z y x digits base m of its position in the block.
  template <typename F>
  inline void for_each_block_view(int m, int e, F &&f)
  {
    const int      L = 2 * m + 1;
    const RowViews x = row_layer_views(e % L, m), y = row_layer_views(e / L % L, m), z = row_layer_views(e / (L * L), m);
    bool           first = true;
    for (int oz = 0; oz < z.n; ++oz)
      for (int oy = 0; oy < y.n; ++oy)
        for (int ox = 0; ox < x.n; ++ox, first = false)
          f((z.cell[oz] * m + y.cell[oy]) * m + x.cell[ox], (z.code[oz] * 3 + y.code[oy]) * 3 + x.code[ox], first);
  }

  // Patch table of the pipelined transfer kernels (mgx_transfer.hip): the 5^3 entities of the children patch of every
  // parent, one word each: first fine DoF | weight shift << 29 | owner bit << 31, 0 for an entity without DoFs.  shift:
  // patch_multiplicity_shifts; own: first_owner_masks of the fine level.  owner_weights: the shift field says who
  // restricts the entity, 0 = this parent (it owns it, and no lower rank holds it: foreign, per fine DoF or null),
  // 1 = another one.  consistent: the children share the entities of the parent's mid planes.
  struct PatchTable
  {
    std::vector<uint32_t> words;
    bool                  consistent = true;
  };
  inline PatchTable patch_table(const uint32_t *children, const uint32_t *idx_fine, const uint32_t *own, const uint8_t *shift,
                                uint32_t n_parents, int p, bool owner_weights, const uint8_t *foreign)
  {
    // what is the same for every parent: the views of the 125 entities, whether they carry DoFs, and the entity of the
    // parent they lie in (the node rule on the 5 layers)
    struct Entity
    {
      int  n = 0, child[8], code[8], cls;
      bool empty;
    } ent[125];
    for (int e = 0; e < 125; ++e)
      {
        const int el[3] = {e % 5, (e / 5) % 5, e / 25};
        ent[e].empty    = row_layer_size(el[0], p) * row_layer_size(el[1], p) * row_layer_size(el[2], p) == 0;
        ent[e].cls      = (node_entity(el[2], 4).code * 3 + node_entity(el[1], 4).code) * 3 + node_entity(el[0], 4).code;
        for_each_block_view(2, e, [&](int ch, int ce, bool) {
          ent[e].child[ent[e].n]  = ch;
          ent[e].code[ent[e].n++] = ce;
        });
      }
    PatchTable out;
    out.words.resize(125 * (size_t)n_parents);
    bool consistent = true;
#pragma omp parallel for schedule(static) reduction(&& : consistent)
    for (uint32_t pc = 0; pc < n_parents; ++pc)
      for (int e = 0; e < 125; ++e)
        {
          const Entity &E     = ent[e];
          uint32_t      base  = 0;
          bool          owned = false;
          for (int v = 0; v < E.n; ++v)
            {
              const uint32_t fc = children[8 * (size_t)pc + E.child[v]];
              const uint32_t b  = idx_fine[27 * (size_t)fc + E.code[v]];
              if (v == 0)
                base = b;
              else if (b != base)
                consistent = false;
              owned = owned || ((own[fc] >> E.code[v]) & 1u);
            }
          uint32_t sh = shift[27 * (size_t)pc + E.cls];
          if (owner_weights)
            sh = (owned && !E.empty && (!foreign || !foreign[base])) ? 0u : 1u;
          out.words[125 * (size_t)pc + e] = E.empty ? 0u : (base | (sh << 29) | ((owned ? 1u : 0u) << 31));
        }
    out.consistent = consistent;
    return out;
  }

  // Colouring of the cells by index mod 8 (the parity colouring of a Morton-ordered mesh): valid if no two cells of one
  // colour share a mesh entity that carries DoFs (idx: the unconstrained table)
  inline bool coloured_by_index_mod_8(const uint32_t *idx, uint32_t n_cells, uint32_t n_dofs, int p)
  {
    std::vector<uint8_t> mask(n_dofs, 0);
    for (uint32_t c = 0; c < n_cells; ++c)
      for (int e = 0; e < 27; ++e)
        {
          if (entity_size(e, p) == 0 || e == 13)
            continue;
          uint8_t      &m   = mask[idx[27 * (size_t)c + e]];
          const uint8_t bit = (uint8_t)(1u << (c & 7u));
          if (m & bit)
            return false;
          m |= bit;
        }
    return true;
  }

  // forest order: cell c is child c % 8 of parent c / 8
  inline bool children_in_forest_order(const uint32_t *children, size_t n)
  {
    for (size_t i = 0; i < n; ++i)
      if (children[i] != (uint32_t)i)
        return false;
    return true;
  }

  // Block table of the fused residual + restriction and prolongation: per brick, in the order of the schedule
  // (brick_order[sb] = brick in cell order, whose parents are PB^3 b ...), the (2 PB + 1)^3 coarse entities of its PB^3
  // sibling parents: their entries of the coarse table idx.  Empty if two parents do not agree on a shared entity in the
  // unconstrained table idx_plain.
  inline std::vector<uint32_t> coarse_block_table(const uint32_t *idx, const uint32_t *idx_plain, const uint32_t *brick_order,
                                                  uint32_t n_bricks, int PB)
  {
    const int             CE1 = 2 * PB + 1, CE3 = CE1 * CE1 * CE1, ppb = PB * PB * PB;
    std::vector<uint32_t> tab((size_t)n_bricks * CE3);
    bool                  consistent = true;
    for (uint32_t sb = 0; sb < n_bricks; ++sb)
      for (int e = 0; e < CE3; ++e)
        {
          uint32_t key = 0;
          for_each_block_view(PB, e, [&](int q, int ce, bool first) {
            const size_t at = 27 * ((size_t)ppb * brick_order[sb] + (size_t)q) + ce;
            if (first)
              {
                tab[(size_t)sb * CE3 + e] = idx[at];
                key                       = idx_plain[at];
              }
            else if (idx_plain[at] != key)
              consistent = false;
          });
        }
    if (!consistent)
      tab.clear();
    return tab;
  }

  // Scratch form of the fused residual + restriction: every brick stores its (PB p + 1)^3 restricted values in a block of
  // its own; per coarse DoF its positions in the blocks, ascending = in brick order: the order of the sums.
  inline IndexRows block_assembly(const uint32_t *tab, uint32_t n_bricks, int PB, int p, uint32_t n_coarse_dofs)
  {
    const int             CE1 = 2 * PB + 1, CE3 = CE1 * CE1 * CE1;
    const uint64_t        CN = (uint64_t)PB * p + 1, NC = CN * CN * CN;
    std::vector<uint32_t> dof((size_t)n_bricks * NC, kInvalidIndex);
    std::vector<NodeEntity> at(CN); // layer, offset and length of the points of a row: the same for every brick
    for (uint32_t a = 0; a < CN; ++a)
      at[a] = row_point_layer((int)a, p);
#pragma omp parallel for schedule(static)
    for (uint32_t sb = 0; sb < n_bricks; ++sb)
      for (uint32_t l = 0; l < NC; ++l)
        {
          const NodeEntity &x = at[l % CN], &y = at[(l / CN) % CN], &z = at[l / (CN * CN)];
          dof[(size_t)sb * NC + l] = entity_dof(tab[(size_t)sb * CE3 + (size_t)((z.code * CE1 + y.code) * CE1 + x.code)], x, y, z);
        }
    IndexRows out;
    out.start.assign((size_t)n_coarse_dofs + 1, 0);
    for (uint32_t d : dof)
      if (d != kInvalidIndex)
        out.start[d + 1]++;
    for (uint32_t d = 0; d < n_coarse_dofs; ++d)
      out.start[d + 1] += out.start[d];
    out.pos.resize(out.start[n_coarse_dofs]);
    std::vector<uint32_t> fill(out.start.begin(), out.start.end() - 1);
    for (size_t k = 0; k < dof.size(); ++k)
      if (dof[k] != kInvalidIndex)
        out.pos[fill[dof[k]]++] = (uint32_t)k;
    return out;
  }

  // Rows of P and of R = P^T for the fine DoFs `shared` on a rank interface.  P is interpolatory: a fine DoF on a shared
  // mesh entity couples to coarse DoFs of that entity only, so the first parent found holds its whole row.  Weights:
  // products of three entries of prolong_1d [2 p + 1][p + 1], dropped below 1e-14.  P (p_*): CSR over the shared list,
  // coarse DoF and weight.  R (r_*): CSR over the coarse DoFs r_cdof that have a row, fine DoF and weight, over the fine
  // DoFs that are not in not_owned (a lower rank restricts those; the coarse sums are added over the ranks).
  // idx_fine, idx_coarse: the constrained tables.  uncovered: a shared DoF lies in no cell; no rows then.
  struct InterfaceRows
  {
    bool                  uncovered = false;
    size_t                n_entries = 0;
    std::vector<uint32_t> p_start, p_cdof, r_cdof, r_start, r_fdof;
    std::vector<double>   p_w, r_w;
  };
  inline InterfaceRows interface_rows(const uint32_t *children, const uint32_t *idx_fine, const uint32_t *idx_coarse,
                                      uint32_t n_parents, uint32_t n_dofs_fine, const uint32_t *shared, uint32_t n_shared,
                                      const uint32_t *not_owned, size_t n_not_owned, const double *prolong_1d, int p)
  {
    const int             n = p + 1;
    std::vector<uint32_t> pos(n_dofs_fine, kInvalidIndex);
    for (uint32_t i = 0; i < n_shared; ++i)
      pos[shared[i]] = i;
    std::vector<uint8_t> foreign(n_shared, 0), done(n_shared, 0);
    for (size_t i = 0; i < n_not_owned; ++i)
      if (pos[not_owned[i]] != kInvalidIndex)
        foreign[pos[not_owned[i]]] = 1;
    struct Entry
    {
      uint32_t si, cdof;
      double   w;
    };
    std::vector<Entry> ent;
    for (uint32_t pc = 0; pc < n_parents; ++pc)
      for (int ch = 0; ch < 8; ++ch)
        {
          const uint32_t *indf = idx_fine + 27 * (size_t)children[8 * (size_t)pc + ch];
          bool            any  = false;
          for (int e = 0; e < 27 && !any; ++e)
            any = indf[e] != kInvalidIndex && indf[e] < n_dofs_fine && pos[indf[e]] != kInvalidIndex && entity_size(e, p) != 0;
          if (!any)
            continue;
          for_each_cell_dof(indf, 3, p, [&](int l, uint32_t d) {
            if (d == kInvalidIndex || pos[d] == kInvalidIndex || done[pos[d]])
              return;
            const uint32_t si = pos[d];
            done[si]          = 1;
            const int F[3]    = {(ch & 1) * p + l % n, ((ch >> 1) & 1) * p + l / n % n, ((ch >> 2) & 1) * p + l / (n * n)};
            for (int az = 0; az < n; ++az)
              for (int ay = 0; ay < n; ++ay)
                for (int ax = 0; ax < n; ++ax)
                  {
                    const double w = prolong_1d[F[0] * n + ax] * prolong_1d[F[1] * n + ay] * prolong_1d[F[2] * n + az];
                    if (std::fabs(w) < 1e-14)
                      continue;
                    const uint32_t c = cell_dof(idx_coarse + 27 * (size_t)pc, 3, p, ax, ay, az);
                    if (c != kInvalidIndex)
                      ent.push_back({si, c, w});
                  }
          });
        }
    InterfaceRows out;
    out.n_entries = ent.size();
    for (uint32_t i = 0; i < n_shared; ++i)
      out.uncovered |= !done[i];
    if (out.uncovered)
      return out;
    // prolongation: rows in the order of the shared list
    std::stable_sort(ent.begin(), ent.end(), [](const Entry &a, const Entry &b) { return a.si < b.si; });
    out.p_start.assign((size_t)n_shared + 1, 0);
    out.p_cdof.reserve(ent.size());
    out.p_w.reserve(ent.size());
    for (const Entry &e : ent)
      {
        out.p_start[e.si + 1]++;
        out.p_cdof.push_back(e.cdof);
        out.p_w.push_back(e.w);
      }
    for (uint32_t i = 0; i < n_shared; ++i)
      out.p_start[i + 1] += out.p_start[i];
    // restriction: rows by coarse DoF, only the fine DoFs this rank owns
    std::vector<Entry> own;
    for (const Entry &e : ent)
      if (!foreign[e.si])
        own.push_back(e);
    std::stable_sort(own.begin(), own.end(), [](const Entry &a, const Entry &b) { return a.cdof < b.cdof; });
    for (size_t k = 0; k < own.size(); ++k)
      {
        if (k == 0 || own[k].cdof != own[k - 1].cdof)
          {
            out.r_cdof.push_back(own[k].cdof);
            out.r_start.push_back((uint32_t)k);
          }
        out.r_fdof.push_back(shared[own[k].si]);
        out.r_w.push_back(own[k].w);
      }
    out.r_start.push_back((uint32_t)own.size());
    return out;
  }
} // namespace mgx
