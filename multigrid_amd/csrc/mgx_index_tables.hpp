// mgx_index_tables.hpp -- what the set-up code derives from the compressed index table of an FE_Q level, for hexahedra
// and quadrilaterals alike: which DoF a node of a cell is (the node rule) and how the cells of a row share their entity
// layers (the row rule), which cell owns an entity, colours of cells that share no DoF, multiplicities of the entities of
// a children patch.  Host only, standard C++: no HIP, no status plumbing -- the callers (mgx_api.cpp, mgx_dg_api.cpp,
// the mesh providers, mgx_transfer_tables.hpp) decide what a result means; tests/index_tables_check.cpp, a program of
// its own built with AddressSanitizer and UBSan, runs all of these, and tests/test_index_tables_host.py checks what it
// prints against a numpy restatement (the owner weights of the 2D restriction: tests/ball_owner_weights_check.cpp, on the
// tables of the disc).
//
// A table holds ne = 3^dim entries per cell, the first DoF of mesh entity e = (cz 3 + cy) 3 + cx (two dimensions:
// cy 3 + cx) with the codes 0 low side, 1 inside, 2 high side per direction.  That first DoF identifies the entity.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgx
{
  // DoFs on mesh entity e of a cell of degree p (vertex 1, line p - 1, face (p - 1)^2, interior (p - 1)^3); holds as it
  // stands for the 9 entities of a quadrilateral
  inline int entity_size(int e, int p)
  {
    return (e % 3 == 1 ? p - 1 : 1) * ((e / 3) % 3 == 1 ? p - 1 : 1) * (e / 9 == 1 ? p - 1 : 1);
  }
  // what depends on the dimension of a level: entities per cell, the cell's interior among them, local values per cell
  inline int    n_entities(int dim) { return dim == 2 ? 9 : 27; }
  inline int    interior_entity(int dim) { return dim == 2 ? 4 : 13; }
  inline size_t n_local_values(int dim, int p) { return dim == 2 ? (size_t)(p + 1) * (p + 1) : (size_t)(p + 1) * (p + 1) * (p + 1); }

  constexpr uint32_t kInvalidIndex = 0xFFFFFFFFu; // entry of a constrained entity (MGX_INVALID_INDEX of mgx.h)

  // THE NODE RULE (read_dof_values_compressed, vector_access_reduced.h:153-247).  Node a of 0..p on a line lies on the
  // entity with code 0 / 1 / 2 at offset a - 1 (else 0) of its len = p - 1 (else 1) nodes; the DoF of node (i, j, k) of
  // a cell is the first DoF of its entity + its lexicographic position in the entity.
  struct NodeEntity
  {
    int code, off, len;
  };
  inline NodeEntity node_entity(int a, int p)
  {
    const int code = a == 0 ? 0 : (a == p ? 2 : 1);
    return {code, code == 1 ? a - 1 : 0, code == 1 ? p - 1 : 1};
  }
  // ... through entry `base` of an entity; holds for any table of first DoFs whose entities are products of lines
  inline uint32_t entity_dof(uint32_t base, const NodeEntity &x, const NodeEntity &y, const NodeEntity &z)
  {
    return base == kInvalidIndex ? base : base + (uint32_t)((z.off * y.len + y.off) * x.len + x.off);
  }
  // ... through the 9 or 27 entries ix of a cell; kInvalidIndex where the entity's entry is
  inline uint32_t cell_dof(const uint32_t *ix, int dim, int p, int i, int j, int k = 0)
  {
    const NodeEntity x = node_entity(i, p), y = node_entity(j, p), z = dim == 2 ? NodeEntity{0, 0, 1} : node_entity(k, p);
    return entity_dof(ix[(z.code * 3 + y.code) * 3 + x.code], x, y, z);
  }
  // f(local index, cell_dof) for the (p + 1)^dim nodes of a cell in lexicographic order, line by line
  template <typename F>
  inline void for_each_cell_dof(const uint32_t *ix, int dim, int p, F &&f)
  {
    const int n = p + 1;
    for (int k = 0, l = 0; k < (dim == 2 ? 1 : n); ++k)
      for (int j = 0; j < n; ++j)
        {
          const NodeEntity y = node_entity(j, p), z = dim == 2 ? NodeEntity{0, 0, 1} : node_entity(k, p);
          const uint32_t  *e = ix + 3 * (3 * z.code + y.code);
          for (int i = 0; i < n; ++i, ++l)
            {
              const NodeEntity x = node_entity(i, p);
              f(l, entity_dof(e[x.code], x, y, z));
            }
        }
  }

  // THE ROW RULE: m cells in a row have 2 m + 1 entity layers and m p + 1 points.  Layer l is seen from cell
  // (l - 1) / 2 with code l - 2 cell (layer 0: code 0 of cell 0), and an even inner layer from the next cell as well,
  // with code 0; it carries p - 1 points if odd, else one.
  struct RowViews
  {
    int n, cell[2], code[2];
  };
  inline RowViews row_layer_views(int l, int m)
  {
    const int cell = l == 0 ? 0 : (l - 1) / 2;
    return {(l % 2 == 0 && l > 0 && l < 2 * m) ? 2 : 1, {cell, cell + 1}, {l - 2 * cell, 0}};
  }
  inline int row_layer_size(int l, int p) { return l % 2 == 1 ? p - 1 : 1; }
  // point a of the m p + 1: code = its layer, offset and length as for a node
  inline NodeEntity row_point_layer(int a, int p)
  {
    const NodeEntity e = node_entity(a % p, p); // (a % p is never p: codes 0 and 1)
    return {2 * (a / p) + e.code, e.off, e.len};
  }

  // Bit e of cell c is set iff c is the first cell in cell order that contains entity e, over the entities that carry
  // DoFs at degree p: the one writer of the entity's DoFs.  An entry that is not below n_dofs owns nothing and sets
  // *out_of_range (the unconstrained table an operator was created from holds none).
  inline std::vector<uint32_t> first_owner_masks(const uint32_t *idx, int ne, uint32_t n_cells, uint32_t n_dofs, int p,
                                                 bool *out_of_range = nullptr)
  {
    std::vector<uint32_t> own(n_cells, 0u);
    std::vector<uint8_t>  seen(n_dofs, 0);
    for (uint32_t c = 0; c < n_cells; ++c)
      for (int e = 0; e < ne; ++e)
        {
          const uint32_t base = idx[(size_t)ne * c + e];
          if (entity_size(e, p) == 0)
            continue;
          if (base >= n_dofs && out_of_range)
            *out_of_range = true;
          if (base < n_dofs && !seen[base])
            {
              seen[base] = 1;
              own[c] |= 1u << e;
            }
        }
    return own;
  }

  // Greedy colouring of the cells in their order: two cells conflict when they share an entity, and an entity counts
  // when it carries DoFs at degree p and its entry is below n_dofs (a constrained entity's is not).  Colour k is
  // order[start[k] .. start[k + 1]), cells ascending.  On a structured mesh these are the 2^dim parity classes.
  struct CellColouring
  {
    bool                  more_than_32 = false; // no colouring: n is 0, order empty
    int                   n            = 0;
    uint32_t              start[33]    = {0};
    std::vector<uint32_t> order;
  };
  inline CellColouring colour_cells_greedy(const uint32_t *idx, int ne, uint32_t n_cells, uint32_t n_dofs, int p)
  {
    CellColouring         out;
    std::vector<uint32_t> used(n_dofs, 0u); // per entity: the colours of the cells that hold it
    std::vector<uint8_t>  colour(n_cells, 0);
    for (uint32_t c = 0; c < n_cells; ++c)
      {
        const uint32_t *ix = idx + (size_t)ne * c;
        uint32_t        key[27], mask = 0;
        int             n_keys = 0, col = 0;
        for (int e = 0; e < ne; ++e)
          if (entity_size(e, p) != 0 && ix[e] < n_dofs)
            {
              key[n_keys++] = ix[e];
              mask |= used[ix[e]];
            }
        while (col < 32 && (mask >> col) & 1u)
          ++col;
        if (col == 32)
          {
            out              = CellColouring();
            out.more_than_32 = true;
            return out;
          }
        colour[c] = (uint8_t)col;
        ++out.start[col + 1]; // (counts first, offsets below)
        out.n = std::max(out.n, col + 1);
        for (int k = 0; k < n_keys; ++k)
          used[key[k]] |= 1u << col;
      }
    for (int k = 0; k < out.n; ++k)
      out.start[k + 1] += out.start[k];
    std::vector<uint32_t> fill(out.start, out.start + 32);
    out.order.resize(n_cells);
    for (uint32_t c = 0; c < n_cells; ++c)
      out.order[fill[colour[c]]++] = c;
    return out;
  }

  // Multiplicities of the 3^dim entities of the children patch of every parent (dim 2 or 3; children [n_parents][2^dim],
  // idx_fine the fine level's unconstrained table): shift[ne parent + e] = log2 of the number of parents whose patch
  // contains entity e, the restriction weight 2^-shift.  Counted at a child vertex that lies in the entity -- low side:
  // the low vertex of child 0, inside: the mid plane = its high vertex, high side: the high vertex of child 1 --
  // since a vertex carries one DoF at every degree.  irregular: some count is no power of two <= 2^dim (three or five
  // cells around a vertex, three blocks around an edge) or some vertex entry no DoF; shift holds no weight there.
  struct PatchShifts
  {
    std::vector<uint8_t> shift;
    bool                 irregular = false;
  };
  inline PatchShifts patch_multiplicity_shifts(int dim, const uint32_t *children, const uint32_t *idx_fine, uint32_t n_parents,
                                               uint32_t n_dofs_fine)
  {
    const int             ne = n_entities(dim);
    std::vector<uint32_t> rep((size_t)ne * n_parents); // the representative vertex of every patch entity
    for (size_t i = 0; i < rep.size(); ++i)
      {
        int child = 0, vertex = 0;
        for (int d = 0, code = (int)(i % ne), stride = 1; d < dim; ++d, code /= 3, stride *= 3)
          {
            child |= (code % 3 == 2) << d;
            vertex += code % 3 ? 2 * stride : 0;
          }
        rep[i] = idx_fine[(size_t)ne * children[((i / ne) << dim) + child] + vertex];
      }
    std::vector<uint8_t> cnt(n_dofs_fine, 0); // (saturating: 255 is irregular like every count above 2^dim)
    for (const uint32_t v : rep)
      if (v < n_dofs_fine && cnt[v] < 255)
        ++cnt[v];
    PatchShifts out;
    out.shift.assign(rep.size(), 0);
    for (size_t i = 0; i < rep.size(); ++i)
      {
        const int c = rep[i] < n_dofs_fine ? cnt[rep[i]] : 0;
        int       s = 0;
        while ((1 << s) < c && s < dim)
          ++s;
        out.irregular |= (1 << s) != c;
        out.shift[i] = (uint8_t)s;
      }
    return out;
  }

  // Owner weights of the restriction in two dimensions, where patch_multiplicity_shifts says irregular (three or five
  // cells around a vertex): byte[9 parent + e] = 0 (weight 1) if a child of the parent is the first owner (own:
  // first_owner_masks of the fine level) of the fine entities that lie in entity e of the parent, else kWeightZero2D
  // (weight 0: the parent that holds the owner restricts them).  The children patch has 5 x 5 fine entities by the row
  // rule; those in one entity of the parent have the same parents, so one byte per parent entity does.  consistent: the
  // fine entities (with DoFs at degree p) of every parent entity agree on whether the parent owns them -- the children
  // of a parent are consecutive in cell order wherever children are 4c .. 4c+3.
  constexpr uint8_t kWeightZero2D = 0xFF;
  struct OwnerWeights2D
  {
    std::vector<uint8_t> weight;
    bool                 consistent = true;
  };
  inline OwnerWeights2D patch_owner_weights_2d(const uint32_t *children, const uint32_t *own, uint32_t n_parents, int p)
  {
    OwnerWeights2D out;
    out.weight.assign(9 * (size_t)n_parents, kWeightZero2D);
    for (uint32_t pc = 0; pc < n_parents; ++pc)
      {
        int owned[9] = {0}, seen[9] = {0}; // fine entities with DoFs in a parent entity: those owned, all
        for (int ly = 0; ly < 5; ++ly)
          for (int lx = 0; lx < 5; ++lx)
            {
              if (row_layer_size(lx, p) * row_layer_size(ly, p) == 0)
                continue;
              const RowViews x = row_layer_views(lx, 2), y = row_layer_views(ly, 2);
              bool           o = false;
              for (int vy = 0; vy < y.n; ++vy)
                for (int vx = 0; vx < x.n; ++vx)
                  o = o || ((own[children[4 * (size_t)pc + 2 * y.cell[vy] + x.cell[vx]]] >> (3 * y.code[vy] + x.code[vx])) & 1u);
              const int e = 3 * node_entity(ly, 4).code + node_entity(lx, 4).code;
              owned[e] += o;
              ++seen[e];
            }
        for (int e = 0; e < 9; ++e)
          {
            out.consistent = out.consistent && (owned[e] == 0 || owned[e] == seen[e]);
            if (seen[e] == 0 || owned[e] == seen[e]) // (an entity without DoFs: its byte is never read)
              out.weight[9 * (size_t)pc + e] = 0;
          }
      }
    return out;
  }
} // namespace mgx
