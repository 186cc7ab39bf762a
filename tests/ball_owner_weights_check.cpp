// Runs the owner-weight rule of the two-dimensional restriction (multigrid_amd/csrc/mgx_index_tables.hpp:
// patch_multiplicity_shifts, first_owner_masks, patch_owner_weights_2d) on the tables of one level pair, read from the
// file named on the command line, and prints lines "<key> <numbers>" for tests/test_ball_reference_2d.py.  Built with
// AddressSanitizer and UBSan; no device, no library.
//
// Input: p n_parents n_fine_cells n_fine_dofs, then children [n_parents][4], then the fine level's unconstrained index
// table [n_fine_cells][9].
// Output: irregular, consistent, weight [n_parents][9] (0: weight 1, 255: weight 0), and, the table expanded to one weight
// per (parent, fine DoF of its children patch) by the node rule and summed per fine DoF: sum_min, sum_max, parents_max.
#include "../multigrid_amd/csrc/mgx_index_tables.hpp"

#include <cstdio>

using namespace mgx;

int main(int argc, char **argv)
{
  if (argc != 2)
    return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f)
    return 2;
  int      p;
  unsigned n_parents, n_cells, n_dofs;
  if (std::fscanf(f, "%d %u %u %u", &p, &n_parents, &n_cells, &n_dofs) != 4)
    return 2;
  std::vector<uint32_t> children(4 * (size_t)n_parents), idx(9 * (size_t)n_cells);
  for (uint32_t &v : children)
    if (std::fscanf(f, "%u", &v) != 1 || v >= n_cells)
      return 2;
  for (uint32_t &v : idx)
    if (std::fscanf(f, "%u", &v) != 1)
      return 2;
  std::fclose(f);

  const PatchShifts           counted = patch_multiplicity_shifts(2, children.data(), idx.data(), n_parents, n_dofs);
  const std::vector<uint32_t> own     = first_owner_masks(idx.data(), 9, n_cells, n_dofs, p);
  const OwnerWeights2D        w       = patch_owner_weights_2d(children.data(), own.data(), n_parents, p);
  std::printf("irregular %d\nconsistent %d\nweight", counted.irregular ? 1 : 0, w.consistent ? 1 : 0);
  for (const uint8_t b : w.weight)
    std::printf(" %d", (int)b);
  std::printf("\n");

  // one weight per (parent, point of its children patch): the byte of the parent entity the point lies in -- what the
  // restriction kernel reads --, summed over the parents of every fine DoF
  const int             m = 2 * p + 1;
  std::vector<double>   sum(n_dofs, 0.);
  std::vector<uint32_t> parents(n_dofs, 0);
  for (uint32_t pc = 0; pc < n_parents; ++pc)
    for (int b = 0; b < m; ++b)
      for (int a = 0; a < m; ++a)
        {
          const int      cy = b > p, cx = a > p; // (a point on a mid line: seen from child 0)
          const uint32_t d  = cell_dof(&idx[9 * (size_t)children[4 * (size_t)pc + 2 * cy + cx]], 2, p, a - cx * p, b - cy * p);
          if (d >= n_dofs)
            return 3;
          const uint8_t byte = w.weight[9 * (size_t)pc + 3 * node_entity(b, 2 * p).code + node_entity(a, 2 * p).code];
          if (byte != 0 && byte != kWeightZero2D)
            return 3;
          sum[d] += byte == 0 ? 1. : 0.;
          ++parents[d];
        }
  double   lo = sum[0], hi = sum[0];
  uint32_t most = 0;
  for (uint32_t d = 0; d < n_dofs; ++d)
    {
      lo   = std::min(lo, sum[d]);
      hi   = std::max(hi, sum[d]);
      most = std::max(most, parents[d]);
    }
  std::printf("sum_min %.17g\nsum_max %.17g\nparents_max %u\ndone 1\n", lo, hi, most);
  return 0;
}
