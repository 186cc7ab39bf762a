// mgx_dg_transfer.hip -- level transfer between two DG spaces of the same basis in d = 2 or 3 dimensions, over one step
// of a level hierarchy.  One kernel template on the lengths NC < NF of a coarse and a fine 1D line and on the dimension;
// written out for d = 3:
//
//   mesh step (REFINED; the DG case of MGTransferMatrixFree<d,Number>::prolongate_and_add / restrict_and_add as
//   MultigridSolverDGPlain uses them, common/multigrid_solver_dg_plain.h:483, :489; d = 2 as poisson_dg_plain/program.cc:65
//   runs it): a cell of degree p and its 2^d children, child k = kx + 2 ky + 4 kz; NC = p+1, NF = 2(p+1)
//     prolongation:  fine[children[c][k]] += (P_kz (x) P_ky (x) P_kx) coarse[c]
//     restriction:   coarse[c] += sum_k (P_kz (x) P_ky (x) P_kx)^T fine[children[c][k]]
//     mat[(h NC + i) NC + j] = P_h[i][j]: coefficient i, in the child's basis, of the parent's function j on the child
//     half h = 0, 1 of [0, 1]
//   degree step (no counterpart in the reference): one cell in the degrees pc < pf on two levels that number their cells
//   alike, so there is no table of children; NC = pc+1, NF = pf+1
//     prolongation:  fine[c] += (E (x) E (x) E) coarse[c]
//     restriction:   coarse[c] += (E (x) E (x) E)^T fine[c]
//     mat[i NC + j] = E[i][j]: coefficient i, in the basis of degree pf, of function j of the basis of degree pc
//
// The NC^d coarse and the NF^d fine values of such a group meet in one LDS tile of NF^d entries (odd row pitch), the
// coarse ones in its corner [0, NC)^d.  The d sum-factorised sweeps run in place on it, one line per thread: the
// prolongation grows NC -> NF along x, then y, then z, the restriction shrinks in the reverse order.  The two steps
// differ only in where the fine values of a tile live in memory: one contiguous run of NF^d in the degree step; 2^d runs
// of NC^d in the mesh step, where the tile is the 2^d block of children and the tile position of an entry is computed
// from its place in the run.  Every fine cell is the child of exactly one parent (checked by the host when the transfer
// is created): one writer per entry, no atomics, no colours, the same bits in every run.  The matrix sits in LDS: it is
// wave-uniform, but 2 (p+1)^2 entries do not fit the scalar registers from p = 7 on, and a thread addresses it with
// compile-time offsets.  A workgroup takes as many groups as 4096 tile values admit, at most 8 in 3D and 64 in 2D
// (DGTransferCfg); the last workgroup is partly filled.
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  namespace
  {
    template <int NF, int NC, typename T, int DIM>
    struct DGTransferCfg
    {
      static_assert(DIM == 2 || DIM == 3, "quadrilaterals or hexahedra");
      static_assert(2 <= NC && NC < NF, "the coarse line is shorter than the fine one");
      static constexpr int MP     = NF | 1; // row pitch, odd: lines along y and z of neighbouring rows on different banks
      static constexpr int TILE   = DIM == 3 ? NF * NF * MP : NF * MP;
      static constexpr int FINE   = DIM == 3 ? NF * NF * NF : NF * NF; // values of a group on the two levels
      static constexpr int COARSE = DIM == 3 ? NC * NC * NC : NC * NC;
      // four waves: two workgroups per CU up to 80 kB of LDS each; the kernel asks for the registers of
      // two waves per SIMD, which is what the LDS of the mesh step at p = 9 in fp64 admits in 3D
      static constexpr int THREADS = 256;
      // groups per workgroup: tiles of at most 4096 values together, at most 8 in 3D and 64 in 2D (where a group has
      // only NC lines in the first sweep).  LDS in fp64: 36 KiB at the most where several groups share a workgroup
      // (NF = 8), 68.8 kB for the one parent of the mesh step at p = 9 in 3D
      //   mesh step, p = 1 ... 9:     3D 8 8 8 4 2 1 1 1 1,  2D 64 64 64 40 28 20 16 12 10
      //   degree step, pf = 2 ... 9:  3D 8 8 8 8 8 8 5 4,    2D 64 64 64 64 64 64 50 40
      static constexpr int CAP    = DIM == 3 ? 8 : 64;
      static constexpr int GROUPS = FINE > 4096 ? 1 : (4096 / FINE > CAP ? CAP : 4096 / FINE);
    };

    // one line of a sweep, in place: NC values at line[j stride] -> NF values (PROLONG), or back
    template <int NF, int NC, typename T, bool PROLONG>
    __device__ __forceinline__ void transfer_line(T *__restrict__ line, const int stride, const T *__restrict__ mat)
    {
      if (PROLONG)
        {
          T in[NC], out[NF];
#pragma unroll
          for (int j = 0; j < NC; ++j)
            in[j] = line[j * stride];
#pragma unroll
          for (int i = 0; i < NF; ++i)
            {
              T acc = mat[i * NC] * in[0];
#pragma unroll
              for (int j = 1; j < NC; ++j)
                acc += mat[i * NC + j] * in[j];
              out[i] = acc;
            }
#pragma unroll
          for (int i = 0; i < NF; ++i)
            line[i * stride] = out[i];
        }
      else
        {
          T in[NF], out[NC];
#pragma unroll
          for (int i = 0; i < NF; ++i)
            in[i] = line[i * stride];
#pragma unroll
          for (int j = 0; j < NC; ++j)
            {
              T acc = mat[j] * in[0];
#pragma unroll
              for (int i = 1; i < NF; ++i)
                acc += mat[i * NC + j] * in[i];
              out[j] = acc;
            }
#pragma unroll
          for (int j = 0; j < NC; ++j)
            line[j * stride] = out[j];
        }
    }

    // the lines of one sweep direction over the groups of the workgroup.  3D, DIR 0: x lines (z, y < NC), 1: y lines
    // (z < NC, x < NF), 2: z lines (y, x < NF); 2D, DIR 0: x lines (y < NC), 1: y lines (x < NF).  Consecutive threads
    // take consecutive x (y for the x lines: pitch MP)
    template <int NF, int NC, typename T, bool PROLONG, int DIM, int DIR>
    __device__ __forceinline__ void transfer_sweep(T *__restrict__ tile, const T *__restrict__ mat, const int n_groups)
    {
      using C              = DGTransferCfg<NF, NC, T, DIM>;
      constexpr int MP     = C::MP;
      constexpr int count  = DIM == 3 ? (DIR == 0 ? NC * NC : (DIR == 1 ? NC * NF : NF * NF)) : (DIR == 0 ? NC : NF);
      constexpr int stride = DIR == 0 ? 1 : (DIR == 1 ? MP : NF * MP);
      for (int it = threadIdx.x; it < n_groups * count; it += C::THREADS)
        {
          const int g = it / count, l = it - g * count;
          const int base = DIM == 3 ? (DIR == 0 ? ((l / NC) * NF + l % NC) * MP : (DIR == 1 ? (l / NF) * NF * MP + l % NF : (l / NF) * MP + l % NF))
                                    : (DIR == 0 ? l * MP : l);
          // an offset the optimiser cannot see through: the matrix entries are read for every line, with compile-time
          // offsets, and not kept in NF NC vector registers across the loop (one wave per SIMD from p = 8 on in the
          // mesh step)
          int mat_offset = 0;
          asm volatile("" : "+v"(mat_offset));
          transfer_line<NF, NC, T, PROLONG>(tile + g * C::TILE + base, stride, mat + mat_offset);
        }
    }

    // CHILD...: uint32_t in a mesh step (REFINED), nothing in a degree step, whose kernel has neither the table of
    // children nor the identity flag (children[c][k] == 2^d c + k: the table is not read) among its arguments
    template <typename>
    using flag_t = int;

    template <int NF, int NC, typename T, bool PROLONG, int DIM, typename... CHILD>
    __global__ void __launch_bounds__((DGTransferCfg<NF, NC, T, DIM>::THREADS), 2)
      dg_transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const CHILD *__restrict__... children, const uint32_t n_groups,
                         const T *__restrict__ m1d, const flag_t<CHILD>... identity)
    {
      constexpr bool REFINED = sizeof...(CHILD) == 1;
      using C                = DGTransferCfg<NF, NC, T, DIM>;
      static_assert(sizeof...(CHILD) <= 1 && (!REFINED || NF == 2 * NC), "a cell and its two halves per direction");
      constexpr int MP = C::MP, FINE = C::FINE, COARSE = C::COARSE, K = 1 << DIM;
      __shared__ T  tile[C::GROUPS * C::TILE];
      __shared__ T  mat[NF * NC];
      const int      tid   = threadIdx.x;
      const uint32_t first = blockIdx.x * (uint32_t)C::GROUPS;
      const int      n_own = (int)min((uint32_t)C::GROUPS, n_groups - first); // >= 1: the grid covers n_groups

      for (int i = tid; i < NF * NC; i += C::THREADS)
        mat[i] = m1d[i];

      // tile position of entry `local` of a run with N entries per direction (x fastest in both) that starts at
      // (kx, ky, kz) N of the tile, k = kx + 2 ky + 4 kz
      auto slot = [](const int k, const int local, auto N_) {
        constexpr int N = decltype(N_)::value;
        if constexpr (!REFINED) // one run per cell, k = 0: the expressions below at k = 0, in the order that keeps the
          {                     // degree step's instruction streams (profiles/dg_transfer_one_kernel_code_static.txt)
            if constexpr (DIM == 3)
              return ((local / (N * N)) * NF + (local / N) % N) * MP + local % N;
            else
              return (local / N) * MP + local % N;
          }
        else if constexpr (DIM == 3)
          {
            const int lx = local % N, ly = (local / N) % N, lz = local / (N * N);
            return (((k >> 2) * N + lz) * NF + ((k >> 1) & 1) * N + ly) * MP + (k & 1) * N + lx;
          }
        else
          {
            const int lx = local % N, ly = local / N;
            return ((k >> 1) * N + ly) * MP + (k & 1) * N + lx;
          }
      };
      constexpr std::integral_constant<int, NF> fine_n{};
      constexpr std::integral_constant<int, NC> coarse_n{};
      // mesh step: the fine cell that is child k of a parent (called with children..., identity...)
      auto child_cell = [](const uint32_t parent, const int k, const uint32_t *__restrict__ table, const int same) {
        return same ? (uint32_t)K * parent + (uint32_t)k : table[K * (size_t)parent + k];
      };

      if (PROLONG)
        {
#pragma unroll 4
          for (int it = tid; it < n_own * COARSE; it += C::THREADS)
            {
              const int g = it / COARSE, local = it - g * COARSE;
              tile[g * C::TILE + slot(0, local, coarse_n)] = src[(size_t)(first + g) * COARSE + local];
            }
          __syncthreads();
          transfer_sweep<NF, NC, T, true, DIM, 0>(tile, mat, n_own);
          __syncthreads();
          transfer_sweep<NF, NC, T, true, DIM, 1>(tile, mat, n_own);
          __syncthreads();
          if constexpr (DIM == 3)
            {
              transfer_sweep<NF, NC, T, true, DIM, 2>(tile, mat, n_own);
              __syncthreads();
            }
#pragma unroll 4
          for (int it = tid; it < n_own * FINE; it += C::THREADS)
            {
              const int g = it / FINE, rem = it - g * FINE;
              if constexpr (REFINED)
                {
                  const int k = rem / COARSE, local = rem - k * COARSE;
                  dst[(size_t)child_cell(first + g, k, children..., identity...) * COARSE + local] += tile[g * C::TILE + slot(k, local, coarse_n)];
                }
              else
                dst[(size_t)(first + g) * FINE + rem] += tile[g * C::TILE + slot(0, rem, fine_n)];
            }
        }
      else
        {
#pragma unroll 4
          for (int it = tid; it < n_own * FINE; it += C::THREADS)
            {
              const int g = it / FINE, rem = it - g * FINE;
              if constexpr (REFINED)
                {
                  const int k = rem / COARSE, local = rem - k * COARSE;
                  tile[g * C::TILE + slot(k, local, coarse_n)] = src[(size_t)child_cell(first + g, k, children..., identity...) * COARSE + local];
                }
              else
                tile[g * C::TILE + slot(0, rem, fine_n)] = src[(size_t)(first + g) * FINE + rem];
            }
          __syncthreads();
          if constexpr (DIM == 3)
            {
              transfer_sweep<NF, NC, T, false, DIM, 2>(tile, mat, n_own);
              __syncthreads();
            }
          transfer_sweep<NF, NC, T, false, DIM, 1>(tile, mat, n_own);
          __syncthreads();
          transfer_sweep<NF, NC, T, false, DIM, 0>(tile, mat, n_own);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_own * COARSE; it += C::THREADS)
            {
              const int g = it / COARSE, local = it - g * COARSE;
              dst[(size_t)(first + g) * COARSE + local] += tile[g * C::TILE + slot(0, local, coarse_n)];
            }
        }
    }
  } // namespace

  bool launch_dg_transfer(hipStream_t s, int number, int fine_degree, int coarse_degree, bool prolong, void *dst, const void *src,
                          uint32_t n_groups, const void *m1d, int dim, const uint32_t *children, bool identity)
  {
    if (n_groups == 0)
      return true;
    bool launched = false;
    dispatch_degree(fine_degree, [&](auto PF) {
      dispatch_degree(coarse_degree, [&](auto PC) {
        if constexpr (PC.value <= PF.value)
          dispatch_number(number, [&](auto t) {
            launched = dispatch_mode<2, 3>(dim, [&](auto DIM) {
              using T                = decltype(t);
              constexpr bool REFINED = PC.value == PF.value; // a line of p+1 values against its two halves
              constexpr int  NC = PC.value + 1, NF = REFINED ? 2 * NC : PF.value + 1;
              using C           = DGTransferCfg<NF, NC, T, DIM.value>;
              const uint32_t nb = (n_groups + C::GROUPS - 1) / C::GROUPS;
              if constexpr (REFINED)
                hipLaunchKernelGGL((prolong ? dg_transfer_kernel<NF, NC, T, true, DIM.value, uint32_t> :
                                              dg_transfer_kernel<NF, NC, T, false, DIM.value, uint32_t>),
                                   dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, children, n_groups, (const T *)m1d,
                                   identity ? 1 : 0);
              else
                hipLaunchKernelGGL((prolong ? dg_transfer_kernel<NF, NC, T, true, DIM.value> : dg_transfer_kernel<NF, NC, T, false, DIM.value>),
                                   dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, n_groups, (const T *)m1d);
            });
          });
      });
    });
    return launched;
  }
} // namespace mgx
