// mgx_dg_transfer.hip -- level transfer between two DG spaces of the same degree and basis in d = 2 or 3 dimensions,
// one cell and its 2^d children (the DG case of MGTransferMatrixFree<d,Number>::prolongate_and_add / restrict_and_add as
// MultigridSolverDGPlain uses them, common/multigrid_solver_dg_plain.h:483, :489; d = 2 as poisson_dg_plain/program.cc:65
// runs it).  One kernel template on the dimension; written out for d = 3, child k = kx + 2 ky + 4 kz:
//
//   prolongation:  fine[children[c][k]] += (P_kz (x) P_ky (x) P_kx) coarse[c]
//   restriction:   coarse[c] += sum_k (P_kz (x) P_ky (x) P_kx)^T fine[children[c][k]]
//
// P_h[i][j] (h = 0, 1): coefficient i, in the child's basis, of the parent's function j on the child half h of [0, 1].
// A parent's (p+1)^d values and the (2(p+1))^d values of its children meet in one LDS tile laid out as the 2^d block of
// children; the d sum-factorised sweeps run in place on it, one line per thread.  Child blocks are read and written as
// contiguous runs of (p+1)^d, the tile position of an entry computed from its place in the run.  Every fine cell is a
// child of exactly one parent (checked by the host when the transfer is created): no atomics, no colours, the same bits
// in every run.  The two matrices sit in LDS: they are wave-uniform, but 2 (p+1)^2 entries do not fit the scalar
// registers from p = 7 on, and a thread addresses them with compile-time offsets.  A workgroup takes as many parents as
// 4096 tile values admit, at most 8 in 3D and 64 in 2D (DGTransferCfg).
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  namespace
  {
    template <int P, typename T, int DIM>
    struct DGTransferCfg
    {
      static_assert(DIM == 2 || DIM == 3, "quadrilaterals or hexahedra");
      static constexpr int N = P + 1, M = 2 * N;
      static constexpr int MP       = M + 1; // row pitch, odd: lines along y and z of neighbouring rows on different banks
      static constexpr int TILE     = DIM == 3 ? M * M * MP : M * MP;
      static constexpr int NC       = DIM == 3 ? N * N * N : N * N; // entries of a cell
      static constexpr int CHILDREN = 1 << DIM;
      // four waves: two workgroups per CU up to 80 kB of LDS each; the kernel asks for the registers of
      // two waves per SIMD, which is what the LDS of p = 9 in fp64 admits in 3D
      static constexpr int THREADS = 256;
      // parents per workgroup: tiles of at most 4096 values together, at most 8 in 3D and 64 in 2D (where a parent has
      // only p+1 lines in the first sweep; 36 KiB of LDS at p = 3 in fp64, the largest):
      // 3D 8 8 8 4 2 1 1 1 1, 2D 64 64 64 40 28 20 16 12 10 for p = 1 ... 9
      static constexpr int VALUES = CHILDREN * NC, CAP = DIM == 3 ? 8 : 64;
      static constexpr int PPB    = VALUES > 4096 ? 1 : (4096 / VALUES > CAP ? CAP : 4096 / VALUES);
    };

    // one line of a sweep, in place: N values at base + j stride -> 2 N values (PROLONG), or back
    template <int N, typename T, bool PROLONG>
    __device__ __forceinline__ void transfer_line(T *__restrict__ line, const int stride, const T *__restrict__ mat)
    {
      if (PROLONG)
        {
          T in[N], out[2 * N];
#pragma unroll
          for (int j = 0; j < N; ++j)
            in[j] = line[j * stride];
#pragma unroll
          for (int m = 0; m < 2 * N; ++m) // m = h N + i: row i of P_h
            {
              T acc = mat[m * N] * in[0];
#pragma unroll
              for (int j = 1; j < N; ++j)
                acc += mat[m * N + j] * in[j];
              out[m] = acc;
            }
#pragma unroll
          for (int m = 0; m < 2 * N; ++m)
            line[m * stride] = out[m];
        }
      else
        {
          T in[2 * N], out[N];
#pragma unroll
          for (int m = 0; m < 2 * N; ++m)
            in[m] = line[m * stride];
#pragma unroll
          for (int j = 0; j < N; ++j)
            {
              T acc = mat[j] * in[0];
#pragma unroll
              for (int m = 1; m < 2 * N; ++m)
                acc += mat[m * N + j] * in[m];
              out[j] = acc;
            }
#pragma unroll
          for (int j = 0; j < N; ++j)
            line[j * stride] = out[j];
        }
    }

    // the lines of one sweep direction over the parents of the workgroup.  3D, DIR 0: x lines (k, j < N), 1: y lines
    // (k < N, i' < M), 2: z lines (j', i' < M); 2D, DIR 0: x lines (j < N), 1: y lines (i' < M).  Consecutive threads
    // take consecutive i' (j for the x lines: pitch MP)
    template <int P, typename T, bool PROLONG, int DIM, int DIR>
    __device__ __forceinline__ void transfer_sweep(T *__restrict__ tile, const T *__restrict__ mat, const int n_parents)
    {
      using C              = DGTransferCfg<P, T, DIM>;
      constexpr int N      = C::N, M = C::M, MP = C::MP;
      constexpr int count  = DIM == 3 ? (DIR == 0 ? N * N : (DIR == 1 ? N * M : M * M)) : (DIR == 0 ? N : M);
      constexpr int stride = DIR == 0 ? 1 : (DIR == 1 ? MP : M * MP);
      for (int it = threadIdx.x; it < n_parents * count; it += C::THREADS)
        {
          const int pp = it / count, l = it - pp * count;
          const int base = DIM == 3 ? (DIR == 0 ? ((l / N) * M + l % N) * MP : (DIR == 1 ? (l / M) * M * MP + l % M : (l / M) * MP + l % M))
                                    : (DIR == 0 ? l * MP : l);
          // an offset the optimiser cannot see through: the matrix entries are read for every line, with compile-time
          // offsets, and not kept in 4 (p+1)^2 vector registers across the loop (one wave per SIMD from p = 8 on)
          int mat_offset = 0;
          asm volatile("" : "+v"(mat_offset));
          transfer_line<N, T, PROLONG>(tile + pp * C::TILE + base, stride, mat + mat_offset);
        }
    }

    template <int P, typename T, bool PROLONG, int DIM>
    __global__ void __launch_bounds__((DGTransferCfg<P, T, DIM>::THREADS), 2)
      dg_transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ children,
                         const uint32_t n_coarse, const T *__restrict__ p1d, const int identity)
    {
      using C         = DGTransferCfg<P, T, DIM>;
      constexpr int N = C::N, M = C::M, MP = C::MP, NC = C::NC, K = C::CHILDREN;
      __shared__ T  tile[C::PPB * C::TILE];
      __shared__ T  mat[2 * N * N];
      const int      tid       = threadIdx.x;
      const uint32_t first     = blockIdx.x * (uint32_t)C::PPB;
      const int      n_parents = (int)min((uint32_t)C::PPB, n_coarse - first); // >= 1: the grid covers n_coarse

      for (int i = tid; i < 2 * N * N; i += C::THREADS)
        mat[i] = p1d[i];

      // tile position of entry `local` of child k (x fastest in both)
      auto fine_slot = [](const int k, const int local) {
        if constexpr (DIM == 3)
          {
            const int lx = local % N, ly = (local / N) % N, lz = local / (N * N);
            return (((k >> 2) * N + lz) * M + ((k >> 1) & 1) * N + ly) * MP + (k & 1) * N + lx;
          }
        else
          {
            const int lx = local % N, ly = local / N;
            return ((k >> 1) * N + ly) * MP + (k & 1) * N + lx;
          }
      };
      auto child_cell = [&](const uint32_t parent, const int k) {
        return identity ? (uint32_t)K * parent + (uint32_t)k : children[K * (size_t)parent + k];
      };

      if (PROLONG)
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * NC; it += C::THREADS)
            {
              const int pp = it / NC, local = it - pp * NC;
              tile[pp * C::TILE + fine_slot(0, local)] = src[(size_t)(first + pp) * NC + local];
            }
          __syncthreads();
          transfer_sweep<P, T, true, DIM, 0>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, true, DIM, 1>(tile, mat, n_parents);
          __syncthreads();
          if constexpr (DIM == 3)
            {
              transfer_sweep<P, T, true, DIM, 2>(tile, mat, n_parents);
              __syncthreads();
            }
#pragma unroll 4
          for (int it = tid; it < n_parents * K * NC; it += C::THREADS)
            {
              const int pp = it / (K * NC), rem = it - pp * K * NC, k = rem / NC, local = rem - k * NC;
              dst[(size_t)child_cell(first + pp, k) * NC + local] += tile[pp * C::TILE + fine_slot(k, local)];
            }
        }
      else
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * K * NC; it += C::THREADS)
            {
              const int pp = it / (K * NC), rem = it - pp * K * NC, k = rem / NC, local = rem - k * NC;
              tile[pp * C::TILE + fine_slot(k, local)] = src[(size_t)child_cell(first + pp, k) * NC + local];
            }
          __syncthreads();
          if constexpr (DIM == 3)
            {
              transfer_sweep<P, T, false, DIM, 2>(tile, mat, n_parents);
              __syncthreads();
            }
          transfer_sweep<P, T, false, DIM, 1>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, false, DIM, 0>(tile, mat, n_parents);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_parents * NC; it += C::THREADS)
            {
              const int pp = it / NC, local = it - pp * NC;
              dst[(size_t)(first + pp) * NC + local] += tile[pp * C::TILE + fine_slot(0, local)];
            }
        }
    }
  } // namespace

  void launch_dg_transfer(hipStream_t s, int number, int p, bool prolong, void *dst, const void *src, const uint32_t *children,
                          uint32_t n_coarse, const void *p1d, bool identity, int dim)
  {
    if (n_coarse == 0)
      return;
    dispatch_degree(p, [&](auto P) {
      dispatch_number(number, [&](auto t) {
        dispatch_mode<2, 3>(dim, [&](auto DIM) {
          using T           = decltype(t);
          using C           = DGTransferCfg<P.value, T, DIM.value>;
          const uint32_t nb = (n_coarse + C::PPB - 1) / C::PPB;
          if (prolong)
            hipLaunchKernelGGL((dg_transfer_kernel<P.value, T, true, DIM.value>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst,
                               (const T *)src, children, n_coarse, (const T *)p1d, identity ? 1 : 0);
          else
            hipLaunchKernelGGL((dg_transfer_kernel<P.value, T, false, DIM.value>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst,
                               (const T *)src, children, n_coarse, (const T *)p1d, identity ? 1 : 0);
        });
      });
    });
  }
} // namespace mgx
