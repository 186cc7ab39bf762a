// mgx_dg_transfer.hip -- level transfer between two DG spaces of the same degree and basis, one cell and its eight
// children (the DG case of MGTransferMatrixFree::prolongate_and_add / restrict_and_add as MultigridSolverDGPlain uses
// them, common/multigrid_solver_dg_plain.h:483, :489).
//
//   prolongation:  fine[children[c][kx + 2 ky + 4 kz]] += (P_kz (x) P_ky (x) P_kx) coarse[c]
//   restriction:   coarse[c] += sum_k (P_kz (x) P_ky (x) P_kx)^T fine[children[c][k]]
//
// P_h[i][j] (h = 0, 1): coefficient i, in the child's basis, of the parent's function j on the child half h of [0, 1].
// A parent's (p+1)^3 values and the (2(p+1))^3 values of its children meet in one LDS tile laid out as the 2 x 2 x 2
// block of children; the three sum-factorised sweeps run in place on it, one line per thread.  Child blocks are read and
// written as contiguous runs of (p+1)^3, the tile position of an entry computed from its place in the run.  Every fine
// cell is a child of exactly one parent (checked by the host when the transfer is created): no atomics, no colours,
// the same bits in every run.  The two matrices sit in LDS: they are wave-uniform, but 2 (p+1)^2 entries do not fit the
// scalar registers from p = 7 on, and a thread addresses them with compile-time offsets.
//
// Two dimensions (MGTransferMatrixFree<2,Number>, as poisson_dg_plain/program.cc:65 runs it): the sibling kernel
// dg_transfer_kernel_2d with a 2 x 2 tile of (2(p+1))^2 values per parent, two sweeps, four children.  A parent has
// only p+1 lines in the first sweep, so a workgroup takes as many parents as 4096 tile values admit, at most 64:
// 64 parents for p = 1 ... 3 (256 x-lines at p = 3), then 40, 28, 20, 16, 12, 10 for p = 4 ... 9.
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  namespace
  {
    template <int P, typename T>
    struct DGTransferCfg
    {
      static constexpr int N = P + 1, M = 2 * N;
      static constexpr int MP      = M + 1;  // row pitch, odd: lines along y and z of neighbouring rows on different banks
      static constexpr int TILE    = M * M * MP;
      static constexpr int N3      = N * N * N;
      // four waves: two workgroups per CU up to 80 kB of LDS each; the kernel asks for the registers of
      // two waves per SIMD, which is what the LDS of p = 9 in fp64 admits
      static constexpr int THREADS = 256;
      // parents per workgroup: tiles of at most 4096 values together, at most 8
      static constexpr int PPB = M * M * M > 4096 ? 1 : (4096 / (M * M * M) > 8 ? 8 : 4096 / (M * M * M));
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

    // the lines of one sweep direction over the parents of the workgroup.  DIR 0: x lines (k, j < N), 1: y lines
    // (k < N, i' < M), 2: z lines (j', i' < M); consecutive threads take consecutive i' (j for the x lines: pitch MP)
    template <int P, typename T, bool PROLONG, int DIR>
    __device__ __forceinline__ void transfer_sweep(T *__restrict__ tile, const T *__restrict__ mat, const int n_parents)
    {
      using C              = DGTransferCfg<P, T>;
      constexpr int N      = C::N, M = C::M, MP = C::MP;
      constexpr int count  = DIR == 0 ? N * N : (DIR == 1 ? N * M : M * M);
      constexpr int stride = DIR == 0 ? 1 : (DIR == 1 ? MP : M * MP);
      for (int it = threadIdx.x; it < n_parents * count; it += C::THREADS)
        {
          const int pp = it / count, l = it - pp * count;
          const int base = DIR == 0 ? ((l / N) * M + l % N) * MP : (DIR == 1 ? (l / M) * M * MP + l % M : (l / M) * MP + l % M);
          // an offset the optimiser cannot see through: the matrix entries are read for every line, with compile-time
          // offsets, and not kept in 4 (p+1)^2 vector registers across the loop (one wave per SIMD from p = 8 on)
          int mat_offset = 0;
          asm volatile("" : "+v"(mat_offset));
          transfer_line<N, T, PROLONG>(tile + pp * C::TILE + base, stride, mat + mat_offset);
        }
    }

    template <int P, typename T, bool PROLONG>
    __global__ void __launch_bounds__((DGTransferCfg<P, T>::THREADS), 2)
      dg_transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ children,
                         const uint32_t n_coarse, const T *__restrict__ p1d, const int identity)
    {
      using C         = DGTransferCfg<P, T>;
      constexpr int N = C::N, M = C::M, MP = C::MP, N3 = C::N3;
      __shared__ T  tile[C::PPB * C::TILE];
      __shared__ T  mat[2 * N * N];
      const int      tid       = threadIdx.x;
      const uint32_t first     = blockIdx.x * (uint32_t)C::PPB;
      const int      n_parents = (int)min((uint32_t)C::PPB, n_coarse - first); // >= 1: the grid covers n_coarse

      for (int i = tid; i < 2 * N * N; i += C::THREADS)
        mat[i] = p1d[i];

      // tile position of entry `local` of child k (x fastest in both)
      auto fine_slot = [](const int k, const int local) {
        const int lx = local % N, ly = (local / N) % N, lz = local / (N * N);
        return (((k >> 2) * N + lz) * M + ((k >> 1) & 1) * N + ly) * MP + (k & 1) * N + lx;
      };
      auto child_cell = [&](const uint32_t parent, const int k) {
        return identity ? 8u * parent + (uint32_t)k : children[8 * (size_t)parent + k];
      };

      if (PROLONG)
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * N3; it += C::THREADS)
            {
              const int pp = it / N3, local = it - pp * N3;
              tile[pp * C::TILE + fine_slot(0, local)] = src[(size_t)(first + pp) * N3 + local];
            }
          __syncthreads();
          transfer_sweep<P, T, true, 0>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, true, 1>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, true, 2>(tile, mat, n_parents);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_parents * 8 * N3; it += C::THREADS)
            {
              const int pp = it / (8 * N3), rem = it - pp * 8 * N3, k = rem / N3, local = rem - k * N3;
              dst[(size_t)child_cell(first + pp, k) * N3 + local] += tile[pp * C::TILE + fine_slot(k, local)];
            }
        }
      else
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * 8 * N3; it += C::THREADS)
            {
              const int pp = it / (8 * N3), rem = it - pp * 8 * N3, k = rem / N3, local = rem - k * N3;
              tile[pp * C::TILE + fine_slot(k, local)] = src[(size_t)child_cell(first + pp, k) * N3 + local];
            }
          __syncthreads();
          transfer_sweep<P, T, false, 2>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, false, 1>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep<P, T, false, 0>(tile, mat, n_parents);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_parents * N3; it += C::THREADS)
            {
              const int pp = it / N3, local = it - pp * N3;
              dst[(size_t)(first + pp) * N3 + local] += tile[pp * C::TILE + fine_slot(0, local)];
            }
        }
    }

    // ---- two dimensions ----
    template <int P, typename T>
    struct DGTransferCfg2
    {
      static constexpr int N = P + 1, M = 2 * N;
      static constexpr int MP      = M + 1; // row pitch, odd: y-lines of neighbouring columns on different banks
      static constexpr int TILE    = M * MP;
      static constexpr int NN      = N * N;
      static constexpr int THREADS = 256;
      // parents per workgroup: tiles of at most 4096 values together, at most 64 (36 KiB of LDS at p = 3 in fp64, the largest)
      static constexpr int PPB = 4096 / (M * M) > 64 ? 64 : 4096 / (M * M);
    };

    // the lines of one sweep direction over the parents of the workgroup.  DIR 0: x lines (j < N), 1: y lines (i' < M)
    template <int P, typename T, bool PROLONG, int DIR>
    __device__ __forceinline__ void transfer_sweep_2d(T *__restrict__ tile, const T *__restrict__ mat, const int n_parents)
    {
      using C              = DGTransferCfg2<P, T>;
      constexpr int N      = C::N, M = C::M, MP = C::MP;
      constexpr int count  = DIR == 0 ? N : M;
      constexpr int stride = DIR == 0 ? 1 : MP;
      for (int it = threadIdx.x; it < n_parents * count; it += C::THREADS)
        {
          const int pp = it / count, l = it - pp * count;
          const int base = DIR == 0 ? l * MP : l;
          int       mat_offset = 0; // (see transfer_sweep)
          asm volatile("" : "+v"(mat_offset));
          transfer_line<N, T, PROLONG>(tile + pp * C::TILE + base, stride, mat + mat_offset);
        }
    }

    template <int P, typename T, bool PROLONG>
    __global__ void __launch_bounds__((DGTransferCfg2<P, T>::THREADS), 2)
      dg_transfer_kernel_2d(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ children,
                            const uint32_t n_coarse, const T *__restrict__ p1d, const int identity)
    {
      using C         = DGTransferCfg2<P, T>;
      constexpr int N = C::N, MP = C::MP, NN = C::NN;
      __shared__ T  tile[C::PPB * C::TILE];
      __shared__ T  mat[2 * N * N];
      const int      tid       = threadIdx.x;
      const uint32_t first     = blockIdx.x * (uint32_t)C::PPB;
      const int      n_parents = (int)min((uint32_t)C::PPB, n_coarse - first); // >= 1: the grid covers n_coarse

      for (int i = tid; i < 2 * N * N; i += C::THREADS)
        mat[i] = p1d[i];

      // tile position of entry `local` of child k (x fastest in both)
      auto fine_slot = [](const int k, const int local) {
        const int lx = local % N, ly = local / N;
        return ((k >> 1) * N + ly) * MP + (k & 1) * N + lx;
      };
      auto child_cell = [&](const uint32_t parent, const int k) {
        return identity ? 4u * parent + (uint32_t)k : children[4 * (size_t)parent + k];
      };

      if (PROLONG)
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * NN; it += C::THREADS)
            {
              const int pp = it / NN, local = it - pp * NN;
              tile[pp * C::TILE + fine_slot(0, local)] = src[(size_t)(first + pp) * NN + local];
            }
          __syncthreads();
          transfer_sweep_2d<P, T, true, 0>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep_2d<P, T, true, 1>(tile, mat, n_parents);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_parents * 4 * NN; it += C::THREADS)
            {
              const int pp = it / (4 * NN), rem = it - pp * 4 * NN, k = rem / NN, local = rem - k * NN;
              dst[(size_t)child_cell(first + pp, k) * NN + local] += tile[pp * C::TILE + fine_slot(k, local)];
            }
        }
      else
        {
#pragma unroll 4
          for (int it = tid; it < n_parents * 4 * NN; it += C::THREADS)
            {
              const int pp = it / (4 * NN), rem = it - pp * 4 * NN, k = rem / NN, local = rem - k * NN;
              tile[pp * C::TILE + fine_slot(k, local)] = src[(size_t)child_cell(first + pp, k) * NN + local];
            }
          __syncthreads();
          transfer_sweep_2d<P, T, false, 1>(tile, mat, n_parents);
          __syncthreads();
          transfer_sweep_2d<P, T, false, 0>(tile, mat, n_parents);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_parents * NN; it += C::THREADS)
            {
              const int pp = it / NN, local = it - pp * NN;
              dst[(size_t)(first + pp) * NN + local] += tile[pp * C::TILE + fine_slot(0, local)];
            }
        }
    }

    template <int P, typename T>
    void dg_transfer_2d_t(hipStream_t s, bool prolong, void *dst, const void *src, const uint32_t *children, uint32_t n_coarse,
                          const void *p1d, bool identity)
    {
      using C           = DGTransferCfg2<P, T>;
      const uint32_t nb = (n_coarse + C::PPB - 1) / C::PPB;
      if (prolong)
        hipLaunchKernelGGL((dg_transfer_kernel_2d<P, T, true>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, children,
                           n_coarse, (const T *)p1d, identity ? 1 : 0);
      else
        hipLaunchKernelGGL((dg_transfer_kernel_2d<P, T, false>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, children,
                           n_coarse, (const T *)p1d, identity ? 1 : 0);
    }

    template <int P, typename T>
    void dg_transfer_t(hipStream_t s, bool prolong, void *dst, const void *src, const uint32_t *children, uint32_t n_coarse,
                       const void *p1d, bool identity)
    {
      using C           = DGTransferCfg<P, T>;
      const uint32_t nb = (n_coarse + C::PPB - 1) / C::PPB;
      if (prolong)
        hipLaunchKernelGGL((dg_transfer_kernel<P, T, true>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, children,
                           n_coarse, (const T *)p1d, identity ? 1 : 0);
      else
        hipLaunchKernelGGL((dg_transfer_kernel<P, T, false>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, children,
                           n_coarse, (const T *)p1d, identity ? 1 : 0);
    }
  } // namespace

  void launch_dg_transfer(hipStream_t s, int number, int p, bool prolong, void *dst, const void *src, const uint32_t *children,
                          uint32_t n_coarse, const void *p1d, bool identity, int dim)
  {
    if (n_coarse == 0)
      return;
    if (dim == 2)
      {
        if (number == 1)
          dispatch_degree(p, [&](auto P) { dg_transfer_2d_t<P.value, double>(s, prolong, dst, src, children, n_coarse, p1d, identity); });
        else
          dispatch_degree(p, [&](auto P) { dg_transfer_2d_t<P.value, float>(s, prolong, dst, src, children, n_coarse, p1d, identity); });
        return;
      }
    if (number == 1)
      {
        dispatch_degree(p, [&](auto P) { dg_transfer_t<P.value, double>(s, prolong, dst, src, children, n_coarse, p1d, identity); });
      }
    else
      {
        dispatch_degree(p, [&](auto P) { dg_transfer_t<P.value, float>(s, prolong, dst, src, children, n_coarse, p1d, identity); });
      }
  }
} // namespace mgx
