// mgx_dg_ptransfer.hip -- level transfer between two DG spaces of different degree (pc < pf) and the same basis on the
// same mesh in d = 2 or 3 dimensions: the p-coarsening partner of mgx_dg_transfer.hip.  Both levels number their cells
// alike, so cell c is the contiguous run of (pc+1)^d entries in the coarse vector and of (pf+1)^d in the fine one and
// there is no table of children.  Written out for d = 3:
//
//   prolongation:  fine[c] += (E (x) E (x) E) coarse[c]
//   restriction:   coarse[c] += (E (x) E (x) E)^T fine[c]
//
// E[i][j]: coefficient i, in the basis of degree pf, of the function j of the basis of degree pc (mgx_dg_degree_embedding).
// A cell's values meet in one LDS tile of (pf+1)^d entries (odd row pitch); the coarse values sit in its corner
// [0, pc]^d.  The d sum-factorised sweeps run in place on it, one line per thread: the prolongation grows pc+1 -> pf+1
// along x, then y, then z, the restriction shrinks in the reverse order.  E sits in LDS ((pf+1)(pc+1) entries, read
// with compile-time offsets, as the h transfer reads its matrices).  One writer per entry: no atomics, the same bits in
// every run.  A workgroup takes as many cells as 4096 tile values admit, at most 8 in 3D and 64 in 2D, the caps of the
// h transfer (DGPTransferCfg); the last workgroup is partly filled.
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  namespace
  {
    template <int PF, int PC, typename T, int DIM>
    struct DGPTransferCfg
    {
      static_assert(DIM == 2 || DIM == 3, "quadrilaterals or hexahedra");
      static_assert(1 <= PC && PC < PF, "the coarse degree is below the fine one");
      static constexpr int NF = PF + 1, NC = PC + 1;
      static constexpr int MP      = NF | 1; // row pitch, odd: lines along y and z of neighbouring rows on different banks
      static constexpr int TILE    = DIM == 3 ? NF * NF * MP : NF * MP;
      static constexpr int FINE    = DIM == 3 ? NF * NF * NF : NF * NF; // entries of a cell on the two levels
      static constexpr int COARSE  = DIM == 3 ? NC * NC * NC : NC * NC;
      static constexpr int THREADS = 256;
      // cells per workgroup: 3D 8 8 8 8 8 8 5 4 for pf = 2 ... 9, 2D 64 64 64 64 64 64 50 40 (36 KiB of LDS at pf = 7
      // in fp64 and either dimension, the largest: two workgroups per CU)
      static constexpr int CAP = DIM == 3 ? 8 : 64;
      static constexpr int CPB = FINE > 4096 ? 1 : (4096 / FINE > CAP ? CAP : 4096 / FINE);
    };

    // one line of a sweep, in place: NC values at line[j stride] -> NF values (PROLONG), or back.  mat[i NC + j] = E[i][j]
    template <int NF, int NC, typename T, bool PROLONG>
    __device__ __forceinline__ void ptransfer_line(T *__restrict__ line, const int stride, const T *__restrict__ mat)
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

    // the lines of one sweep direction over the cells of the workgroup.  3D, DIR 0: x lines (z, y < NC), 1: y lines
    // (z < NC, x < NF), 2: z lines (y, x < NF); 2D, DIR 0: x lines (y < NC), 1: y lines (x < NF).  Consecutive threads
    // take consecutive x (y for the x lines: pitch MP)
    template <int PF, int PC, typename T, bool PROLONG, int DIM, int DIR>
    __device__ __forceinline__ void ptransfer_sweep(T *__restrict__ tile, const T *__restrict__ mat, const int n_cells)
    {
      using C              = DGPTransferCfg<PF, PC, T, DIM>;
      constexpr int NF     = C::NF, NC = C::NC, MP = C::MP;
      constexpr int count  = DIM == 3 ? (DIR == 0 ? NC * NC : (DIR == 1 ? NC * NF : NF * NF)) : (DIR == 0 ? NC : NF);
      constexpr int stride = DIR == 0 ? 1 : (DIR == 1 ? MP : NF * MP);
      for (int it = threadIdx.x; it < n_cells * count; it += C::THREADS)
        {
          const int cc = it / count, l = it - cc * count;
          const int base = DIM == 3 ? (DIR == 0 ? ((l / NC) * NF + l % NC) * MP : (DIR == 1 ? (l / NF) * NF * MP + l % NF : (l / NF) * MP + l % NF))
                                    : (DIR == 0 ? l * MP : l);
          // an offset the optimiser cannot see through: the matrix entries are read for every line, with compile-time
          // offsets, and not kept in (pf+1)(pc+1) vector registers across the loop (as in mgx_dg_transfer.hip)
          int mat_offset = 0;
          asm volatile("" : "+v"(mat_offset));
          ptransfer_line<NF, NC, T, PROLONG>(tile + cc * C::TILE + base, stride, mat + mat_offset);
        }
    }

    template <int PF, int PC, typename T, bool PROLONG, int DIM>
    __global__ void __launch_bounds__((DGPTransferCfg<PF, PC, T, DIM>::THREADS), 2)
      dg_ptransfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t n_cells, const T *__restrict__ e1d)
    {
      using C          = DGPTransferCfg<PF, PC, T, DIM>;
      constexpr int NF = C::NF, NC = C::NC, MP = C::MP;
      __shared__ T  tile[C::CPB * C::TILE];
      __shared__ T  mat[NF * NC];
      const int      tid   = threadIdx.x;
      const uint32_t first = blockIdx.x * (uint32_t)C::CPB;
      const int      n_own = (int)min((uint32_t)C::CPB, n_cells - first); // >= 1: the grid covers n_cells

      for (int i = tid; i < NF * NC; i += C::THREADS)
        mat[i] = e1d[i];

      // tile position of entry `local` of a cell with N entries per direction (x fastest in both)
      auto slot = [](const int local, auto N_) {
        constexpr int N = decltype(N_)::value;
        if constexpr (DIM == 3)
          return ((local / (N * N)) * NF + (local / N) % N) * MP + local % N;
        else
          return (local / N) * MP + local % N;
      };
      constexpr std::integral_constant<int, NF> fine_n{};
      constexpr std::integral_constant<int, NC> coarse_n{};

      if (PROLONG)
        {
#pragma unroll 4
          for (int it = tid; it < n_own * C::COARSE; it += C::THREADS)
            {
              const int cc = it / C::COARSE, local = it - cc * C::COARSE;
              tile[cc * C::TILE + slot(local, coarse_n)] = src[(size_t)(first + cc) * C::COARSE + local];
            }
          __syncthreads();
          ptransfer_sweep<PF, PC, T, true, DIM, 0>(tile, mat, n_own);
          __syncthreads();
          ptransfer_sweep<PF, PC, T, true, DIM, 1>(tile, mat, n_own);
          __syncthreads();
          if constexpr (DIM == 3)
            {
              ptransfer_sweep<PF, PC, T, true, DIM, 2>(tile, mat, n_own);
              __syncthreads();
            }
#pragma unroll 4
          for (int it = tid; it < n_own * C::FINE; it += C::THREADS)
            {
              const int cc = it / C::FINE, local = it - cc * C::FINE;
              dst[(size_t)(first + cc) * C::FINE + local] += tile[cc * C::TILE + slot(local, fine_n)];
            }
        }
      else
        {
#pragma unroll 4
          for (int it = tid; it < n_own * C::FINE; it += C::THREADS)
            {
              const int cc = it / C::FINE, local = it - cc * C::FINE;
              tile[cc * C::TILE + slot(local, fine_n)] = src[(size_t)(first + cc) * C::FINE + local];
            }
          __syncthreads();
          if constexpr (DIM == 3)
            {
              ptransfer_sweep<PF, PC, T, false, DIM, 2>(tile, mat, n_own);
              __syncthreads();
            }
          ptransfer_sweep<PF, PC, T, false, DIM, 1>(tile, mat, n_own);
          __syncthreads();
          ptransfer_sweep<PF, PC, T, false, DIM, 0>(tile, mat, n_own);
          __syncthreads();
#pragma unroll 4
          for (int it = tid; it < n_own * C::COARSE; it += C::THREADS)
            {
              const int cc = it / C::COARSE, local = it - cc * C::COARSE;
              dst[(size_t)(first + cc) * C::COARSE + local] += tile[cc * C::TILE + slot(local, coarse_n)];
            }
        }
    }
  } // namespace

  bool launch_dg_ptransfer(hipStream_t s, int number, int pf, int pc, bool prolong, void *dst, const void *src, uint32_t n_cells,
                           const void *e1d, int dim)
  {
    if (n_cells == 0)
      return true;
    bool launched = false;
    dispatch_degree(pf, [&](auto PF) {
      dispatch_degree(pc, [&](auto PC) {
        if constexpr (PC.value < PF.value)
          dispatch_number(number, [&](auto t) {
            launched = dispatch_mode<2, 3>(dim, [&](auto DIM) {
              using T           = decltype(t);
              using C           = DGPTransferCfg<PF.value, PC.value, T, DIM.value>;
              const uint32_t nb = (n_cells + C::CPB - 1) / C::CPB;
              if (prolong)
                hipLaunchKernelGGL((dg_ptransfer_kernel<PF.value, PC.value, T, true, DIM.value>), dim3(nb), dim3(C::THREADS), 0, s,
                                   (T *)dst, (const T *)src, n_cells, (const T *)e1d);
              else
                hipLaunchKernelGGL((dg_ptransfer_kernel<PF.value, PC.value, T, false, DIM.value>), dim3(nb), dim3(C::THREADS), 0, s,
                                   (T *)dst, (const T *)src, n_cells, (const T *)e1d);
            });
          });
      });
    });
    return launched;
  }
} // namespace mgx
