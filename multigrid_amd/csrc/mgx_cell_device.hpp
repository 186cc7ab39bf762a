// mgx_cell_device.hpp -- device helpers of the per-cell kernels (mgx_kernels.hip, mgx_nonlinear.hip): the thread
// mapping of a cell, the in-register line products and the gather / scatter of an x-line through the reference's
// 27-entry compressed index table.
#pragma once

#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
#ifndef MGX_GENERAL_WG_THREADS
#define MGX_GENERAL_WG_THREADS 256 // 128 measured: no gain
#endif
  template <int P, int WG = 256>
  struct Cfg
  {
    static constexpr int N        = P + 1;
    static constexpr int LN       = N | 1; // x-line pitch, odd => conflict-free ds_read_b64
    static constexpr int TPC      = N * N; // threads per cell
    static constexpr int CPB      = (WG / TPC) < 1 ? 1 : (WG / TPC);
    static constexpr int THREADS  = ((CPB * TPC + 63) / 64) * 64;
    static constexpr int CELL_LDS = N * N * LN;
  };

  // out[a] = sum_b M[a*N+b] in[b]
  template <int N, typename T>
  __device__ __forceinline__ void mv(const T *__restrict__ M, const T (&in)[N], T (&out)[N])
  {
#pragma unroll
    for (int a = 0; a < N; ++a)
      {
        T s = M[a * N] * in[0];
#pragma unroll
        for (int b = 1; b < N; ++b)
          s = fma(M[a * N + b], in[b], s);
        out[a] = s;
      }
  }

  // out[a] = sum_b M[b*N+a] in[b]
  template <int N, typename T>
  __device__ __forceinline__ void mvT(const T *__restrict__ M, const T (&in)[N], T (&out)[N])
  {
#pragma unroll
    for (int a = 0; a < N; ++a)
      {
        T s = M[a] * in[0];
#pragma unroll
        for (int b = 1; b < N; ++b)
          s = fma(M[b * N + a], in[b], s);
        out[a] = s;
      }
  }

  // entity code (0 = low vertex plane, 1 = interior, 2 = high) and offset inside the entity of
  // the 1D node index j (vector_access_reduced.h:232-247): the device copy of the host's one node rule, mgx::node_entity
  // (mgx_index_tables.hpp), which the tables these kernels read are built with
  template <int P>
  __device__ __forceinline__ void node_code(int j, int &code, int &offs)
  {
    code = (j == 0) ? 0 : (j == P ? 2 : 1);
    offs = (code == 1) ? j - 1 : 0;
  }

  template <int P>
  struct LineIndex
  {
    uint32_t b0, b1, b2; // first DoF of the left / interior / right entity of this x-line
    uint32_t off;        // offset of the line inside those entities
  };

  // address computation of read_dof_values_compressed for the x-line (j,k) of `cell`
  // (vector_access_reduced.h:153-229)
  template <int P>
  __device__ __forceinline__ LineIndex<P> line_index(const uint32_t *__restrict__ idx27, uint32_t cell, int j,
                                                     int k)
  {
    int cy, oy, cz, oz;
    node_code<P>(j, cy, oy);
    node_code<P>(k, cz, oz);
    LineIndex<P>    L;
    const uint32_t *ind = idx27 + 27u * (size_t)cell + 3 * (3 * cz + cy);
    L.b0                = ind[0];
    L.b1                = ind[1];
    L.b2                = ind[2];
    L.off               = (uint32_t)((cy == 1 ? P - 1 : 1) * oz + oy);
    return L;
  }

  template <int P, typename T>
  __device__ __forceinline__ void gather_line(const T *__restrict__ src, const LineIndex<P> &L, T (&r)[P + 1])
  {
    r[0] = L.b0 != kInvalid ? src[L.b0 + L.off] : T(0);
#pragma unroll
    for (int i = 0; i < P - 1; ++i)
      r[1 + i] = L.b1 != kInvalid ? src[L.b1 + L.off * (uint32_t)(P - 1) + (uint32_t)i] : T(0);
    r[P] = L.b2 != kInvalid ? src[L.b2 + L.off] : T(0);
  }

  template <int P, typename T>
  __device__ __forceinline__ void scatter_add_line(T *__restrict__ dst, const LineIndex<P> &L,
                                                   const T (&r)[P + 1])
  {
    if (L.b0 != kInvalid)
      unsafeAtomicAdd(&dst[L.b0 + L.off], r[0]);
    if (L.b1 != kInvalid)
      {
#pragma unroll
        for (int i = 0; i < P - 1; ++i)
          unsafeAtomicAdd(&dst[L.b1 + L.off * (uint32_t)(P - 1) + (uint32_t)i], r[1 + i]);
      }
    if (L.b2 != kInvalid)
      unsafeAtomicAdd(&dst[L.b2 + L.off], r[P]);
  }

  // the same without atomics: for launches over cells of one colour (no two of them share a DoF)
  template <int P, typename T>
  __device__ __forceinline__ void scatter_add_line_plain(T *__restrict__ dst, const LineIndex<P> &L,
                                                         const T (&r)[P + 1])
  {
    if (L.b0 != kInvalid)
      dst[L.b0 + L.off] += r[0];
    if (L.b1 != kInvalid)
      {
#pragma unroll
        for (int i = 0; i < P - 1; ++i)
          dst[L.b1 + L.off * (uint32_t)(P - 1) + (uint32_t)i] += r[1 + i];
      }
    if (L.b2 != kInvalid)
      dst[L.b2 + L.off] += r[P];
  }

  // Ordered assembly (levels without a brick schedule): instead of adding into the vector, a cell
  // stores its (p+1)^3 local results at scratch[cell (p+1)^3 + (k n + j) n + i]; assemble_kernel
  // below then adds, for every DoF, its contributions in ascending cell order -- no atomics, the
  // sum does not depend on the order in which the workgroups happen to run
  template <int P, typename T>
  __device__ __forceinline__ void store_line_local(T *__restrict__ scratch, uint32_t cell, int j, int k,
                                                   const T (&r)[P + 1])
  {
    constexpr int N = P + 1;
    T            *o = scratch + (size_t)cell * (N * N * N) + (size_t)((k * N + j) * N);
#pragma unroll
    for (int i = 0; i < N; ++i)
      o[i] = r[i];
  }
} // namespace mgx
