// mgx_cell_device_2d.hpp -- device helpers of the per-cell kernels on quadrilaterals (mgx_kernels_2d.hip,
// mgx_nonlinear_2d.hip): the thread mapping of a cell, the line products in their unrolled and rolled forms, and the
// gather / scatter of a cell through the 9-entry compressed index table.
#pragma once

#include "mgx_cell_device.hpp"
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  template <int P>
  struct Cfg2
  {
    static constexpr int N        = P + 1;
    static constexpr int N2       = N * N;
    static constexpr int LN       = N | 1; // line pitch, odd
    static constexpr int CPB      = 256 / N; // cells per workgroup
    static constexpr int THREADS  = ((CPB * N + 63) / 64) * 64;
    static constexpr int CELL_LDS = N * LN;
  };

  // the forms of the cell loop (mgx_kernels_2d.hip) and of its residual form (mgx_rhs_2d.hip)
  enum CellForm2
  {
    kDiagonalCoefficient = 0, // coef [xx,yy], weight per point
    kTensorPerMesh       = 1, // coef [xx,yy,xy] (affine cells), weight per point
    kTensorPerPoint      = 2  // coef_q [cell][3][n^2], weight folded in
  };
  inline int cell_form(const OperatorData &op)
  {
    return op.coef_q ? kTensorPerPoint : (op.full_tensor ? kTensorPerMesh : kDiagonalCoefficient);
  }
  // the lists of a launcher: none, once over all cells into the scratch array of the ordered assembly, where the operator
  // has one; else its cell colours (operator_create has made sure that a level without the tables is coloured)
  inline CellLists cell_lists_2d(const OperatorData &op) { return op.asm_start ? CellLists() : op.cell_colours.lists(); }

  // Line products of the cell loop.  An n x n matrix of doubles is 2 n^2 scalar registers when its product with a line is
  // unrolled: at n >= 9 that is more than a wave has (the compiler then parks them in vector registers lane by lane).
  // Those instantiations (ROLLED) take the line from LDS value by value in a loop that is not unrolled and keep only
  // one column (row, transposed) of the matrix in scalar registers at a time; the sums are formed in the same order.
  template <int P, typename T>
  constexpr bool rolled_products()
  {
    return sizeof(T) == 8 && P >= 8;
  }
  // out = M line (TR: M^T line), line[i * stride] in LDS
  template <int N, typename T, bool TR, bool ROLLED>
  __device__ __forceinline__ void lds_product(const T *__restrict__ M, const T *line, int stride, T (&out)[N])
  {
    if constexpr (ROLLED)
      {
#pragma unroll
        for (int a = 0; a < N; ++a)
          out[a] = T(0);
#pragma unroll 1
        for (int b = 0; b < N; ++b)
          {
            const T x = line[b * stride];
#pragma unroll
            for (int a = 0; a < N; ++a)
              out[a] = fma(TR ? M[b * N + a] : M[a * N + b], x, out[a]);
          }
      }
    else
      {
        T in[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
          in[i] = line[i * stride];
        if (TR)
          mvT<N, T>(M, in, out);
        else
          mv<N, T>(M, in, out);
      }
  }
  // the same for a line held in registers; ROLLED: through the LDS line `park`, which the thread owns at this point
  template <int N, typename T, bool TR, bool ROLLED>
  __device__ __forceinline__ void reg_product(const T *__restrict__ M, const T (&in)[N], T *park, int stride, T (&out)[N])
  {
    if constexpr (ROLLED)
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          park[i * stride] = in[i];
        lds_product<N, T, TR, true>(M, park, stride, out);
      }
    else if (TR)
      mvT<N, T>(M, in, out);
    else
      mv<N, T>(M, in, out);
  }

  // the x-line j of a cell: first DoF of its left / interior / right entity and the offset of the line inside the left
  // and right ones (the interior of a y-line); the interior entity is an x-line (j = 0, p) or the quad interior
  template <int P>
  __device__ __forceinline__ LineIndex<P> line_index_2d(const uint32_t *__restrict__ idx9, uint32_t cell, int j)
  {
    int cy, oy;
    node_code<P>(j, cy, oy);
    const uint32_t *ind = idx9 + 9u * (size_t)cell + 3 * cy;
    LineIndex<P>    L;
    L.b0  = ind[0];
    L.b1  = ind[1];
    L.b2  = ind[2];
    L.off = (uint32_t)oy;
    return L;
  }

  // nodal values of a cell into its LDS tile, tile[j * LN + i]; thread t of the cell's n (constrained entity: zero)
  template <int P, typename T>
  __device__ __forceinline__ void gather_cell_2d(const T *__restrict__ src, const uint32_t *__restrict__ ix, int t,
                                                 T *__restrict__ tile)
  {
    constexpr int N = P + 1, LN = N | 1, I = P - 1;
    int           cy, oy;
    node_code<P>(t, cy, oy);
    const uint32_t b0 = ix[3 * cy], b2 = ix[3 * cy + 2];
    tile[t * LN]     = b0 != kInvalid ? src[b0 + (uint32_t)oy] : T(0);
    tile[t * LN + P] = b2 != kInvalid ? src[b2 + (uint32_t)oy] : T(0);
    if constexpr (P > 1)
      {
        if (cy != 1) // the bottom and the top x-line
          {
            const uint32_t b1 = ix[3 * cy + 1];
#pragma unroll
            for (int i = 0; i < I; ++i)
              tile[t * LN + 1 + i] = b1 != kInvalid ? src[b1 + (uint32_t)i] : T(0);
          }
        const uint32_t bi = ix[4];
#pragma unroll
        for (int e0 = 0; e0 < I * I; e0 += N)
          {
            const int e = e0 + t;
            if (e < I * I)
              tile[(1 + e / I) * LN + 1 + e % I] = bi != kInvalid ? src[bi + (uint32_t)e] : T(0);
          }
      }
  }

  // dst += the tile, the same way; the cells of the launch share no DoF
  template <int P, typename T>
  __device__ __forceinline__ void scatter_add_cell_2d(T *__restrict__ dst, const uint32_t *__restrict__ ix, int t,
                                                      const T *__restrict__ tile)
  {
    constexpr int N = P + 1, LN = N | 1, I = P - 1;
    int           cy, oy;
    node_code<P>(t, cy, oy);
    const uint32_t b0 = ix[3 * cy], b2 = ix[3 * cy + 2];
    if (b0 != kInvalid)
      dst[b0 + (uint32_t)oy] += tile[t * LN];
    if (b2 != kInvalid)
      dst[b2 + (uint32_t)oy] += tile[t * LN + P];
    if constexpr (P > 1)
      {
        if (cy != 1)
          {
            const uint32_t b1 = ix[3 * cy + 1];
            if (b1 != kInvalid)
              {
#pragma unroll
                for (int i = 0; i < I; ++i)
                  dst[b1 + (uint32_t)i] += tile[t * LN + 1 + i];
              }
          }
        const uint32_t bi = ix[4];
        if (bi != kInvalid)
          {
#pragma unroll
            for (int e0 = 0; e0 < I * I; e0 += N)
              {
                const int e = e0 + t;
                if (e < I * I)
                  dst[bi + (uint32_t)e] += tile[(1 + e / I) * LN + 1 + e % I];
              }
          }
      }
  }

  // The n^2 results of every cell of a workgroup into the scratch array of the ordered assembly: the cells of the
  // workgroup are consecutive, so their values are one contiguous run; tiles: [cell][CELL_LDS] from `tiles`
  template <int P, typename T>
  __device__ __forceinline__ void store_tiles_2d(T *__restrict__ scratch, const T *tiles, uint32_t n_cells, int tid)
  {
    using C              = Cfg2<P>;
    const uint32_t cell0 = blockIdx.x * C::CPB;
    const uint32_t left  = n_cells - cell0;
    const int      count = (int)(left < (uint32_t)C::CPB ? left : (uint32_t)C::CPB) * C::N2;
    T             *o     = scratch + (size_t)cell0 * C::N2;
    for (int f = tid; f < count; f += C::THREADS)
      {
        const int c = f / C::N2, e = f - c * C::N2;
        o[f]        = tiles[c * C::CELL_LDS + (e / C::N) * C::LN + e % C::N];
      }
  }
} // namespace mgx
