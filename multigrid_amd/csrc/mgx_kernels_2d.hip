// mgx_kernels_2d.hip -- the FE_Q Laplace operator on quadrilaterals (mgx_operator_desc::dim == 2): cell loop in its
// three forms, diagonal, and the level transfers.  The design of mgx_kernels.hip one dimension down.
//
// Mapping: a cell of FE_Q(p) has n^2 = (p+1)^2 points.  ONE thread owns one line of n values in registers, n threads
// own a cell, and a 256-thread workgroup packs floor(256 / n) cells (p = 4: 51 cells = 255 threads).  A sweep along the
// line a thread holds is an in-register (n x n)(n) product with wave-uniform matrix entries; between an x-sweep and a
// y-sweep the cell is transposed through an LDS tile with the odd line pitch n | 1 (rows are written and read with
// unit stride, columns with an odd stride: no bank is hit twice by the lanes of a cell).
//
// Gather and scatter go through the 9-entry compressed index table (the rule of vector_access_reduced.h with two
// codes).  The quad interior of a cell is ONE contiguous block of (p-1)^2 DoFs: the n threads of a cell move it with
// unit stride (element e by thread e mod n) into the LDS tile instead of every thread walking its own line of p-1
// values at a stride of p-1 between lanes, which would touch (p-1) times as many memory lines per load instruction.
// Edges and vertices are moved by the thread that owns their line.  The results leave the same way; into the scratch
// array of the ordered assembly the whole workgroup stores its cells' n^2 values each as one contiguous run.
//
// No kernel of this unit uses an atomic: the cells are added up by assemble_kernel / assemble_cheb_kernel in cell order
// or by launches over cells of one colour, the restriction by launches over parents of one colour.
#include "mgx_index_tables.hpp" // kWeightZero2D
#include "mgx_internal.hpp"
#include "mgx_cell_device_2d.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  // ------------------------------------------------------------------------------------------
  // Cell loop: local_apply of laplace_operator.h:527-558 with the quadrature-point operation :436-523 in two
  // dimensions.  Thread t of a cell is the row thread of x-line / quadrature row t and the column thread of column t.
  //   rows:    nodal -> quadrature along x
  //   columns: ... along y (u at the points of the column); y-derivative of the column in registers
  //   kDiagonalCoefficient: the y part c1 w D^T D is finished in the column's registers; rows: x part c0 w D^T D;
  //     columns: sum, S^T along y; rows: S^T along x.  Four transpositions.
  //   tensor forms: the x-derivative (rows) meets the y-derivative at the column thread through LDS, which applies
  //     the tensor (as cell_loop_general_kernel does for z-lines) and hands the x part of the flux back.  Five.
  // scratch: the n^2 results of every cell to the ordered assembly (no cell_list then); else cell_list: cells of one
  // colour, added to dst with plain read-modify-writes.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, int FORM>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    cell_loop_2d_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ idx9, uint32_t n_cells,
                        const Basis1D<T> *__restrict__ B, const T *__restrict__ coef_q, T c0, T c1, T c2,
                        const uint32_t *__restrict__ cell_list, T *__restrict__ scratch)
  {
    using C          = Cfg2<P>;
    constexpr int N  = C::N, LN = C::LN, N2 = C::N2;
    constexpr bool TENSOR = FORM != kDiagonalCoefficient;
    constexpr bool ROLLED = rolled_products<P, T>();
    constexpr bool TWO    = TENSOR || ROLLED; // a second tile: the x part of the flux / parked lines
    __shared__ T U[C::CPB * C::CELL_LDS];
    __shared__ T GX[TWO ? C::CPB * C::CELL_LDS : 1];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / N;
    const int      t      = tid - lc * N;
    const uint32_t pos    = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (pos < n_cells);
    const uint32_t cell   = (cell_list && active) ? cell_list[pos] : pos;
    const int      slot   = lc < C::CPB ? lc : 0;
    T             *Uc     = U + slot * C::CELL_LDS;
    T             *Xc     = GX + (TWO ? slot * C::CELL_LDS : 0);
    const int      row = t * LN, col = t;
    T              r[N], q[N], vy[N];

    if (active)
      gather_cell_2d<P, T>(src, idx9 + 9u * (size_t)cell, t, Uc);
    __syncthreads();
    if (active) // nodal -> quadrature along x
      {
        lds_product<N, T, false, ROLLED>(B->S, Uc + row, 1, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[row + i] = q[i];
      }
    __syncthreads();
    if (active) // along y; the y-derivative of this column
      {
        lds_product<N, T, false, ROLLED>(B->S, Uc + col, LN, q);
#pragma unroll
        for (int j = 0; j < N; ++j)
          Uc[col + j * LN] = q[j];
        reg_product<N, T, false, ROLLED>(B->D, q, Uc + col, LN, r); // (ROLLED: the column already holds q)
        if (!TENSOR)
          {
            const T f = c1 * B->w[t];
#pragma unroll
            for (int j = 0; j < N; ++j)
              r[j] *= f * B->w[j];
            reg_product<N, T, true, ROLLED>(B->D, r, Xc + col, LN, vy);
          }
        else
          {
#pragma unroll
            for (int j = 0; j < N; ++j)
              vy[j] = r[j];
          }
      }
    __syncthreads();
    if (active) // the x-derivative of this row
      {
        lds_product<N, T, false, ROLLED>(B->D, Uc + row, 1, r);
        if (!TENSOR)
          {
            const T f = c0 * B->w[t];
#pragma unroll
            for (int i = 0; i < N; ++i)
              r[i] *= f * B->w[i];
            reg_product<N, T, true, ROLLED>(B->D, r, Xc + row, 1, q);
#pragma unroll
            for (int i = 0; i < N; ++i)
              Uc[row + i] = q[i];
          }
        else
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              Xc[row + i] = r[i];
          }
      }
    __syncthreads();
    if (TENSOR)
      {
        if (active) // the tensor at the n points (t, j) of this column
          {
            const T *cq = coef_q + (size_t)cell * 3 * N2 + (size_t)t;
#pragma unroll
            for (int j = 0; j < N; ++j)
              {
                T t0, t1, t2;
                if (FORM == kTensorPerPoint)
                  t0 = cq[j * N], t1 = cq[N2 + j * N], t2 = cq[2 * N2 + j * N];
                else
                  {
                    const T w = B->w[t] * B->w[j];
                    t0 = c0 * w, t1 = c1 * w, t2 = c2 * w;
                  }
                const T gx = Xc[col + j * LN], gy = vy[j];
                Xc[col + j * LN] = t0 * gx + t2 * gy;
                r[j]             = t2 * gx + t1 * gy;
              }
            reg_product<N, T, true, ROLLED>(B->D, r, Uc + col, LN, vy); // (the values in U have been used up)
          }
        __syncthreads();
        if (active) // transposed x-derivative
          {
            lds_product<N, T, true, ROLLED>(B->D, Xc + row, 1, q);
#pragma unroll
            for (int i = 0; i < N; ++i)
              Uc[row + i] = q[i];
          }
        __syncthreads();
      }
    if (active) // add the y part, quadrature -> nodal along y
      {
#pragma unroll
        for (int j = 0; j < N; ++j)
          r[j] = Uc[col + j * LN] + vy[j];
        reg_product<N, T, true, ROLLED>(B->S, r, Uc + col, LN, q);
#pragma unroll
        for (int j = 0; j < N; ++j)
          Uc[col + j * LN] = q[j];
      }
    __syncthreads();
    if (active) // along x
      {
        lds_product<N, T, true, ROLLED>(B->S, Uc + row, 1, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[row + i] = q[i];
      }
    __syncthreads();
    if (scratch)
      {
        // the cells of the workgroup are consecutive: their n^2 values each are one contiguous run of the scratch array
        const uint32_t cell0 = blockIdx.x * C::CPB;
        const uint32_t left  = n_cells - cell0;
        const int      count = (int)(left < (uint32_t)C::CPB ? left : (uint32_t)C::CPB) * N2;
        T             *o     = scratch + (size_t)cell0 * N2;
        for (int f = tid; f < count; f += C::THREADS)
          {
            const int c = f / N2, e = f - c * N2;
            o[f]        = U[c * C::CELL_LDS + (e / N) * LN + e % N];
          }
      }
    else if (active)
      scatter_add_cell_2d<P, T>(dst, idx9 + 9u * (size_t)cell, t, Uc);
  }

  // ------------------------------------------------------------------------------------------
  // Diagonal of the cell matrix (local_compute_diagonal, laplace_operator.h:770-800), one thread per x-line j of a cell.
  // Diagonal coefficient: d_ij = c0 a[i] m[j] + c1 m[i] a[j] with a[i] = sum_q w_q (dphi_i(x_q))^2, m[i] = sum_q w_q
  // phi_i(x_q)^2.  Tensor forms: d_ij = sum_q C(q) : grad phi_ij(q) grad phi_ij(q) from S and G = D S.
  // ------------------------------------------------------------------------------------------
  template <typename T>
  struct Diag1D2
  {
    T a[kMaxN], m[kMaxN];
  };

  template <int P, typename T, int FORM>
  __global__ void __launch_bounds__(256)
    cell_diagonal_2d_kernel(T *__restrict__ diag, const uint32_t *__restrict__ idx9, uint32_t n_cells, Diag1D2<T> d1,
                            const Basis1D<T> *__restrict__ B, const T *__restrict__ G1, const T *__restrict__ coef_q, T c0,
                            T c1, T c2, const uint32_t *__restrict__ cell_list, T *__restrict__ scratch)
  {
    constexpr int  N = P + 1, N2 = N * N;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pos = gid / N;
    if (pos >= n_cells)
      return;
    const uint32_t cell = cell_list ? cell_list[pos] : pos;
    const int      j    = gid % N;
    T              r[N];
    if (FORM == kDiagonalCoefficient)
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          r[i] = c0 * d1.a[i] * d1.m[j] + c1 * d1.m[i] * d1.a[j];
      }
    else
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          r[i] = T(0);
        const T *cq = coef_q + (size_t)cell * 3 * N2;
        // (not unrolled: the n^2 entries of S and G a full unrolling asks for at once do not fit the scalar registers)
#pragma unroll 1
        for (int qy = 0; qy < N; ++qy)
          {
            const T sy = B->S[qy * N + j], gy1 = G1[qy * N + j];
#pragma unroll 1
            for (int qx = 0; qx < N; ++qx)
              {
                T t0, t1, t2;
                if (FORM == kTensorPerPoint)
                  t0 = cq[qy * N + qx], t1 = cq[N2 + qy * N + qx], t2 = cq[2 * N2 + qy * N + qx];
                else
                  {
                    const T w = B->w[qx] * B->w[qy];
                    t0 = c0 * w, t1 = c1 * w, t2 = c2 * w;
                  }
#pragma unroll
                for (int i = 0; i < N; ++i)
                  {
                    const T dx = G1[qx * N + i] * sy, dy = B->S[qx * N + i] * gy1;
                    r[i] += t0 * dx * dx + t1 * dy * dy + T(2) * t2 * dx * dy;
                  }
              }
          }
      }
    if (scratch)
      {
        T *o = scratch + (size_t)cell * N2 + (size_t)(j * N);
#pragma unroll
        for (int i = 0; i < N; ++i)
          o[i] = r[i];
        return;
      }
    scatter_add_line_plain<P, T>(diag, line_index_2d<P>(idx9, cell, j), r);
  }

  // ------------------------------------------------------------------------------------------
  // Transfers (MGTransferMatrixFree), one workgroup per parent: the (p+1)^2 coarse values are taken to the (2p+1)^2
  // points of the children patch by two LDS-staged sweeps with the dense embedding P1 -- correct for every embedding,
  // symmetric under reversal or not.
  // ------------------------------------------------------------------------------------------
  template <int P>
  struct TCfg2
  {
    static constexpr int N       = P + 1;
    static constexpr int M       = 2 * P + 1;
    static constexpr int THREADS = ((M * M + 63) / 64) * 64 > 256 ? 256 : ((M * M + 63) / 64) * 64;
  };

  template <int P>
  __device__ __forceinline__ int patch_code_2d(int a)
  {
    return a == 0 ? 0 : (a == 2 * P ? 2 : 1);
  }

  // weight of the restriction from a byte of TransferData::weight_shift: 2^-shift for 0, 1, 2 (1 / (1 << shift), as ever),
  // 0 for kWeightZero2D; the division is not guarded by the comparison, so the compiler selects and does not branch
  template <typename T>
  __device__ __forceinline__ T restrict_weight_2d(uint8_t shift)
  {
    const T w = T(1) / T(1 << (shift & 3));
    return shift == kWeightZero2D ? T(0) : w;
  }

  // Every fine DoF is written by exactly one fine cell, the first (in cell order) that contains its entity (own9, from
  // the fine index table), hence by one parent.  The values the parents compute for a shared DoF are bitwise the
  // same (the rows of P1 at coinciding nodes are exact unit vectors).
  template <int P, typename T>
  __global__ void __launch_bounds__(TCfg2<P>::THREADS)
    prolongate_2d_kernel(T *__restrict__ fine, const T *__restrict__ coarse, const uint32_t *__restrict__ idx_c,
                         const uint32_t *__restrict__ idx_f, const uint32_t *__restrict__ children,
                         const uint32_t *__restrict__ own9, uint32_t n_parents, const Basis1D<T> *__restrict__ B, int add)
  {
    constexpr int N = P + 1, M = 2 * P + 1;
    __shared__ T  p1[M * N];
    __shared__ T  in[N * N];
    __shared__ T  t1[N * M];
    __shared__ T  out[M * M];
    const uint32_t pc = blockIdx.x;
    if (pc >= n_parents)
      return;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < M * N; i += nt)
      p1[i] = B->P1[i];
    for (int j = tid; j < N; j += nt)
      {
        T r[N];
        gather_line<P, T>(coarse, line_index_2d<P>(idx_c, pc, j), r);
#pragma unroll
        for (int i = 0; i < N; ++i)
          in[j * N + i] = r[i];
      }
    __syncthreads();
    for (int o = tid; o < N * M; o += nt) // x: [j][a]
      {
        const int a = o % M, j = o / M;
        T         s = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
          s = fma(p1[a * N + i], in[j * N + i], s);
        t1[o] = s;
      }
    __syncthreads();
    for (int o = tid; o < M * M; o += nt) // y: [b][a]
      {
        const int a = o % M, b = o / M;
        T         s = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
          s = fma(p1[b * N + j], t1[j * M + a], s);
        out[o] = s;
      }
    __syncthreads();
    for (int w = tid; w < 4 * N; w += nt)
      {
        const int          ch = w / N, j = w % N;
        const uint32_t     fc = children[4u * (size_t)pc + ch];
        const int          ox = (ch & 1) * P, b = (ch >> 1) * P + j;
        const LineIndex<P> L  = line_index_2d<P>(idx_f, fc, j);
        int                cy, oy;
        node_code<P>(j, cy, oy);
        const uint32_t own = own9[fc] >> (3 * cy); // bits 0, 1, 2: left, interior, right entity of the line
        if (L.b0 != kInvalid && (own & 1u))
          {
            T *p = fine + L.b0 + L.off;
            *p   = add ? *p + out[b * M + ox] : out[b * M + ox];
          }
        if (L.b1 != kInvalid && (own & 2u))
          {
#pragma unroll
            for (int i = 0; i < P - 1; ++i)
              {
                T *p = fine + L.b1 + L.off * (uint32_t)(P - 1) + (uint32_t)i;
                *p   = add ? *p + out[b * M + ox + 1 + i] : out[b * M + ox + 1 + i];
              }
          }
        if (L.b2 != kInvalid && (own & 4u))
          {
            T *p = fine + L.b2 + L.off;
            *p   = add ? *p + out[b * M + ox + P] : out[b * M + ox + P];
          }
      }
  }

  // coarse += P^T (weights .* fine): the launch covers the parents parent_list[0 .. n_parents) of one colour (they share
  // no coarse DoF), plain read-modify-writes.  wshift [n_parents][9], one byte per entity of the parent: 0, 1, 2 = the
  // weight 2^-shift of a regular mesh; kWeightZero2D = weight 0, the owner rule of a mesh with three or five cells around
  // a vertex (another parent restricts the fine DoFs of that entity, with shift 0).
  template <int P, typename T>
  __global__ void __launch_bounds__(TCfg2<P>::THREADS)
    restrict_2d_kernel(T *__restrict__ coarse, const T *__restrict__ fine, const uint32_t *__restrict__ idx_c,
                       const uint32_t *__restrict__ idx_f, const uint32_t *__restrict__ children,
                       const uint8_t *__restrict__ wshift, const uint32_t *__restrict__ parent_list, uint32_t n_parents,
                       const Basis1D<T> *__restrict__ B)
  {
    constexpr int N = P + 1, M = 2 * P + 1;
    __shared__ T  p1[M * N];
    __shared__ T  in[N * N];
    __shared__ T  t1[N * M];
    __shared__ T  out[M * M];
    if (blockIdx.x >= n_parents)
      return;
    const uint32_t pc  = parent_list[blockIdx.x];
    const int      tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < M * N; i += nt)
      p1[i] = B->P1[i];
    // the weighted fine patch (points that two children hold are written twice with the same value)
    for (int w = tid; w < 4 * N; w += nt)
      {
        const int      ch = w / N, j = w % N;
        const uint32_t fc = children[4u * (size_t)pc + ch];
        const int      ox = (ch & 1) * P, b = (ch >> 1) * P + j;
        T              r[N];
        gather_line<P, T>(fine, line_index_2d<P>(idx_f, fc, j), r);
        // (the three weights of the line first, without a branch: the byte loads are in flight together)
        const uint8_t *ws = wshift + 9u * (size_t)pc + 3 * patch_code_2d<P>(b);
        const T        w0 = restrict_weight_2d<T>(ws[0]), w1 = restrict_weight_2d<T>(ws[1]), w2 = restrict_weight_2d<T>(ws[2]);
#pragma unroll
        for (int i = 0; i < N; ++i)
          {
            const int c = patch_code_2d<P>(ox + i);
            out[b * M + ox + i] = r[i] * (c == 0 ? w0 : (c == 2 ? w2 : w1));
          }
      }
    __syncthreads();
    for (int o = tid; o < N * M; o += nt) // y^T: [j][a]
      {
        const int a = o % M, j = o / M;
        T         s = 0;
#pragma unroll
        for (int b = 0; b < M; ++b)
          s = fma(p1[b * N + j], out[b * M + a], s);
        t1[o] = s;
      }
    __syncthreads();
    for (int o = tid; o < N * N; o += nt) // x^T: [j][i]
      {
        const int i = o % N, j = o / N;
        T         s = 0;
#pragma unroll
        for (int a = 0; a < M; ++a)
          s = fma(p1[a * N + i], t1[j * M + a], s);
        in[o] = s;
      }
    __syncthreads();
    for (int j = tid; j < N; j += nt)
      {
        T r[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
          r[i] = in[j * N + i];
        scatter_add_line_plain<P, T>(coarse, line_index_2d<P>(idx_c, pc, j), r);
      }
  }

  // ------------------------------------------------------------------------------------------
  // Transfer between the DG space and the FE_Q space of the same mesh and degree, cell by cell: dg_cg_transfer_kernel of
  // mgx_kernels.hip one dimension down (laplace_operator_dg.h:1798-1819 residual -> FE_Q, :1863-1894 FE_Q -> DG).  The
  // DG vector holds (p+1)^2 contiguous values per cell, cells in the order of the index table; P1 [n][n] takes the
  // values in the Gauss-Lobatto nodes to the coefficients of the DG basis.
  // TO_DG: dg[cell] += (P1 x P1) c[cell]   else: cg += (P1 x P1)^T dg[cell], constrained rows skipped.
  // The cells of a launch are cell_list[i] or cell_first + cell_stride * i, i < n_cells; those of a restriction share no
  // FE_Q DoF (the caller's launches see to it): plain read-modify-writes, no atomics.
  // Thread t of a cell: the x-product on the x-line t, one transposition through the cell's tile, the y-product on the
  // y-line t.  The FE_Q side goes through the tile (gather_cell_2d / scatter_add_cell_2d); the DG side is read by
  // x-lines and written by y-lines, so the lanes of a cell touch consecutive words.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, bool TO_DG>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    dg_cg_transfer_kernel_2d(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ idx9, uint32_t n_cells,
                             const T *__restrict__ P1, const uint32_t *__restrict__ cell_list, uint32_t cell_first,
                             uint32_t cell_stride)
  {
    using C               = Cfg2<P>;
    constexpr int  N      = C::N, LN = C::LN, N2 = C::N2;
    constexpr bool ROLLED = rolled_products<P, T>();
    __shared__ T   U[C::CPB * C::CELL_LDS];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / N;
    const int      t      = tid - lc * N;
    const uint32_t pos    = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (pos < n_cells);
    // (inactive threads name no cell: they only meet the barriers)
    const uint32_t cell = !active ? 0u : (cell_list ? cell_list[pos] : cell_first + cell_stride * pos);
    T             *Uc   = U + (lc < C::CPB ? lc : 0) * C::CELL_LDS;
    const int      row = t * LN, col = t;
    T              r[N], q[N];

    if constexpr (TO_DG)
      {
        if (active)
          gather_cell_2d<P, T>(src, idx9 + 9u * (size_t)cell, t, Uc);
        __syncthreads();
        if (active) // along x
          {
            lds_product<N, T, false, ROLLED>(P1, Uc + row, 1, q);
#pragma unroll
            for (int i = 0; i < N; ++i)
              Uc[row + i] = q[i];
          }
        __syncthreads();
        if (active) // along y; entry (j, t) of the cell
          {
            lds_product<N, T, false, ROLLED>(P1, Uc + col, LN, q);
            T *d = dst + (size_t)cell * N2 + (size_t)t;
#pragma unroll
            for (int j = 0; j < N; ++j)
              d[j * N] += q[j];
          }
      }
    else
      {
        if (active) // along x
          {
            const T *s = src + (size_t)cell * N2 + (size_t)(t * N);
#pragma unroll
            for (int i = 0; i < N; ++i)
              r[i] = s[i];
            reg_product<N, T, true, ROLLED>(P1, r, Uc + row, 1, q);
#pragma unroll
            for (int i = 0; i < N; ++i)
              Uc[row + i] = q[i];
          }
        __syncthreads();
        if (active) // along y
          {
            lds_product<N, T, true, ROLLED>(P1, Uc + col, LN, q);
#pragma unroll
            for (int j = 0; j < N; ++j)
              Uc[col + j * LN] = q[j];
          }
        __syncthreads();
        if (active)
          scatter_add_cell_2d<P, T>(dst, idx9 + 9u * (size_t)cell, t, Uc);
      }
  }

  // ------------------------------------------------------------------------------------------
  // launchers
  // ------------------------------------------------------------------------------------------
  template <int P, typename T>
  static void cell_loop_2d_t(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *tail_src,
                             uint32_t n_head, const ChebPost *post)
  {
    using C = Cfg2<P>;
    T *scratch = for_each_cell_list<T>(op, cell_lists_2d(op), true, [&](const uint32_t *list, uint32_t count, T *scr) {
      const uint32_t nb = (count + C::CPB - 1) / C::CPB;
      dispatch_mode<kDiagonalCoefficient, kTensorPerMesh, kTensorPerPoint>(cell_form(op), [&](auto FORM) {
        hipLaunchKernelGGL((cell_loop_2d_kernel<P, T, FORM.value>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src,
                           op.idx27, count, (const Basis1D<T> *)op.basis, (const T *)op.coef_q, (T)op.coef[0], (T)op.coef[1],
                           (T)op.coef[2], list, scr);
      });
    });
    if (scratch && post)
      launch_assemble_cheb(s, op, dst, n_head, *post);
    else if (scratch)
      launch_assemble(s, op, 0, dst, tail_src, n_head);
  }

  void launch_cell_loop_2d(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *tail_src,
                           uint32_t n_head, const ChebPost *post)
  {
    dispatch_number_degree(op.number, op.p, [&](auto t, auto P) {
      cell_loop_2d_t<P.value, decltype(t)>(s, op, dst, src, tail_src, n_head, post);
    });
  }

  template <int P, typename T>
  static void cell_diag_2d_t(hipStream_t s, const OperatorData &op, void *diag, const double *a, const double *m)
  {
    constexpr int N = P + 1;
    Diag1D2<T>    d1;
    for (int i = 0; i < N; ++i)
      {
        d1.a[i] = (T)a[i];
        d1.m[i] = (T)m[i];
      }
    T *scratch = for_each_cell_list<T>(op, cell_lists_2d(op), true, [&](const uint32_t *list, uint32_t count, T *scr) {
      const uint32_t nb = (uint32_t)(((uint64_t)count * N + 255) / 256);
      dispatch_mode<kDiagonalCoefficient, kTensorPerMesh, kTensorPerPoint>(cell_form(op), [&](auto FORM) {
        hipLaunchKernelGGL((cell_diagonal_2d_kernel<P, T, FORM.value>), dim3(nb), dim3(256), 0, s, (T *)diag, op.idx27, count,
                           d1, (const Basis1D<T> *)op.basis, (const T *)op.grad_1d, (const T *)op.coef_q, (T)op.coef[0],
                           (T)op.coef[1], (T)op.coef[2], list, scr);
      });
    });
    if (scratch)
      launch_assemble(s, op, 0, diag, nullptr, 0u);
  }

  void launch_cell_diagonal_2d(hipStream_t s, const OperatorData &op, void *diag, const double *a1d, const double *m1d)
  {
    dispatch_number_degree(op.number, op.p, [&](auto t, auto P) { cell_diag_2d_t<P.value, decltype(t)>(s, op, diag, a1d, m1d); });
  }

  void launch_prolongate_2d(hipStream_t s, const TransferData &t, void *fine, const void *coarse, bool add,
                            bool with_constraints)
  {
    const OperatorData &c = *t.coarse, &f = *t.fine;
    const uint32_t     *idx_c = with_constraints ? c.idx27 : c.idx27_plain;
    dispatch_number_degree(c.number, c.p, [&](auto number, auto P) {
      using T = decltype(number);
      hipLaunchKernelGGL((prolongate_2d_kernel<P.value, T>), dim3(c.n_cells), dim3(TCfg2<P.value>::THREADS), 0, s, (T *)fine,
                         (const T *)coarse, idx_c, f.idx27_plain, t.children, t.own27, c.n_cells, (const Basis1D<T> *)c.basis,
                         add ? 1 : 0);
    });
  }

  void launch_restrict_add_2d(hipStream_t s, const TransferData &t, void *coarse, const void *fine, bool with_constraints)
  {
    const OperatorData &c = *t.coarse, &f = *t.fine;
    const uint32_t     *idx_c = with_constraints ? c.idx27 : c.idx27_plain;
    dispatch_number_degree(c.number, c.p, [&](auto number, auto P) {
      using T = decltype(number);
      // (the parents of a colour share no DoF; a transfer always has the colours: never one launch over all parents)
      for_each_cell_list<T>(c, t.parent_colours.lists(), false, [&](const uint32_t *list, uint32_t count, T *) {
        hipLaunchKernelGGL((restrict_2d_kernel<P.value, T>), dim3(count), dim3(TCfg2<P.value>::THREADS), 0, s, (T *)coarse,
                           (const T *)fine, idx_c, f.idx27_plain, t.children, t.weight_shift, list, count,
                           (const Basis1D<T> *)c.basis);
      });
    });
  }

  // the restriction launch by launch: the lists of `launches`, else its classes of cells k, k + stride, ...
  void launch_dg_cg_transfer_2d(hipStream_t s, int number, int p, bool to_dg, void *dst, const void *src, const uint32_t *idx9,
                                uint32_t n_cells, const void *P1, const DisjointCells &launches)
  {
    dispatch_number_degree(number, p, [&](auto number_type, auto P) {
      using T = decltype(number_type);
      using C = Cfg2<P.value>;
      const auto launch = [&](auto TO_DG, const uint32_t *list, uint32_t first, uint32_t stride, uint32_t count) {
        if (count > 0)
          hipLaunchKernelGGL((dg_cg_transfer_kernel_2d<P.value, T, TO_DG.value>), dim3((count + C::CPB - 1) / C::CPB),
                             dim3(C::THREADS), 0, s, (T *)dst, (const T *)src, idx9, count, (const T *)P1, list, first, stride);
      };
      const CellLists &lists = launches.lists;
      if (to_dg)
        launch(std::true_type(), nullptr, 0u, 1u, n_cells);
      else if (lists.n > 0)
        for (int k = 0; k < lists.n; ++k)
          launch(std::false_type(), lists.cells + lists.start[k], 0u, 1u, lists.start[k + 1] - lists.start[k]);
      else
        for (uint32_t k = 0; k < launches.stride && k < n_cells; ++k)
          launch(std::false_type(), nullptr, k, launches.stride, (n_cells - k + launches.stride - 1) / launches.stride);
    });
  }
} // namespace mgx
