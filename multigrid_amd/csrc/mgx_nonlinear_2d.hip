// mgx_nonlinear_2d.hip -- solution-dependent coefficients on quadrilaterals (MinimalSurfaceOperator and
// LaplaceProblem::solve of minimal_surface/program.cc with dimension = 2):
//   evaluate_coefficient_2d_kernel   :120-165  merged_coefficient from the gradient of a state vector
//   nl_residual_2d_kernel            :169-197  the nonlinear residual
//   interpolate_to_coarse_2d_kernel  :425-457  the state on the next coarser level
// The counterpart of mgx_nonlinear.hip and of the MINSURF form of mgx_kernels.hip with the thread mapping of
// mgx_kernels_2d.hip: one thread owns a line of n values, n threads a cell, floor(256 / n) cells a workgroup.
//
// Geometry: one metric M = J^-1 J^-T [xx, yy, xy] and one det J per level (affine cells).  With g the reference-space
// gradient at a quadrature point, v = M g, s = g . v = |grad u|^2 and JxW_q = w_q det J:
//   first_time:  coef_q = JxW_q M
//   otherwise:   coef_q = JxW_q (M - v v^T / (1 + s)) / sqrt(1 + s)
// Curved cells (PERQ): U = JxW_q J^-1 J^-T [cell][3][n^2] and w = JxW_q [cell][n^2] of every point; u = U g,
// s = g . u / w:  coef_q = U or (U - u u^T / (w (1 + s))) / sqrt(1 + s).
// The residual of a point is the flux -a JxW_q M g (-a u on curved cells), a = 1 or 1 / sqrt(1 + s).
// No kernel of this unit uses an atomic.
#include "mgx_cell_device_2d.hpp"
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  // LDS of a workgroup: the two tiles per cell of the sweeps, which become the staging area of the 3 n^2 tensor values
  // per cell once the gradients sit in registers (values of the sweep type T; the tensor type is no wider)
  template <int P>
  constexpr int eval_lds_values()
  {
    using C = Cfg2<P>;
    return C::CPB * (2 * C::CELL_LDS > 3 * C::N2 ? 2 * C::CELL_LDS : 3 * C::N2);
  }

  // The first half of the tensor forms of cell_loop_2d_kernel up to the gradient at the n points (t, j) of the thread's
  // column: gx[j], gy[j].  Uc, Xc: the cell's two tiles; the caller synchronises before it reuses them.
  template <int P, typename T, bool ROLLED>
  __device__ __forceinline__ void reference_gradient_2d(const T *__restrict__ state, const uint32_t *__restrict__ ix, int t,
                                                        bool active, const Basis1D<T> *__restrict__ B, T *Uc, T *Xc,
                                                        T (&gx)[P + 1], T (&gy)[P + 1])
  {
    constexpr int N = P + 1, LN = N | 1;
    const int     row = t * LN, col = t;
    T             q[N];
    if (active) // the state with its boundary values (dof-handler slot 1)
      gather_cell_2d<P, T>(state, ix, t, Uc);
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
        reg_product<N, T, false, ROLLED>(B->D, q, Uc + col, LN, gy); // (ROLLED: the column already holds q)
      }
    __syncthreads();
    if (active) // the x-derivative of this row, to the column threads through LDS
      {
        lds_product<N, T, false, ROLLED>(B->D, Uc + row, 1, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Xc[row + i] = q[i];
      }
    __syncthreads();
    if (active)
      {
#pragma unroll
        for (int j = 0; j < N; ++j)
          gx[j] = Xc[col + j * LN];
      }
  }

  // ------------------------------------------------------------------------------------------
  // T: number type of the state, the 1D tables and the arithmetic; TO: number type of coef_q (TO = float with
  // T = double: the fp32 operator of a level receives the rounded fp64 tensor, mgx_solver_update_coefficient).
  // The kernel reads n^2 state values per cell (and 4 n^2 geometry values with PERQ) and writes 3 n^2 tensor entries.
  // The blocks [3][n^2] of the consecutive cells of a workgroup are one contiguous run of coef_q: they are staged in
  // the LDS the sweeps no longer need and leave with unit stride over the whole workgroup.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, typename TO, bool MINSURF, bool PERQ>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    evaluate_coefficient_2d_kernel(TO *__restrict__ coef_q, const T *__restrict__ state, const uint32_t *__restrict__ idx_plain,
                                   uint32_t n_cells, const Basis1D<T> *__restrict__ B, T m0, T m1, T m2, T det,
                                   const T *__restrict__ unit_q, const T *__restrict__ jxw_q)
  {
    using C         = Cfg2<P>;
    constexpr int N = C::N, N2 = C::N2;
    static_assert(sizeof(TO) <= sizeof(T), "staging area");
    __shared__ T W[eval_lds_values<P>()];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / N;
    const int      t      = tid - lc * N;
    const uint32_t cell   = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (cell < n_cells);
    const int      slot   = lc < C::CPB ? lc : 0;
    T             *Uc     = W + slot * C::CELL_LDS;
    T             *Xc     = W + (C::CPB + slot) * C::CELL_LDS;
    T              gx[N], gy[N];
    reference_gradient_2d<P, T, rolled_products<P, T>()>(state, idx_plain + 9u * (size_t)(active ? cell : 0u), t, active, B, Uc,
                                                         Xc, gx, gy);
    __syncthreads(); // the tiles become the staging area
    TO *stage = reinterpret_cast<TO *>(W) + slot * 3 * N2;
    if (active) // the tensor at the n points (t, j) of this column
      {
        const T *uq = PERQ ? unit_q + (size_t)cell * 3 * N2 + (size_t)t : nullptr;
        const T *wq = PERQ ? jxw_q + (size_t)cell * N2 + (size_t)t : nullptr;
        const T  wt = PERQ ? T(0) : B->w[t] * det;
#pragma unroll
        for (int j = 0; j < N; ++j)
          {
            T c0, c1, c2;
            if (PERQ)
              {
                c0 = uq[j * N], c1 = uq[N2 + j * N], c2 = uq[2 * N2 + j * N];
                if (MINSURF)
                  {
                    const T w  = wq[j * N];
                    const T u0 = c0 * gx[j] + c2 * gy[j];
                    const T u1 = c2 * gx[j] + c1 * gy[j];
                    const T d  = T(1) + (gx[j] * u0 + gy[j] * u1) / w;
                    const T f  = T(1) / sqrt(d);
                    const T wd = w * d;
                    c0 = f * (c0 - u0 * u0 / wd), c1 = f * (c1 - u1 * u1 / wd), c2 = f * (c2 - u0 * u1 / wd);
                  }
              }
            else
              {
                const T jxw = wt * B->w[j];
                if (MINSURF) // :133-139
                  {
                    const T v0 = m0 * gx[j] + m2 * gy[j];
                    const T v1 = m2 * gx[j] + m1 * gy[j];
                    const T d  = T(1) + (gx[j] * v0 + gy[j] * v1);
                    const T f  = jxw / sqrt(d);
                    c0 = f * (m0 - v0 * v0 / d), c1 = f * (m1 - v1 * v1 / d), c2 = f * (m2 - v0 * v1 / d);
                  }
                else // first_time: the unit tensor
                  c0 = jxw * m0, c1 = jxw * m1, c2 = jxw * m2;
              }
            stage[j * N + t]          = (TO)c0;
            stage[N2 + j * N + t]     = (TO)c1;
            stage[2 * N2 + j * N + t] = (TO)c2;
          }
      }
    __syncthreads();
    const uint32_t cell0 = blockIdx.x * C::CPB;
    const uint32_t left  = n_cells - cell0;
    const int      count = (int)(left < (uint32_t)C::CPB ? left : (uint32_t)C::CPB) * 3 * N2;
    TO            *out   = coef_q + (size_t)cell0 * 3 * N2;
    const TO      *all   = reinterpret_cast<const TO *>(W);
    for (int f = tid; f < count; f += C::THREADS)
      out[f] = all[f];
  }

  // ------------------------------------------------------------------------------------------
  // dst_i = - sum_q grad phi_i . a JxW_q M g: the tensor forms of cell_loop_2d_kernel with the flux of the law in place
  // of the tensor product.  state through idx_plain (boundary values included), the result through idx9 (cell_list:
  // cells of one colour, plain adds) or, for every cell, into the scratch array of the ordered assembly.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, bool MINSURF, bool PERQ>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    nl_residual_2d_kernel(T *__restrict__ dst, const T *__restrict__ state, const uint32_t *__restrict__ idx9,
                          const uint32_t *__restrict__ idx_plain, uint32_t n_cells, const Basis1D<T> *__restrict__ B, T m0, T m1,
                          T m2, T det, const T *__restrict__ unit_q, const T *__restrict__ jxw_q,
                          const uint32_t *__restrict__ cell_list, T *__restrict__ scratch)
  {
    using C               = Cfg2<P>;
    constexpr int  N      = C::N, LN = C::LN, N2 = C::N2;
    // (the rolled line products one degree earlier than the linear cell loop: with the flux of the law between the
    // sweeps, the unrolled products of n = 8 -- 128 scalar registers per matrix -- no longer fit without a spill)
    constexpr bool ROLLED = sizeof(T) == 8 && P >= 7;
    __shared__ T U[C::CPB * C::CELL_LDS];
    __shared__ T GX[C::CPB * C::CELL_LDS];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / N;
    const int      t      = tid - lc * N;
    const uint32_t pos    = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (pos < n_cells);
    const uint32_t cell   = active ? (cell_list ? cell_list[pos] : pos) : 0u;
    const int      slot   = lc < C::CPB ? lc : 0;
    T             *Uc     = U + slot * C::CELL_LDS;
    T             *Xc     = GX + slot * C::CELL_LDS;
    const int      row = t * LN, col = t;
    T              gx[N], gy[N], q[N], vy[N];
    reference_gradient_2d<P, T, ROLLED>(state, idx_plain + 9u * (size_t)cell, t, active, B, Uc, Xc, gx, gy);
    if (active) // the flux at the n points (t, j) of this column (only this thread reads and writes them in Xc)
      {
        const T *uq = PERQ ? unit_q + (size_t)cell * 3 * N2 + (size_t)t : nullptr;
        const T *wq = PERQ ? jxw_q + (size_t)cell * N2 + (size_t)t : nullptr;
        const T  wt = PERQ ? T(0) : B->w[t] * det;
#pragma unroll
        for (int j = 0; j < N; ++j)
          {
            T f0, f1, a;
            if (PERQ)
              {
                const T c0 = uq[j * N], c1 = uq[N2 + j * N], c2 = uq[2 * N2 + j * N];
                f0 = c0 * gx[j] + c2 * gy[j];
                f1 = c2 * gx[j] + c1 * gy[j];
                a  = MINSURF ? T(-1) / sqrt(T(1) + (gx[j] * f0 + gy[j] * f1) / wq[j * N]) : T(-1);
              }
            else
              {
                f0 = m0 * gx[j] + m2 * gy[j];
                f1 = m2 * gx[j] + m1 * gy[j];
                const T jxw = wt * B->w[j];
                a = MINSURF ? -jxw / sqrt(T(1) + (gx[j] * f0 + gy[j] * f1)) : -jxw;
              }
            Xc[col + j * LN] = a * f0;
            q[j]             = a * f1;
          }
        reg_product<N, T, true, ROLLED>(B->D, q, Uc + col, LN, vy); // (the values in U have been used up)
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
    if (active) // add the y part, quadrature -> nodal along y
      {
#pragma unroll
        for (int j = 0; j < N; ++j)
          gy[j] = Uc[col + j * LN] + vy[j];
        reg_product<N, T, true, ROLLED>(B->S, gy, Uc + col, LN, q);
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
      store_tiles_2d<P, T>(scratch, U, n_cells, tid);
    else if (active)
      scatter_add_cell_2d<P, T>(dst, idx9 + 9u * (size_t)cell, t, Uc);
  }

  // ------------------------------------------------------------------------------------------
  // State interpolation to the coarser level (:425-457): one workgroup per coarse cell gathers the (2p+1)^2 points of its
  // children patch (points that children share carry the same fine DoF), applies the 1D matrix r1 along y, then x, and
  // WRITES the (p+1)^2 coarse values.  A coarse DoF shared by several cells is written by the first cell (in cell
  // order) that contains its entity (own_c, 9 bits): one writer, the same value in every run.
  // ------------------------------------------------------------------------------------------
  template <int P>
  struct ICfg2
  {
    static constexpr int N       = P + 1;
    static constexpr int M       = 2 * P + 1;
    static constexpr int THREADS = ((M * N + 63) / 64) * 64 > 256 ? 256 : ((M * N + 63) / 64) * 64;
  };

  template <int P, typename T>
  __global__ void __launch_bounds__(ICfg2<P>::THREADS)
    interpolate_to_coarse_2d_kernel(T *__restrict__ coarse, const T *__restrict__ fine, const uint32_t *__restrict__ idx_c,
                                    const uint32_t *__restrict__ idx_f, const uint32_t *__restrict__ children,
                                    const uint32_t *__restrict__ own_c, uint32_t n_parents, const T *__restrict__ r1d)
  {
    constexpr int N = P + 1, M = 2 * P + 1;
    __shared__ T  r1[M * N];
    __shared__ T  in[N * N];
    __shared__ T  t1[N * M];
    __shared__ T  out[M * M];
    const uint32_t pc = blockIdx.x;
    if (pc >= n_parents)
      return;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < M * N; i += nt)
      r1[i] = r1d[i];
    for (int w = tid; w < 4 * N; w += nt) // the fine patch
      {
        const int      ch = w / N, j = w % N;
        const uint32_t fc = children[4u * (size_t)pc + ch];
        const int      ox = (ch & 1) * P, b = (ch >> 1) * P + j;
        T              r[N];
        gather_line<P, T>(fine, line_index_2d<P>(idx_f, fc, j), r);
#pragma unroll
        for (int i = 0; i < N; ++i)
          out[b * M + ox + i] = r[i];
      }
    __syncthreads();
    for (int o = tid; o < N * M; o += nt) // y: [j][a]
      {
        const int a = o % M, j = o / M;
        T         s = 0;
#pragma unroll
        for (int b = 0; b < M; ++b)
          s = fma(r1[b * N + j], out[b * M + a], s);
        t1[o] = s;
      }
    __syncthreads();
    for (int o = tid; o < N * N; o += nt) // x: [j][i]
      {
        const int i = o % N, j = o / N;
        T         s = 0;
#pragma unroll
        for (int a = 0; a < M; ++a)
          s = fma(r1[a * N + i], t1[j * M + a], s);
        in[o] = s;
      }
    __syncthreads();
    for (int j = tid; j < N; j += nt)
      {
        const LineIndex<P> L = line_index_2d<P>(idx_c, pc, j);
        int                cy, oy;
        node_code<P>(j, cy, oy);
        const uint32_t own = own_c[pc] >> (3 * cy); // bits 0, 1, 2: left, interior, right entity of the line
        const T       *r   = in + j * N;
        if (L.b0 != kInvalid && (own & 1u))
          coarse[L.b0 + L.off] = r[0];
        if (L.b1 != kInvalid && (own & 2u))
          {
#pragma unroll
            for (int i = 0; i < P - 1; ++i)
              coarse[L.b1 + L.off * (uint32_t)(P - 1) + (uint32_t)i] = r[1 + i];
          }
        if (L.b2 != kInvalid && (own & 4u))
          coarse[L.b2 + L.off] = r[P];
      }
  }

  // ------------------------------------------------------------------------------------------
  // launchers
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, typename TO>
  static void evaluate_coefficient_2d_t(hipStream_t s, const OperatorData &op, void *coef_q, bool minimal_surface, const double *M,
                                        double det, const void *unit_q, const void *jxw_q, const void *state)
  {
    using C           = Cfg2<P>;
    const uint32_t nb = (op.n_cells + C::CPB - 1) / C::CPB;
    const bool curved = unit_q != nullptr;
    dispatch_mode<0, 1>(minimal_surface, [&](auto MINSURF) {
      dispatch_mode<0, 1>(curved, [&](auto PERQ) {
        hipLaunchKernelGGL((evaluate_coefficient_2d_kernel<P, T, TO, MINSURF.value != 0, PERQ.value != 0>), dim3(nb),
                           dim3(C::THREADS), 0, s, (TO *)coef_q, (const T *)state, op.idx27_plain, op.n_cells,
                           (const Basis1D<T> *)op.basis, (T)(curved ? 0. : M[0]), (T)(curved ? 0. : M[1]), (T)(curved ? 0. : M[2]),
                           (T)(curved ? 0. : det), (const T *)unit_q, (const T *)(curved ? jxw_q : nullptr));
      });
    });
  }

  void launch_evaluate_coefficient_2d(hipStream_t s, const OperatorData &op, void *coef_q, int coef_number, bool minimal_surface,
                                      const double *metric, double det, const void *unit_q, const void *jxw_q, const void *state)
  {
    if (op.n_cells == 0)
      return;
    dispatch_degree(op.p, [&](auto P) {
      auto run = [&](auto t, auto to) {
        evaluate_coefficient_2d_t<P.value, decltype(t), decltype(to)>(s, op, coef_q, minimal_surface, metric, det, unit_q, jxw_q,
                                                                      state);
      };
      // (number type of the state and the arithmetic, number type of the tensor)
      if (op.number == MGX_F64 && coef_number == MGX_F64)
        run(double(), double());
      else if (op.number == MGX_F64)
        run(double(), float());
      else // (fp32 tables: fp32 tensor)
        run(float(), float());
    });
  }

  template <int P, typename T>
  static void nl_residual_2d_t(hipStream_t s, const OperatorData &op, bool minimal_surface, const double *M, double det,
                               const void *unit_q, const void *jxw_q, void *dst, const void *state)
  {
    using C           = Cfg2<P>;
    const bool curved = unit_q != nullptr;
    // once over all cells into the scratch array of the ordered assembly where the operator has one (dst is written by
    // the assembly), else once per cell colour (dst zeroed by the caller)
    const CellLists lists = op.asm_start ? CellLists() : op.cell_colours.lists();
    T *scratch = for_each_cell_list<T>(op, lists, true, [&](const uint32_t *list, uint32_t count, T *scr) {
      const uint32_t nb = (count + C::CPB - 1) / C::CPB;
      dispatch_mode<0, 1>(minimal_surface, [&](auto MINSURF) {
        dispatch_mode<0, 1>(curved, [&](auto PERQ) {
          hipLaunchKernelGGL((nl_residual_2d_kernel<P, T, MINSURF.value != 0, PERQ.value != 0>), dim3(nb), dim3(C::THREADS), 0, s,
                             (T *)dst, (const T *)state, op.idx27, op.idx27_plain, count, (const Basis1D<T> *)op.basis,
                             (T)(curved ? 0. : M[0]), (T)(curved ? 0. : M[1]), (T)(curved ? 0. : M[2]), (T)(curved ? 0. : det),
                             (const T *)unit_q, (const T *)(curved ? jxw_q : nullptr), list, scr);
        });
      });
    });
    if (scratch)
      launch_assemble(s, op, 0, dst, nullptr, 0u);
  }

  void launch_cell_nl_residual_2d(hipStream_t s, const OperatorData &op, bool minimal_surface, const double *metric, double det,
                                  const void *unit_q, const void *jxw_q, void *dst, const void *state)
  {
    dispatch_number_degree(op.number, op.p, [&](auto t, auto P) {
      nl_residual_2d_t<P.value, decltype(t)>(s, op, minimal_surface, metric, det, unit_q, jxw_q, dst, state);
    });
  }

  void launch_interpolate_to_coarse_2d(hipStream_t s, const TransferData &t, const void *r1d, const uint32_t *own_c, void *coarse,
                                       const void *fine)
  {
    const OperatorData &c = *t.coarse, &f = *t.fine;
    if (c.n_cells == 0)
      return;
    dispatch_number_degree(c.number, c.p, [&](auto number, auto P) {
      using T = decltype(number);
      hipLaunchKernelGGL((interpolate_to_coarse_2d_kernel<P.value, T>), dim3(c.n_cells), dim3(ICfg2<P.value>::THREADS), 0, s,
                         (T *)coarse, (const T *)fine, c.idx27_plain, f.idx27_plain, t.children, own_c, c.n_cells, (const T *)r1d);
    });
  }
} // namespace mgx
