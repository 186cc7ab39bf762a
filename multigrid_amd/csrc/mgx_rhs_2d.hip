// mgx_rhs_2d.hip -- what states a linear problem on quadrilaterals: the residual form of the cell loop
// (LaplaceOperator::compute_residual, laplace_operator.h:804-845 -- right-hand side and boundary lifting) and the L2 error
// against a function given at the quadrature points (compute_l2_error, multigrid_solver.h:298-343).
//
// Both kernels have the thread mapping of cell_loop_2d_kernel (mgx_kernels_2d.hip): one thread per line, n = p + 1
// threads per cell, floor(256 / n) cells per workgroup, LDS tiles with the odd pitch.  The residual form is a kernel of
// its own and not a flag of cell_loop_2d_kernel, in a unit of its own: the instantiations of vmult stay the code they
// are (registers, LDS and kernel arguments; profiles/poisson_shell_2d.md has both tables), and the two units compile
// side by side.  Against the plain cell loop it differs as RESID does in cell_loop_general_kernel (mgx_kernels.hip):
// the source is gathered through the unconstrained table and negated, rhs_q joins the integrand of the test-function
// values before the two S^T sweeps, and the results leave through the constrained table.
//
// No atomics: the cells are added up by assemble_kernel in cell order or by launches over cells of one colour; the
// error sums are formed per workgroup in a fixed order and added by reduce4_kernel in index order.
#include "mgx_internal.hpp"
#include "mgx_cell_device_2d.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  // ------------------------------------------------------------------------------------------
  // dst (+)= sum over the cells of  S^T [ rhs_q - D^T (C D S u) ],  u = src through idx_plain (boundary values in the
  // constrained entries), rows through idx9 (constrained rows stay out).  rhs_q [n_cells][n^2] = f(x_q) JxW_q, q = qy n +
  // qx, nullptr: no such term.  scratch / cell_list as in cell_loop_2d_kernel.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T, int FORM>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    cell_residual_2d_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ idx9,
                            const uint32_t *__restrict__ idx_plain, uint32_t n_cells, const Basis1D<T> *__restrict__ B,
                            const T *__restrict__ coef_q, T c0, T c1, T c2, const T *__restrict__ rhs_q,
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
      gather_cell_2d<P, T>(src, idx_plain + 9u * (size_t)cell, t, Uc);
    __syncthreads();
    if (active) // nodal -> quadrature along x, negated (:823-824)
      {
        lds_product<N, T, false, ROLLED>(B->S, Uc + row, 1, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[row + i] = -q[i];
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
    if (active) // add the y part and f JxW (:839), quadrature -> nodal along y
      {
#pragma unroll
        for (int j = 0; j < N; ++j)
          r[j] = Uc[col + j * LN] + vy[j];
        if (rhs_q) // point (t, j): the n threads of a cell read n consecutive values per j
          {
            const T *fq = rhs_q + (size_t)cell * N2 + (size_t)t;
#pragma unroll
            for (int j = 0; j < N; ++j)
              r[j] += fq[j * N];
          }
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
      store_tiles_2d<P, T>(scratch, U, n_cells, tid);
    else if (active)
      scatter_add_cell_2d<P, T>(dst, idx9 + 9u * (size_t)cell, t, Uc);
  }

  // ------------------------------------------------------------------------------------------
  // partials[workgroup][4] = { sum (u_h - u_q)^2 JxW_q, sum JxW_q, 0, 0 } over the cells of the workgroup: vec through
  // idx_plain, S x S to the quadrature points in the operator's number type, differences, products and sums in fp64.
  // A thread adds the n points of its column in order, a wave its lanes by shuffles, the workgroup its waves in order.
  // ------------------------------------------------------------------------------------------
  template <int P, typename T>
  __global__ void __launch_bounds__(Cfg2<P>::THREADS)
    l2_error_2d_kernel(const T *__restrict__ vec, const uint32_t *__restrict__ idx_plain, uint32_t n_cells,
                       const Basis1D<T> *__restrict__ B, const T *__restrict__ u_q, const T *__restrict__ jxw_q,
                       double *__restrict__ partials)
  {
    using C               = Cfg2<P>;
    constexpr int  N      = C::N, LN = C::LN, N2 = C::N2;
    constexpr bool ROLLED = rolled_products<P, T>();
    constexpr int  WAVES  = C::THREADS / 64;
    __shared__ T      U[C::CPB * C::CELL_LDS];
    __shared__ double red[2 * WAVES];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / N;
    const int      t      = tid - lc * N;
    const uint32_t cell   = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (cell < n_cells);
    T             *Uc     = U + (lc < C::CPB ? lc : 0) * C::CELL_LDS;
    const int      row = t * LN, col = t;
    T              q[N];
    double         err = 0., vol = 0.;

    if (active)
      gather_cell_2d<P, T>(vec, idx_plain + 9u * (size_t)cell, t, Uc);
    __syncthreads();
    if (active) // nodal -> quadrature along x
      {
        lds_product<N, T, false, ROLLED>(B->S, Uc + row, 1, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[row + i] = q[i];
      }
    __syncthreads();
    if (active) // along y: u_h at the points (t, j)
      {
        lds_product<N, T, false, ROLLED>(B->S, Uc + col, LN, q);
        const size_t at = (size_t)cell * N2 + (size_t)t;
#pragma unroll
        for (int j = 0; j < N; ++j)
          {
            const double d = (double)q[j] - (double)u_q[at + j * N], w = (double)jxw_q[at + j * N];
            err += d * d * w;
            vol += w;
          }
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      {
        err += __shfl_down(err, o);
        vol += __shfl_down(vol, o);
      }
    if ((tid & 63) == 0)
      red[2 * (tid >> 6)] = err, red[2 * (tid >> 6) + 1] = vol;
    __syncthreads();
    if (tid < 4)
      {
        double s = 0.;
        if (tid < 2)
          {
            s = red[tid];
#pragma unroll
            for (int w = 1; w < WAVES; ++w)
              s += red[2 * w + tid];
          }
        partials[4 * (size_t)blockIdx.x + tid] = s;
      }
  }

  // ------------------------------------------------------------------------------------------
  // launchers
  // ------------------------------------------------------------------------------------------
  template <int P, typename T>
  static void cell_residual_2d_t(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *rhs_q)
  {
    using C = Cfg2<P>;
    T *scratch = for_each_cell_list<T>(op, cell_lists_2d(op), true, [&](const uint32_t *list, uint32_t count, T *scr) {
      const uint32_t nb = (count + C::CPB - 1) / C::CPB;
      dispatch_mode<kDiagonalCoefficient, kTensorPerMesh, kTensorPerPoint>(cell_form(op), [&](auto FORM) {
        hipLaunchKernelGGL((cell_residual_2d_kernel<P, T, FORM.value>), dim3(nb), dim3(C::THREADS), 0, s, (T *)dst, (const T *)src,
                           op.idx27, op.idx27_plain, count, (const Basis1D<T> *)op.basis, (const T *)op.coef_q, (T)op.coef[0],
                           (T)op.coef[1], (T)op.coef[2], (const T *)rhs_q, list, scr);
      });
    });
    if (scratch)
      launch_assemble(s, op, 0, dst, nullptr, 0u);
  }

  void launch_cell_residual_2d(hipStream_t s, const OperatorData &op, void *dst, const void *src, const void *rhs_q)
  {
    dispatch_number_degree(op.number, op.p, [&](auto t, auto P) { cell_residual_2d_t<P.value, decltype(t)>(s, op, dst, src, rhs_q); });
  }

  uint32_t l2_error_grid_2d(int p, uint32_t n_cells)
  {
    const uint32_t cpb = 256u / (uint32_t)(p + 1);
    return (n_cells + cpb - 1) / cpb;
  }

  void launch_l2_error_2d(hipStream_t s, const OperatorData &op, const void *vec, const void *u_q, const void *jxw_q,
                          double *partials)
  {
    if (op.n_cells == 0)
      return;
    dispatch_number_degree(op.number, op.p, [&](auto number, auto P) {
      using T = decltype(number);
      using C = Cfg2<P.value>;
      hipLaunchKernelGGL((l2_error_2d_kernel<P.value, T>), dim3((op.n_cells + C::CPB - 1) / C::CPB), dim3(C::THREADS), 0, s,
                         (const T *)vec, op.idx27_plain, op.n_cells, (const Basis1D<T> *)op.basis, (const T *)u_q,
                         (const T *)jxw_q, partials);
    });
  }
} // namespace mgx
