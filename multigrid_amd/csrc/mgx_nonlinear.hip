// mgx_nonlinear.hip -- solution-dependent coefficients of the general tensor branch
// (MinimalSurfaceOperator and LaplaceProblem::solve of minimal_surface/program.cc):
//   evaluate_coefficient_kernel   :120-165  merged_coefficient from the gradient of a state vector
//   interpolate_to_coarse_kernel  :425-457  the state on the next coarser level
// The nonlinear residual (:169-197) is a form of the general per-cell kernel (mgx_kernels.hip, MINSURF).
//
// Geometry: one metric M = J^-1 J^-T and one det J per level (affine cells).  With g the reference-space gradient at
// a quadrature point, v = M g, s = g . v = |grad u|^2 and JxW_q = w_q det J:
//   first_time:  coef_q = JxW_q M
//   otherwise:   coef_q = JxW_q (M - v v^T / (1 + s)) / sqrt(1 + s)
// which is J^-1 (I - G G^T / (1 + |G|^2)) / sqrt(1 + |G|^2) J^-T JxW of :133-155 with G = J^-T g.
// Curved cells: JxW_q M and JxW_q of every point instead (evaluate_coefficient_kernel, PERQ).
#include "mgx_cell_device.hpp"
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

namespace mgx
{
  template <typename T>
  struct Vec16;
  template <>
  struct Vec16<double>
  {
    using type                 = double2;
    static constexpr int WIDTH = 2;
  };
  template <>
  struct Vec16<float>
  {
    using type                 = float4;
    static constexpr int WIDTH = 4;
  };

  // ------------------------------------------------------------------------------------------
  // Thread mapping of the per-cell kernels (mgx_cell_device.hpp): a tile of n x n threads per cell, one line of n values
  // per thread, transposes through LDS; the first half of cell_loop_general_kernel up to the gradient at the points of
  // the thread's z-line.  The kernel reads (p+1)^3 state values per cell (about one per point: p^3 unique ones) and
  // writes 6 (p+1)^3 tensor entries: its traffic is its own store stream.  The six planes of a cell are contiguous in
  // coef_q ([cell][6][n^3]); they are staged in the LDS the sweeps no longer need, three planes at a time (3 n^3 <= the
  // 3 n^2 (n|1) values of the sweep arrays, so the staging costs no occupancy), and leave as 16-byte stores, consecutive
  // lanes on consecutive addresses; the few elements in front of / behind the 16-byte-aligned body of a chunk go out
  // one by one (3 n^3 values of a chunk start on an 8-byte boundary for odd n in fp32).
  // T: number type of the state, the 1D tables and the arithmetic; TO: number type of coef_q (TO = float with
  // T = double: the fp32 operator of a level receives the rounded fp64 tensor, mgx_solver_update_coefficient).
  // ------------------------------------------------------------------------------------------
  // PERQ: per-point geometry of curved cells instead of m0 .. m5 and det -- unit_q[cell][6][n^3] = U = JxW_q J^-1 J^-T
  // and jxw_q[cell][n^3] = w = JxW_q in the number type T.  The thread reads the seven values of a point of its z-line
  // where it needs them (lane (a, b) at offset b n + a of plane k: consecutive lanes on consecutive addresses, as the
  // stores are), and with u = U g, s = g . u / w:  coef_q = U (first_time) or (U - u u^T / (w (1 + s))) / sqrt(1 + s),
  // the law above with M = U / w.
  template <int P, typename T, typename TO, bool MINSURF, bool PERQ = false>
  __global__ void __launch_bounds__(Cfg<P>::THREADS)
    evaluate_coefficient_kernel(TO *__restrict__ coef_q, const T *__restrict__ state, const uint32_t *__restrict__ idx_plain,
                                uint32_t n_cells, const Basis1D<T> *__restrict__ B, T m0, T m1, T m2, T m3, T m4, T m5, T det,
                                const T *__restrict__ unit_q = nullptr, const T *__restrict__ jxw_q = nullptr)
  {
    using C          = Cfg<P>;
    constexpr int N  = C::N;
    constexpr int LN = C::LN;
    constexpr int PL = N * LN;
    constexpr int N3 = N * N * N;
    constexpr int V  = Vec16<TO>::WIDTH;
    using VT         = typename Vec16<TO>::type;
    static_assert(3 * N3 <= 3 * C::CELL_LDS && sizeof(TO) <= sizeof(T), "staging area");
    __shared__ T W[C::CPB * 3 * C::CELL_LDS];

    const int      tid    = threadIdx.x;
    const int      lc     = tid / C::TPC;
    const int      t      = tid - lc * C::TPC;
    const int      a      = t % N;
    const int      b      = t / N;
    const uint32_t cell   = blockIdx.x * C::CPB + lc;
    const bool     active = (lc < C::CPB) && (cell < n_cells);
    const int      slot   = lc < C::CPB ? lc : 0;
    T             *Uc = W + slot * 3 * C::CELL_LDS, *Xc = Uc + C::CELL_LDS, *Yc = Uc + 2 * C::CELL_LDS;
    const int      xl = (b * N + a) * LN, yl = b * PL + a, zl = b * LN + a;
    T              r[N], q[N], gx[N], gy[N], gz[N];
    if (active) // nodal -> quadrature along x; the state with its boundary values (dof-handler slot 1)
      {
        gather_line<P, T>(state, line_index<P>(idx_plain, cell, a, b), r);
        mv<N, T>(B->S, r, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[xl + i] = q[i];
      }
    __syncthreads();
    if (active) // along y
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          r[i] = Uc[yl + i * LN];
        mv<N, T>(B->S, r, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[yl + i * LN] = q[i];
      }
    __syncthreads();
    if (active) // along z; z-derivative of this z-line in registers
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          r[i] = Uc[zl + i * PL];
        mv<N, T>(B->S, r, q);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Uc[zl + i * PL] = q[i];
        mv<N, T>(B->D, q, gz);
      }
    __syncthreads();
    if (active) // x- and y-derivatives, to the z-line owners through LDS
      {
#pragma unroll
        for (int i = 0; i < N; ++i)
          q[i] = Uc[xl + i];
        mv<N, T>(B->D, q, r);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Xc[xl + i] = r[i];
#pragma unroll
        for (int i = 0; i < N; ++i)
          q[i] = Uc[yl + i * LN];
        mv<N, T>(B->D, q, r);
#pragma unroll
        for (int i = 0; i < N; ++i)
          Yc[yl + i * LN] = r[i];
      }
    __syncthreads();
    if (active)
      {
#pragma unroll
        for (int k = 0; k < N; ++k)
          {
            gx[k] = Xc[zl + k * PL];
            gy[k] = Yc[zl + k * PL];
          }
      }
    __syncthreads(); // the sweep arrays become the staging area
    // the tensor at the N points (a, b, k) of this z-line; the diagonal entries are staged first, the off-diagonal
    // ones wait in gx, gy, gz
    TO       *stage = reinterpret_cast<TO *>(Uc);
    const int sp    = b * N + a;
    if (active)
      {
        const T  wab = PERQ ? T(0) : B->w[a] * B->w[b];
        const T *uq  = PERQ ? unit_q + (size_t)cell * 6 * N3 + (size_t)sp : nullptr;
        const T *wq  = PERQ ? jxw_q + (size_t)cell * N3 + (size_t)sp : nullptr;
#pragma unroll
        for (int k = 0; k < N; ++k)
          {
            const T jxw = wab * B->w[k] * det;
            T       c0, c1, c2, c3, c4, c5;
            if (PERQ)
              {
                const T *up = uq + k * N * N;
                c0 = up[0], c1 = up[N3], c2 = up[2 * N3], c3 = up[3 * N3], c4 = up[4 * N3], c5 = up[5 * N3];
                if (MINSURF)
                  {
                    const T w  = wq[k * N * N];
                    const T u0 = c0 * gx[k] + c3 * gy[k] + c4 * gz[k];
                    const T u1 = c3 * gx[k] + c1 * gy[k] + c5 * gz[k];
                    const T u2 = c4 * gx[k] + c5 * gy[k] + c2 * gz[k];
                    const T d  = T(1) + (gx[k] * u0 + gy[k] * u1 + gz[k] * u2) / w;
                    const T f  = T(1) / sqrt(d);
                    const T wd = w * d;
                    c0 = f * (c0 - u0 * u0 / wd), c1 = f * (c1 - u1 * u1 / wd), c2 = f * (c2 - u2 * u2 / wd);
                    c3 = f * (c3 - u0 * u1 / wd), c4 = f * (c4 - u0 * u2 / wd), c5 = f * (c5 - u1 * u2 / wd);
                  }
              }
            else if (MINSURF) // :133-139
              {
                const T v0 = m0 * gx[k] + m3 * gy[k] + m4 * gz[k];
                const T v1 = m3 * gx[k] + m1 * gy[k] + m5 * gz[k];
                const T v2 = m4 * gx[k] + m5 * gy[k] + m2 * gz[k];
                const T d  = T(1) + (gx[k] * v0 + gy[k] * v1 + gz[k] * v2);
                const T f  = jxw / sqrt(d);
                c0 = f * (m0 - v0 * v0 / d), c1 = f * (m1 - v1 * v1 / d), c2 = f * (m2 - v2 * v2 / d);
                c3 = f * (m3 - v0 * v1 / d), c4 = f * (m4 - v0 * v2 / d), c5 = f * (m5 - v1 * v2 / d);
              }
            else // first_time: the unit tensor
              c0 = jxw * m0, c1 = jxw * m1, c2 = jxw * m2, c3 = jxw * m3, c4 = jxw * m4, c5 = jxw * m5;
            stage[k * N * N + sp]          = (TO)c0;
            stage[N3 + k * N * N + sp]     = (TO)c1;
            stage[2 * N3 + k * N * N + sp] = (TO)c2;
            gx[k] = c3, gy[k] = c4, gz[k] = c5;
          }
      }
#pragma unroll
    for (int half = 0; half < 2; ++half)
      {
        __syncthreads();
        if (active)
          {
            const size_t g0   = ((size_t)cell * 6 + 3 * half) * N3; // first element of the chunk of 3 N3
            const int    head = (int)((V - (int)(g0 % V)) % V);
            const int    nvec = (3 * N3 - head) / V;
            const int    tail = 3 * N3 - head - nvec * V;
            TO          *out  = coef_q + g0;
            for (int i = t; i < nvec; i += C::TPC)
              {
                TO v[V];
#pragma unroll
                for (int j = 0; j < V; ++j)
                  v[j] = stage[head + i * V + j];
                VT pack;
                if constexpr (V == 2)
                  pack = VT{v[0], v[1]};
                else
                  pack = VT{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<VT *>(out + head + i * V) = pack;
              }
            if (t < head)
              out[t] = stage[t];
            if (t < tail)
              out[head + nvec * V + t] = stage[head + nvec * V + t];
          }
        if (half == 0)
          {
            __syncthreads();
            if (active)
              {
#pragma unroll
                for (int k = 0; k < N; ++k)
                  {
                    stage[k * N * N + sp]          = (TO)gx[k];
                    stage[N3 + k * N * N + sp]     = (TO)gy[k];
                    stage[2 * N3 + k * N * N + sp] = (TO)gz[k];
                  }
              }
          }
      }
  }

  // ------------------------------------------------------------------------------------------
  // State interpolation to the coarser level (:425-457): one workgroup per coarse cell gathers the (2p+1)^3 points of its
  // children patch (points that children share carry the same fine DoF), applies the 1D matrix r1 along z, y, x and
  // WRITES the (p+1)^3 coarse values.  A coarse DoF shared by several cells is written by the first cell (in cell
  // order) that contains its entity: one writer, the same value in every run.
  // ------------------------------------------------------------------------------------------
  template <int P>
  struct ICfg
  {
    static constexpr int N       = P + 1;
    static constexpr int M       = 2 * P + 1;
    static constexpr int THREADS = ((M * M + 63) / 64) * 64 > 1024 ? 1024 : ((M * M + 63) / 64) * 64;
  };

  template <int P, typename T>
  __global__ void __launch_bounds__(ICfg<P>::THREADS)
    interpolate_to_coarse_kernel(T *__restrict__ coarse, const T *__restrict__ fine, const uint32_t *__restrict__ idx_c,
                                 const uint32_t *__restrict__ idx_f, const uint32_t *__restrict__ children,
                                 const uint32_t *__restrict__ own_c, uint32_t n_parents, const T *__restrict__ r1d)
  {
    constexpr int N = P + 1, M = 2 * P + 1;
    __shared__ T  r1[M * N];
    __shared__ T  in[N * N * N];
    __shared__ T  t1[N * N * M];
    __shared__ T  t2[N * M * M];
    __shared__ T  out[M * M * M];
    const uint32_t pc = blockIdx.x;
    if (pc >= n_parents)
      return;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < M * N; i += nt)
      r1[i] = r1d[i];
    for (int w = tid; w < 8 * N * N; w += nt) // the fine patch
      {
        const int      ch = w / (N * N), t = w % (N * N), j = t % N, k = t / N;
        const uint32_t fc = children[8u * (size_t)pc + ch];
        const int      ox = (ch & 1) * P, oy = ((ch >> 1) & 1) * P, oz = (ch >> 2) * P;
        const int      b = oy + j, c = oz + k;
        T              r[N];
        gather_line<P, T>(fine, line_index<P>(idx_f, fc, j, k), r);
#pragma unroll
        for (int i = 0; i < N; ++i)
          out[(c * M + b) * M + ox + i] = r[i];
      }
    __syncthreads();
    for (int o = tid; o < N * M * M; o += nt) // z: [k][b][a]
      {
        const int ba = o % (M * M), k = o / (M * M);
        T         s = 0;
#pragma unroll
        for (int c = 0; c < M; ++c)
          s = fma(r1[c * N + k], out[c * M * M + ba], s);
        t2[o] = s;
      }
    __syncthreads();
    for (int o = tid; o < N * N * M; o += nt) // y: [k][j][a]
      {
        const int a = o % M, j = (o / M) % N, k = o / (M * N);
        T         s = 0;
#pragma unroll
        for (int b = 0; b < M; ++b)
          s = fma(r1[b * N + j], t2[(k * M + b) * M + a], s);
        t1[o] = s;
      }
    __syncthreads();
    for (int o = tid; o < N * N * N; o += nt) // x: [k][j][i]
      {
        const int i = o % N, kj = o / N;
        T         s = 0;
#pragma unroll
        for (int a = 0; a < M; ++a)
          s = fma(r1[a * N + i], t1[kj * M + a], s);
        in[o] = s;
      }
    __syncthreads();
    for (int t = tid; t < N * N; t += nt)
      {
        const int    j = t % N, k = t / N;
        LineIndex<P> L = line_index<P>(idx_c, pc, j, k);
        int          cy, o1, cz, o2;
        node_code<P>(j, cy, o1);
        node_code<P>(k, cz, o2);
        const uint32_t own = own_c[pc] >> (9 * cz + 3 * cy); // bits 0, 1, 2: left, interior, right entity of the line
        const T       *r   = in + (k * N + j) * N;
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

  template <int P, typename T, typename TO>
  static void evaluate_coefficient_t(hipStream_t s, const OperatorData &op, void *coef_q, bool minimal_surface, const double *M,
                                     double det, const void *unit_q, const void *jxw_q, const void *state)
  {
    using C           = Cfg<P>;
    const uint32_t nb = (op.n_cells + C::CPB - 1) / C::CPB;
    // the geometry: U and JxW_q at every point (curved cells; metric and det are not read), or M and det J
    const bool       curved = unit_q != nullptr;
    const CellTensor geo    = curved ? CellTensor::at_points(unit_q) : CellTensor::per_mesh(M);
    dispatch_mode<0, 1>(minimal_surface, [&](auto MINSURF) {
      dispatch_mode<0, 1>(curved, [&](auto PERQ) {
        hipLaunchKernelGGL((evaluate_coefficient_kernel<P, T, TO, MINSURF.value != 0, PERQ.value != 0>), dim3(nb), dim3(C::THREADS), 0,
                           s, (TO *)coef_q, (const T *)state, op.idx27_plain, op.n_cells, (const Basis1D<T> *)op.basis, (T)geo.c[0],
                           (T)geo.c[1], (T)geo.c[2], (T)geo.c[3], (T)geo.c[4], (T)geo.c[5], (T)(curved ? 0. : det),
                           (const T *)geo.per_point, (const T *)(curved ? jxw_q : nullptr));
      });
    });
  }

  void launch_evaluate_coefficient(hipStream_t s, const OperatorData &op, void *coef_q, int coef_number, bool minimal_surface,
                                   const double *metric, double det, const void *unit_q, const void *jxw_q, const void *state)
  {
    if (op.dim == 2)
      return launch_evaluate_coefficient_2d(s, op, coef_q, coef_number, minimal_surface, metric, det, unit_q, jxw_q, state);
    dispatch_degree(op.p, [&](auto P) {
      auto run = [&](auto t, auto to) {
        evaluate_coefficient_t<P.value, decltype(t), decltype(to)>(s, op, coef_q, minimal_surface, metric, det, unit_q, jxw_q, state);
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
  static void interpolate_t(hipStream_t s, const TransferData &t, const void *r1d, const uint32_t *own_c, void *coarse,
                            const void *fine)
  {
    const OperatorData &c = *t.coarse, &f = *t.fine;
    hipLaunchKernelGGL((interpolate_to_coarse_kernel<P, T>), dim3(c.n_cells), dim3(ICfg<P>::THREADS), 0, s, (T *)coarse,
                       (const T *)fine, c.idx27_plain, f.idx27_plain, t.children, own_c, c.n_cells, (const T *)r1d);
  }

  void launch_interpolate_to_coarse(hipStream_t s, const TransferData &t, const void *r1d, const uint32_t *own_c, void *coarse,
                                    const void *fine)
  {
    if (t.coarse->dim == 2)
      return launch_interpolate_to_coarse_2d(s, t, r1d, own_c, coarse, fine);
    dispatch_number_degree(t.coarse->number, t.coarse->p, [&](auto number, auto P) {
      interpolate_t<P.value, decltype(number)>(s, t, r1d, own_c, coarse, fine);
    });
  }
} // namespace mgx
