// mgx_dg_rhs.hip -- right-hand side with Dirichlet boundary data and the sums of the L2 error of the DG (symmetric
// interior penalty) operator on the device, in two and three dimensions (mgx_dg_compute_rhs, mgx_dg_compute_l2_error).
//
// Reference behaviour (not code): the volume term of common/multigrid_solver_dg_plain.h:163-185 and
// compute_l2_error :219-259; the boundary term is the one the face-based form common/laplace_operator_dg_face.h:146-157
// implies for boundary values g on a Dirichlet face F with outward normal n and penalty sigma_F,
//   b_i += int_F g (sigma_F phi_i - d_n phi_i).
//
// Design (MI355X).  The cell kernel's mapping: (p+1)^(dim-1) threads per cell, 256 / that many cells per workgroup;
// thread (a, b) owns the x-line (j, k) = (a, b), the y-line (i, k) = (a, b), the z-line (i, j) = (a, b) and the point
// (a, b) of every face, lines are in registers, and a cell's tile in the LDS (odd row and plane pitch) carries them
// from one sweep to the next.  All arithmetic is in double, whatever the operator's number type; the 1D matrices S, D
// and the end values b, g are the operator's constant block (converted on the fly in fp32), the geometry factors
// (sigma, fw, cn, det J) the host's doubles.  Everything is assembled in the Gauss points -- where the test functions
// are the collocation polynomials l_q --
//   H[q] = JxW_q f(x_q) + sum over the Dirichlet faces (d, s) of  b_s[q_d] V[q_t] + g_s[q_d] W[q_t],
//   V = sigma_F B - n_s (sum over the tangential a of cn[d][a] D_a^T B),  W = -n_s cn[d][d] B,  B = w fw[d] g,
// (n_s = +1 on the upper, -1 on the lower face; the two face arrays stay in the registers of the face point's owner,
// who also owns the line they are expanded along), then S^T is applied in dim sweeps.  The sweeps end with the lines
// of the last direction, whose owners store one coalesced row of the cell per entry; the sampled values are read the
// same way.  A cell reads its Dirichlet faces off the neighbour table: the branch is uniform per cell, every barrier
// is outside it.  One writer per entry, no atomics: the same bits in every run.
//
// Operators with Neumann faces run a variant of the right-hand side kernel (MIXED) that tells the two kinds of boundary
// entry apart and adds int_F h phi_i on the Neumann faces: V = B, W = 0 with B = w fw[d] h in the face point -- no
// tangential part, so B never leaves the registers of the point's owner.  h is sampled in the face points, or the
// normal derivative n . grad u of a sine product u: d_k u = amplitude wave[k] cos(.) prod_{d != k} sin(.), from the
// sines and cosines the complex products hold anyway, n the outward unit normal of the operator's geometry.  A third
// function means a third table of the cell-independent factors; the kernels of operators without Neumann faces keep
// their two.
//
// The sine product amplitude prod_d sin(wave[d] x_d + phase[d]) with x = origin + J (pos + xi) is separable in the
// reference coordinates through the complex exponential: sin(t_d + sum_a wave[d] J[d][a] xi_a) is the imaginary part of
// e^{i t_d} prod_a e^{i wave[d] J[d][a] xi_a}.  The factors of the second kind do not depend on the cell: dim^2 (p+3)
// sines and cosines per workgroup (the p+1 Gauss points and the two ends), dim per cell for t_d, and complex products
// from there -- not dim (p+1)^dim sines per cell.
//
// The error kernel applies S in dim sweeps, subtracts u in the Gauss points, weights with JxW and leaves four block
// sums (two of them used) for the ordered second stage the merged CG iterations use (block_sum4_cells, launch_reduce4).
#include "mgx_dg_device.hpp"

#include <type_traits>

namespace
{
  using namespace mgx::dg;
  using namespace mgx::dg::device;

  // NFN: functions whose sine-product tables the LDS holds (f and g; the MIXED kernel: and h)
  template <int P, int DIM, int NFN = 2>
  struct RhsCfg
  {
    static constexpr int N     = P + 1;
    static constexpr int TPC   = DIM == 3 ? N * N : N;       // threads per cell = points of a face = lines of a direction
    static constexpr int NN    = TPC * N;                    // entries of a cell
    static constexpr int WG    = 256;
    static constexpr int CPW   = WG / TPC;                   // 3D: p = 1 ... 9: 64 28 16 10 7 5 4 3 2 cells
    static constexpr int PX    = N | 1;                      // odd row pitch
    static constexpr int PL    = DIM == 3 ? (N * PX) | 1 : 0; // odd plane pitch
    static constexpr int TILE  = DIM == 3 ? N * PL : N * PX;
    static constexpr int NF    = 2 * DIM;
    static constexpr int BASES = 2 * DIM * NFN;              // e^{i t_d} of every function
    static constexpr int CELL  = (TILE + NF * TPC + BASES) | 1;
    static constexpr int TAB1  = DIM * DIM * (N + 2) * 2;    // e^{i wave[d] J[d][a] xi} of one function
    static constexpr int LDS   = CPW * CELL + NFN * TAB1;
    static_assert(LDS * (int)sizeof(double) <= 65536, "cells of a workgroup do not fit the LDS");
  };

  template <typename T>
  struct RhsArgs
  {
    DGFunctionArgs    f, g; // right-hand side: f in the cells, g on the Dirichlet faces; error: f is u
    const T          *src;
    T                *dst;
    double           *partials;
    const int32_t    *neigh;
    const DGConst<T> *c;
    const int32_t    *pos; // [n_cells][dim] or nullptr
    uint32_t          n_cells;
    DGRhsGeometry     geo;
  };

  // ... of the MIXED right-hand side: and the flux on the Neumann faces, or the potential it derives from
  template <typename T>
  struct RhsArgsMixed : RhsArgs<T>
  {
    DGFunctionArgs h;
  };

  // out[i] = sum_q M[q*N+i] in[q] with a matrix of another number type
  template <int N, typename T>
  __device__ __forceinline__ void mul_t_wide(const T *__restrict__ M, const double (&in)[N], double (&out)[N])
  {
#pragma unroll
    for (int i = 0; i < N; ++i)
      out[i] = (double)M[i] * in[0];
#pragma unroll
    for (int q = 1; q < N; ++q)
#pragma unroll
      for (int i = 0; i < N; ++i)
        out[i] = fma((double)M[q * N + i], in[q], out[i]);
  }
  // coefficients of the test functions from those of the collocation polynomials: out[i] = sum_q S[q][i] in[q]
  template <int N, typename T>
  __device__ __forceinline__ void sweep_S(const DGConst<T> *__restrict__ c, const double (&in)[N], double (&out)[N])
  {
    if constexpr (std::is_same<T, double>::value)
      mul_S<N>(c, in, out);
    else
      mul_t_wide<N>(c->S, in, out);
  }
  // values in the Gauss points: out[q] = sum_i S[q][i] in[i]
  template <int N, typename T>
  __device__ __forceinline__ void sweep_St(const DGConst<T> *__restrict__ c, const double (&in)[N], double (&out)[N])
  {
    if constexpr (std::is_same<T, double>::value)
      mul_St<N>(c, in, out);
    else
      mul_t_wide<N>(c->St, in, out);
  }

  // first entry and stride in a cell's tile of the line of direction d that thread (a, b) owns
  template <typename C, int DIM>
  __device__ __forceinline__ int line_base(int d, int a, int b)
  {
    if constexpr (DIM == 3)
      return d == 0 ? a * C::PX + b * C::PL : (d == 1 ? a + b * C::PL : a + b * C::PX);
    else
      return d == 0 ? a * C::PX : a;
  }
  template <typename C, int DIM>
  __device__ __forceinline__ int line_stride(int d)
  {
    if constexpr (DIM == 3)
      return d == 0 ? 1 : (d == 1 ? C::PX : C::PL);
    else
      return d == 0 ? 1 : C::PX;
  }

  // the cell-independent factors of a sine product, by the whole workgroup: tab[((d DIM + a) (N+2) + q) 2] =
  // {cos, sin}(wave[d] J[d][a] xi_q), xi_q the Gauss points, then 0 and 1
  template <int N, int DIM>
  __device__ __forceinline__ void sine_table(const DGFunctionArgs &fn, const DGRhsGeometry &geo, double *tab, int tid, int threads)
  {
    if (fn.kind != MGX_DG_FN_SINE_PRODUCT)
      return;
    for (int e = tid; e < DIM * DIM * (N + 2); e += threads)
      {
        const int    q = e % (N + 2), da = e / (N + 2), d = da / DIM, a = da % DIM;
        const double xi = q < N ? geo.xq[q] : (q == N ? 0.0 : 1.0);
        double       s, c;
        sincos(fn.wave[d] * geo.jac[d * 3 + a] * xi, &s, &c);
        tab[2 * e]     = c;
        tab[2 * e + 1] = s;
      }
  }
  // the cell's factors e^{i t_d}, t_d = wave[d] x_d(pos) + phase[d]
  template <int DIM>
  __device__ __forceinline__ void sine_base(const DGFunctionArgs &fn, const DGRhsGeometry &geo, const int32_t *pos, int d, double *base)
  {
    double x = geo.origin[d];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      x += geo.jac[d * 3 + a] * (double)pos[a];
    double s, c;
    sincos(fn.wave[d] * x + fn.phase[d], &s, &c);
    base[2 * d]     = c;
    base[2 * d + 1] = s;
  }
  // the sine product in the point with the 1D indices ix (0 ... N-1: Gauss point, N: xi = 0, N+1: xi = 1)
  template <int N, int DIM>
  __device__ __forceinline__ double sine_value(double amplitude, const double *tab, const double *base, const int (&ix)[DIM])
  {
    double v = amplitude;
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      {
        double re = base[2 * d], im = base[2 * d + 1];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
          {
            const double *t  = tab + ((d * DIM + a) * (N + 2) + ix[a]) * 2;
            const double  r2 = re * t[0] - im * t[1];
            im               = fma(re, t[1], im * t[0]);
            re               = r2;
          }
        v *= im;
      }
    return v;
  }

  // the gradient of the sine product in that point: grad[k] = amplitude wave[k] cos(.) prod_{d != k} sin(.)
  template <int N, int DIM>
  __device__ __forceinline__ void sine_gradient(const DGFunctionArgs &fn, const double *tab, const double *base, const int (&ix)[DIM],
                                                double (&grad)[DIM])
  {
    double co[DIM], si[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      {
        double re = base[2 * d], im = base[2 * d + 1];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
          {
            const double *t  = tab + ((d * DIM + a) * (N + 2) + ix[a]) * 2;
            const double  r2 = re * t[0] - im * t[1];
            im               = fma(re, t[1], im * t[0]);
            re               = r2;
          }
        co[d] = re;
        si[d] = im;
      }
#pragma unroll
    for (int k = 0; k < DIM; ++k)
      {
        double v = fn.amplitude * fn.wave[k] * co[k];
#pragma unroll
        for (int d = 0; d < DIM; ++d)
          if (d != k)
            v *= si[d];
        grad[k] = v;
      }
  }

  // what both kernels begin with: thread -> cell and lines, the LDS of the cell, the tables of the sine products
  template <int P, int DIM, typename T, int NFN = 2>
  struct CellSetup
  {
    using C = RhsCfg<P, DIM, NFN>;
    int      tid, cw, t, a, b;
    bool     active, store;
    uint32_t cell;
    double  *U, *F, *base, *tab;

    template <typename ARGS>
    __device__ __forceinline__ CellSetup(const ARGS &A, double *lds)
    {
      tid    = threadIdx.x;
      cw     = tid / C::TPC;
      t      = tid - cw * C::TPC;
      a      = DIM == 3 ? t % C::N : t;
      b      = DIM == 3 ? t / C::N : 0;
      active = cw < C::CPW;
      cell   = blockIdx.x * C::CPW + (active ? cw : 0);
      store  = active && cell < A.n_cells;
      if (cell >= A.n_cells)
        cell = A.n_cells - 1;
      U    = lds + (active ? cw : 0) * C::CELL;
      F    = U + C::TILE;
      base = F + C::NF * C::TPC;
      tab  = lds + C::CPW * C::CELL;
      sine_table<C::N, DIM>(A.f, A.geo, tab, tid, C::WG);
      sine_table<C::N, DIM>(A.g, A.geo, tab + C::TAB1, tid, C::WG);
      if constexpr (NFN > 2)
        sine_table<C::N, DIM>(A.h, A.geo, tab + 2 * C::TAB1, tid, C::WG);
      if (active)
        for (int k = t; k < 2 * DIM; k += C::TPC)
          {
            const DGFunctionArgs &fn = k < DIM ? A.f : A.g;
            if (fn.kind == MGX_DG_FN_SINE_PRODUCT)
              sine_base<DIM>(fn, A.geo, A.pos + (size_t)cell * DIM, k % DIM, base + (k < DIM ? 0 : 2 * DIM));
          }
      if constexpr (NFN > 2) // (a loop of its own: a choice between three functions copies the arguments to scratch)
        if (active && A.h.kind == MGX_DG_FN_SINE_PRODUCT)
          for (int d = t; d < DIM; d += C::TPC)
            sine_base<DIM>(A.h, A.geo, A.pos + (size_t)cell * DIM, d, base + 4 * DIM);
      __syncthreads();
    }
    // 1D indices of point q of the thread's line of the last direction
    __device__ __forceinline__ void line_point(int q, int (&ix)[DIM]) const
    {
      ix[0] = a;
      if constexpr (DIM == 3)
        ix[1] = b;
      ix[DIM - 1] = q;
    }
    // ... of the thread's point of face 2 d + s
    __device__ __forceinline__ void face_point(int d, int s, int (&ix)[DIM]) const
    {
      int k = 0;
#pragma unroll
      for (int e = 0; e < DIM; ++e)
        ix[e] = e == d ? C::N + s : (k++ == 0 ? a : b);
    }
    // quadrature weight of that face point / of point q of the line of the last direction, without the geometry
    __device__ __forceinline__ double face_weight(const DGRhsGeometry &geo) const
    {
      return DIM == 3 ? geo.wq[a] * geo.wq[b] : geo.wq[a];
    }
  };

  // MIXED: the operator has Neumann faces (see the head of the file)
  template <int P, int DIM, typename T, bool MIXED>
  __global__ void __launch_bounds__((RhsCfg<P, DIM>::WG))
    dg_rhs_kernel(const std::conditional_t<MIXED, RhsArgsMixed<T>, RhsArgs<T>> A)
  {
    using C         = RhsCfg<P, DIM, MIXED ? 3 : 2>;
    constexpr int N = C::N, TPC = C::TPC, NF = C::NF;
    __shared__ __attribute__((aligned(16))) double lds[C::LDS];
    const DGConst<T> *__restrict__ c = A.c;
    const CellSetup<P, DIM, T, MIXED ? 3 : 2> K(A, lds);
    const int a = K.a, b = K.b, t = K.t;

    bool dirichlet[NF], neumann[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
      {
        if constexpr (MIXED)
          {
            const int32_t entry = A.neigh[(size_t)K.cell * NF + f];
            dirichlet[f]        = A.g.kind != MGX_DG_FN_NONE && entry == MGX_DG_BOUNDARY;
            neumann[f]          = A.h.kind != MGX_DG_FN_NONE && entry == MGX_DG_NEUMANN;
          }
        else
          {
            dirichlet[f] = A.g.kind != MGX_DG_FN_NONE && A.neigh[(size_t)K.cell * NF + f] < 0;
            neumann[f]   = false;
          }
      }

    // ---- 1. the line of the last direction: JxW f in its Gauss points; B = w fw g in the thread's face points
    double h[N];
#pragma unroll
    for (int q = 0; q < N; ++q)
      h[q] = 0;
    if (K.active)
      {
        if (A.f.kind != MGX_DG_FN_NONE)
          {
            const double wf = A.geo.det * K.face_weight(A.geo);
#pragma unroll
            for (int q = 0; q < N; ++q)
              {
                int ix[DIM];
                K.line_point(q, ix);
                const double v = A.f.kind == MGX_DG_FN_SINE_PRODUCT ? sine_value<N, DIM>(A.f.amplitude, K.tab, K.base, ix)
                                                                    : A.f.cell_values[(size_t)K.cell * C::NN + t + q * TPC];
                h[q] = v * wf * A.geo.wq[q];
              }
          }
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (dirichlet[f])
            {
              int ix[DIM];
              K.face_point(f / 2, f % 2, ix);
              const double v = A.g.kind == MGX_DG_FN_SINE_PRODUCT
                                 ? sine_value<N, DIM>(A.g.amplitude, K.tab + C::TAB1, K.base + 2 * DIM, ix)
                                 : A.g.face_values[((size_t)K.cell * NF + f) * TPC + t];
              K.F[f * TPC + t] = v * K.face_weight(A.geo) * A.geo.fw[f / 2];
            }
      }
    __syncthreads();

    // ---- 2. the two arrays of every Dirichlet face in the thread's face point: V is tested with the trace, W with the
    // normal derivative along the line; the tangential part of the normal derivative is D^T along the face lines
    double V[NF], W[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
      {
        V[f] = W[f] = 0;
        if (K.active && dirichlet[f])
          {
            const int     d = f / 2;
            const double  ns = f % 2 ? 1.0 : -1.0;
            const double *B  = K.F + f * TPC;
            const int     t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
            double        acc = 0;
#pragma unroll
            for (int r = 0; r < N; ++r)
              acc = fma((double)c->D[r * N + a], B[DIM == 3 ? r + b * N : r], acc);
            double tang = A.geo.cn[d][t1] * acc;
            if constexpr (DIM == 3)
              {
                acc = 0;
#pragma unroll
                for (int r = 0; r < N; ++r)
                  acc = fma((double)c->D[r * N + b], B[a + r * N], acc);
                tang = fma(A.geo.cn[d][t2], acc, tang);
              }
            V[f] = 2.0 * A.geo.sigma[d] * B[t] - ns * tang;
            W[f] = -ns * A.geo.cn[d][d] * B[t];
          }
        if constexpr (MIXED)
          if (K.active && neumann[f])
            {
              // V = B = w fw[d] h, W = 0
              const int d = f / 2;
              double    flux;
              if (A.h.kind == MGX_DG_FN_SINE_PRODUCT)
                {
                  int    ix[DIM];
                  double grad[DIM];
                  K.face_point(d, f % 2, ix);
                  sine_gradient<N, DIM>(A.h, K.tab + 2 * C::TAB1, K.base + 4 * DIM, ix, grad);
                  flux = 0;
#pragma unroll
                  for (int k = 0; k < DIM; ++k)
                    flux = fma(A.geo.normal[d][k], grad[k], flux);
                  flux = f % 2 ? flux : -flux;
                }
              else
                flux = A.h.face_values[((size_t)K.cell * NF + f) * TPC + t];
              V[f] = flux * K.face_weight(A.geo) * A.geo.fw[d];
            }
      }

    // ---- 3. the faces of every direction join in the Gauss points, last direction first; the lines of the first
    // direction go on to the coefficients of the test functions
#pragma unroll
    for (int d = DIM - 1; d >= 0; --d)
      {
        const int base = line_base<C, DIM>(d, a, b), stride = line_stride<C, DIM>(d);
        if (K.active)
          {
            if (d != DIM - 1)
              ld_line<N>(K.U, base, stride, h);
            if (dirichlet[2 * d] || dirichlet[2 * d + 1] || neumann[2 * d] || neumann[2 * d + 1])
              {
#pragma unroll
                for (int q = 0; q < N; ++q)
                  h[q] += (double)c->b[0][q] * V[2 * d] + (double)c->b[1][q] * V[2 * d + 1] + (double)c->g[0][q] * W[2 * d] +
                          (double)c->g[1][q] * W[2 * d + 1];
              }
            if (d == 0)
              {
                double o[N];
                sweep_S<N>(c, h, o);
                st_line<N>(K.U, base, stride, o);
              }
            else
              st_line<N>(K.U, base, stride, h);
          }
        __syncthreads();
      }
    // ---- 4. the other directions; the owners of the last one store
#pragma unroll
    for (int d = 1; d < DIM; ++d)
      {
        const int base = line_base<C, DIM>(d, a, b), stride = line_stride<C, DIM>(d);
        double    o[N];
        if (K.active)
          {
            ld_line<N>(K.U, base, stride, h);
            sweep_S<N>(c, h, o);
            if (d != DIM - 1)
              st_line<N>(K.U, base, stride, o);
          }
        if (d != DIM - 1)
          __syncthreads();
        else if (K.store)
          {
#pragma unroll
            for (int q = 0; q < N; ++q)
              A.dst[(size_t)K.cell * C::NN + t + q * TPC] = (T)o[q];
          }
      }
  }

  template <int P, int DIM, typename T>
  __global__ void __launch_bounds__((RhsCfg<P, DIM>::WG)) dg_l2_error_kernel(const RhsArgs<T> A)
  {
    using C         = RhsCfg<P, DIM>;
    constexpr int N = C::N, TPC = C::TPC;
    __shared__ __attribute__((aligned(16))) double lds[C::LDS];
    const DGConst<T> *__restrict__ c = A.c;
    const CellSetup<P, DIM, T> K(A, lds);
    const int a = K.a, b = K.b, t = K.t;

    // values of the vector in the Gauss points: S along x, y(, z)
    double v[N];
#pragma unroll
    for (int q = 0; q < N; ++q)
      v[q] = 0;
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      {
        const int base = line_base<C, DIM>(d, a, b), stride = line_stride<C, DIM>(d);
        if (K.active)
          {
            double u[N];
            if (d == 0)
              {
#pragma unroll
                for (int i = 0; i < N; ++i)
                  u[i] = (double)A.src[(size_t)K.cell * C::NN + t * N + i];
              }
            else
              ld_line<N>(K.U, base, stride, u);
            sweep_St<N>(c, u, v);
            if (d != DIM - 1)
              st_line<N>(K.U, base, stride, v);
          }
        if (d != DIM - 1)
          __syncthreads();
      }
    double sum[4] = {0., 0., 0., 0.};
    if (K.store)
      {
        const double wf = A.geo.det * K.face_weight(A.geo);
#pragma unroll
        for (int q = 0; q < N; ++q)
          {
            int ix[DIM];
            K.line_point(q, ix);
            const double u = A.f.kind == MGX_DG_FN_SINE_PRODUCT ? sine_value<N, DIM>(A.f.amplitude, K.tab, K.base, ix)
                                                                : A.f.cell_values[(size_t)K.cell * C::NN + t + q * TPC];
            const double jxw = wf * A.geo.wq[q], e = v[q] - u;
            sum[0] = fma(e * e, jxw, sum[0]);
            sum[1] += jxw;
          }
      }
    __syncthreads(); // the tile becomes the scratch of the block sums
    block_sum4_cells<C::WG>(sum, lds, K.tid, A.partials);
  }

  template <typename F>
  bool dispatch_rhs(const DGRhsOperands &op, F &&launch_one)
  {
    bool launched = false;
    mgx::dispatch_number(op.number, [&](auto t) {
      mgx::dispatch_degree(op.degree, [&](auto P) { launched = mgx::dispatch_mode<2, 3>(op.dim, [&](auto DIM) { launch_one(P, DIM, t); }); });
    });
    return launched;
  }

  template <typename T>
  RhsArgs<T> make_args(const DGRhsOperands &op, const DGFunctionArgs &f, const DGFunctionArgs &g, const void *src, void *dst,
                       double *partials)
  {
    return RhsArgs<T>{f, g, (const T *)src, (T *)dst, partials, op.neigh, (const DGConst<T> *)op.consts, op.cell_pos, op.n_cells, op.geo};
  }
} // namespace

namespace mgx::dg
{
  uint32_t rhs_grid(int p, uint32_t n_cells, int dim)
  {
    uint32_t groups = n_cells;
    mgx::dispatch_degree(p, [&](auto P) {
      mgx::dispatch_mode<2, 3>(dim, [&](auto DIM) { groups = (n_cells + RhsCfg<P.value, DIM.value>::CPW - 1) / RhsCfg<P.value, DIM.value>::CPW; });
    });
    return groups;
  }

  bool launch_dg_rhs(hipStream_t s, const DGRhsOperands &op, const DGFunctionArgs &f, const DGFunctionArgs &g,
                     const DGFunctionArgs &h, void *dst)
  {
    return dispatch_rhs(op, [&](auto P, auto DIM, auto t) {
      using T               = decltype(t);
      const dim3       grid = dim3(rhs_grid(op.degree, op.n_cells, op.dim)), block = dim3(RhsCfg<P.value, DIM.value>::WG);
      const RhsArgs<T> args = make_args<T>(op, f, g, nullptr, dst, nullptr);
      if (op.has_neumann)
        {
          RhsArgsMixed<T> mixed;
          static_cast<RhsArgs<T> &>(mixed) = args;
          mixed.h                          = h;
          hipLaunchKernelGGL((dg_rhs_kernel<P.value, DIM.value, T, true>), grid, block, 0, s, mixed);
        }
      else
        hipLaunchKernelGGL((dg_rhs_kernel<P.value, DIM.value, T, false>), grid, block, 0, s, args);
    });
  }

  bool launch_dg_l2_error(hipStream_t s, const DGRhsOperands &op, const DGFunctionArgs &u, const void *vec, double *partials)
  {
    return dispatch_rhs(op, [&](auto P, auto DIM, auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((dg_l2_error_kernel<P.value, DIM.value, T>), dim3(rhs_grid(op.degree, op.n_cells, op.dim)),
                         dim3(RhsCfg<P.value, DIM.value>::WG), 0, s, make_args<T>(op, u, DGFunctionArgs{}, vec, nullptr, partials));
    });
  }
} // namespace mgx::dg
