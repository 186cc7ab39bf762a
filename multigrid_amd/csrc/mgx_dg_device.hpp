// mgx_dg_device.hpp -- what the cell kernels of the DG (symmetric interior penalty) operator in three dimensions
// (mgx_dg_kernels.hip) and in two (mgx_dg_kernels_2d.hip) share: the constant block and the argument block of a launch;
// the launch side (dispatch_cells fills the argument block and selects the instantiation, cell_groups counts the
// workgroups; each translation unit instantiates them with its own configuration and kernels); the 1D line products
// (dense on 2-vectors, even-odd, eigenvector basis) that both kernels sweep their cells with; and the block sums of the
// merged CG iterations (block_sum4_cells).  Nothing here knows the dimension of a cell; what does (the LDS layout, the
// ownership of lines and face points) stays with the kernel, and so do the mapping from workgroup to cell and the
// epilogues of the actions: shared versions of those changed the registers, or the choice of fused multiply-adds and
// with it the last bit of some results, of kernels that sit on a register edge.
#pragma once

#include "mgx_internal.hpp"

#include "mgx_dg_host.hpp"

namespace mgx::dg
{
  // the 2D unit's side of launch_dg_cells and cell_grid (mgx_internal.hpp), which the 3D unit defines: false: no kernel
  // for this degree, basis or action
  bool     launch_dg_cells_2d(hipStream_t s, const CellOperands &op, const DGLaunch &launch);
  uint32_t cell_grid_2d(int number, int p, uint32_t n_cells);
  // the variants for operators with Neumann faces (op.has_neumann), each in a unit of its own built from the source
  // of the cell kernel of its dimension (MGX_DG_NEUMANN_UNIT); 3D: every action but kRestrict
  bool launch_dg_cells_neumann(hipStream_t s, const CellOperands &op, const DGLaunch &launch);
  bool launch_dg_cells_2d_neumann(hipStream_t s, const CellOperands &op, const DGLaunch &launch);
} // namespace mgx::dg

namespace mgx::dg::device
{
  using mgx::kMaxN;

  // ------------------------------------------------------------------------------------------
  // device data
  // Even-odd form of an n x n matrix M with M[q][i] = s M[n-1-q][n-1-i] (s = +1: values of a
  // symmetric basis in symmetric points; s = -1: derivatives), H = n / 2:
  //   eo[q H + i] = { (M[q][i] + M[n-1-q][i]) / 2, (M[q][i] - M[n-1-q][i]) / 2 }   (q, i < H)
  //   mrow[i] = M[H][i], mcol[q] = M[q][H], mm = M[H][H]                           (n odd)
  template <typename T>
  struct EOLine
  {
    T eo[2 * (kMaxN / 2) * (kMaxN / 2)];
    T mrow[kMaxN / 2], mcol[kMaxN / 2], mm;
  };

  template <typename T>
  struct DGConst
  {
    T S[kMaxN * kMaxN];  // S[q*n+i]   element basis -> values in the Gauss points
    T D[kMaxN * kMaxN];  // D[q*n+r]   derivative of the Gauss-point Lagrange basis in the Gauss points
    T E[kMaxN * kMaxN];  // E[i*n+e]   eigenvector e of (Laplace + penalty, mass) in the element basis
    T St[kMaxN * kMaxN], Dt[kMaxN * kMaxN], Et[kMaxN * kMaxN]; // their transposes (mul() reads these)
    // even-odd form of S, St (symmetric under reversal of both indices) and D, Dt (antisymmetric),
    // matrix_vector_kernel.h:47-113; see mul_eo below
    EOLine<T> eoS, eoSt, eoD, eoDt;
    // eigenvectors sorted by parity (even ones first): E[n-1-i][e] = +-E[i][e].  With H = n / 2, Ne = n - H
    // even and No = H odd ones: epair[i No + k] = {E[i][k], E[i][Ne + k]} (i < H, k < No),
    // elast[i] = E[i][Ne - 1] and emid[e] = E[H][e] (n odd).  (eo_e: the host found the parities pure; it refuses
    // the operator otherwise -- a run-time choice between the two forms in the kernel costs 10-15 %)
    T   epair[2 * (kMaxN / 2) * (kMaxN / 2)], elast[kMaxN / 2], emid[kMaxN / 2 + 1];
    int eo_e;
    T w[kMaxN];          // Gauss weights on [0,1]
    T b[2][kMaxN], g[2][kMaxN];   // Gauss-point Lagrange basis at x = 0 / 1: value, derivative
    T fb[2][kMaxN], fg[2][kMaxN]; // element basis at x = 0 / 1: value, derivative
    T K[6];              // det J * J^-1 J^-T: xx yy zz xy xz yz (two dimensions: xx yy xy)
    T cn[3][4];          // cn[d][a] = n_d . grad xi_a, n_d the unit normal towards +xi_d
    T fw[4];             // face JxW without the quadrature weight, per direction
    T sigma[4];          // penalty (p+1)^2 |n_d . grad xi_d|
    T hderiv;            // derivative of the first Hermite-like function at x = 0
  };

  template <typename T>
  struct DGArgs
  {
    const T          *src;
    const T          *rhs;
    T                *dst;
    const int32_t    *neigh;
    const DGConst<T> *c;
    const T          *inv_diag; // [4^dim][(p+1)^dim]; kPcgSums: the inverse lumped mass of a cell instead, [(p+1)^dim]
    const uint32_t   *cell_list; // cells of this launch (nullptr: cells cell_first ... in order)
    uint32_t          cell_first;
    uint32_t          n_cells;   // cells of this launch
    uint32_t          n_owned;   // owned cells of the operator: neighbour entries >= n_owned are ghosts
    T                 f1, f2;
    int               iteration_index;
    // cells of a launch without a list: cell_first + cell_stride * i
    uint32_t          cell_stride;
    // kCgSums, kPcgSums: [gridDim.x][4] block sums.  kRestrict: the FE_Q vector the transformed residual is added into,
    // the compressed index table of the FE_Q cells (in the order of the DG cells), the 1D change of basis
    // [n][n] and whether the cells of the launch share no FE_Q DoF (plain adds instead of atomics)
    double           *partials;
    T                *cg;
    const uint32_t   *idx27;
    const T          *P1;
    int               plain;
  };

  // Row of the table of inverse diagonals of a cell in an operator with Neumann faces: the kinds of its NF faces
  // (kind_of_entry: interior, Dirichlet, Neumann) as the digits of a number in base 3, face 0 lowest.  The host builds
  // the rows that occur in the operator's cells (mgx_dg_api.cpp, build_inverse_diagonal).
  template <int NF>
  __host__ __device__ __forceinline__ unsigned face_kind_code(const int (&nb)[NF])
  {
    unsigned code = 0, weight = 1;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      {
        code += weight * (unsigned)kind_of_entry(nb[f]);
        weight *= 3u;
      }
    return code;
  }

  // ------------------------------------------------------------------------------------------
  // launch side: each translation unit instantiates these with the configuration and the kernels of its dimension

  // workgroups of a launch over n_cells cells, C the configuration of the kernel (CPW cells per workgroup)
  template <typename C>
  constexpr uint32_t cell_groups(uint32_t n_cells)
  {
    return (n_cells + C::CPW - 1) / C::CPW;
  }
  // ... C = CFG<p, number type>; a degree no kernel is built for: one cell per workgroup
  template <template <int, typename> class CFG>
  uint32_t cell_groups(int number, int p, uint32_t n_cells)
  {
    uint32_t groups = n_cells;
    mgx::dispatch_degree(p, [&](auto P) {
      mgx::dispatch_number(number, [&](auto t) { groups = cell_groups<CFG<decltype(P)::value, decltype(t)>>(n_cells); });
    });
    return groups;
  }

  // The argument block of a launch from what the launches of an operator share and the launch itself, and number type x
  // degree x basis x action (one of ACTIONS) -> launch_one(P, TYPE, ACTION, args), the first three integral constants.
  // false: no kernel is built for this combination
  template <int... ACTIONS, typename F>
  bool dispatch_cells(const CellOperands &op, const DGLaunch &l, F &&launch_one)
  {
    bool launched = false;
    mgx::dispatch_number(op.number, [&](auto t) {
      using T = decltype(t);
      const DGArgs<T> a{(const T *)l.src, (const T *)l.rhs, (T *)l.dst, op.neigh, (const DGConst<T> *)op.consts,
                        (const T *)(l.action == kPcgSums ? l.lumped : op.inv_diag),
                        l.cell_list, l.cell_first, l.n_cells, op.n_owned, (T)l.f1, (T)l.f2, l.iteration_index, l.cell_stride,
                        l.partials, (T *)l.cg, l.idx27, (const T *)l.P1, l.plain};
      mgx::dispatch_degree(op.degree, [&](auto P) {
        mgx::dispatch_mode<MGX_DG_HERMITE, MGX_DG_GAUSS_LOBATTO, MGX_DG_GAUSS>(op.basis, [&](auto TYPE) {
          launched = mgx::dispatch_mode<ACTIONS...>(l.action, [&](auto ACTION) { launch_one(P, TYPE, ACTION, a); });
        });
      });
    });
    return launched;
  }

  // ------------------------------------------------------------------------------------------
  // line products
  template <int N, typename T>
  __device__ __forceinline__ void ld_line(const T *a, int base, int stride, T (&r)[N])
  {
#pragma unroll
    for (int q = 0; q < N; ++q)
      r[q] = a[base + q * stride];
  }

  template <int N, typename T>
  __device__ __forceinline__ void st_line(T *a, int base, int stride, const T (&r)[N])
  {
#pragma unroll
    for (int q = 0; q < N; ++q)
      a[base + q * stride] = r[q];
  }

  // out[i] = sum_q M[q*N+i] in[q]   (M wave-uniform: scalar loads).  Two neighbouring outputs share
  // the input value and take two consecutive matrix entries: written on 2-vectors so that fp32
  // becomes v_pk_fma_f32 with the matrix pair in a scalar register pair.
  template <int N, typename T>
  __device__ __forceinline__ void mul_t(const T *__restrict__ M, const T (&in)[N], T (&out)[N])
  {
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int H = N / 2;
    T2            acc[H > 0 ? H : 1];
    T             last = 0;
#pragma unroll
    for (int q = 0; q < N; ++q)
      {
        const T2 x = {in[q], in[q]};
#pragma unroll
        for (int h = 0; h < H; ++h)
          {
            const T2 m = {M[q * N + 2 * h], M[q * N + 2 * h + 1]};
            acc[h]     = q == 0 ? m * x : __builtin_elementwise_fma(m, x, acc[h]);
          }
        if (N % 2)
          last = q == 0 ? M[N - 1] * in[0] : fma(M[q * N + N - 1], in[q], last);
      }
#pragma unroll
    for (int h = 0; h < H; ++h)
      {
        out[2 * h]     = acc[h][0];
        out[2 * h + 1] = acc[h][1];
      }
    if (N % 2)
      out[N - 1] = last;
  }

  // out[q] = sum_i M[q*N+i] in[i], given the transposed matrix Mt[i*N+q] = M[q*N+i]
  template <int N, typename T>
  __device__ __forceinline__ void mul(const T *__restrict__ Mt, const T (&in)[N], T (&out)[N])
  {
    mul_t<N, T>(Mt, in, out);
  }

  // The same product, out[i] = sum_q M[q][i] in[q], for a matrix with the reversal symmetry of sign SIGN
  // in even-odd form (the reference's apply_1d_matvec_kernel, matrix_vector_kernel.h:47-113): the input
  // is split into xe = in[q] + in[n-1-q] and xo = in[q] - in[n-1-q]; u = ce^T xe and v = co^T xo are two
  // independent half-size products (one 2-vector FMA per entry: v_pk_fma_f32 in fp32), out[i] = u + v,
  // out[n-1-i] = SIGN (u - v).  n^2 multiply-adds become n^2 / 2 + n additions.
  template <int N, typename T, int SIGN>
  __device__ __forceinline__ void mul_eo(const EOLine<T> &A, const T (&in)[N], T (&out)[N])
  {
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int H = N / 2;
    T2            x[H > 0 ? H : 1];
#pragma unroll
    for (int q = 0; q < H; ++q)
      x[q] = T2{in[q] + in[N - 1 - q], in[q] - in[N - 1 - q]};
#pragma unroll
    for (int i = 0; i < H; ++i)
      {
        T2 acc = T2{A.eo[2 * i], A.eo[2 * i + 1]} * x[0];
#pragma unroll
        for (int q = 1; q < H; ++q)
          acc = __builtin_elementwise_fma(T2{A.eo[2 * (q * H + i)], A.eo[2 * (q * H + i) + 1]}, x[q], acc);
        if (N % 2)
          acc[0] = fma(A.mrow[i], in[H], acc[0]);
        out[i]         = acc[0] + acc[1];
        out[N - 1 - i] = SIGN > 0 ? acc[0] - acc[1] : acc[1] - acc[0];
      }
    if (N % 2)
      {
        T m = SIGN > 0 ? A.mm * in[H] : T(0);
#pragma unroll
        for (int q = 0; q < H; ++q)
          m = fma(A.mcol[q], SIGN > 0 ? x[q][0] : x[q][1], m);
        out[H] = m;
      }
  }

  // which form a (degree, number type) instantiation uses.  In fp32 the dense product already runs on
  // 2-vectors (13 packed FMAs per line at p = 4 against 12 instructions plus the additions of the
  // even-odd one): the gain starts small and grows with the degree; fp64 has no packed FMA.
  template <int N, typename T>
  struct LineForm
  {
#ifdef MGX_DG_EVEN_ODD
    static constexpr bool eo = MGX_DG_EVEN_ODD != 0;
#else
    static constexpr bool eo = N >= 5; // measured (merged Chebyshev step, MI355X): fp32 p = 3 -2 %, p = 4 +4 %, p = 6 +32 %, p = 8 +60 %; fp64 p = 4 +13 %, p = 8 +118 %
#endif
  };
  // the four sweeps of the kernel: values S / S^T (symmetric), derivative D / D^T (antisymmetric);
  // in (mul_t convention) out[i] = sum_q M[q][i] in[q]
  template <int N, typename T>
  __device__ __forceinline__ void mul_S(const DGConst<T> *__restrict__ c, const T (&in)[N], T (&out)[N]) // mul_t(c->S)
  {
    if constexpr (LineForm<N, T>::eo)
      mul_eo<N, T, 1>(c->eoS, in, out);
    else
      mul_t<N, T>(c->S, in, out);
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_St(const DGConst<T> *__restrict__ c, const T (&in)[N], T (&out)[N]) // mul(c->St)
  {
    if constexpr (LineForm<N, T>::eo)
      mul_eo<N, T, 1>(c->eoSt, in, out);
    else
      mul_t<N, T>(c->St, in, out);
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_D(const DGConst<T> *__restrict__ c, const T (&in)[N], T (&out)[N]) // mul_t(c->D)
  {
    if constexpr (LineForm<N, T>::eo)
      mul_eo<N, T, -1>(c->eoD, in, out);
    else
      mul_t<N, T>(c->D, in, out);
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_Dt(const DGConst<T> *__restrict__ c, const T (&in)[N], T (&out)[N]) // mul(c->Dt)
  {
    if constexpr (LineForm<N, T>::eo)
      mul_eo<N, T, -1>(c->eoDt, in, out);
    else
      mul_t<N, T>(c->Dt, in, out);
  }

  template <int N, typename T>
  __device__ __forceinline__ T dot_line(const T *__restrict__ v, const T (&in)[N])
  {
    T s = v[0] * in[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
      s += v[i] * in[i];
    return s;
  }

  template <int N, typename T>
  __device__ __forceinline__ void copy_line(const T (&in)[N], T (&out)[N])
  {
#pragma unroll
    for (int i = 0; i < N; ++i)
      out[i] = in[i];
  }

  // kPcgSums, one entry: q = (A p)_i, p, r and the inverse lumped mass m of the entry's local index.  As in kCgSums the
  // products are formed in the number type and summed in double; m r is the product the update kernel of the solver forms.
  template <typename T>
  __device__ __forceinline__ void pcg_sums_add(double (&sum)[4], T q, T p, T r, T m)
  {
    const T mr = m * r;
    sum[0] += (double)(q * p);
    sum[1] += (double)(r * mr);
    sum[2] += (double)(q * mr);
    sum[3] += (double)(q * (m * q));
  }

  // the four sums of a workgroup of THREADS threads -> partials[blockIdx.x][4]: shuffles within a wave, then the waves'
  // sums through `red` (4 doubles per wave, LDS the caller no longer reads) in the order of the waves.  Every thread of
  // the workgroup calls it.
  template <int THREADS>
  __device__ __forceinline__ void block_sum4_cells(double (&sum)[4], double *red, int tid, double *__restrict__ partials)
  {
    constexpr int WAVES = THREADS / 64;
    static_assert(THREADS % 64 == 0, "whole waves");
#pragma unroll
    for (int k = 0; k < 4; ++k)
      {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
          sum[k] += __shfl_down(sum[k], o);
        if ((tid & 63) == 0)
          red[(tid >> 6) * 4 + k] = sum[k];
      }
    __syncthreads();
    if (tid < 4)
      {
        double t4 = red[tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
          t4 += red[w * 4 + tid];
        partials[(size_t)blockIdx.x * 4 + tid] = t4;
      }
  }

  // q[e] = sum_i E[i][e] r[i] (to the eigenvector basis) and r[i] = sum_e E[i][e] q[e] (back): every
  // eigenvector is even or odd, so the even ones see r[i] + r[n-1-i] only, the odd ones r[i] - r[n-1-i]
  template <int N, typename T>
  __device__ __forceinline__ void mul_E(const DGConst<T> *__restrict__ c, const T (&r)[N], T (&q)[N])
  {
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int H = N / 2, Ne = N - H, No = H;
    if constexpr (!LineForm<N, T>::eo)
      return mul_t<N, T>(c->E, r, q);
    T2 x[H > 0 ? H : 1];
#pragma unroll
    for (int i = 0; i < H; ++i)
      x[i] = T2{r[i] + r[N - 1 - i], r[i] - r[N - 1 - i]};
#pragma unroll
    for (int k = 0; k < No; ++k)
      {
        T2 acc = T2{c->epair[2 * k], c->epair[2 * k + 1]} * x[0];
#pragma unroll
        for (int i = 1; i < H; ++i)
          acc = __builtin_elementwise_fma(T2{c->epair[2 * (i * No + k)], c->epair[2 * (i * No + k) + 1]}, x[i], acc);
        if (N % 2)
          acc[0] = fma(c->emid[k], r[H], acc[0]);
        q[k]      = acc[0];
        q[Ne + k] = acc[1];
      }
    if (N % 2)
      {
        T m = c->emid[Ne - 1] * r[H];
#pragma unroll
        for (int i = 0; i < H; ++i)
          m = fma(c->elast[i], x[i][0], m);
        q[Ne - 1] = m;
      }
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_Et(const DGConst<T> *__restrict__ c, const T (&q)[N], T (&r)[N])
  {
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int H = N / 2, Ne = N - H, No = H;
    if constexpr (!LineForm<N, T>::eo)
      return mul_t<N, T>(c->Et, q, r);
#pragma unroll
    for (int i = 0; i < H; ++i)
      {
        T2 acc = T2{c->epair[2 * (i * No)], c->epair[2 * (i * No) + 1]} * T2{q[0], q[Ne]};
#pragma unroll
        for (int k = 1; k < No; ++k)
          acc = __builtin_elementwise_fma(T2{c->epair[2 * (i * No + k)], c->epair[2 * (i * No + k) + 1]}, T2{q[k], q[Ne + k]}, acc);
        if (N % 2)
          acc[0] = fma(c->elast[i], q[Ne - 1], acc[0]);
        r[i]         = acc[0] + acc[1];
        r[N - 1 - i] = acc[0] - acc[1];
      }
    if (N % 2)
      {
        T m = c->emid[0] * q[0];
#pragma unroll
        for (int e = 1; e < Ne; ++e)
          m = fma(c->emid[e], q[e], m);
        r[H] = m;
      }
  }
} // namespace mgx::dg::device
