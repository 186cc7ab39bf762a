// mgx_dg_kernels_2d.hip -- the gfx950 cell kernel of the DG (symmetric interior penalty) Laplace operator on an affine
// mesh of quadrilaterals, with the merged Chebyshev update and the sums of the merged CG iteration: LaplaceOperatorCompactCombine<2,p,Number,type> and
// JacobiTransformed<2,p,Number,type>.  The line products, the block sums, the constant block, the argument block and the
// launch side (dispatch_cells, cell_groups) are those of the 3D kernel (mgx_dg_device.hpp); this file holds what depends
// on the dimension and is reached through launch_dg_cells / cell_grid of the 3D unit.
//
// Reference behaviour (not code): common/laplace_operator_dg.h -- the dim == 2 branches of operation_on_cells
// (:1147 cell loop, :1359-1457 / :1418 neighbour access, :1568-1577 Dirichlet faces, :1675-1716 cell term),
// JacobiTransformed :2028-2256 (:2162 dim == 2), as driven by poisson_dg_plain/program.cc:65.
//
// Design (MI355X), the 3D kernel one dimension down: a workgroup of 256 threads takes CPW = 256 / (p+1) consecutive
// cells (64 at p = 3); the p+1 threads of a cell each own the x-line j = a, the y-line i = a and the point a of each of
// the four faces, so a face's own trace and normal derivative fall out of the sweep that has the line in registers and
// never leave them.  Per cell the LDS holds the values U in the Gauss points, the y-component of the gradient (the
// x-component lives in registers of the x-line's owner) and three arrays of p+1 words per face of the direction in
// work (neighbour trace -> sum of the traces, neighbour normal derivative -> weighted jump, tangential part).  Rows
// have an odd pitch, the per-cell stride is congruent to p+1 modulo the 32 banks.  Neighbour data is read straight
// from the source vector: two nodes per face point for the Hermite-like basis, a contracted line otherwise.  The
// inverse diagonal of the block-Jacobi preconditioner is a table of 16 x (p+1)^2 values (one set per combination of
// Dirichlet faces).  No atomics; every entry has one writer: the same bits in every run.  (Action kRestrict adds the
// residual into an FE_Q vector, where cells share entries: its launches cover cells that share none, one after the other.)
#include "mgx_dg_device.hpp"

namespace
{
  using namespace mgx::dg;
  using namespace mgx::dg::device;

  // compiled twice, as mgx_dg_kernels.hip is: MGX_DG_NEUMANN_UNIT = 1 holds the variant of the cell kernel for operators
  // with Neumann faces and its launch, nothing else
#ifndef MGX_DG_NEUMANN_UNIT
#define MGX_DG_NEUMANN_UNIT 0
#endif
  constexpr bool kNeumannUnit = MGX_DG_NEUMANN_UNIT != 0;

  template <int P, typename T>
  struct DGCfg2
  {
    static constexpr int N     = P + 1;
    static constexpr int NN    = N * N;
    static constexpr int PX    = (N % 2 == 0) ? N + 1 : N; // odd row pitch: conflict-free y-lines
    static constexpr int AREA  = N * PX;
    static constexpr int FS    = N;                        // one face array
    static constexpr int CELL0 = 2 * AREA + 6 * FS;
    // per-cell stride congruent to the threads per cell modulo the 32 banks: accesses "thread index + constant"
    // (y-lines, face points) of neighbouring cells in one half-wave fall on consecutive banks
    static constexpr int CELL  = CELL0 + (((N - CELL0) % 32) + 32) % 32;
    static constexpr int WG    = 256;
    static constexpr int CPW   = WG / N; // p = 1 ... 9: 128 85 64 51 42 36 32 28 25 cells, at most 58.2 KiB (p = 9, fp64)
    static constexpr int THREADS = WG;
    static_assert(CPW * CELL * (int)sizeof(T) <= 65536, "cells of a workgroup do not fit the LDS");
  };

  // block-Jacobi in the eigenvector basis on the x-lines held in registers:  r <- T D^-1 T^T r
  // (JacobiTransformed::do_local_operation, laplace_operator_dg.h:2086-2097; dim == 2: two directions).  U is scratch.
  template <int P, typename T>
  __device__ __forceinline__ void jacobi_local_2d(const DGConst<T> *__restrict__ c, const T *__restrict__ inv_diag, T *U, bool active,
                                                  int a, T (&r)[P + 1])
  {
    using C         = DGCfg2<P, T>;
    constexpr int N = C::N, PX = C::PX;
    T             q[N];
    if (active)
      {
        mul_E<N>(c, r, q); // out[e] = sum_i E[i][e] r[i]
        st_line<N>(U, a * PX, 1, q);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, a, PX, r);
        mul_E<N>(c, r, q);
#pragma unroll
        for (int k = 0; k < N; ++k)
          q[k] *= inv_diag[k * N + a];
        mul_Et<N>(c, q, r); // out[i] = sum_e E[i][e] q[e]
        st_line<N>(U, a, PX, r);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, a * PX, 1, q);
        mul_Et<N>(c, q, r);
      }
  }

  // One direction of the transposed embedding of FE_Q(p) in the DG space (laplace_operator_dg.h:1803,
  // local_basis_transformer->apply<true>): out[m] = sum_i P1[i][m] in[i], summed in the order of the stand-alone transfer
  // (dg_cg_transfer_kernel_2d).  An unrolled product keeps all of P1 in scalar registers, 2 n^2 of them in double: more
  // than a wave has from p = 8 on (profiles/feq_2d_code_static.txt).  Those instantiations (rolled_P1) take the line from
  // LDS value by value in a loop that is not unrolled, with one row of P1 in scalar registers at a time.
  template <int P, typename T>
  constexpr bool rolled_P1()
  {
    return sizeof(T) == 8 && P >= 8;
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_P1t(const T *__restrict__ P1, const T (&in)[N], T (&out)[N])
  {
#pragma unroll
    for (int m = 0; m < N; ++m)
      {
        T s = P1[m] * in[0];
#pragma unroll
        for (int i = 1; i < N; ++i)
          s = fma(P1[i * N + m], in[i], s);
        out[m] = s;
      }
  }
  template <int N, typename T>
  __device__ __forceinline__ void mul_P1t_rolled(const T *__restrict__ P1, const T *line, int stride, T (&out)[N])
  {
#pragma unroll
    for (int m = 0; m < N; ++m)
      out[m] = T(0);
#pragma unroll 1
    for (int i = 0; i < N; ++i)
      {
        const T x = line[i * stride];
#pragma unroll
        for (int m = 0; m < N; ++m)
          out[m] = fma(P1[i * N + m], x, out[m]);
      }
  }

  // r[0 .. p] of the y-line i of an FE_Q cell added into the vector through the cell's nine entries ix of the compressed
  // index table (first DoF of every vertex / line / quad entity, [3 cy + cx]; constrained: 0xFFFFFFFF).  Plain
  // read-modify-writes: the cells of a launch share no FE_Q DoF.  For one j the lanes of a cell touch consecutive DoFs of
  // the quad interior and of the bottom and top lines.  p = 1: the entries of the entities without DoFs are not read.
  template <int P, typename T>
  __device__ __forceinline__ void add_fe_q_column_2d(T *__restrict__ dst, const uint32_t *__restrict__ ix, int i, const T (&r)[P + 1])
  {
    const int      cx = i == 0 ? 0 : (i == P ? 2 : 1);
    const uint32_t ox = cx == 1 ? (uint32_t)(i - 1) : 0u;
    const uint32_t b0 = ix[cx], b2 = ix[6 + cx];
    if (b0 != 0xFFFFFFFFu)
      dst[b0 + ox] += r[0];
    if constexpr (P > 1)
      {
        const uint32_t b1 = ix[3 + cx];
        if (b1 != 0xFFFFFFFFu)
          {
#pragma unroll
            for (int j = 1; j < P; ++j)
              dst[b1 + (cx == 1 ? (uint32_t)((j - 1) * (P - 1)) + ox : (uint32_t)(j - 1))] += r[j];
          }
      }
    if (b2 != 0xFFFFFFFFu)
      dst[b2 + ox] += r[P];
  }

  // NEUMANN: as in the 3D kernel -- a negative neighbour entry is MGX_DG_BOUNDARY or MGX_DG_NEUMANN, the inverse diagonals
  // are indexed by the kinds of the four faces in base 3
  template <int P, typename T, int TYPE, int ACTION, bool NEUMANN>
  __global__ void __launch_bounds__((DGCfg2<P, T>::THREADS)) dg_cell_kernel_2d(const DGArgs<T> A)
  {
    using C         = DGCfg2<P, T>;
    constexpr int N = C::N, NN = C::NN, PX = C::PX, AREA = C::AREA, FS = C::FS;
    __shared__ __attribute__((aligned(16))) T lds[C::CPW * C::CELL];

    const DGConst<T> *__restrict__ c = A.c;
    const int  tid    = threadIdx.x;
    const int  cw     = tid / N;
    const int  a      = tid - cw * N; // owner of the x-line j = a, the y-line i = a and the face points a
    const bool active = cw < C::CPW;
    // XCD-aware block order (see the 3D kernel): every XCD takes one contiguous eighth of the cells
    const uint32_t xq = gridDim.x / 8, xr = gridDim.x % 8, xcd = blockIdx.x % 8;
    const uint32_t bid = xcd * xq + (xcd < xr ? xcd : xr) + blockIdx.x / 8;
    uint32_t   cell   = bid * C::CPW + (active ? cw : 0);
    const bool store  = active && cell < A.n_cells;
    if (cell >= A.n_cells)
      cell = A.n_cells - 1;
    cell = A.cell_list ? A.cell_list[cell] : cell * A.cell_stride + A.cell_first;

    T *U  = lds + (active ? cw : 0) * C::CELL;
    T *GY = U + AREA;
    T *F  = U + 2 * AREA; // face scratch of the direction in work: [2 faces][3][FS]

    const T *__restrict__ src = A.src;
    const size_t cbase = (size_t)cell * NN;
    const size_t lbase = cbase + a * N;
    T            xs[N]; // the source x-line: needed again by the Chebyshev update
    int          nb[4];
    unsigned     cat = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f)
      {
        nb[f] = A.neigh[(size_t)cell * 4 + f];
        if constexpr (!NEUMANN)
          cat |= (nb[f] < 0 ? 1u : 0u) << f;
      }
    if constexpr (NEUMANN)
      cat = face_kind_code<4>(nb);

    if constexpr (ACTION == kJacobi)
      {
        T r[N];
        if (active)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              r[i] = src[lbase + i];
          }
        jacobi_local_2d<P, T>(c, A.inv_diag + (size_t)cat * NN, U, active, a, r);
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              A.dst[lbase + i] = A.f2 * r[i];
          }
        return;
      }

    // own traces (value, reference normal derivative) of the 4 faces at this thread's face point, and what the faces
    // give back to the integration (value / normal-derivative test function)
    T To[4], No[4], Vf[4], Wf[4];

    // ---- 1. source x-line -> Gauss values along x
    if (active)
      {
        T u[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
          xs[i] = src[lbase + i];
        if constexpr (TYPE != MGX_DG_GAUSS)
          mul_St<N>(c, xs, u);
        else
          copy_line<N>(xs, u);
        st_line<N>(U, a * PX, 1, u);
      }
    __syncthreads();

    // ---- 2. y-lines: Gauss values along y, y-derivative, traces on the y faces
    if (active)
      {
        T u[N], v[N];
        ld_line<N>(U, a, PX, u);
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            mul_St<N>(c, u, v);
            st_line<N>(U, a, PX, v);
          }
        else
          copy_line<N>(u, v);
        mul_Dt<N>(c, v, u);
        st_line<N>(GY, a, PX, u);
        To[2] = dot_line<N>(c->b[0], v);
        To[3] = dot_line<N>(c->b[1], v);
        No[2] = dot_line<N>(c->g[0], v);
        No[3] = dot_line<N>(c->g[1], v);
      }
    __syncthreads();

    // ---- 3. x-lines: traces on the x faces
    if (active)
      {
        T u[N];
        ld_line<N>(U, a * PX, 1, u);
        To[0] = dot_line<N>(c->b[0], u);
        To[1] = dot_line<N>(c->b[1], u);
        No[0] = dot_line<N>(c->g[0], u);
        No[1] = dot_line<N>(c->g[1], u);
      }

    // ---- 4. faces, one direction at a time (two faces): per face three arrays of p+1 words -- neighbour trace, then
    // sum of the traces | neighbour normal derivative, then weighted jump | tangential part of the result.  A
    // Dirichlet face mirrors the own values (:1568-1577).
#pragma unroll
    for (int d = 0; d < 2; ++d)
      {
        const int sd = d == 0 ? 1 : N; // stride of the normal direction in a cell
        const int s1 = d == 0 ? N : 1; // ... of the tangential one
        const int t1 = 1 - d;
        auto      E0 = [&](int s) { return F + (3 * s) * FS; };
        auto      E1 = [&](int s) { return F + (3 * s + 1) * FS; };
        auto      AT = [&](int s) { return F + (3 * s + 2) * FS; };
        if (active)
          {
#pragma unroll
            for (int s = 0; s < 2; ++s)
              {
                const int f  = 2 * d + s;
                T         ev = 0, ed = 0;
                if (nb[f] >= 0)
                  {
                    const T *__restrict__ xn = src + (size_t)nb[f] * NN + a * s1;
                    if constexpr (TYPE == MGX_DG_HERMITE)
                      {
                        // the neighbour's two nodes next to the face (its upper face for our lower one and vice versa)
                        const int l0 = s == 0 ? N - 1 : 0, l1 = s == 0 ? (N > 1 ? N - 2 : 0) : (N > 1 ? 1 : 0);
                        const T   v0 = xn[l0 * sd], v1 = xn[l1 * sd];
                        ev           = v0;
                        ed           = s == 0 ? c->hderiv * (v1 - v0) : c->hderiv * (v0 - v1);
                      }
                    else
                      {
                        T line[N];
#pragma unroll
                        for (int i = 0; i < N; ++i)
                          line[i] = xn[i * sd];
                        ev = dot_line<N>(c->fb[1 - s], line);
                        ed = dot_line<N>(c->fg[1 - s], line);
                      }
                  }
                E0(s)[a] = ev;
                E1(s)[a] = ed;
              }
          }
        __syncthreads();
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            // neighbour traces: change to the Gauss points along the face, four lines per cell
            if (active)
              for (int L = a; L < 4; L += N)
                {
                  T  u[N], v[N];
                  T *arr = F + (L / 2 * 3 + L % 2) * FS;
                  ld_line<N>(arr, 0, 1, u);
                  mul_St<N>(c, u, v);
                  st_line<N>(arr, 0, 1, v);
                }
            __syncthreads();
          }
        // in the quadrature point: sum of the traces -> E0, weighted jump -> E1; sum of the normal derivatives and the
        // weighted jump stay in registers
        T sN[2], wJ[2];
        if (active)
          {
            const T wq = c->w[a] * c->fw[d];
#pragma unroll
            for (int s = 0; s < 2; ++s)
              {
                const int  f = 2 * d + s;
                // NEUMANN: te = -To, ne = -No and no jump: the face gives nothing to the form (see the 3D kernel)
                const bool dirichlet = NEUMANN ? nb[f] == MGX_DG_BOUNDARY : nb[f] < 0;
                const bool neumann   = NEUMANN && nb[f] == MGX_DG_NEUMANN;
                const T    te = dirichlet ? To[f] : (neumann ? -To[f] : E0(s)[a]);
                const T    ne = dirichlet ? No[f] : (neumann ? -No[f] : E1(s)[a]);
                sN[s]         = No[f] + ne;
                wJ[s]         = wq * (dirichlet ? T(2) * To[f] : To[f] - te);
                if (neumann)
                  wJ[s] = T(0);
                E0(s)[a]      = To[f] + te;
                E1(s)[a]      = wJ[s];
              }
          }
        __syncthreads();
        // tangential part of the normal derivative, one line product along each face (s = +-1 its side):
        //   AT = -s/2 c_t (w d_t sumT + d_t^T wj)
        if (active)
          for (int s = a; s < 2; s += N)
            {
              const T half_s = s ? T(0.5) : T(-0.5);
              const T ct     = c->cn[d][t1];
              T       st[N], wj[N], ds[N], dj[N];
              ld_line<N>(E0(s), 0, 1, st);
              ld_line<N>(E1(s), 0, 1, wj);
              mul_Dt<N>(c, st, ds);
              mul_D<N>(c, wj, dj);
#pragma unroll
              for (int i = 0; i < N; ++i)
                ds[i] = -half_s * ct * (c->w[i] * c->fw[d] * ds[i] + dj[i]);
              st_line<N>(AT(s), 0, 1, ds);
            }
        __syncthreads();
        // value test function  V = sigma wj - s/2 w c_n sumN + tangential part,
        // normal derivative test function  W = -s/2 c_n wj
        if (active)
          {
            const T wq = c->w[a] * c->fw[d];
#pragma unroll
            for (int s = 0; s < 2; ++s)
              {
                const int f      = 2 * d + s;
                const T   half_s = s ? T(0.5) : T(-0.5);
                Vf[f] = c->sigma[d] * wJ[s] - half_s * wq * c->cn[d][d] * sN[s] + AT(s)[a];
                Wf[f] = -half_s * c->cn[d][d] * wJ[s];
              }
          }
        __syncthreads(); // the face scratch is reused by the next direction
      }

    // face contributions to a line's integration
    auto add_faces = [&](int d, T(&o)[N]) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        o[i] += c->b[0][i] * Vf[2 * d] + c->b[1][i] * Vf[2 * d + 1] + c->g[0][i] * Wf[2 * d] + c->g[1][i] * Wf[2 * d + 1];
    };

    // ---- 5. x-lines: gradient, coefficient (laplace_operator_dg.h:1700-1716), integration along x
    if (active)
      {
        T u[N], gx[N], gy[N], o[N];
        ld_line<N>(U, a * PX, 1, u);
        mul_Dt<N>(c, u, gx);
        ld_line<N>(GY, a * PX, 1, gy);
#pragma unroll
        for (int i = 0; i < N; ++i)
          {
            const T wq = c->w[a] * c->w[i];
            const T fx = wq * (c->K[0] * gx[i] + c->K[2] * gy[i]);
            const T fy = wq * (c->K[2] * gx[i] + c->K[1] * gy[i]);
            gx[i]      = fx;
            gy[i]      = fy;
          }
        st_line<N>(GY, a * PX, 1, gy);
        mul_D<N>(c, gx, o);
        add_faces(0, o);
        st_line<N>(U, a * PX, 1, o);
      }
    __syncthreads();
    // ---- 6. y-lines, then back to the element basis along y
    if (active)
      {
        T fy[N], o[N], u[N];
        ld_line<N>(GY, a, PX, fy);
        ld_line<N>(U, a, PX, u);
        mul_D<N>(c, fy, o);
        add_faces(1, o);
#pragma unroll
        for (int i = 0; i < N; ++i)
          o[i] += u[i];
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            mul_S<N>(c, o, u);
            st_line<N>(U, a, PX, u);
          }
        else
          st_line<N>(U, a, PX, o);
      }
    __syncthreads();
    // ---- 7. x-lines: result in the element basis, epilogue of the action
    T y[N];
    if (active)
      {
        T u[N];
        ld_line<N>(U, a * PX, 1, u);
        if constexpr (TYPE != MGX_DG_GAUSS)
          mul_S<N>(c, u, y);
        else
          copy_line<N>(u, y);
      }
    if constexpr (ACTION == kVmult)
      {
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              A.dst[lbase + i] = y[i];
          }
      }
    else if constexpr (ACTION == kResidual)
      {
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              A.dst[lbase + i] = A.rhs[lbase + i] - y[i];
          }
      }
    else if constexpr (ACTION == kRestrict)
      {
        // laplace_operator_dg.h:1798-1819: the residual, taken to the FE_Q basis of the cell by P1^T along x (this
        // thread's x-line) and along y (its y-line), added into A.cg through the 9-entry table A.idx27.  The x-line goes
        // back to the row of U this thread has just read and nobody else has: no barrier in front of the store.
        constexpr bool ROLLED = rolled_P1<P, T>();
        T              q[N];
        if (active)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              y[i] = A.rhs[lbase + i] - y[i];
            if constexpr (ROLLED)
              {
                st_line<N>(U, a * PX, 1, y);
                mul_P1t_rolled<N, T>(A.P1, U + a * PX, 1, q);
              }
            else
              mul_P1t<N, T>(A.P1, y, q);
            st_line<N>(U, a * PX, 1, q);
          }
        __syncthreads();
        if (active)
          {
            if constexpr (ROLLED)
              mul_P1t_rolled<N, T>(A.P1, U + a, PX, q);
            else
              {
                ld_line<N>(U, a, PX, y);
                mul_P1t<N, T>(A.P1, y, q);
              }
          }
        if (store)
          add_fe_q_column_2d<P, T>(A.cg, A.idx27 + 9u * (size_t)cell, a, q);
      }
    else if constexpr (ACTION == kPcgSums)
      {
        // the product stored and the four sums of the merged CG iteration, weighted by the inverse lumped mass m of the
        // DoF's local index (A.inv_diag carries the table here; solver_dg/program.cc:134-148):
        // dst.src, rhs.(m rhs), dst.(m rhs), dst.(m dst) over the cells of the launch
        double sum[4] = {0., 0., 0., 0.};
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              {
                const T m = A.inv_diag[a * N + i], r = A.rhs[lbase + i];
                A.dst[lbase + i] = y[i];
                pcg_sums_add(sum, y[i], xs[i], r, m);
              }
          }
        __syncthreads(); // the x-lines above were read from U
        block_sum4_cells<C::THREADS>(sum, reinterpret_cast<double *>(lds), tid, A.partials);
      }
    else
      {
        // laplace_operator_dg.h:1839-1860
        if (active)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              y[i] = A.rhs[lbase + i] - y[i];
          }
        jacobi_local_2d<P, T>(c, A.inv_diag + (size_t)cat * NN, U, active, a, y);
        if (store)
          {
            const T f1p = T(1) + A.f1;
            if (A.iteration_index == 1)
              {
#pragma unroll
                for (int i = 0; i < N; ++i)
                  A.dst[lbase + i] = A.f2 * y[i] + f1p * xs[i];
              }
            else
              {
#pragma unroll
                for (int i = 0; i < N; ++i)
                  A.dst[lbase + i] = A.f2 * y[i] + f1p * xs[i] - A.f1 * A.dst[lbase + i];
              }
          }
      }
  }

  template <int P, int TYPE, int ACTION, typename T>
  void launch_one_2d(hipStream_t s, const DGArgs<T> &a)
  {
    using C = DGCfg2<P, T>;
    hipLaunchKernelGGL((dg_cell_kernel_2d<P, T, TYPE, ACTION, kNeumannUnit>), dim3(cell_groups<C>(a.n_cells)), dim3(C::THREADS), 0, s, a);
  }
} // namespace

namespace mgx::dg
{
#if MGX_DG_NEUMANN_UNIT
  bool launch_dg_cells_2d_neumann(hipStream_t s, const CellOperands &op, const DGLaunch &l)
  {
    return dispatch_cells<kVmult, kChebyshev, kResidual, kJacobi, kPcgSums>(
      op, l, [&](auto P, auto TYPE, auto ACTION, const auto &a) { launch_one_2d<P.value, TYPE.value, ACTION.value>(s, a); });
  }
#else
  // kRestrict in this unit only: the solver on the FE_Q hierarchy refuses operators with Neumann faces
  bool launch_dg_cells_2d(hipStream_t s, const CellOperands &op, const DGLaunch &l)
  {
    return dispatch_cells<kVmult, kRestrict, kChebyshev, kResidual, kJacobi, kPcgSums>(
      op, l, [&](auto P, auto TYPE, auto ACTION, const auto &a) { launch_one_2d<P.value, TYPE.value, ACTION.value>(s, a); });
  }

  uint32_t cell_grid_2d(int number, int p, uint32_t n_cells) { return cell_groups<DGCfg2>(number, p, n_cells); }
#endif
} // namespace mgx::dg
