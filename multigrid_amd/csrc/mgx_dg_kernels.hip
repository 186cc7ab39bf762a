// mgx_dg_kernels.hip -- device code of the DG (symmetric interior penalty) Laplace operator on an affine mesh with the
// merged Chebyshev update: the gfx950 cell kernel with its line products, its constant block and its launch, and the
// small kernels of the ghost exchange and of the smoother's start vector.  What the host code (mgx_dg_api.cpp) sees of
// it is the DG section of mgx_internal.hpp; the data format of the device (DGConst, DGArgs), the launch side
// (dispatch_cells, cell_groups), the line products and the block sums are mgx_dg_device.hpp, which the cell kernel of
// two dimensions (mgx_dg_kernels_2d.hip) shares.  launch_dg_cells and cell_grid here hand dim == 2 to that unit.
//
// Reference behaviour (not code): common/laplace_operator_dg.h -- LaplaceOperatorCompactCombine
// :350-2024 (cell-based loop operation_on_cells :1110-1861), JacobiTransformed :2028-2256,
// LocalBasisTransformer :92-350; 1D line kernel with face values common/matrix_vector_kernel.h
// :30-216.  The bilinear form is the one of common/laplace_operator_dg_face.h:66-160.
//
// Design (MI355X): a workgroup of 128 threads takes CPW = 128 / (p+1)^2 consecutive cells; the
// (p+1)^2 threads of a cell each own one line of the cell per sweep direction (registers) and one
// quadrature point of each of the 6 faces.  Per cell the LDS holds the values U in the Gauss
// points, two gradient components, and four (p+1)^2 arrays per face (own trace, own normal
// derivative, neighbour trace, neighbour normal derivative), which the face phase turns in place
// into the two arrays the integration needs.  The traces of a line's two end faces fall out of
// the sweep that has the line in registers (the `do_dg` idea of matrix_vector_kernel.h:114-141).
// Neighbour data is read straight from the source vector: two node layers per face for the
// Hermite-like basis (laplace_operator_dg.h:1359-1457), a contracted full cell otherwise.  The
// inverse diagonal of the block-Jacobi preconditioner depends only on which faces of a cell are
// Dirichlet faces: a table of at most 64 x (p+1)^3 values replaces the reference's per-cell
// stream, so the fused Chebyshev step moves 4 vector accesses per DoF (source, right-hand side,
// old iterate, new iterate) where the reference's model counts 5 (matvec_dg_cheby/program.cc:178).
#include "mgx_dg_device.hpp"

#include <cstring>

namespace
{
  using namespace mgx::dg;
  using namespace mgx::dg::device; // DGConst, DGArgs and the line products, shared with the 2D kernel
  using mgx::kMaxN;

  // This file is compiled twice (Makefile).  The second unit, MGX_DG_NEUMANN_UNIT = 1, holds the variant of the cell
  // kernel for operators with Neumann faces (neighbour entry MGX_DG_NEUMANN) and nothing else; operators without such
  // faces run the kernels of the first unit, whose code the variant does not touch.
#ifndef MGX_DG_NEUMANN_UNIT
#define MGX_DG_NEUMANN_UNIT 0
#endif
  constexpr bool kNeumannUnit = MGX_DG_NEUMANN_UNIT != 0;

  template <int P, typename T>
  struct DGCfg
  {
    static constexpr int N    = P + 1;
    static constexpr int NN2  = N * N;
    static constexpr int N3   = N * N * N;
    static constexpr int PX   = (N % 2 == 0) ? N + 1 : N; // odd row pitch: conflict-free x-lines
    static constexpr int VOL  = N * N * PX;
    static constexpr int FS   = N * PX;
    // per-cell LDS stride: congruent to the threads per cell modulo the 32 banks (of 4 B for fp32,
    // of 8 B for fp64 accesses), so that accesses of the form "thread index + constant" (z-lines,
    // face points) of neighbouring cells in one half-wave fall on consecutive banks
    static constexpr int CELL0 = 3 * VOL + 6 * FS;
    static constexpr int CELLP = CELL0 + (((NN2 - CELL0) % 32) + 32) % 32;
#ifndef MGX_DG_WG_THREADS
#define MGX_DG_WG_THREADS 128 // measured: 128-thread workgroups 4-11 % faster than 256 (barriers span two waves)
#endif
    // fp32, higher degrees: the size that fills its lanes best (p = 8: one cell = 81 of 128 lanes, three
    // cells = 243 of 256).  Measured on the merged Chebyshev step against 128 threads: p = 5 192 threads +3 %
    // (256: -4 %), p = 6 256 threads +7 % (192: -7 %), p = 8 256 threads +13 % (192: +9 %), p = 9 256: -11 %.
    static constexpr int WG    = sizeof(T) != 4 ? MGX_DG_WG_THREADS : (P == 5 ? 192 : (P == 6 || P == 8 ? 256 : MGX_DG_WG_THREADS));
    static constexpr int CPW_T = (WG / NN2) > 0 ? WG / NN2 : 1;
    static constexpr int CPW_L = 65536 / (CELLP * (int)sizeof(T));
    static constexpr int CPW   = CPW_T < CPW_L ? CPW_T : CPW_L;
    // ... unless the padding costs a workgroup per CU (p = 3: 13 instead of 14; measured +4.7 % without it,
    // while p = 4 and 5, where the count stays, are 1 % faster with it)
    static constexpr int CELL = (163840 / (CPW * CELL0 * (int)sizeof(T)) > 163840 / (CPW * CELLP * (int)sizeof(T))) ? CELL0 : CELLP;
    static constexpr int THREADS = ((CPW * NN2 + 63) / 64) * 64;
    // Waves per SIMD the register allocation is asked to allow (fp32; the fp64 kernels are bound by their
    // LDS at 3 waves).  One more than the compiler takes by itself where the LDS admits it and the cut is
    // below ~10 registers -- measured on the merged Chebyshev step: p = 4 76 -> 72 VGPRs, 6 -> 7 waves,
    // +3...7 % (8 waves = 64 VGPRs spill: -10 %); p = 5 89 -> 80, 5 -> 6 waves, +8...11 %; p = 6 +1...2 %;
    // p = 8 112 -> 96, 4 -> 5 waves, +7...8 %.
    static constexpr int MINW = sizeof(T) != 4 ? 1 : (P == 4 ? 7 : (P == 5 || P == 6 ? 6 : (P == 8 ? 5 : 1)));
    static_assert(CPW >= 1, "cell does not fit the LDS");
  };


  // block-Jacobi in the eigenvector basis on the x-lines held in registers:  r <- T D^-1 T^T r
  // (JacobiTransformed::do_local_operation, laplace_operator_dg.h:2086-2097).  U is scratch.
  template <int P, typename T>
  __device__ __forceinline__ void jacobi_local(const DGConst<T> *__restrict__ c, const T *__restrict__ inv_diag, T *U,
                                               bool active, int a, int b, T (&r)[P + 1])
  {
    using C         = DGCfg<P, T>;
    constexpr int N = C::N, PX = C::PX;
    T             q[N];
    if (active)
      {
        mul_E<N>(c, r, q); // out[e] = sum_i E[i][e] r[i]
        st_line<N>(U, (b * N + a) * PX, 1, q);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, b * N * PX + a, PX, r);
        mul_E<N>(c, r, q);
        st_line<N>(U, b * N * PX + a, PX, q);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, b * PX + a, N * PX, r);
        mul_E<N>(c, r, q);
#pragma unroll
        for (int k = 0; k < N; ++k)
          q[k] *= inv_diag[(k * N + b) * N + a];
        mul_Et<N>(c, q, r); // out[i] = sum_e E[i][e] q[e]
        st_line<N>(U, b * PX + a, N * PX, r);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, b * N * PX + a, PX, q);
        mul_Et<N>(c, q, r);
        st_line<N>(U, b * N * PX + a, PX, r);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, (b * N + a) * PX, 1, q);
        mul_Et<N>(c, q, r);
      }
  }

  // residual x-lines in registers -> coefficients of the FE_Q basis of the cell: r <- (P1 x P1 x P1)^T r
  // (the transposed embedding, laplace_operator_dg.h:1803 local_basis_transformer->apply<true>).  U is scratch.
  template <int P, typename T>
  __device__ __forceinline__ void to_fe_q_local(const T *__restrict__ P1, T *U, bool active, int a, int b, T (&r)[P + 1])
  {
    using C         = DGCfg<P, T>;
    constexpr int N = C::N, PX = C::PX;
    T             q[N];
    auto mulT = [&](const T(&in)[N], T(&out)[N]) { // out[m] = sum_i P1[i][m] in[i]
#pragma unroll
      for (int m = 0; m < N; ++m)
        {
          T s = P1[m] * in[0];
#pragma unroll
          for (int i = 1; i < N; ++i)
            s = fma(P1[i * N + m], in[i], s);
          out[m] = s;
        }
    };
    if (active)
      {
        mulT(r, q);
        st_line<N>(U, (b * N + a) * PX, 1, q);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, b * N * PX + a, PX, r);
        mulT(r, q);
        st_line<N>(U, b * N * PX + a, PX, q);
      }
    __syncthreads();
    if (active)
      {
        ld_line<N>(U, b * PX + a, N * PX, r);
        mulT(r, q);
        st_line<N>(U, b * PX + a, N * PX, q);
      }
    __syncthreads();
    if (active)
      ld_line<N>(U, (b * N + a) * PX, 1, r);
  }

  // r[0 .. p] of the x-line (j, k) of an FE_Q cell added into the vector through the compressed index table
  // (27 entities per cell: first DoF of every vertex / line / quad / hex entity, vector_access_reduced.h:153-247)
  template <int P, typename T>
  __device__ __forceinline__ void add_fe_q_line(T *__restrict__ dst, const uint32_t *__restrict__ idx27, uint32_t cell, int j,
                                                int k, const T (&r)[P + 1], bool plain)
  {
    const int       cy = j == 0 ? 0 : (j == P ? 2 : 1), cz = k == 0 ? 0 : (k == P ? 2 : 1);
    const int       oy = cy == 1 ? j - 1 : 0, oz = cz == 1 ? k - 1 : 0;
    const uint32_t *ind = idx27 + 27u * (size_t)cell + 3 * (3 * cz + cy);
    const uint32_t  off = (uint32_t)((cy == 1 ? P - 1 : 1) * oz + oy);
    const uint32_t  b0 = ind[0], b1 = ind[1], b2 = ind[2];
    auto add = [&](uint32_t at, T v) {
      if (plain)
        dst[at] += v;
      else
        unsafeAtomicAdd(&dst[at], v);
    };
    if (b0 != 0xFFFFFFFFu)
      add(b0 + off, r[0]);
    if (b1 != 0xFFFFFFFFu)
      {
#pragma unroll
        for (int i = 0; i < P - 1; ++i)
          add(b1 + off * (uint32_t)(P - 1) + (uint32_t)i, r[1 + i]);
      }
    if (b2 != 0xFFFFFFFFu)
      add(b2 + off, r[P]);
  }

  // GHOSTS (Hermite-like basis on a decomposed mesh): neighbour entries >= A.n_owned are ghost faces
  // NEUMANN: a negative neighbour entry is MGX_DG_BOUNDARY or MGX_DG_NEUMANN, and the inverse diagonals are indexed by
  // the kinds of the six faces in base 3 (face_kind_code); without it every negative entry is a Dirichlet face
  template <int P, typename T, int TYPE, int ACTION, bool GHOSTS, bool NEUMANN>
  __global__ void __launch_bounds__((DGCfg<P, T>::THREADS), (DGCfg<P, T>::MINW)) dg_cell_kernel(const DGArgs<T> A)
  {
    using C         = DGCfg<P, T>;
    constexpr int N = C::N, NN2 = C::NN2, N3 = C::N3, PX = C::PX, VOL = C::VOL, FS = C::FS;
    __shared__ __attribute__((aligned(16))) T lds[C::CPW * C::CELL];
#ifdef MGX_DG_LDS_PAD // occupancy experiment (tools/experiments): extra LDS per workgroup, in bytes
    __shared__ char lds_pad[MGX_DG_LDS_PAD];
    if (A.n_cells == 0xFFFFFFFFu) // never true; keeps the array allocated
      {
        lds_pad[threadIdx.x] = 1;
        __syncthreads();
        A.dst[0] = (T)lds_pad[(threadIdx.x + 1) % MGX_DG_LDS_PAD];
      }
#endif

    const DGConst<T> *__restrict__ c = A.c;
    const int  tid    = threadIdx.x;
    const int  cw     = tid / NN2;
    const int  t      = tid - cw * NN2;
    const int  a      = t % N, b = t / N; // line owner (a, b) = face point (a, b)
    const bool active = cw < C::CPW;
    // XCD-aware block order: the dispatcher deals workgroups round-robin over the 8 XCDs (each with its
    // own L2); give every XCD one contiguous eighth of the cells, which lie along a space-filling curve,
    // so that most face neighbours are read through the L2 that holds them (measured: vmult +1...4 %,
    // the VALU-bound merged Chebyshev step +0.3 %)
    const uint32_t xq = gridDim.x / 8, xr = gridDim.x % 8, xcd = blockIdx.x % 8;
    const uint32_t bid = xcd * xq + (xcd < xr ? xcd : xr) + blockIdx.x / 8;
    uint32_t   cell   = bid * C::CPW + (active ? cw : 0);
    const bool store  = active && cell < A.n_cells;
    if (cell >= A.n_cells)
      cell = A.n_cells - 1;
    cell = A.cell_list ? A.cell_list[cell] : cell * A.cell_stride + A.cell_first;

    T *U  = lds + (active ? cw : 0) * C::CELL;
    T *GY = U + VOL, *GZ = U + 2 * VOL;
    T *F  = U + 3 * VOL; // face scratch of the direction in work: [2 faces][3][FS]
    const int fidx = b * PX + a;

    const T *__restrict__ src = A.src;
    const size_t cbase = (size_t)cell * N3;
    T            xs[N]; // the source x-line: needed again by the Chebyshev update
    int          nb[6];
    unsigned     cat = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f)
      {
        nb[f] = A.neigh[(size_t)cell * 6 + f];
        if constexpr (!NEUMANN)
          cat |= (nb[f] < 0 ? 1u : 0u) << f;
      }
    if constexpr (NEUMANN)
      cat = face_kind_code<6>(nb);

    if constexpr (ACTION == kJacobi)
      {
        T r[N];
        if (active)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              r[i] = src[cbase + (b * N + a) * N + i];
          }
        jacobi_local<P, T>(c, A.inv_diag + (size_t)cat * N3, U, active, a, b, r);
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              A.dst[cbase + (b * N + a) * N + i] = A.f2 * r[i];
          }
        return;
      }

    // own traces (value, reference normal derivative) of the 6 faces at this thread's face point,
    // and what the faces give back to the integration (value / normal-derivative test function):
    // registers -- the line owner (a, b) of a sweep direction is the owner of face point (a, b)
    T To[6], No[6], Vf[6], Wf[6];

    // ---- 1. source x-line -> Gauss values along x
    if (active)
      {
        T u[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
          xs[i] = src[cbase + (b * N + a) * N + i];
        if constexpr (TYPE != MGX_DG_GAUSS)
          mul_St<N>(c, xs, u);
        else
          copy_line<N>(xs, u);
        st_line<N>(U, (b * N + a) * PX, 1, u);
      }
    __syncthreads();

    // ---- 2. Gauss values along y
    if constexpr (TYPE != MGX_DG_GAUSS)
      {
        if (active)
          {
            T u[N], v[N];
            ld_line<N>(U, b * N * PX + a, PX, u);
            mul_St<N>(c, u, v);
            st_line<N>(U, b * N * PX + a, PX, v);
          }
        __syncthreads();
      }

    // ---- 3. z-lines: Gauss values along z, z-derivative, traces on the z faces
    if (active)
      {
        T u[N], v[N];
        ld_line<N>(U, b * PX + a, N * PX, u);
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            mul_St<N>(c, u, v);
            st_line<N>(U, b * PX + a, N * PX, v);
          }
        else
          copy_line<N>(u, v);
        mul_Dt<N>(c, v, u);
        st_line<N>(GZ, b * PX + a, N * PX, u);
        To[4] = dot_line<N>(c->b[0], v);
        To[5] = dot_line<N>(c->b[1], v);
        No[4] = dot_line<N>(c->g[0], v);
        No[5] = dot_line<N>(c->g[1], v);
      }
    __syncthreads();

    // ---- 4. y-lines: y-derivative and traces on the y faces; x-lines: traces on the x faces
    if (active)
      {
        T u[N], v[N];
        ld_line<N>(U, b * N * PX + a, PX, u);
        mul_Dt<N>(c, u, v);
        st_line<N>(GY, b * N * PX + a, PX, v);
        To[2] = dot_line<N>(c->b[0], u);
        To[3] = dot_line<N>(c->b[1], u);
        No[2] = dot_line<N>(c->g[0], u);
        No[3] = dot_line<N>(c->g[1], u);
        ld_line<N>(U, (b * N + a) * PX, 1, u);
        To[0] = dot_line<N>(c->b[0], u);
        To[1] = dot_line<N>(c->b[1], u);
        No[0] = dot_line<N>(c->g[0], u);
        No[1] = dot_line<N>(c->g[1], u);
      }

    // ---- 5. faces, one direction at a time (two faces): per face three arrays of (p+1)^2 words --
    // neighbour trace, then sum of the traces | neighbour normal derivative, then weighted jump |
    // tangential part of the result.  A Dirichlet face mirrors the own values (:1568-1577).
#pragma unroll
    for (int d = 0; d < 3; ++d)
      {
        const int sd = d == 0 ? 1 : (d == 1 ? N : N * N); // stride of the normal direction in a cell
        const int s1 = d == 0 ? N : 1;                    // ... of the two tangential ones (ascending)
        const int s2 = d == 2 ? N : N * N;
        const int t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
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
                    const T *__restrict__ xn = src + (size_t)nb[f] * N3 + a * s1 + b * s2;
                    if constexpr (TYPE == MGX_DG_HERMITE)
                      {
                        // owned neighbour: its two node layers next to the face (its upper face for our
                        // lower one and vice versa); ghost: the (value, normal derivative) pair of the
                        // face point as its owner computed it (k_pack_faces; laplace_operator_dg.h:1015-1039
                        // sends the same pair).  Two loads either way, no divergent branch.
                        const int l0 = s == 0 ? N - 1 : 0, l1 = s == 0 ? (N > 1 ? N - 2 : 0) : (N > 1 ? 1 : 0);
                        if constexpr (GHOSTS)
                          {
                            // 32-bit entry offsets (a vector holds fewer than 2^32 entries): one select
                            const uint32_t nbu   = (uint32_t)nb[f];
                            const bool     ghost = nbu >= A.n_owned;
                            const uint32_t base  = ghost ? A.n_owned * (uint32_t)N3 + ((nbu - A.n_owned) * NN2 + b * N + a) * 2
                                                         : nbu * (uint32_t)N3 + a * s1 + b * s2;
                            const T v0 = src[base + (ghost ? 0 : l0 * sd)], v1 = src[base + (ghost ? 1 : l1 * sd)];
                            ev         = v0;
                            ed         = ghost ? v1 : (s == 0 ? c->hderiv * (v1 - v0) : c->hderiv * (v0 - v1));
                          }
                        else
                          {
                            const T v0 = xn[l0 * sd], v1 = xn[l1 * sd];
                            ev         = v0;
                            ed         = s == 0 ? c->hderiv * (v1 - v0) : c->hderiv * (v0 - v1);
                          }
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
                E0(s)[fidx] = ev;
                E1(s)[fidx] = ed;
              }
          }
        __syncthreads();
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            // neighbour traces: in-face change to the Gauss points, first then second direction
            if (active)
              for (int L = t; L < 4 * N; L += NN2)
                {
                  T  u[N], v[N];
                  T *arr = F + ((L / N) / 2 * 3 + (L / N) % 2) * FS + (L % N) * PX;
                  ld_line<N>(arr, 0, 1, u);
                  mul_St<N>(c, u, v);
                  st_line<N>(arr, 0, 1, v);
                }
            __syncthreads();
            if (active)
              for (int L = t; L < 4 * N; L += NN2)
                {
                  T  u[N], v[N];
                  T *arr = F + ((L / N) / 2 * 3 + (L / N) % 2) * FS + (L % N);
                  ld_line<N>(arr, 0, PX, u);
                  mul_St<N>(c, u, v);
                  st_line<N>(arr, 0, PX, v);
                }
            __syncthreads();
          }
        // in the quadrature point: sum of the traces -> E0, weighted jump -> E1; sum of the normal
        // derivatives and the weighted jump stay in registers
        T sN[2], wJ[2];
        if (active)
          {
            const T wq = c->w[a] * c->w[b] * c->fw[d];
#pragma unroll
            for (int s = 0; s < 2; ++s)
              {
                const int  f = 2 * d + s;
                // NEUMANN: te = -To, ne = -No and no jump -- sum of the traces, sum of the normal derivatives and the
                // weighted jump are exact zeros and the face gives nothing to the form, on sheared cells too (mirroring
                // the value alone would leave the tangential part of the mean normal derivative).  Written as selects.
                const bool dirichlet = NEUMANN ? nb[f] == MGX_DG_BOUNDARY : nb[f] < 0;
                const bool neumann   = NEUMANN && nb[f] == MGX_DG_NEUMANN;
                const T    te = dirichlet ? To[f] : (neumann ? -To[f] : E0(s)[fidx]);
                const T    ne = dirichlet ? No[f] : (neumann ? -No[f] : E1(s)[fidx]);
                sN[s]         = No[f] + ne;
                wJ[s]         = wq * (dirichlet ? T(2) * To[f] : To[f] - te);
                if (neumann)
                  wJ[s] = T(0);
                E0(s)[fidx]   = To[f] + te;
                E1(s)[fidx]   = wJ[s];
              }
          }
        __syncthreads();
        // tangential part, lines of the first tangential direction (s = +-1 the side of the face):
        //   AT = -s/2 c_t1 (w d_t1 sumT + d_t1^T wj)
        if (active)
          for (int L = t; L < 2 * N; L += NN2)
            {
              const int s = L / N, l = L % N;
              const T   half_s = s ? T(0.5) : T(-0.5);
              const T   ct = c->cn[d][t1];
              T         st[N], wj[N], ds[N], dj[N];
              ld_line<N>(E0(s), l * PX, 1, st);
              ld_line<N>(E1(s), l * PX, 1, wj);
              mul_Dt<N>(c, st, ds);
              mul_D<N>(c, wj, dj);
              const T wl = c->w[l] * c->fw[d];
#pragma unroll
              for (int i = 0; i < N; ++i)
                ds[i] = -half_s * ct * (c->w[i] * wl * ds[i] + dj[i]);
              st_line<N>(AT(s), l * PX, 1, ds);
            }
        __syncthreads();
        if (active)
          for (int L = t; L < 2 * N; L += NN2)
            {
              const int s = L / N, l = L % N;
              const T   half_s = s ? T(0.5) : T(-0.5);
              const T   ct = c->cn[d][t2];
              T         st[N], wj[N], v[N], ds[N], dj[N];
              ld_line<N>(E0(s), l, PX, st);
              ld_line<N>(E1(s), l, PX, wj);
              ld_line<N>(AT(s), l, PX, v);
              mul_Dt<N>(c, st, ds);
              mul_D<N>(c, wj, dj);
              const T wl = c->w[l] * c->fw[d];
#pragma unroll
              for (int i = 0; i < N; ++i)
                v[i] -= half_s * ct * (c->w[i] * wl * ds[i] + dj[i]);
              st_line<N>(AT(s), l, PX, v);
            }
        __syncthreads();
        // value test function  V = sigma wj - s/2 w c_n sumN + tangential part,
        // normal derivative test function  W = -s/2 c_n wj
        if (active)
          {
            const T wq = c->w[a] * c->w[b] * c->fw[d];
#pragma unroll
            for (int s = 0; s < 2; ++s)
              {
                const int f      = 2 * d + s;
                const T   half_s = s ? T(0.5) : T(-0.5);
                Vf[f] = c->sigma[d] * wJ[s] - half_s * wq * c->cn[d][d] * sN[s] + AT(s)[fidx];
                Wf[f] = -half_s * c->cn[d][d] * wJ[s];
              }
          }
      }

    // face contributions to a line's integration
    auto add_faces = [&](int d, T(&o)[N]) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        o[i] += c->b[0][i] * Vf[2 * d] + c->b[1][i] * Vf[2 * d + 1] + c->g[0][i] * Wf[2 * d] + c->g[1][i] * Wf[2 * d + 1];
    };
    __syncthreads(); // GY complete; the face scratch is not touched below

    // ---- 6. x-lines: gradient, coefficient (laplace_operator_dg.h:1700-1716), integration along x
    if (active)
      {
        T u[N], gx[N], gy[N], gz[N], o[N];
        ld_line<N>(U, (b * N + a) * PX, 1, u);
        mul_Dt<N>(c, u, gx);
        ld_line<N>(GY, (b * N + a) * PX, 1, gy);
        ld_line<N>(GZ, (b * N + a) * PX, 1, gz);
        const T wab = c->w[a] * c->w[b];
#pragma unroll
        for (int i = 0; i < N; ++i)
          {
            const T wq = wab * c->w[i];
            const T fx = wq * (c->K[0] * gx[i] + c->K[3] * gy[i] + c->K[4] * gz[i]);
            const T fy = wq * (c->K[3] * gx[i] + c->K[1] * gy[i] + c->K[5] * gz[i]);
            const T fz = wq * (c->K[4] * gx[i] + c->K[5] * gy[i] + c->K[2] * gz[i]);
            gx[i]      = fx;
            gy[i]      = fy;
            gz[i]      = fz;
          }
        st_line<N>(GY, (b * N + a) * PX, 1, gy);
        st_line<N>(GZ, (b * N + a) * PX, 1, gz);
        mul_D<N>(c, gx, o);
        add_faces(0, o);
        st_line<N>(U, (b * N + a) * PX, 1, o);
      }
    __syncthreads();
    // ---- 7. y-lines
    if (active)
      {
        T fy[N], o[N], u[N];
        ld_line<N>(GY, b * N * PX + a, PX, fy);
        ld_line<N>(U, b * N * PX + a, PX, u);
        mul_D<N>(c, fy, o);
        add_faces(1, o);
#pragma unroll
        for (int i = 0; i < N; ++i)
          o[i] += u[i];
        st_line<N>(U, b * N * PX + a, PX, o);
      }
    __syncthreads();
    // ---- 8. z-lines, then back to the element basis along z
    if (active)
      {
        T fz[N], o[N], u[N];
        ld_line<N>(GZ, b * PX + a, N * PX, fz);
        ld_line<N>(U, b * PX + a, N * PX, u);
        mul_D<N>(c, fz, o);
        add_faces(2, o);
#pragma unroll
        for (int i = 0; i < N; ++i)
          o[i] += u[i];
        if constexpr (TYPE != MGX_DG_GAUSS)
          {
            mul_S<N>(c, o, u);
            st_line<N>(U, b * PX + a, N * PX, u);
          }
        else
          st_line<N>(U, b * PX + a, N * PX, o);
      }
    __syncthreads();
    if constexpr (TYPE != MGX_DG_GAUSS)
      {
        if (active)
          {
            T u[N], v[N];
            ld_line<N>(U, b * N * PX + a, PX, u);
            mul_S<N>(c, u, v);
            st_line<N>(U, b * N * PX + a, PX, v);
          }
        __syncthreads();
      }
    // ---- 10. x-lines: result in the element basis, epilogue of the action
    T y[N];
    if (active)
      {
        T u[N];
        ld_line<N>(U, (b * N + a) * PX, 1, u);
        if constexpr (TYPE != MGX_DG_GAUSS)
          mul_S<N>(c, u, y);
        else
          copy_line<N>(u, y);
      }
    const size_t lbase = cbase + (b * N + a) * N;
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
        // laplace_operator_dg.h:1798-1819
        if (active)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              y[i] = A.rhs[lbase + i] - y[i];
          }
        __syncthreads(); // the x-lines above were read from U
        to_fe_q_local<P, T>(A.P1, U, active, a, b, y);
        if (store)
          add_fe_q_line<P, T>(A.cg, A.idx27, cell, a, b, y, A.plain != 0);
      }
    else if constexpr (ACTION == kCgSums)
      {
        // laplace_operator_dg.h:1827-1838: dst.src, rhs.rhs, dst.rhs, dst.dst over the cells of the launch.  The reduction is
        // block_sum4_cells written out: calling it makes the compiler fuse the other product of rhs.rhs in fp64 from p = 4 on
        // (the last bit of that sum)
        double sum[4] = {0., 0., 0., 0.};
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              {
                const T r        = A.rhs[lbase + i];
                A.dst[lbase + i] = y[i];
                sum[0] += (double)(y[i] * xs[i]);
                sum[1] += (double)(r * r);
                sum[2] += (double)(y[i] * r);
                sum[3] += (double)(y[i] * y[i]);
              }
          }
        constexpr int WAVES = C::THREADS / 64;
        double       *red   = reinterpret_cast<double *>(lds);
        __syncthreads();
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
            A.partials[(size_t)blockIdx.x * 4 + tid] = t4;
          }
      }
    else if constexpr (ACTION == kPcgSums)
      {
        // kCgSums with the inverse lumped mass m of the DoF's local index (A.inv_diag carries the table here; the
        // preconditioner of solver_dg/program.cc:134-148): dst.src, rhs.(m rhs), dst.(m rhs), dst.(m dst)
        double sum[4] = {0., 0., 0., 0.};
        if (store)
          {
#pragma unroll
            for (int i = 0; i < N; ++i)
              {
                const T m = A.inv_diag[(b * N + a) * N + i], r = A.rhs[lbase + i];
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
        jacobi_local<P, T>(c, A.inv_diag + (size_t)cat * N3, U, active, a, b, y);
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


#if !MGX_DG_NEUMANN_UNIT
  template <typename T>
  void fill_const(const Host1D &h, const Geometry &g, DGConst<T> &c)
  {
    std::memset(&c, 0, sizeof(c));
    const int n = h.n;
    for (int i = 0; i < n * n; ++i)
      {
        c.S[i] = (T)h.S[i];
        c.D[i] = (T)h.D[i];
        c.E[i] = (T)h.E[i];
      }
    for (int r = 0; r < n; ++r)
      for (int q = 0; q < n; ++q)
        {
          c.St[r * n + q] = (T)h.S[q * n + r];
          c.Dt[r * n + q] = (T)h.D[q * n + r];
          c.Et[r * n + q] = (T)h.E[q * n + r];
        }
    // even-odd tables (the symmetry itself is checked when the operator is created)
    auto eo_fill = [&](EOLine<T> &e, auto M) { // M(q, i)
      const int H = n / 2;
      for (int q = 0; q < H; ++q)
        for (int i = 0; i < H; ++i)
          {
            e.eo[2 * (q * H + i)]     = (T)(0.5 * (M(q, i) + M(n - 1 - q, i)));
            e.eo[2 * (q * H + i) + 1] = (T)(0.5 * (M(q, i) - M(n - 1 - q, i)));
          }
      if (n % 2)
        {
          for (int i = 0; i < H; ++i)
            {
              e.mrow[i] = (T)M(H, i);
              e.mcol[i] = (T)M(i, H);
            }
          e.mm = (T)M(H, H);
        }
    };
    {
      const int H = n / 2, Ne = n - H, No = H;
      c.eo_e      = h.e_parity ? 1 : 0;
      for (int i = 0; i < H; ++i)
        {
          for (int k = 0; k < No; ++k)
            {
              c.epair[2 * (i * No + k)]     = (T)h.E[i * n + k];
              c.epair[2 * (i * No + k) + 1] = (T)h.E[i * n + Ne + k];
            }
          c.elast[i] = (T)h.E[i * n + Ne - 1];
        }
      for (int e = 0; e < Ne; ++e)
        c.emid[e] = (n % 2) ? (T)h.E[H * n + e] : (T)0;
    }
    eo_fill(c.eoS, [&](int q, int i) { return h.S[q * n + i]; });
    eo_fill(c.eoSt, [&](int q, int i) { return h.S[i * n + q]; });
    eo_fill(c.eoD, [&](int q, int i) { return h.D[q * n + i]; });
    eo_fill(c.eoDt, [&](int q, int i) { return h.D[i * n + q]; });
    for (int i = 0; i < n; ++i)
      {
        c.w[i] = (T)h.wq[i];
        for (int s = 0; s < 2; ++s)
          {
            c.b[s][i]  = (T)h.b[s][i];
            c.g[s][i]  = (T)h.g[s][i];
            c.fb[s][i] = (T)h.fb[s][i];
            c.fg[s][i] = (T)h.fg[s][i];
          }
      }
    for (int i = 0; i < 6; ++i) // (two dimensions: xx yy xy, the rest zero)
      c.K[i] = (T)g.K[i];
    for (int d = 0; d < 3; ++d)
      {
        for (int a = 0; a < 3; ++a)
          c.cn[d][a] = (T)g.cn[d][a];
        c.fw[d]    = (T)g.fw[d];
        c.sigma[d] = (T)g.sigma[d];
      }
    c.hderiv = (T)h.hderiv;
  }
#endif

  template <int P, int TYPE, int ACTION, typename T>
  void launch_one(hipStream_t s, const DGArgs<T> &a, bool ghosts)
  {
    using C             = DGCfg<P, T>;
    const uint32_t grid = cell_groups<C>(a.n_cells);
    if constexpr (TYPE == MGX_DG_HERMITE && ACTION != kJacobi)
      if (ghosts)
        {
          hipLaunchKernelGGL((dg_cell_kernel<P, T, TYPE, ACTION, true, kNeumannUnit>), dim3(grid), dim3(C::THREADS), 0, s, a);
          return;
        }
    hipLaunchKernelGGL((dg_cell_kernel<P, T, TYPE, ACTION, false, kNeumannUnit>), dim3(grid), dim3(C::THREADS), 0, s, a);
  }

#if !MGX_DG_NEUMANN_UNIT

  template <typename T>
  __global__ void __launch_bounds__(256)
    k_pack_cells(T *__restrict__ buf, const T *__restrict__ vec, const uint32_t *__restrict__ cells, uint32_t count,
                 uint32_t n3)
  {
    const uint64_t total = (uint64_t)count * n3;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
      {
        const uint32_t c = (uint32_t)(i / n3), k = (uint32_t)(i - (uint64_t)c * n3);
        buf[i] = vec[(uint64_t)cells[c] * n3 + k];
      }
  }

  // Hermite-like basis: what the neighbour needs of a cell is the value and the normal derivative
  // on the shared face, from the two node layers next to it (laplace_operator_dg.h:1015-1039)
  template <typename T>
  __global__ void __launch_bounds__(256)
    k_pack_faces(T *__restrict__ buf, const T *__restrict__ vec, const uint32_t *__restrict__ cells,
                 const uint8_t *__restrict__ faces, uint32_t count, int N, T hderiv)
  {
    const uint32_t nn2   = (uint32_t)(N * N);
    const uint64_t total = (uint64_t)count * nn2;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
      {
        const uint32_t c = (uint32_t)(i / nn2), j = (uint32_t)(i - (uint64_t)c * nn2);
        const int      a = (int)(j % N), b = (int)(j / N), f = faces[c], d = f / 2, upper = f % 2;
        const int      sd = d == 0 ? 1 : (d == 1 ? N : N * N), s1 = d == 0 ? N : 1, s2 = d == 2 ? N : N * N;
        const T *__restrict__ x = vec + (uint64_t)cells[c] * nn2 * N + a * s1 + b * s2;
        const T v0 = x[(upper ? N - 1 : 0) * sd];
        const T v1 = x[(upper ? (N > 1 ? N - 2 : 0) : (N > 1 ? 1 : 0)) * sd];
        buf[2 * i]     = v0;
        buf[2 * i + 1] = upper ? hderiv * (v1 - v0) : hderiv * (v0 - v1);
      }
  }

  template <typename T>
  __global__ void __launch_bounds__(256)
    k_start_vector(T *__restrict__ v, const uint32_t *__restrict__ cell_id, uint32_t n_cells, uint32_t n3, double mean)
  {
    const uint64_t total = (uint64_t)n_cells * n3;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
      {
        const uint32_t c = (uint32_t)(i / n3);
        const uint64_t g = (uint64_t)(cell_id ? cell_id[c] : c) * n3 + (i - (uint64_t)c * n3);
        v[i]             = (T)((double)(g % 11u) - mean);
      }
  }
#endif

} // namespace

#if MGX_DG_NEUMANN_UNIT
namespace mgx::dg
{
  // every action but kRestrict: the solver on the FE_Q hierarchy refuses operators with Neumann faces
  bool launch_dg_cells_neumann(hipStream_t s, const CellOperands &op, const DGLaunch &l)
  {
    return dispatch_cells<kVmult, kCgSums, kChebyshev, kResidual, kJacobi, kPcgSums>(
      op, l, [&](auto P, auto TYPE, auto ACTION, const auto &a) { launch_one<P.value, TYPE.value, ACTION.value>(s, a, op.has_ghosts); });
  }
} // namespace mgx::dg
#else
namespace mgx::dg
{
  int launch_dg_cells(hipStream_t s, const CellOperands &op, const DGLaunch &l)
  {
    if (l.n_cells == 0)
      return MGX_OK;
    const bool launched =
      op.has_neumann ? (op.dim == 2 ? launch_dg_cells_2d_neumann(s, op, l) : launch_dg_cells_neumann(s, op, l)) :
      op.dim == 2 ? launch_dg_cells_2d(s, op, l)
                  : dispatch_cells<kVmult, kRestrict, kCgSums, kChebyshev, kResidual, kJacobi, kPcgSums>(
                      op, l, [&](auto P, auto TYPE, auto ACTION, const auto &a) { launch_one<P.value, TYPE.value, ACTION.value>(s, a, op.has_ghosts); });
    if (!launched)
      return mgx::report_error(MGX_ERR_UNSUPPORTED, "DG cell kernel: no kernel for degree " + std::to_string(op.degree) + ", basis " +
                                                      std::to_string(op.basis) + ", action " + std::to_string(l.action));
    MGX_HIP(hipGetLastError());
    return MGX_OK;
  }

  uint32_t cell_grid(int number, int p, uint32_t n_cells, int dim)
  {
    return dim == 2 ? cell_grid_2d(number, p, n_cells) : cell_groups<DGCfg>(number, p, n_cells);
  }

  std::vector<char> const_block(int number, const Host1D &h, const Geometry &g)
  {
    std::vector<char> block;
    mgx::dispatch_number(number, [&](auto t) {
      block.resize(sizeof(DGConst<decltype(t)>));
      fill_const(h, g, *(DGConst<decltype(t)> *)block.data());
    });
    return block;
  }

  void launch_pack_cells(hipStream_t s, int number, void *buf, const void *vec, const uint32_t *cells, uint32_t count, uint32_t n3)
  {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)count * n3 + 255) / 256, 4096);
    mgx::dispatch_number(number, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_pack_cells<T>, dim3(grid), dim3(256), 0, s, (T *)buf, (const T *)vec, cells, count, n3);
    });
  }

  void launch_pack_faces(hipStream_t s, int number, void *buf, const void *vec, const uint32_t *cells, const uint8_t *faces,
                         uint32_t count, int N, double hderiv)
  {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)count * (uint32_t)(N * N) + 255) / 256, 4096);
    mgx::dispatch_number(number, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_pack_faces<T>, dim3(grid), dim3(256), 0, s, (T *)buf, (const T *)vec, cells, faces, count, N, (T)hderiv);
    });
  }

  void launch_start_vector(hipStream_t s, int number, void *v, const uint32_t *cell_id, uint32_t n_cells, uint32_t n3, double mean)
  {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_cells * n3 + 255) / 256, 8192);
    mgx::dispatch_number(number, [&](auto t) {
      hipLaunchKernelGGL(k_start_vector<decltype(t)>, dim3(grid), dim3(256), 0, s, (decltype(t) *)v, cell_id, n_cells, n3, mean);
    });
  }
} // namespace mgx::dg
#endif
