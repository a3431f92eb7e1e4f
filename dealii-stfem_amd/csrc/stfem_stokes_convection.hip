// Stokes two-field operator: the convection term of the Navier-Stokes modes, for velocity degree DEG = 2 (FE_Q(2)^3, QGauss(3)) and
// DEG = 3 (FE_Q(3)^3, QGauss(4), reached through the _space entries of include/stfem_stokes_convection_space.h).  It replaces, of
//   StokesMatrixFreeOperator::do_cell_integral_local<OperatorMode::form / jacobian> (reference include/operators.h:1525-1575),
// what those modes add to OperatorMode::none: with the linearisation velocity b (velocity_lin, read from data_lin as
// read_dof_values reads it) and the source velocity u at the operator's own (DEG + 1)^3 Gauss points
//   form     (1562-1567): grad_u -= outer_product(u, b)            -> out_u += - int (u (x) b) : grad v
//   jacobian (1554-1561): grad_u -= b (x) u + u (x) b              -> out_u += - int (b (x) u + u (x) b) : grad v
// and of the weak (Nitsche) boundary faces (1738-1743), in both modes: nitsche_u_1 -= min(b.n, 0) u.  Outflow faces add nothing (bfp
// carries a factor 0.0, dn the outflow penalty, which this library does not hold); a degree-3 context has no weak faces.  Pressure
// rows and constrained velocity rows receive nothing.
// The launches follow those of the linear operator of the same set (stokes_launch): every destination they touch has been written,
// so they read, add and write - eight colour launches each (cells of one colour share no DoF), ascending, no atomics, no zeroing, a
// fixed summation order, bitwise reproducible.  A variable-coefficient term has no Kronecker form: the same kernels serve boxes (CART)
// and general meshes.
#include "stfem_stokes_internal.h"

namespace {

// The layout of stokes_cell_kernel (stfem_stokes_cell.hip): lane t = a + (DEG + 1) b + (DEG + 1)^2 c of a cell is its velocity node and
// its Gauss point (a, b, c) - degree 2: one half-wave per cell, 27 active lanes, 256 threads = 8 cells at a time; degree 3: one wave
// per cell, 4 cells at a time -, persistent workgroups that walk runs of cells as the cell kernel's do (prm.interleave at degree 2),
// the next cell's DoFs (6 doubles per lane and source: u and b) fetched while this one is computed, two wave-private LDS regions per
// cell handed between the sum-factorised 1D stages and ordered with wave_fence(): no workgroup barrier inside the cell loop.
//   evaluate  (values only, six fields u_0..2, b_0..2): lane (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point
//   integrate (gradients only, nine fields F[i][e]):    lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node
// The rows of the lane's quadrature index (evaluation) are held in registers, the columns of its node index (integration) as the cell
// kernel has them (COLUMNS_HELD: in registers at degree 2, read from LDS where they are used at degree 3).
// CART: constant diagonal Jacobian (the context was created without vertices); otherwise MappingQ1 from the eight cell vertices.
// MULTI: every source s has its own b_s; the weighted results are summed in registers per destination (up to MAXSRC), one scatter;
// otherwise one source, the weights applied at scatter time to up to MAXOUT destinations.
// JACOBIAN: the flux of the jacobian mode, otherwise that of the form mode.
template <int DEG, bool CART, bool MULTI, bool JACOBIAN>
__global__ __launch_bounds__(256) void stokes_convection_kernel(const ConvectionParamsT<DEG> prm)
{
  constexpr int N1 = DEG + 1, N2 = N1 * N1, NN = N1 * N2; // nodes = quadrature points per direction, per cell: 27 or 64
  constexpr int LANES = NN <= 32 ? 32 : 64, CELLS = 256 / LANES;
  constexpr int R = 9 * NN; // doubles per cell of each region (largest stage: 9 arrays of NN)
  // the 1D tables [q*N1+a] behind the regions, in the same array (profiles/stokes_cell_merge.txt)
  __shared__ double smem[CELLS * 2 * R + 2 * N2];
  double *const tS = smem + CELLS * 2 * R, *const tD = tS + N2;
  if (threadIdx.x < N2) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x / LANES, tl = threadIdx.x % LANES;
  const bool lane_on = NN == LANES || tl < NN;
  const int t = lane_on ? tl : 0;
  const int a = t % N1, b = (t / N1) % N1, c = t / N2;
  double *X = smem + slot * (2 * R), *Y = X + R;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  const Coef<N1, 1, true> Sa(tS + N1 * a), Sb(tS + N1 * b), Sc(tS + N1 * c);
  const Coef<N1, N1, COLUMNS_HELD<DEG>> SaT(tS + a), DaT(tD + a), SbT(tS + b), DbT(tD + b), ScT(tS + c), DcT(tD + c);
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  // the walk over the cells of the colour: as in stokes_cell_kernel
  const long long nslot = (long long)gridDim.x * CELLS, run = (ncells + nslot - 1) / nslot;
  const long long wg_first = (long long)blockIdx.x * CELLS * run, wg_end = wg_first + CELLS * run;
  const bool interleave = DEG == 2 && prm.interleave;
  const int STRIDE = interleave ? CELLS : 1;
  const long long first = interleave ? wg_first + slot : ((long long)blockIdx.x * CELLS + slot) * run;
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && (interleave ? cell < wg_end : cell < first + run);
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = DEG * q.cx + a, iy = DEG * q.cy + b, iz = DEG * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    return q;
  };
  double un[3] = {0, 0, 0}, bn[3] = {0, 0, 0};
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained entries of u and of b read as 0
    const double *us = prm.us[MULTI ? s : 0], *bs = prm.bs[MULTI ? s : 0];
    if (q.ok && lane_on && !q.con) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) { un[comp] = us[comp * prm.Nu + q.gu]; bn[comp] = bs[comp * prm.Nu + q.gu]; }
    } else {
      un[0] = un[1] = un[2] = bn[0] = bn[1] = bn[2] = 0.0;
    }
  };
  CellIds nxt = ids(first);
  fetch(nxt, 0);
  double accU[MULTI ? MAXSRC : 1][3]; // several sources: the sums over them, per destination
#pragma unroll
  for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = 0.0;
  for (long long it2 = 0; it2 < run * nsrc; ++it2) {
    const long long it = it2 / nsrc;
    const int src = int(it2 - it * nsrc);
    const CellIds cur = nxt;
    const int cx = cur.cx, cy = cur.cy, cz = cur.cz;
    const bool con = cur.con;
    const long long gu = cur.gu;
    const bool active = cur.ok && lane_on;

    // ---- gather: X = u[3][NN], b[3][NN]
    if (lane_on) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) { X[comp * NN + t] = un[comp]; X[(3 + comp) * NN + t] = bn[comp]; }
    }
    nxt = ids(first + STRIDE * ((it2 + 1) / nsrc));
    fetch(nxt, int((it2 + 1) % nsrc));
    wave_fence();
    // ---- evaluate, x: (n_x, n_y, n_z) -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int f = 0; f < 6; ++f) Y[f * NN + t] = dot<N1>(Sa, X + f * NN + N1 * b + N2 * c);
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z) -> X
#pragma unroll
    for (int f = 0; f < 6; ++f) X[f * NN + t] = dot<N1>(Sb, Y + f * NN + a + N2 * c, N1);
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): values in registers
    double val[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) val[f] = dot<N1>(Sc, X + f * NN + a + N1 * b, N2);

    // ---- quadrature-point operation (operators.h:1554-1567): F[i][j] = - u_i b_j (- b_i u_j), pulled back -> Y[(i*3+e)*NN + t]
    if (CART) {
      const double JxW = prm.detJ * wabc;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          double F = val[i] * val[3 + e];
          if (JACOBIAN) F = fma(val[3 + i], val[e], F);
          Y[(i * 3 + e) * NN + t] = -F * JxW * prm.hinv[e];
        }
    } else {
      const double xi[3] = {prm.xq[a], prm.xq[b], prm.xq[c]};
      double Ji[3][3];
      const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji); // (at this lane's point)
      const double JxW = det * wabc;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double F[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          double f = val[i] * val[3 + d];
          if (JACOBIAN) f = fma(val[3 + i], val[d], f);
          F[d] = -f * JxW;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) Y[(i * 3 + e) * NN + t] = Ji[e][0] * F[0] + Ji[e][1] * F[1] + Ji[e][2] * F[2];
      }
    }
    wave_fence();
    // ---- integrate, z: quadrature point -> (q_x, q_y, n_z) -> X (the z derivative on the field e = 2)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *f0 = Y + (i * 3) * NN + a + N1 * b;
      X[(i * 3) * NN + t] = dot<N1>(ScT, f0, N2);
      X[(i * 3 + 1) * NN + t] = dot<N1>(ScT, f0 + NN, N2);
      X[(i * 3 + 2) * NN + t] = dot<N1>(DcT, f0 + 2 * NN, N2);
    }
    wave_fence();
    // ---- y: -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *g0 = X + (i * 3) * NN + a + N2 * c;
      Y[(i * 2) * NN + t] = dot<N1>(SbT, g0, N1);
      Y[(i * 2 + 1) * NN + t] = dot<N1>(DbT, g0 + NN, N1) + dot<N1>(SbT, g0 + 2 * NN, N1);
    }
    wave_fence();
    // ---- x: -> node (a, b, c)
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *h0 = Y + (i * 2) * NN + N1 * b + N2 * c;
      r[i] = dot<N1>(DaT, h0) + dot<N1>(SaT, h0 + NN);
    }

    // ---- distribute_local_to_global (add): constrained velocity rows receive nothing
    if constexpr (MULTI) {
#pragma unroll
      for (int o = 0; o < MAXSRC; ++o)
        if (o < prm.nout) {
          const double kU = prm.wKu[src][o];
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(kU, r[comp], accU[o][comp]);
        }
    }
    if (active && !con && src == nsrc - 1) {
      // (the sums are registers: their loop is unrolled and guarded; the launcher keeps nout within the instantiation's bound)
      constexpr int NO_UNROLL = MULTI ? MAXSRC : 1;
      const int no = MULTI ? MAXSRC : prm.nout;
#pragma unroll NO_UNROLL
      for (int o = 0; o < no; ++o) {
        if (MULTI && o >= prm.nout) continue;
        double *d = prm.out_u[o] + gu;
        double v[3];
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) v[comp] = d[comp * prm.Nu];
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) {
          if constexpr (MULTI) d[comp * prm.Nu] = v[comp] + accU[o][comp];
          else d[comp * prm.Nu] = v[comp] + prm.wKu[0][o] * r[comp];
        }
      }
    }
    if (MULTI && src == nsrc - 1) {
#pragma unroll
      for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = 0.0;
    }
    wave_fence(); // the next cell's gather overwrites X
  }
}

// The inflow term of the weak faces (degree 2), in the layout of stokes_boundary_kernel (stfem_stokes_boundary.hip): one half-wave per
// boundary CELL, handled by its lowest weak face for all of them; the nine lanes of a face's quadrature points evaluate u and b there and
// F = - min(b.n, 0) u JxW (operators.h:1738-1743, submitted as a value), the 27 node lanes integrate.  prm.weak_mask holds the weak
// faces that are not outflow faces.
template <bool MULTI>
__global__ __launch_bounds__(256) void stokes_inflow_kernel(const ConvectionParams prm)
{
  __shared__ double tS[9], tE[6], tX[3], tW[3];
  __shared__ double sX[8][162], sF[8][9][3];
  if (threadIdx.x < 9) tS[threadIdx.x] = prm.Su[threadIdx.x];
  if (threadIdx.x < 6) tE[threadIdx.x] = prm.Eu[threadIdx.x];
  if (threadIdx.x < 3) { tX[threadIdx.x] = prm.xq[threadIdx.x]; tW[threadIdx.x] = prm.wq[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  const int nc[3] = {prm.ncx, prm.ncy, prm.ncz};
  double *X = sX[slot];
  for (long long item = (long long)blockIdx.x * 8 + slot; item - slot < prm.foff[6]; item += (long long)gridDim.x * 8) {
    bool ok = item < prm.foff[6];
    int f0 = 0;
    for (int f = 0; f < 6; ++f)
      if (ok && item >= prm.foff[f] && item < prm.foff[f + 1]) f0 = f;
    int cc[3];
    { // (selects, no arrays indexed at run time: those would live in scratch)
      const int d = f0 >> 1, s = f0 & 1, t1 = d == 0 ? 1 : 0;
      const long long e = ok ? item - prm.foff[f0] : 0;
      const int nd = d == 0 ? nc[0] : (d == 1 ? nc[1] : nc[2]), n1 = d == 0 ? nc[1] : nc[0];
      const int e1 = int(e % n1), e2 = int(e / n1);
#pragma unroll
      for (int k = 0; k < 3; ++k) cc[k] = k == d ? (s ? nd - 1 : 0) : (k == t1 ? e1 : e2);
    }
    const int cx = cc[0], cy = cc[1], cz = cc[2];
    ok = ok && ((cx & 1) + 2 * (cy & 1) + 4 * (cz & 1)) == prm.colour;
    int faces = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const int d = f >> 1, s = f & 1;
      if ((prm.weak_mask >> f & 1) && cc[d] == (s ? nc[d] - 1 : 0)) faces |= 1 << f;
    }
    ok = ok && (faces & ((1 << f0) - 1)) == 0;
    if (!__builtin_amdgcn_readfirstlane(__ballot(ok) != 0)) continue; // (wave-uniform skip only: the two half-waves fence together)
    const int ix = 2 * cx + a, iy = 2 * cy + b, iz = 2 * cz + c;
    const bool con = constrained_u(prm, ix, iy, iz);
    const long long gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    double accU[MULTI ? MAXSRC : 1][3];
#pragma unroll
    for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = 0.0;
    const int nsrc = MULTI ? prm.nsrc : 1;
    for (int src = 0; src < nsrc; ++src) {
      { // gather (read_dof_values: constrained entries read as 0)
        const double *us = prm.us[src], *bs = prm.bs[src];
        if (lane27)
          for (int comp = 0; comp < 3; ++comp) {
            X[comp * 27 + t] = (ok && !con) ? us[comp * prm.Nu + gu] : 0.0;
            X[(3 + comp) * 27 + t] = (ok && !con) ? bs[comp * prm.Nu + gu] : 0.0;
          }
      }
      wave_fence();
      double rU[3] = {0, 0, 0};
      for (int f = 0; f < 6; ++f) {
        if (!__builtin_amdgcn_readfirstlane(__ballot(ok && (faces >> f & 1)) != 0)) continue;
        const bool on = ok && (faces >> f & 1); // per half-wave
        const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0;
        const int q1 = t32 % 3, q2 = (t32 / 3) % 3;
        // value of node n along direction dir at face point (qa, qb)
        auto tv = [&](int dir, int qa, int qb, int n) { return dir == d ? tE[s * 3 + n] : tS[(dir == t1 ? qa : qb) * 3 + n]; };
        if (on && t32 < 9) { // this lane's face point
          double xi[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) xi[k] = k == d ? double(s) : tX[k == t1 ? q1 : q2];
          double Ji[3][3];
          const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
          // (not mapping_q1_face_normal: m stays un-normalised and b . m is divided by |m| once, other roundings than b . (m / |m|))
          double m[3], len = 0.0;
          for (int k = 0; k < 3; ++k) {
            m[k] = (s ? 1.0 : -1.0) * (d == 0 ? Ji[0][k] : (d == 1 ? Ji[1][k] : Ji[2][k]));
            len += m[k] * m[k];
          }
          len = sqrt(len);
          const double JxW = fabs(det) * len * tW[q1] * tW[q2];
          double uval[3] = {0, 0, 0}, bval[3] = {0, 0, 0};
          for (int kc = 0; kc < 3; ++kc)
            for (int kb = 0; kb < 3; ++kb)
              for (int ka = 0; ka < 3; ++ka) {
                const double w = tv(0, q1, q2, ka) * tv(1, q1, q2, kb) * tv(2, q1, q2, kc);
                for (int comp = 0; comp < 3; ++comp) {
                  uval[comp] += w * X[comp * 27 + ka + 3 * kb + 9 * kc];
                  bval[comp] += w * X[(3 + comp) * 27 + ka + 3 * kb + 9 * kc];
                }
              }
          const double bnrm = (bval[0] * m[0] + bval[1] * m[1] + bval[2] * m[2]) / len;
          const double inflow = fmin(bnrm, 0.0);
          for (int comp = 0; comp < 3; ++comp) sF[slot][t32][comp] = -inflow * uval[comp] * JxW;
        }
        wave_fence();
        if (on && lane27) { // integrate: test values of node (a, b, c)
          for (int q = 0; q < 9; ++q) {
            const int qa = q % 3, qb = q / 3;
            const double v = tv(0, qa, qb, a) * tv(1, qa, qb, b) * tv(2, qa, qb, c);
            for (int comp = 0; comp < 3; ++comp) rU[comp] += v * sF[slot][q][comp];
          }
        }
        wave_fence(); // the next face reuses the point buffer
      }
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
            for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(prm.wKu[src][o], rU[comp], accU[o][comp]);
          }
      } else {
        for (int comp = 0; comp < 3; ++comp) accU[0][comp] = rU[comp];
      }
      wave_fence(); // the next source overwrites X
    }
    // distribute_local_to_global (add): constrained velocity rows are not written
    if (ok && lane27 && !con) {
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
            double *dptr = prm.out_u[o] + gu;
            for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += accU[o][comp];
          }
      } else {
        for (int o = 0; o < prm.nout; ++o) {
          double *dptr = prm.out_u[o] + gu;
          for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += prm.wKu[0][o] * accU[0][comp];
        }
      }
    }
  }
}

template <int DEG> const void *convection_kernel(int which) // which = 4 JACOBIAN + 2 MULTI + CART
{
  const void *const kerns[8] = {
    (const void *)stokes_convection_kernel<DEG, false, false, false>, (const void *)stokes_convection_kernel<DEG, true, false, false>,
    (const void *)stokes_convection_kernel<DEG, false, true, false>,  (const void *)stokes_convection_kernel<DEG, true, true, false>,
    (const void *)stokes_convection_kernel<DEG, false, false, true>,  (const void *)stokes_convection_kernel<DEG, true, false, true>,
    (const void *)stokes_convection_kernel<DEG, false, true, true>,   (const void *)stokes_convection_kernel<DEG, true, true, true>};
  return kerns[which];
}

// The kernel argument at degree DEG: with the inflow fields at degree 2
template <int DEG> using Convection = std::conditional_t<DEG == 2, ConvectionParams, ConvectionParamsT<DEG>>;

// The launches of `set` at degree DEG: geometry and tables from the context's description of that degree, sources and weights from
// `set`, lin[s] beside source s.  The destinations that receive the term are those with a non-zero weight of the K part.
template <int DEG> int convection_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *lin, int mode, hipStream_t st)
{
  const StokesParamsT<DEG> &g = c->desc<DEG>();
  Convection<DEG> k;
  k.vertices = g.vertices;
  k.ncx = g.ncx; k.ncy = g.ncy; k.ncz = g.ncz;
  for (int d = 0; d < 3; ++d) { k.ndu[d] = g.ndu[d]; k.hinv[d] = g.hinv[d]; }
  k.Nu = g.Nu;
  k.dmask = g.dmask;
  for (int i = 0; i < (DEG + 1) * (DEG + 1); ++i) { k.Su[i] = g.Su[i]; k.Du[i] = g.Du[i]; }
  for (int i = 0; i < DEG + 1; ++i) { k.xq[i] = g.xq[i]; k.wq[i] = g.wq[i]; }
  k.interleave = g.interleave; k.colour = 0; k.cart = g.cart;
  k.detJ = g.detJ;
  k.nsrc = set.nsrc;
  for (int s = 0; s < MAXSRC; ++s) {
    k.us[s] = s < set.nsrc ? set.us[s] : nullptr;
    k.bs[s] = s < set.nsrc ? lin[s] : nullptr;
    if (s < set.nsrc && !lin[s]) return STFEM_ERR_INVALID_ARGUMENT;
  }
  k.nout = stokes_k_destinations(set, k.out_u, k.wKu);
  if (k.nout == 0) return STFEM_OK;
  if constexpr (DEG == 2) { // the inflow term on the weak faces
    k.weak_mask = c->bnd.weak_mask;
    for (int f = 0; f < 7; ++f) k.foff[f] = c->bnd.foff[f];
    for (int i = 0; i < 6; ++i) k.Eu[i] = c->bnd.Eu[i];
  }
  void *args[] = {&k};

  const bool multi = set.nsrc > 1, jac = mode == STFEM_CONVECTION_JACOBIAN;
  const int which = (jac ? 4 : 0) + (multi ? 2 : 0) + (k.cart ? 1 : 0);
  const void *kern = convection_kernel<DEG>(which);
  static int resident_of[8] = {};
  const int resident = stokes_resident(resident_of[which], kern);
  stfem_launch_begin();
  stokes_colour_launches(c, DEG == 3 ? 4 : 8, resident, c->convection_plan, [&](int colour, unsigned grid) {
    k.colour = colour;
    (void)hipLaunchKernel(kern, dim3(grid), dim3(256), args, 0, st);
    c->convection_launched = true; // (stfem_stokes_last_convection_plan)
  });
  if constexpr (DEG == 2) {
    const long long items = k.weak_mask ? k.foff[6] : 0;
    if (items > 0) {
      const unsigned grid = (unsigned)std::min<long long>((items + 7) / 8, 4ll * c->n_cu);
      for (int colour = 0; colour < 8; ++colour) {
        k.colour = colour;
        if (multi) hipLaunchKernelGGL(stokes_inflow_kernel<true>, dim3(grid), dim3(256), 0, st, k);
        else hipLaunchKernelGGL(stokes_inflow_kernel<false>, dim3(grid), dim3(256), 0, st, k);
      }
    }
  }
  return stfem_launch_end("stokes_convection_kernel");
}

} // namespace

int stokes_convection_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *lin, int mode, hipStream_t st)
{
  if (mode != STFEM_CONVECTION_FORM && mode != STFEM_CONVECTION_JACOBIAN) return STFEM_ERR_INVALID_ARGUMENT;
  if (set.nsrc < 1 || set.nsrc > MAXSRC || set.nout > (set.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiations' bounds)
  return stokes_with_degree(c, [&](auto deg) { return convection_launch<deg()>(c, set, lin, mode, st); });
}
