// Stokes two-field operator: the convection term of the Navier-Stokes modes.  It replaces, of
//   StokesMatrixFreeOperator::do_cell_integral_local<OperatorMode::form / jacobian> (reference include/operators.h:1525-1575),
// what those modes add to OperatorMode::none: with the linearisation velocity b (velocity_lin, read from data_lin as
// read_dof_values reads it) and the source velocity u at the operator's own 3 x 3 x 3 Gauss points
//   form     (1562-1567): grad_u -= outer_product(u, b)            -> out_u += - int (u (x) b) : grad v
//   jacobian (1554-1561): grad_u -= b (x) u + u (x) b              -> out_u += - int (b (x) u + u (x) b) : grad v
// and of the weak (Nitsche) boundary faces (1738-1743), in both modes: nitsche_u_1 -= min(b.n, 0) u.  Outflow faces add nothing (bfp
// carries a factor 0.0, dn the outflow penalty, which this library does not hold).  Pressure rows and constrained velocity rows
// receive nothing.
// The launches follow those of the linear operator of the same set (stokes_launch): every destination they touch has been written,
// so they read, add and write - eight colour launches each (cells of one colour share no DoF), ascending, no atomics, bitwise
// reproducible.  A variable-coefficient term has no Kronecker form: the same kernels serve boxes (CART) and general meshes.
#include "stfem_stokes_internal.h"

#include <algorithm>

namespace {

// The layout of stokes_cell_kernel (stfem_stokes_cell.hip): one half-wave per cell, 27 active lanes, 256 threads = 8 cells at a time,
// persistent workgroups, the next cell's DoFs fetched while this one is computed, two wave-private LDS regions per cell handed between
// the sum-factorised 1D stages.
//   evaluate  (values only, six fields u_0..2, b_0..2): lane (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point
//   integrate (gradients only, nine fields F[i][e]):    lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node
// CART: constant diagonal Jacobian.  MULTI: every source s has its own b_s; the weighted results are summed in registers per destination
// (up to MAXSRC), one scatter; otherwise one source, the weights applied at scatter time to up to MAXOUT destinations.
// JACOBIAN: the flux of the jacobian mode, otherwise that of the form mode.
template <bool CART, bool MULTI, bool JACOBIAN>
__global__ __launch_bounds__(256) void stokes_convection_kernel(const ConvectionParams prm)
{
  constexpr int RX = 243, RY = 243; // doubles per cell of the two regions (largest stage: 9 x 27)
  __shared__ double smem[8 * (RX + RY)];
  __shared__ double tS[9], tD[9]; // 1D tables [q*3+a]
  if (threadIdx.x < 9) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  double *X = smem + slot * (RX + RY), *Y = X + RX;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  double Sa[3], Sb[3], Sc[3], SaT[3], DaT[3], SbT[3], DbT[3], ScT[3], DcT[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    Sa[n] = tS[a * 3 + n]; Sb[n] = tS[b * 3 + n]; Sc[n] = tS[c * 3 + n];
    SaT[n] = tS[n * 3 + a]; DaT[n] = tD[n * 3 + a]; SbT[n] = tS[n * 3 + b]; DbT[n] = tD[n * 3 + b];
    ScT[n] = tS[n * 3 + c]; DcT[n] = tD[n * 3 + c];
  }
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  // the walk over the cells of the colour: as in stokes_cell_kernel
  const long long nhalf = (long long)gridDim.x * 8, run = (ncells + nhalf - 1) / nhalf;
  const long long wg_first = (long long)blockIdx.x * 8 * run, wg_end = wg_first + 8 * run;
  const int STRIDE = prm.interleave ? 8 : 1;
  const long long first = prm.interleave ? wg_first + slot : ((long long)blockIdx.x * 8 + slot) * run;
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && (prm.interleave ? cell < wg_end : cell < first + run);
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = 2 * q.cx + a, iy = 2 * q.cy + b, iz = 2 * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    return q;
  };
  double un[3] = {0, 0, 0}, bn[3] = {0, 0, 0};
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained entries of u and of b read as 0
    const double *us = prm.us[MULTI ? s : 0], *bs = prm.bs[MULTI ? s : 0];
    if (q.ok && lane27 && !q.con) {
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
    const bool active = cur.ok && lane27;

    // ---- gather: X = u[3][27], b[3][27]
    if (lane27) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) { X[comp * 27 + t] = un[comp]; X[(3 + comp) * 27 + t] = bn[comp]; }
    }
    nxt = ids(first + STRIDE * ((it2 + 1) / nsrc));
    fetch(nxt, int((it2 + 1) % nsrc));
    wave_fence();
    // ---- evaluate, x: (n_x, n_y, n_z) -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const double *u = X + f * 27 + 3 * b + 9 * c;
      Y[f * 27 + t] = fma(Sa[2], u[2], fma(Sa[1], u[1], Sa[0] * u[0]));
    }
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z) -> X
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const double *v = Y + f * 27 + a + 9 * c;
      X[f * 27 + t] = fma(Sb[2], v[6], fma(Sb[1], v[3], Sb[0] * v[0]));
    }
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): values in registers
    double val[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const double *v = X + f * 27 + a + 3 * b;
      val[f] = fma(Sc[2], v[18], fma(Sc[1], v[9], Sc[0] * v[0]));
    }

    // ---- quadrature-point operation (operators.h:1554-1567): F[i][j] = - u_i b_j (- b_i u_j), pulled back -> Y[(i*3+e)*27 + t]
    if (CART) {
      const double JxW = prm.detJ * wabc;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          double F = val[i] * val[3 + e];
          if (JACOBIAN) F = fma(val[3 + i], val[e], F);
          Y[(i * 3 + e) * 27 + t] = -F * JxW * prm.hinv[e];
        }
    } else {
      const double x = prm.xq[a], y = prm.xq[b], z = prm.xq[c];
      const double fx[2] = {1 - x, x}, fy[2] = {1 - y, y}, fz[2] = {1 - z, z}, dd[2] = {-1.0, 1.0};
      double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      const long long nvx = prm.ncx + 1, nvy = prm.ncy + 1;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const double *V = prm.vertices + 3 * ((cx + i) + nvx * ((cy + j) + nvy * (long long)(cz + k)));
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              const double Vd = V[d];
              J[d][0] += Vd * dd[i] * fy[j] * fz[k];
              J[d][1] += Vd * fx[i] * dd[j] * fz[k];
              J[d][2] += Vd * fx[i] * fy[j] * dd[k];
            }
          }
      const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      const double id = 1.0 / det;
      double Ji[3][3];
      Ji[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
      Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
      Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
      Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * id;
      Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
      Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
      Ji[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
      Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
      Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
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
        for (int e = 0; e < 3; ++e) Y[(i * 3 + e) * 27 + t] = Ji[e][0] * F[0] + Ji[e][1] * F[1] + Ji[e][2] * F[2];
      }
    }
    wave_fence();
    // ---- integrate, z: quadrature point -> (q_x, q_y, n_z) -> X (the z derivative on the field e = 2)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *f0 = Y + (i * 3) * 27 + a + 3 * b, *f1 = f0 + 27, *f2 = f0 + 54;
      X[(i * 3) * 27 + t] = fma(ScT[2], f0[18], fma(ScT[1], f0[9], ScT[0] * f0[0]));
      X[(i * 3 + 1) * 27 + t] = fma(ScT[2], f1[18], fma(ScT[1], f1[9], ScT[0] * f1[0]));
      X[(i * 3 + 2) * 27 + t] = fma(DcT[2], f2[18], fma(DcT[1], f2[9], DcT[0] * f2[0]));
    }
    wave_fence();
    // ---- y: -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *g0 = X + (i * 3) * 27 + a + 9 * c, *g1 = g0 + 27, *g2 = g0 + 54;
      Y[(i * 2) * 27 + t] = fma(SbT[2], g0[6], fma(SbT[1], g0[3], SbT[0] * g0[0]));
      Y[(i * 2 + 1) * 27 + t] = fma(DbT[2], g1[6], fma(DbT[1], g1[3], DbT[0] * g1[0])) +
                                fma(SbT[2], g2[6], fma(SbT[1], g2[3], SbT[0] * g2[0]));
    }
    wave_fence();
    // ---- x: -> node (a, b, c)
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double *h0 = Y + (i * 2) * 27 + 3 * b + 9 * c, *h1 = h0 + 27;
      r[i] = fma(DaT[2], h0[2], fma(DaT[1], h0[1], DaT[0] * h0[0])) + fma(SaT[2], h1[2], fma(SaT[1], h1[1], SaT[0] * h1[0]));
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

// The inflow term of the weak faces, in the layout of stokes_boundary_kernel (stfem_stokes_boundary.hip): one half-wave per boundary
// CELL, handled by its lowest weak face for all of them; the nine lanes of a face's quadrature points evaluate u and b there and
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
          const double fx[2] = {1 - xi[0], xi[0]}, fy[2] = {1 - xi[1], xi[1]}, fz[2] = {1 - xi[2], xi[2]}, dd[2] = {-1.0, 1.0};
          double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
          const long long nvx = prm.ncx + 1, nvy = prm.ncy + 1;
          for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 2; ++j)
              for (int i = 0; i < 2; ++i) {
                const double *V = prm.vertices + 3 * ((cx + i) + nvx * ((cy + j) + nvy * (long long)(cz + k)));
                for (int e = 0; e < 3; ++e) {
                  const double Ve = V[e];
                  J[e][0] += Ve * dd[i] * fy[j] * fz[k];
                  J[e][1] += Ve * fx[i] * dd[j] * fz[k];
                  J[e][2] += Ve * fx[i] * fy[j] * dd[k];
                }
              }
          const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                             J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
          const double id = 1.0 / det;
          double Ji[3][3];
          Ji[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
          Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
          Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
          Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * id;
          Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
          Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
          Ji[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
          Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
          Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
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

} // namespace

int stokes_convection_launch(stfem_stokes_ctx *c, const StokesParams &prm, const double *const *lin, int mode, hipStream_t st)
{
  if (mode != STFEM_CONVECTION_FORM && mode != STFEM_CONVECTION_JACOBIAN) return STFEM_ERR_INVALID_ARGUMENT;
  if (prm.nsrc < 1 || prm.nsrc > MAXSRC || prm.nout > (prm.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiations' bounds)
  ConvectionParams k;
  k.vertices = prm.vertices;
  k.ncx = prm.ncx; k.ncy = prm.ncy; k.ncz = prm.ncz;
  for (int d = 0; d < 3; ++d) { k.ndu[d] = prm.ndu[d]; k.xq[d] = prm.xq[d]; k.wq[d] = prm.wq[d]; k.hinv[d] = prm.hinv[d]; }
  k.Nu = prm.Nu;
  k.dmask = prm.dmask;
  for (int i = 0; i < 9; ++i) { k.Su[i] = prm.Su[i]; k.Du[i] = prm.Du[i]; }
  k.interleave = prm.interleave; k.colour = 0; k.cart = prm.cart;
  k.detJ = prm.detJ;
  k.nsrc = prm.nsrc;
  for (int s = 0; s < MAXSRC; ++s) {
    k.us[s] = s < prm.nsrc ? prm.us[s] : nullptr;
    k.bs[s] = s < prm.nsrc ? lin[s] : nullptr;
    if (s < prm.nsrc && !lin[s]) return STFEM_ERR_INVALID_ARGUMENT;
  }
  // the destinations that receive the term: those with a non-zero weight of the K part
  k.nout = 0;
  for (int o = 0; o < MAXOUT; ++o) {
    k.out_u[o] = nullptr;
    for (int s = 0; s < MAXSRC; ++s) k.wKu[s][o] = 0.0;
  }
  for (int o = 0; o < prm.nout; ++o) {
    bool use = false;
    for (int s = 0; s < prm.nsrc; ++s) use = use || prm.wKu[s][o] != 0.0;
    if (!use || !prm.out_u[o]) continue;
    k.out_u[k.nout] = prm.out_u[o];
    for (int s = 0; s < prm.nsrc; ++s) k.wKu[s][k.nout] = prm.wKu[s][o];
    ++k.nout;
  }
  if (k.nout == 0) return STFEM_OK;
  k.weak_mask = c->bnd.weak_mask;
  for (int f = 0; f < 7; ++f) k.foff[f] = c->bnd.foff[f];
  for (int i = 0; i < 6; ++i) k.Eu[i] = c->bnd.Eu[i];

  const bool multi = prm.nsrc > 1, jac = mode == STFEM_CONVECTION_JACOBIAN;
  const int which = (jac ? 4 : 0) + (multi ? 2 : 0) + (k.cart ? 1 : 0);
  const void *kerns[8] = {(const void *)stokes_convection_kernel<false, false, false>, (const void *)stokes_convection_kernel<true, false, false>,
                          (const void *)stokes_convection_kernel<false, true, false>,  (const void *)stokes_convection_kernel<true, true, false>,
                          (const void *)stokes_convection_kernel<false, false, true>,  (const void *)stokes_convection_kernel<true, false, true>,
                          (const void *)stokes_convection_kernel<false, true, true>,   (const void *)stokes_convection_kernel<true, true, true>};
  const void *kern = kerns[which];
  // resident workgroups per CU of the instantiations, asked once (not on the launch path); persistent workgroups as in stokes_cell_launch
  static int resident_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int &resident = resident_of[which];
  if (resident < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, 256, 0) != hipSuccess || resident < 1)) resident = 2;
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) { // ascending, like every colour sequence of the operator
    const long long n = (long long)((c->nc[0] - (colour & 1) + 1) / 2) * ((c->nc[1] - ((colour >> 1) & 1) + 1) / 2) *
                        ((c->nc[2] - (colour >> 2) + 1) / 2);
    if (n == 0) continue;
    k.colour = colour;
    const unsigned grid = (unsigned)std::min<long long>((n + 7) / 8, (long long)c->n_cu * resident);
    void *args[] = {(void *)&k};
    (void)hipLaunchKernel(kern, dim3(grid), dim3(256), args, 0, st);
    c->convection_launched = true; // (stfem_stokes_last_convection_plan)
    c->convection_plan[0] = (int)grid;
    c->convection_plan[1] = (int)((n + 8ll * grid - 1) / (8ll * grid));
  }
  const long long items = k.weak_mask ? k.foff[6] : 0;
  if (items > 0) {
    const unsigned grid = (unsigned)std::min<long long>((items + 7) / 8, 4ll * c->n_cu);
    for (int colour = 0; colour < 8; ++colour) {
      k.colour = colour;
      if (multi) hipLaunchKernelGGL(stokes_inflow_kernel<true>, dim3(grid), dim3(256), 0, st, k);
      else hipLaunchKernelGGL(stokes_inflow_kernel<false>, dim3(grid), dim3(256), 0, st, k);
    }
  }
  return stfem_launch_end("stokes_convection_kernel");
}
