// Stokes two-field operator, general meshes: the cell kernel.  It replaces, for the cell loop (LoopType::Cell: no weak boundary
// ids, delta0 = 0):
//   StokesMatrixFreeOperator::do_cell_integral_range / do_cell_integral_local
//       (reference include/operators.h:1501-1575, OperatorMode::none):
//       pressure.submit_value(div u); velocity.submit_gradient(nu grad u - p I)
//   the vector mass operator behind d/dt u (MatrixFreeOperator<dim, dim, Number>, operators.h:1135-1173)
//   SystemMatrixStokes::vmult -> tensorproduct_eval (operators.h:696-700, 825-867): per source time
//       dof one K.vmult + scatter with Alpha and one M.vmult + scatter with Beta.
// Here ONE launch per source time dof evaluates the cell once and scatters
//       wKu_j * (nu K u - B^T p) + wM_j * M u   into every velocity destination block j,
//       wKp_j * (div u, q)                       into every pressure destination block j
// in eight launches, one per cell colour (cells of one colour share no DoF), with plain loads and
// stores: no atomics, no zeroing, bitwise reproducible.  No CPU fallback.
//
// Thread layout: one wave owns two cells (32 lanes each, 27 = 3^3 active).  Evaluation and
// integration are sum-factorised (three 1D stages each, see stokes_cell_kernel); the MappingQ1
// Jacobian is evaluated on the fly from the eight cell vertices (24 doubles per cell instead of a
// stored metric), or is a constant diagonal on axis-aligned boxes.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// 256 threads = 4 waves = 8 cells at a time; the workgroups walk over the cells.
// Sum-factorised: evaluation and integration are three 1D stages each (x, y, z), handed from lane to
// lane through two wave-private LDS regions per cell that alternate as source and destination.
//   evaluate : lane (a, b, c) = (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point (q_x, q_y, q_z)
//   integrate: lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node (n_x, n_y, n_z); the eight
//              lanes with a, b, c < 2 also carry the pressure node (a, b, c)
// The lane's rows / columns of the 1D tables stay in registers for the whole kernel.
// CART: axis-aligned uniform cells (the context was created without vertices): constant diagonal Jacobian.
// MULTI: several sources per cell, weighted sums in registers (one set per destination pair, up to MAXSRC), one scatter; otherwise
//        one source (index 0), no sums, the weights applied at scatter time to up to MAXOUT destination pairs (see StokesParams)
// PDG: FE_DGP(1) pressure (a template parameter: the FE_Q(1) instantiations stay what they were)
template <bool CART, bool MULTI, bool PDG>
__global__ __launch_bounds__(256) void stokes_cell_kernel(const StokesParams prm)
{
  constexpr int RX = 351, RY = 351; // doubles per cell of the two regions (largest stage: 13 x 27)
  __shared__ double smem[8 * (RX + RY)];
  __shared__ double tS[9], tD[9], tP[6], tL[3]; // 1D tables [q*3+a], [q*3+a], [q*2+a]; l at the Gauss points
  if (threadIdx.x < 9) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < 6) tP[threadIdx.x] = prm.Sp[threadIdx.x];
  if (threadIdx.x < 3) tL[threadIdx.x] = prm.l1q[threadIdx.x];
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  const int a1 = a < 2 ? a : 1, b1 = b < 2 ? b : 1, c1 = c < 2 ? c : 1; // (pressure stages: clamped, unused where >= 2)
  double *X = smem + slot * (RX + RY), *Y = X + RX;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  double Sa[3], Da[3], Sb[3], Db[3], Sc[3], Dc[3], SaT[3], DaT[3], SbT[3], DbT[3], ScT[3], DcT[3];
  double Pa[2], Pb[2], Pc[2], PaT[3], PbT[3], PcT[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    Sa[n] = tS[a * 3 + n]; Da[n] = tD[a * 3 + n]; Sb[n] = tS[b * 3 + n]; Db[n] = tD[b * 3 + n];
    Sc[n] = tS[c * 3 + n]; Dc[n] = tD[c * 3 + n];
    SaT[n] = tS[n * 3 + a]; DaT[n] = tD[n * 3 + a]; SbT[n] = tS[n * 3 + b]; DbT[n] = tD[n * 3 + b];
    ScT[n] = tS[n * 3 + c]; DcT[n] = tD[n * 3 + c];
    PaT[n] = tP[n * 2 + a1]; PbT[n] = tP[n * 2 + b1]; PcT[n] = tP[n * 2 + c1];
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) { Pa[n] = tP[a * 2 + n]; Pb[n] = tP[b * 2 + n]; Pc[n] = tP[c * 2 + n]; }
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  // this lane also carries a pressure DoF of the cell: FE_Q(1) node (a, b, c), or FE_DGP(1) function t
  const bool pnode = PDG ? t32 < 4 : (lane27 && a < 2 && b < 2 && c < 2);
  const int pslot = PDG ? t32 : a + 2 * b + 4 * c; // its slot in the cell's pressure values X[81 ..]
  const double la = PDG ? tL[a] : 0.0, lb = PDG ? tL[b] : 0.0, lc = PDG ? tL[c] : 0.0; // DGP: the linear functions at this lane's quadrature point
  // the cells of one colour share no DoF: the eight colours run as eight launches, lowest first, and
  // scatter with plain loads and stores (no atomics, no zeroing of the destinations, deterministic)
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;

  // every half-wave walks through its own contiguous run of cells: cells sharing nodes are handled one
  // after the other by the same lanes instead of at the same time by neighbouring ones (their atomics
  // on the shared nodes would serialise in L2)
  const long long nhalf = (long long)gridDim.x * 8, run = (ncells + nhalf - 1) / nhalf;
  // STRIDE = 1: every half-wave walks its own contiguous run of cells; STRIDE = 8: the eight half-waves of the workgroup take eight
  // consecutive cells of the workgroup's run at a time (their rows are 32 bytes apart: denser sectors per gather / scatter instruction)
  const long long wg_first = (long long)blockIdx.x * 8 * run, wg_end = wg_first + 8 * run;
  const int STRIDE = prm.interleave ? 8 : 1;
  const long long first = prm.interleave ? wg_first + slot : ((long long)blockIdx.x * 8 + slot) * run;
  // the DoFs of a cell are fetched while the previous cell is being computed
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu, gp;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && (prm.interleave ? cell < wg_end : cell < first + run);
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = 2 * q.cx + a, iy = 2 * q.cy + b, iz = 2 * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    q.gp = PDG ? (q.cx + (long long)prm.ncx * (q.cy + (long long)prm.ncy * q.cz)) * 4 + (t32 & 3)
                   : (q.cx + a1) + (long long)prm.ndp[0] * ((q.cy + b1) + (long long)prm.ndp[1] * (q.cz + c1));
    return q;
  };
  double un[3] = {0, 0, 0}, pn = 0.0;
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained velocity entries read as 0
    const double *us = prm.us[MULTI ? s : 0], *ps = prm.ps[MULTI ? s : 0];
    if (q.ok && lane27 && !q.con) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) un[comp] = us[comp * prm.Nu + q.gu];
    } else {
      un[0] = un[1] = un[2] = 0.0;
    }
    pn = (q.ok && pnode && ps) ? ps[q.gp] : 0.0;
  };
  CellIds nxt = ids(first);
  fetch(nxt, 0);
  double accU[MULTI ? MAXSRC : 1][3], accP[MULTI ? MAXSRC : 1]; // several sources: the sums over them, per destination pair
#pragma unroll
  for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = accP[o] = 0.0;
  for (long long it2 = 0; it2 < run * nsrc; ++it2) {
    const long long it = it2 / nsrc;
    const int src = int(it2 - it * nsrc);
    const CellIds cur = nxt;
    const bool cell_ok = cur.ok;
    const int cx = cur.cx, cy = cur.cy, cz = cur.cz;
    const bool con = cur.con;
    const long long gu = cur.gu, gp = cur.gp;
    const bool active = cell_ok && lane27;

    // ---- gather: X = u[3][27], p[8]
    if (lane27) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) X[comp * 27 + t] = un[comp];
    }
    if (pnode) X[81 + pslot] = pn;
    nxt = ids(first + STRIDE * ((it2 + 1) / nsrc));
    fetch(nxt, int((it2 + 1) % nsrc));
    wave_fence();
    double pdgv[4] = {0, 0, 0, 0};
    if (PDG) {
#pragma unroll
      for (int j = 0; j < 4; ++j) pdgv[j] = X[81 + j];
    }

    // ---- evaluate, x: (n_x, n_y, n_z) -> (q_x, n_y, n_z): values and x derivatives -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *u = X + comp * 27 + 3 * b + 9 * c;
      const double u0 = u[0], u1 = u[1], u2 = u[2];
      Y[(comp * 2) * 27 + t] = fma(Sa[2], u2, fma(Sa[1], u1, Sa[0] * u0));
      Y[(comp * 2 + 1) * 27 + t] = fma(Da[2], u2, fma(Da[1], u1, Da[0] * u0));
    }
    Y[162 + t] = fma(Pa[1], X[81 + 1 + 2 * b1 + 4 * c1], Pa[0] * X[81 + 2 * b1 + 4 * c1]); // pressure (n_y, n_z < 2)
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z): value, d/dx, d/dy -> X
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *v = Y + (comp * 2) * 27 + a + 9 * c, *d = v + 27;
      const double v0 = v[0], v1 = v[3], v2 = v[6], d0 = d[0], d1 = d[3], d2 = d[6];
      X[(comp * 3) * 27 + t] = fma(Sb[2], v2, fma(Sb[1], v1, Sb[0] * v0));
      X[(comp * 3 + 1) * 27 + t] = fma(Sb[2], d2, fma(Sb[1], d1, Sb[0] * d0));
      X[(comp * 3 + 2) * 27 + t] = fma(Db[2], v2, fma(Db[1], v1, Db[0] * v0));
    }
    X[243 + t] = fma(Pb[1], Y[162 + a + 3 + 9 * c1], Pb[0] * Y[162 + a + 9 * c1]);
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): value and reference gradient in registers
    double uval[3], gref[3][3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *v = X + (comp * 3) * 27 + a + 3 * b, *dx = v + 27, *dy = v + 54;
      const double v0 = v[0], v1 = v[9], v2 = v[18];
      uval[comp] = fma(Sc[2], v2, fma(Sc[1], v1, Sc[0] * v0));
      gref[comp][0] = fma(Sc[2], dx[18], fma(Sc[1], dx[9], Sc[0] * dx[0]));
      gref[comp][1] = fma(Sc[2], dy[18], fma(Sc[1], dy[9], Sc[0] * dy[0]));
      gref[comp][2] = fma(Dc[2], v2, fma(Dc[1], v1, Dc[0] * v0));
    }
    double pval = fma(Pc[1], X[243 + a + 3 * b + 9], Pc[0] * X[243 + a + 3 * b]);
    if (PDG) pval = pdgv[0] + la * pdgv[1] + lb * pdgv[2] + lc * pdgv[3];

    // ---- quadrature-point operation (operators.h:1547-1553, 1570; weights applied at scatter time) -> Y
    if (CART) {
      const double JxW = prm.detJ * wabc;
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const double g = gref[comp][e] * prm.hinv[e];
          Y[(comp * 3 + e) * 27 + t] = (prm.nu * g - (comp == e ? pval : 0.0)) * JxW * prm.hinv[e];
        }
        Y[(10 + comp) * 27 + t] = uval[comp] * JxW;
      }
      Y[9 * 27 + t] = (gref[0][0] * prm.hinv[0] + gref[1][1] * prm.hinv[1] + gref[2][2] * prm.hinv[2]) * JxW;
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
      double divu = 0.0;
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
        double F[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const double g = gref[comp][0] * Ji[0][d] + gref[comp][1] * Ji[1][d] + gref[comp][2] * Ji[2][d];
          if (comp == d) divu += g;
          F[d] = (prm.nu * g - (comp == d ? pval : 0.0)) * JxW;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) Y[(comp * 3 + e) * 27 + t] = Ji[e][0] * F[0] + Ji[e][1] * F[1] + Ji[e][2] * F[2];
        Y[(10 + comp) * 27 + t] = uval[comp] * JxW;
      }
      Y[9 * 27 + t] = divu * JxW;
    }
    wave_fence();
    double rPdg = 0.0;
    if (PDG && t32 < 4) { // (q_j, div u): the cell's own four test functions, summed over the 27 quadrature points
      const double *fd = Y + 9 * 27;
      for (int q = 0; q < 27; ++q) {
        const int qa = q % 3, qb = (q / 3) % 3, qc = q / 9;
        const double l = t32 == 0 ? 1.0 : tL[t32 == 1 ? qa : (t32 == 2 ? qb : qc)];
        rPdg = fma(l, fd[q], rPdg);
      }
    }

    // ---- integrate, z: quadrature point -> (q_x, q_y, n_z) -> X
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *f0 = Y + (comp * 3) * 27 + a + 3 * b, *f1 = f0 + 27, *f2 = f0 + 54, *fm = Y + (10 + comp) * 27 + a + 3 * b;
      X[(comp * 4) * 27 + t] = fma(ScT[2], f0[18], fma(ScT[1], f0[9], ScT[0] * f0[0]));
      X[(comp * 4 + 1) * 27 + t] = fma(ScT[2], f1[18], fma(ScT[1], f1[9], ScT[0] * f1[0]));
      X[(comp * 4 + 2) * 27 + t] = fma(DcT[2], f2[18], fma(DcT[1], f2[9], DcT[0] * f2[0]));
      X[(comp * 4 + 3) * 27 + t] = fma(ScT[2], fm[18], fma(ScT[1], fm[9], ScT[0] * fm[0]));
    }
    {
      const double *fd = Y + 9 * 27 + a + 3 * b;
      X[324 + t] = fma(PcT[2], fd[18], fma(PcT[1], fd[9], PcT[0] * fd[0]));
    }
    wave_fence();
    // ---- y: -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *g0 = X + (comp * 4) * 27 + a + 9 * c, *g1 = g0 + 27, *g2 = g0 + 54, *gm = g0 + 81;
      Y[(comp * 3) * 27 + t] = fma(SbT[2], g0[6], fma(SbT[1], g0[3], SbT[0] * g0[0]));
      Y[(comp * 3 + 1) * 27 + t] = fma(DbT[2], g1[6], fma(DbT[1], g1[3], DbT[0] * g1[0])) +
                                   fma(SbT[2], g2[6], fma(SbT[1], g2[3], SbT[0] * g2[0]));
      Y[(comp * 3 + 2) * 27 + t] = fma(SbT[2], gm[6], fma(SbT[1], gm[3], SbT[0] * gm[0]));
    }
    {
      const double *gd = X + 324 + a + 9 * c;
      Y[243 + t] = fma(PbT[2], gd[6], fma(PbT[1], gd[3], PbT[0] * gd[0]));
    }
    wave_fence();
    // ---- x: -> node (a, b, c)
    double rK[3], rM[3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *h0 = Y + (comp * 3) * 27 + 3 * b + 9 * c, *h1 = h0 + 27, *hm = h0 + 54;
      rK[comp] = fma(DaT[2], h0[2], fma(DaT[1], h0[1], DaT[0] * h0[0])) + fma(SaT[2], h1[2], fma(SaT[1], h1[1], SaT[0] * h1[0]));
      rM[comp] = fma(SaT[2], hm[2], fma(SaT[1], hm[1], SaT[0] * hm[0]));
    }
    const double *hd = Y + 243 + 3 * b + 9 * c;
    const double rP = PDG ? rPdg : fma(PaT[2], hd[2], fma(PaT[1], hd[1], PaT[0] * hd[0]));

    // ---- distribute_local_to_global: constrained velocity rows stay 0.  A DoF on a face shared with a
    // neighbouring cell is first touched by the cell whose colour bits are 0 in all shared directions.
    if constexpr (MULTI) {
#pragma unroll
      for (int o = 0; o < MAXSRC; ++o)
        if (o < prm.nout) {
          const double kU = prm.wKu[src][o], kM = prm.wM[src][o];
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(kU, rK[comp], fma(kM, rM[comp], accU[o][comp]));
          accP[o] = fma(prm.wKp[src][o], rP, accP[o]);
        }
    }
    if (active && src == nsrc - 1) {
      const bool fu = !((a == 0 && cx > 0 && px) || (a == 2 && cx < prm.ncx - 1 && px) ||
                        (b == 0 && cy > 0 && py) || (b == 2 && cy < prm.ncy - 1 && py) ||
                        (c == 0 && cz > 0 && pz) || (c == 2 && cz < prm.ncz - 1 && pz));
      const bool fp = PDG || !((a == 0 && cx > 0 && px) || (a == 1 && cx < prm.ncx - 1 && px) ||
                                    (b == 0 && cy > 0 && py) || (b == 1 && cy < prm.ncy - 1 && py) ||
                                    (c == 0 && cz > 0 && pz) || (c == 1 && cz < prm.ncz - 1 && pz));
      // what destination pair o receives: the sums over the sources, or the one source's results with the pair's weights
      auto valU = [&](int o, int comp) {
        if constexpr (MULTI) return accU[o][comp];
        else return prm.wKu[0][o] * rK[comp] + prm.wM[0][o] * rM[comp];
      };
      auto valP = [&](int o) {
        if constexpr (MULTI) return accP[o];
        else return prm.wKp[0][o] * rP;
      };
      // (the sums are registers: their loop is unrolled and guarded; the launcher keeps nout within the instantiation's bound)
      constexpr int NO_UNROLL = MULTI ? MAXSRC : 1;
      const int no = MULTI ? MAXSRC : prm.nout;
#pragma unroll NO_UNROLL
      for (int o = 0; o < no; ++o) {
        if (MULTI && o >= prm.nout) continue;
        if (prm.out_u[o]) {
          double *d = prm.out_u[o] + gu;
          if (prm.store_u[o] && fu) {
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) d[comp * prm.Nu] = con ? 0.0 : valU(o, comp);
          } else if (!con) {
            double v[3];
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) v[comp] = d[comp * prm.Nu];
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) d[comp * prm.Nu] = v[comp] + valU(o, comp);
          }
        }
        if (pnode && prm.out_p[o]) {
          double *d = prm.out_p[o] + gp;
          if (prm.store_p[o] && fp) *d = valP(o);
          else *d += valP(o);
        }
      }
    }
    if (MULTI && src == nsrc - 1) {
#pragma unroll
      for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = accP[o] = 0.0;
    }
    wave_fence(); // the next cell's gather overwrites X
  }
}

} // namespace

int stokes_cell_launch(stfem_stokes_ctx *c, StokesParams &prm, hipStream_t st)
{
  const int which = (prm.pdg ? 4 : 0) + (prm.nsrc > 1 ? 2 : 0) + (prm.cart ? 1 : 0);
  if (prm.nsrc < 1 || prm.nsrc > MAXSRC || prm.nout > (prm.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiation's bounds)
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) { // ascending: see store_u / store_p
    const long long n = (long long)((c->nc[0] - (colour & 1) + 1) / 2) * ((c->nc[1] - ((colour >> 1) & 1) + 1) / 2) *
                        ((c->nc[2] - (colour >> 2) + 1) / 2);
    if (n == 0) continue;
    prm.colour = colour;
    // persistent workgroups: exactly as many as stay resident (measured on 64^3 cells, cG(1): 2 per CU 0.41 ms, 3: 0.50, 4: 0.43,
    // 8: 0.45, one workgroup per 8 cells: 0.52 - long runs keep the prefetch of the next cell's DoFs going and leave no partial round)
    static const int grid_env = [] {
      const char *e = getenv("STFEM_STOKES_GRID"); // workgroups per CU of a colour launch (experiments)
      return e ? std::max(1, atoi(e)) : 0;
    }();
    const void *kerns[8] = {(const void *)stokes_cell_kernel<false, false, false>, (const void *)stokes_cell_kernel<true, false, false>,
                            (const void *)stokes_cell_kernel<false, true, false>,  (const void *)stokes_cell_kernel<true, true, false>,
                            (const void *)stokes_cell_kernel<false, false, true>,  (const void *)stokes_cell_kernel<true, false, true>,
                            (const void *)stokes_cell_kernel<false, true, true>,   (const void *)stokes_cell_kernel<true, true, true>};
    const void *kern = kerns[which];
    // resident workgroups per CU of the instantiations, asked once (not on the launch path)
    static int resident_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int &resident = resident_of[which];
    if (resident < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, 256, 0) != hipSuccess || resident < 1)) resident = 2;
    const unsigned grid = (unsigned)std::min<long long>((n + 7) / 8, (long long)c->n_cu * (grid_env ? grid_env : resident));
    void *args[] = {(void *)&prm};
    (void)hipLaunchKernel(kern, dim3(grid), dim3(256), args, 0, st);
  }
  return stfem_launch_end("stokes_cell_kernel");
}
