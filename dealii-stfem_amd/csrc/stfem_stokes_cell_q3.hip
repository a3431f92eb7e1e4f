// Stokes two-field operator at velocity degree 3: the cell kernel of FE_Q(3)^3 x FE_Q(2) / FE_DGP(2) with QGauss(4), the pair the
// reference builds for time degree 2 (tests/tp_03stokes.cc:79-86: FE_Q(k+1)^dim x FE_DGP(k) or FE_Q(k), QGauss(k+2)).  It computes
// what stokes_cell_kernel (stfem_stokes_cell.hip) computes for FE_Q(2)^3 x FE_Q(1) / FE_DGP(1):
//       out_u[o] (=, +=) sum_s wKu[s][o] (nu K u_s - B^T p_s) + wM[s][o] M u_s,    out_p[o] (=, +=) sum_s wKp[s][o] B u_s
// in eight launches, one per cell colour, with plain loads and stores: no atomics, no zeroing, bitwise reproducible.  It serves
// boxes too (CART): a context of degree 3 has no Kronecker path.  No CPU fallback.
//
// Thread layout: a cell has 4^3 = 64 velocity nodes and 64 quadrature points - one wave is one cell, lane t = a + 4 b + 16 c is
// node (a, b, c) and quadrature point (a, b, c); four cells at a time per 256-thread workgroup.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// Sum-factorised like the FE_Q(2) kernel: three 1D stages each way through two wave-private LDS regions per cell that alternate as
// source and destination, ordered with wave_fence() (a cell never leaves its wave: no workgroup barrier inside the cell loop).
//   evaluate : lane (a, b, c) = (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point (q_x, q_y, q_z)
//   integrate: lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node (n_x, n_y, n_z)
// The FE_Q(2) pressure rides on the 27 lanes with a, b, c < 3 (node (a, b, c)); the other lanes compute on clamped indices and
// their results are not used.  The ten FE_DGP(2) functions are evaluated directly at the lane's point and integrated by lanes 0..9
// as sums over the 64 points in ascending order.
// CART: axis-aligned uniform cells (no vertices): constant diagonal Jacobian.  MULTI: several sources per cell, weighted sums in
// registers, one scatter (see StokesParams).  PDG: FE_DGP(2) pressure (a template parameter: the FE_Q(2) instantiations carry none of it).
template <bool CART, bool MULTI, bool PDG>
__global__ __launch_bounds__(256) void stokes_cell_q3_kernel(const StokesQ3Params prm)
{
  constexpr int N = 64, R = 13 * N; // doubles per cell of each region (largest stage: 13 arrays of 64)
  constexpr int XP = 3 * N;         // the cell's pressure values in the gather: X[XP ..] (27 nodes or 10 functions)
  // the 1D tables behind the regions, in the same array: [q*4+a], [q*4+a], [q*3+a]; Legendre [degree*4+q], degree 0 = 1.  The
  // evaluation rows stay in registers; the integration columns and the pressure tables are read where they are used (all of them in
  // registers: 256 VGPRs and spills to AGPRs, one wave per SIMD)
  __shared__ double smem[4 * 2 * R + 16 + 16 + 12 + 12];
  double *const tS = smem + 4 * 2 * R, *const tD = tS + 16, *const tP = tD + 16, *const tL = tP + 12;
  if (threadIdx.x < 16) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < 12) tP[threadIdx.x] = prm.Sp[threadIdx.x];
  if (threadIdx.x < 4) { tL[threadIdx.x] = 1.0; tL[4 + threadIdx.x] = prm.l1q[threadIdx.x]; tL[8 + threadIdx.x] = prm.l2q[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int a = t & 3, b = (t >> 2) & 3, c = t >> 4;
  const int a2 = a < 3 ? a : 2, b2 = b < 3 ? b : 2, c2 = c < 3 ? c : 2; // (pressure stages: clamped, unused where 3)
  double *X = smem + slot * (2 * R), *Y = X + R;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  double Sa[4], Da[4], Sb[4], Db[4], Sc[4], Dc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    Sa[n] = tS[a * 4 + n]; Da[n] = tD[a * 4 + n]; Sb[n] = tS[b * 4 + n]; Db[n] = tD[b * 4 + n];
    Sc[n] = tS[c * 4 + n]; Dc[n] = tD[c * 4 + n];
  }
  const double *const SaT = tS + a, *const DaT = tD + a, *const SbT = tS + b, *const DbT = tD + b, *const ScT = tS + c, *const DcT = tD + c; // [4 q]
  const double *const Pa = tP + 3 * a, *const Pb = tP + 3 * b, *const Pc = tP + 3 * c;   // [n]
  const double *const PaT = tP + a2, *const PbT = tP + b2, *const PcT = tP + c2;         // [3 q]
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  // this lane also carries a pressure DoF of the cell: FE_Q(2) node (a, b, c), or FE_DGP(2) function t
  const bool pnode = PDG ? t < 10 : (a < 3 && b < 3 && c < 3);
  const int pslot = PDG ? (t < 10 ? t : 9) : a2 + 3 * b2 + 9 * c2; // its slot in the cell's pressure values X[XP ..]
  // FE_DGP(2): the ten functions at this lane's quadrature point, (i, j, k) = degrees in x, y, z, total <= 2, i fastest
  double phi[PDG ? 10 : 1];
  int ei = 0, ej = 0, ek = 0; // the degrees of the function lanes 0..9 integrate
  if constexpr (PDG) {
    const double L1a = tL[4 + a], L2a = tL[8 + a], L1b = tL[4 + b], L2b = tL[8 + b], L1c = tL[4 + c], L2c = tL[8 + c];
    phi[0] = 1.0; phi[1] = L1a; phi[2] = L2a; phi[3] = L1b; phi[4] = L1a * L1b; phi[5] = L2b;
    phi[6] = L1c; phi[7] = L1a * L1c; phi[8] = L1b * L1c; phi[9] = L2c;
    ei = (t == 1 || t == 4 || t == 7) ? 1 : (t == 2 ? 2 : 0);
    ej = (t == 3 || t == 4 || t == 8) ? 1 : (t == 5 ? 2 : 0);
    ek = (t == 6 || t == 7 || t == 8) ? 1 : (t == 9 ? 2 : 0);
  } else {
    phi[0] = 0.0;
  }
  // the cells of one colour share no DoF: the eight colours run as eight launches, lowest first, and scatter with plain loads and
  // stores (no atomics, no zeroing of the destinations, deterministic)
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  // every wave walks through its own contiguous run of cells
  const long long nwave = (long long)gridDim.x * 4, run = (ncells + nwave - 1) / nwave;
  const long long first = ((long long)blockIdx.x * 4 + slot) * run;
  // the DoFs of a cell are fetched while the previous cell is being computed
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu, gp;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && cell < first + run;
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = 3 * q.cx + a, iy = 3 * q.cy + b, iz = 3 * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    q.gp = PDG ? (q.cx + (long long)prm.ncx * (q.cy + (long long)prm.ncy * q.cz)) * 10 + pslot
               : (2 * q.cx + a2) + (long long)prm.ndp[0] * ((2 * q.cy + b2) + (long long)prm.ndp[1] * (2 * q.cz + c2));
    return q;
  };
  double un[3] = {0, 0, 0}, pn = 0.0;
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained velocity entries read as 0
    const double *us = prm.us[MULTI ? s : 0], *ps = prm.ps[MULTI ? s : 0];
    if (q.ok && !q.con) {
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
    const bool active = cur.ok;
    const int cx = cur.cx, cy = cur.cy, cz = cur.cz;
    const bool con = cur.con;
    const long long gu = cur.gu, gp = cur.gp;

    // ---- gather: X = u[3][64], p[27 or 10]
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) X[comp * N + t] = un[comp];
    if (pnode) X[XP + pslot] = pn;
    nxt = ids(first + (it2 + 1) / nsrc);
    fetch(nxt, int((it2 + 1) % nsrc));
    wave_fence();
    double pval = 0.0;
    if constexpr (PDG) {
#pragma unroll
      for (int j = 0; j < 10; ++j) pval = fma(phi[j], X[XP + j], pval);
    }

    // ---- evaluate, x: (n_x, n_y, n_z) -> (q_x, n_y, n_z): values and x derivatives -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *u = X + comp * N + 4 * b + 16 * c;
      const double u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
      Y[(comp * 2) * N + t] = fma(Sa[3], u3, fma(Sa[2], u2, fma(Sa[1], u1, Sa[0] * u0)));
      Y[(comp * 2 + 1) * N + t] = fma(Da[3], u3, fma(Da[2], u2, fma(Da[1], u1, Da[0] * u0)));
    }
    if constexpr (!PDG) { // pressure (n_y, n_z < 3)
      const double *p = X + XP + 3 * b2 + 9 * c2;
      Y[6 * N + t] = fma(Pa[2], p[2], fma(Pa[1], p[1], Pa[0] * p[0]));
    }
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z): value, d/dx, d/dy -> X
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *v = Y + (comp * 2) * N + a + 16 * c, *d = v + N;
      const double v0 = v[0], v1 = v[4], v2 = v[8], v3 = v[12], d0 = d[0], d1 = d[4], d2 = d[8], d3 = d[12];
      X[(comp * 3) * N + t] = fma(Sb[3], v3, fma(Sb[2], v2, fma(Sb[1], v1, Sb[0] * v0)));
      X[(comp * 3 + 1) * N + t] = fma(Sb[3], d3, fma(Sb[2], d2, fma(Sb[1], d1, Sb[0] * d0)));
      X[(comp * 3 + 2) * N + t] = fma(Db[3], v3, fma(Db[2], v2, fma(Db[1], v1, Db[0] * v0)));
    }
    if constexpr (!PDG) {
      const double *p = Y + 6 * N + a + 16 * c2;
      X[9 * N + t] = fma(Pb[2], p[8], fma(Pb[1], p[4], Pb[0] * p[0]));
    }
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): value and reference gradient in registers
    double uval[3], gref[3][3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *v = X + (comp * 3) * N + a + 4 * b, *dx = v + N, *dy = v + 2 * N;
      const double v0 = v[0], v1 = v[16], v2 = v[32], v3 = v[48];
      uval[comp] = fma(Sc[3], v3, fma(Sc[2], v2, fma(Sc[1], v1, Sc[0] * v0)));
      gref[comp][0] = fma(Sc[3], dx[48], fma(Sc[2], dx[32], fma(Sc[1], dx[16], Sc[0] * dx[0])));
      gref[comp][1] = fma(Sc[3], dy[48], fma(Sc[2], dy[32], fma(Sc[1], dy[16], Sc[0] * dy[0])));
      gref[comp][2] = fma(Dc[3], v3, fma(Dc[2], v2, fma(Dc[1], v1, Dc[0] * v0)));
    }
    if constexpr (!PDG) {
      const double *p = X + 9 * N + a + 4 * b;
      pval = fma(Pc[2], p[32], fma(Pc[1], p[16], Pc[0] * p[0]));
    }

    // ---- quadrature-point operation (operators.h:1547-1553, 1570; weights applied at scatter time) -> Y:
    // arrays comp * 3 + e: the flux in reference coordinates, 9: div u, 10 + comp: the mass term
    if (CART) {
      const double JxW = prm.detJ * wabc;
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const double g = gref[comp][e] * prm.hinv[e];
          Y[(comp * 3 + e) * N + t] = (prm.nu * g - (comp == e ? pval : 0.0)) * JxW * prm.hinv[e];
        }
        Y[(10 + comp) * N + t] = uval[comp] * JxW;
      }
      Y[9 * N + t] = (gref[0][0] * prm.hinv[0] + gref[1][1] * prm.hinv[1] + gref[2][2] * prm.hinv[2]) * JxW;
    } else {
      const double xi[3] = {prm.xq[a], prm.xq[b], prm.xq[c]};
      double Ji[3][3], det;
      cip_jacobian(prm, cx, cy, cz, xi, Ji, det); // (J^-1 and det J of the trilinear mapping at this lane's point)
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
        for (int e = 0; e < 3; ++e) Y[(comp * 3 + e) * N + t] = Ji[e][0] * F[0] + Ji[e][1] * F[1] + Ji[e][2] * F[2];
        Y[(10 + comp) * N + t] = uval[comp] * JxW;
      }
      Y[9 * N + t] = divu * JxW;
    }
    wave_fence();
    double rP = 0.0;
    if constexpr (PDG) { // (q_j, div u): the cell's own ten test functions, each summed over the 64 quadrature points in ascending order
      if (t < 10) {
        const double *fd = Y + 9 * N;
        for (int qc = 0; qc < 4; ++qc)
          for (int qb = 0; qb < 4; ++qb) {
            const double lbc = tL[ej * 4 + qb] * tL[ek * 4 + qc];
#pragma unroll
            for (int qa = 0; qa < 4; ++qa) rP = fma(tL[ei * 4 + qa] * lbc, fd[qa + 4 * qb + 16 * qc], rP);
          }
      }
    }

    // ---- integrate, z: quadrature point -> (q_x, q_y, n_z) -> X: per component flux_x, flux_y (values in z), flux_z (derivative), mass
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *f0 = Y + (comp * 3) * N + a + 4 * b, *f1 = f0 + N, *f2 = f0 + 2 * N, *fm = Y + (10 + comp) * N + a + 4 * b;
      X[(comp * 4) * N + t] = fma(ScT[12], f0[48], fma(ScT[8], f0[32], fma(ScT[4], f0[16], ScT[0] * f0[0])));
      X[(comp * 4 + 1) * N + t] = fma(ScT[12], f1[48], fma(ScT[8], f1[32], fma(ScT[4], f1[16], ScT[0] * f1[0])));
      X[(comp * 4 + 2) * N + t] = fma(DcT[12], f2[48], fma(DcT[8], f2[32], fma(DcT[4], f2[16], DcT[0] * f2[0])));
      X[(comp * 4 + 3) * N + t] = fma(ScT[12], fm[48], fma(ScT[8], fm[32], fma(ScT[4], fm[16], ScT[0] * fm[0])));
    }
    if constexpr (!PDG) {
      const double *fd = Y + 9 * N + a + 4 * b;
      X[12 * N + t] = fma(PcT[9], fd[48], fma(PcT[6], fd[32], fma(PcT[3], fd[16], PcT[0] * fd[0])));
    }
    wave_fence();
    // ---- y: -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *g0 = X + (comp * 4) * N + a + 16 * c, *g1 = g0 + N, *g2 = g0 + 2 * N, *gm = g0 + 3 * N;
      Y[(comp * 3) * N + t] = fma(SbT[12], g0[12], fma(SbT[8], g0[8], fma(SbT[4], g0[4], SbT[0] * g0[0])));
      Y[(comp * 3 + 1) * N + t] = fma(DbT[12], g1[12], fma(DbT[8], g1[8], fma(DbT[4], g1[4], DbT[0] * g1[0]))) +
                                  fma(SbT[12], g2[12], fma(SbT[8], g2[8], fma(SbT[4], g2[4], SbT[0] * g2[0])));
      Y[(comp * 3 + 2) * N + t] = fma(SbT[12], gm[12], fma(SbT[8], gm[8], fma(SbT[4], gm[4], SbT[0] * gm[0])));
    }
    if constexpr (!PDG) {
      const double *gd = X + 12 * N + a + 16 * c;
      Y[9 * N + t] = fma(PbT[9], gd[12], fma(PbT[6], gd[8], fma(PbT[3], gd[4], PbT[0] * gd[0])));
    }
    wave_fence();
    // ---- x: -> node (a, b, c)
    double rK[3], rM[3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *h0 = Y + (comp * 3) * N + 4 * b + 16 * c, *h1 = h0 + N, *hm = h0 + 2 * N;
      rK[comp] = fma(DaT[12], h0[3], fma(DaT[8], h0[2], fma(DaT[4], h0[1], DaT[0] * h0[0]))) +
                 fma(SaT[12], h1[3], fma(SaT[8], h1[2], fma(SaT[4], h1[1], SaT[0] * h1[0])));
      rM[comp] = fma(SaT[12], hm[3], fma(SaT[8], hm[2], fma(SaT[4], hm[1], SaT[0] * hm[0])));
    }
    if constexpr (!PDG) {
      const double *hd = Y + 9 * N + 4 * b + 16 * c;
      rP = fma(PaT[9], hd[3], fma(PaT[6], hd[2], fma(PaT[3], hd[1], PaT[0] * hd[0])));
    }

    // ---- distribute_local_to_global: constrained velocity rows stay 0.  A DoF on a face shared with a neighbouring cell is first
    // touched by the cell whose colour bits are 0 in all shared directions (last node index: 3 velocity, 2 FE_Q(2) pressure).
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
      const bool fu = !((a == 0 && cx > 0 && px) || (a == 3 && cx < prm.ncx - 1 && px) ||
                        (b == 0 && cy > 0 && py) || (b == 3 && cy < prm.ncy - 1 && py) ||
                        (c == 0 && cz > 0 && pz) || (c == 3 && cz < prm.ncz - 1 && pz));
      const bool fp = PDG || !((a == 0 && cx > 0 && px) || (a == 2 && cx < prm.ncx - 1 && px) ||
                                    (b == 0 && cy > 0 && py) || (b == 2 && cy < prm.ncy - 1 && py) ||
                                    (c == 0 && cz > 0 && pz) || (c == 2 && cz < prm.ncz - 1 && pz));
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

int stokes_cell_q3_launch(stfem_stokes_ctx *c, const StokesParams &set, hipStream_t st)
{
  if (set.nsrc < 1 || set.nsrc > MAXSRC || set.nout > (set.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiation's bounds)
  StokesQ3Params prm = c->q3;
  prm.nsrc = set.nsrc; prm.nout = set.nout;
  for (int s = 0; s < MAXSRC; ++s) {
    prm.us[s] = s < set.nsrc ? set.us[s] : nullptr;
    prm.ps[s] = s < set.nsrc ? set.ps[s] : nullptr;
    for (int o = 0; o < MAXOUT; ++o) { prm.wKu[s][o] = set.wKu[s][o]; prm.wKp[s][o] = set.wKp[s][o]; prm.wM[s][o] = set.wM[s][o]; }
  }
  for (int o = 0; o < MAXOUT; ++o) {
    prm.out_u[o] = o < set.nout ? set.out_u[o] : nullptr;
    prm.out_p[o] = o < set.nout ? set.out_p[o] : nullptr;
    prm.store_u[o] = set.store_u[o]; prm.store_p[o] = set.store_p[o];
  }
  const bool cart = c->base.cart != 0;
  const int which = (c->pspace ? 4 : 0) + (prm.nsrc > 1 ? 2 : 0) + (cart ? 1 : 0);
  const void *kerns[8] = {(const void *)stokes_cell_q3_kernel<false, false, false>, (const void *)stokes_cell_q3_kernel<true, false, false>,
                          (const void *)stokes_cell_q3_kernel<false, true, false>,  (const void *)stokes_cell_q3_kernel<true, true, false>,
                          (const void *)stokes_cell_q3_kernel<false, false, true>,  (const void *)stokes_cell_q3_kernel<true, false, true>,
                          (const void *)stokes_cell_q3_kernel<false, true, true>,   (const void *)stokes_cell_q3_kernel<true, true, true>};
  const void *kern = kerns[which];
  // persistent workgroups: as many as stay resident, asked once per instantiation (not on the launch path)
  static int resident_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int &resident = resident_of[which];
  if (resident < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, 256, 0) != hipSuccess || resident < 1)) resident = 2;
  // STFEM_STOKES_Q3_WORKGROUPS=<n>, read at every launch: at most n workgroups per colour launch (tests: several cells per wave on a small mesh)
  long long cap = 0;
  if (const char *e = getenv("STFEM_STOKES_Q3_WORKGROUPS")) cap = std::max(1ll, atoll(e));
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) { // ascending: see store_u / store_p
    const long long n = (long long)((c->nc[0] - (colour & 1) + 1) / 2) * ((c->nc[1] - ((colour >> 1) & 1) + 1) / 2) *
                        ((c->nc[2] - (colour >> 2) + 1) / 2);
    if (n == 0) continue;
    prm.colour = colour;
    long long grid = std::min<long long>((n + 3) / 4, (long long)c->n_cu * resident);
    if (cap) grid = std::min(grid, cap);
    void *args[] = {(void *)&prm};
    (void)hipLaunchKernel(kern, dim3((unsigned)grid), dim3(256), args, 0, st);
    c->q3_launched = true;
    c->q3_plan[0] = (int)grid;
    c->q3_plan[1] = (int)((n + grid * 4 - 1) / (grid * 4));
  }
  return stfem_launch_end("stokes_cell_q3_kernel");
}
