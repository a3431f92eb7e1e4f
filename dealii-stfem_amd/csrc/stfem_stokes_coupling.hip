// Stokes two-field operator, axis-aligned uniform meshes: the coupling kernels of the operator's Kronecker form (the launches are put
// together by stokes_cart_launch, stfem_stokes.hip).
// On boxes of identical cells the velocity part  nu K u_c + wM M u_c  of every component is the SCALAR space-time operator of
// FE_Q(2): it runs as the scalar pencil sweep (stfem_st_vmult on a Q2 context: owner-writes, every DoF stored once), the
// components being blocks.  What is left of the cell loop (operators.h:1547-1570) is the coupling
//     out_u_c -= B_c^T p,   out_p = sum_c B_c u_c,   B_c = (q, d u_c / d x_c),
// whose cell matrices are Kronecker products of 1D mixed matrices (N = int phi_a psi_j, C = int phi_a' psi_j), so both run in
// GATHER form - one thread per destination DoF sums what its <= 8 cells contribute, in a fixed order: no colours, no atomics,
// every destination touched once.  (Measured on 64^3 cells the eight colour launches of the cell kernel were bound by their
// access pattern and LDS traffic: profiles/r2/stokes.)
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

// FE_Q(1): the pressure nodes a velocity line node i couples to: first index p0, weights of up to three (value / derivative forms)
__device__ __forceinline__ void q1_row(const CouplingParams &P, int i, int nc, int &p0, double (&wn)[3], double (&wc)[3])
{
  if (i & 1) { // midpoint of cell c
    p0 = i >> 1;
    wn[0] = P.N[1][0]; wn[1] = P.N[1][1]; wn[2] = 0.0;
    wc[0] = P.C[1][0]; wc[1] = P.C[1][1]; wc[2] = 0.0;
  } else { // vertex between cells c - 1 (its node 2) and c (its node 0)
    const int c = i >> 1;
    const bool lo = c > 0, hi = c < nc;
    p0 = c - 1;
    wn[0] = lo ? P.N[2][0] : 0.0; wn[1] = (lo ? P.N[2][1] : 0.0) + (hi ? P.N[0][0] : 0.0); wn[2] = hi ? P.N[0][1] : 0.0;
    wc[0] = lo ? P.C[2][0] : 0.0; wc[1] = (lo ? P.C[2][1] : 0.0) + (hi ? P.C[0][0] : 0.0); wc[2] = hi ? P.C[0][1] : 0.0;
  }
}

// out_u[o][c][node] -= sum_s wKu[o][s] (B_c^T p_s)[node]: one thread per velocity node.  NS / NO: compile-time bounds of the
// source / destination loops (their accumulators then live in registers; with run-time bounds the generic instantiation
// needed 246 VGPRs and scratch)
template <int NS, int NO, bool PDG>
__global__ __launch_bounds__(256, NO <= 2 ? 3 : 2) void stokes_grad_kernel(const CouplingParams P)
{
  const long long node = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= P.Nu) return;
  const int ix = int(node % P.ndu[0]), iy = int((node / P.ndu[0]) % P.ndu[1]), iz = int(node / ((long long)P.ndu[0] * P.ndu[1]));
  const bool con = ((P.dmask & 1) && ix == 0) || ((P.dmask & 2) && ix == P.ndu[0] - 1) || ((P.dmask & 4) && iy == 0) ||
                   ((P.dmask & 8) && iy == P.ndu[1] - 1) || ((P.dmask & 16) && iz == 0) || ((P.dmask & 32) && iz == P.ndu[2] - 1);
  if (con) return; // constrained rows are not written (they hold the sweep's exact zero)
  double acc[NO][3];
#pragma unroll
  for (int o = 0; o < NO; ++o) acc[o][0] = acc[o][1] = acc[o][2] = 0.0;
  // the destination values this thread updates are fetched first: their latency runs beside the pressure gather's (the kernel is
  // bound by dependent memory round trips, not by bytes: profiles/r3/stokes)
  double old[NO <= 2 ? NO : 1][3];
  if constexpr (NO <= 2) {
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int c = 0; c < 3; ++c) old[o][c] = (o < P.nout && P.out_u[o]) ? P.out_u[o][c * P.Nu + node] : 0.0;
  }
  const int nc[3] = {P.ncx, P.ncy, P.ncz};
  const int idx[3] = {ix, iy, iz};
  if constexpr (!PDG) {
    int p0[3];
    double wn[3][3], wc[3][3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      q1_row(P, d == 0 ? ix : (d == 1 ? iy : iz), d == 0 ? P.ncx : (d == 1 ? P.ncy : P.ncz), p0[d], wn[d], wc[d]);
#pragma unroll
      for (int e = 0; e < 3; ++e) wn[d][e] *= P.h[d]; // the value forms carry the cell size, the derivative forms do not
    }
    // entries beyond the lattice carry weight 0: clamp their index and keep the loops free of branches (27 independent loads)
    int jx[3], jy[3], jz[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      jx[e] = min(max(p0[0] + e, 0), P.ndp[0] - 1);
      jy[e] = min(max(p0[1] + e, 0), P.ndp[1] - 1);
      jz[e] = min(max(p0[2] + e, 0), P.ndp[2] - 1);
    }
    _Pragma("unroll 1") for (int s = 0; s < P.nsrc; ++s) { // (a run-time loop: only the destination loops need compile-time bounds)
      double g[3] = {0, 0, 0};
      const double *ps = P.p[s];
#pragma unroll
      for (int ez = 0; ez < 3; ++ez) { // separable sums (no table of the 81 weight products)
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int ey = 0; ey < 3; ++ey) {
          const double *row = ps + (long long)P.ndp[0] * (jy[ey] + (long long)P.ndp[1] * jz[ez]);
          double sc = 0.0, sn = 0.0;
#pragma unroll
          for (int ex = 0; ex < 3; ++ex) {
            const double pv = row[jx[ex]];
            sc = fma(wc[0][ex], pv, sc);
            sn = fma(wn[0][ex], pv, sn);
          }
          a0 = fma(wn[1][ey], sc, a0);
          a1 = fma(wc[1][ey], sn, a1);
          a2 = fma(wn[1][ey], sn, a2);
        }
        g[0] = fma(wn[2][ez], a0, g[0]);
        g[1] = fma(wn[2][ez], a1, g[1]);
        g[2] = fma(wc[2][ez], a2, g[2]);
        if constexpr (NO > 2) __builtin_amdgcn_sched_barrier(0); // (many destinations: nine loads in flight at a time keep the registers)
      }
      _Pragma("unroll") for (int o = 0; o < NO; ++o)
        if (o < P.nout)
          for (int c = 0; c < 3; ++c) acc[o][c] = fma(P.wKu[o][s], g[c], acc[o][c]);
    }
  } else {
    // FE_DGP(1), four functions per cell.  Per direction the node lies in up to two cells: slot 0 = the cell it is local node 1 (odd
    // index) or 2 (even index) of, slot 1 = the cell above an even node (local node 0).  A missing cell keeps a clamped index and
    // zero weights, so that the 8 x 4 coefficient loads are independent and the loops free of branches and of indexed reads of the
    // kernel arguments (round 3: the divergent loops over run-time slot counts took 55 us on 64^3 cells)
    int cell[3][2];
    double wN0[3][2], wN1[3][2], wC0[3][2], wC1[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int half = idx[d] >> 1;
      const bool odd = idx[d] & 1;
      const int below = odd ? half : half - 1;
      const bool v0 = below >= 0, v1 = !odd && half < nc[d];
      cell[d][0] = max(below, 0);
      cell[d][1] = min(half, nc[d] - 1);
      const double n0 = odd ? P.N[1][0] : P.N[2][0], n1 = odd ? P.N[1][1] : P.N[2][1];
      const double c0 = odd ? P.C[1][0] : P.C[2][0], c1 = odd ? P.C[1][1] : P.C[2][1];
      wN0[d][0] = v0 ? P.h[d] * n0 : 0.0;
      wN1[d][0] = v0 ? P.h[d] * n1 : 0.0;
      wC0[d][0] = v0 ? c0 : 0.0;
      wC1[d][0] = v0 ? c1 : 0.0;
      wN0[d][1] = v1 ? P.h[d] * P.N[0][0] : 0.0;
      wN1[d][1] = v1 ? P.h[d] * P.N[0][1] : 0.0;
      wC0[d][1] = v1 ? P.C[0][0] : 0.0;
      wC1[d][1] = v1 ? P.C[0][1] : 0.0;
    }
    _Pragma("unroll 1") for (int s = 0; s < P.nsrc; ++s) { // (a run-time loop: only the destination loops need compile-time bounds)
      double g[3] = {0, 0, 0};
#pragma unroll
      for (int ez = 0; ez < 2; ++ez)
#pragma unroll
        for (int ey = 0; ey < 2; ++ey)
#pragma unroll
          for (int ex = 0; ex < 2; ++ex) {
            const double *pc = P.p[s] + 4 * (cell[0][ex] + (long long)P.ncx * (cell[1][ey] + (long long)P.ncy * cell[2][ez]));
            const double q0 = pc[0], q1 = pc[1], q2 = pc[2], q3 = pc[3];
            const double Nx0 = wN0[0][ex], Nx1 = wN1[0][ex], Ny0 = wN0[1][ey], Ny1 = wN1[1][ey], Nz0 = wN0[2][ez], Nz1 = wN1[2][ez];
            const double Cx0 = wC0[0][ex], Cx1 = wC1[0][ex], Cy0 = wC0[1][ey], Cy1 = wC1[1][ey], Cz0 = wC0[2][ez], Cz1 = wC1[2][ez];
            // int (q0 + q1 l(xi) + q2 l(eta) + q3 l(zeta)) d phi / d x_c
            g[0] += (q0 * Cx0 + q1 * Cx1) * Ny0 * Nz0 + Cx0 * (q2 * Ny1 * Nz0 + q3 * Ny0 * Nz1);
            g[1] += (q0 * Cy0 + q2 * Cy1) * Nx0 * Nz0 + Cy0 * (q1 * Nx1 * Nz0 + q3 * Nx0 * Nz1);
            g[2] += (q0 * Cz0 + q3 * Cz1) * Nx0 * Ny0 + Cz0 * (q1 * Nx1 * Ny0 + q2 * Nx0 * Ny1);
          }
_Pragma("unroll") for (int o = 0; o < NO; ++o)
        if (o < P.nout)
          for (int c = 0; c < 3; ++c) acc[o][c] = fma(P.wKu[o][s], g[c], acc[o][c]);
    }
  }
_Pragma("unroll") for (int o = 0; o < NO; ++o)
    if (o < P.nout && P.out_u[o])
      for (int c = 0; c < 3; ++c) {
        if constexpr (NO <= 2) P.out_u[o][c * P.Nu + node] = old[o][c] - acc[o][c];
        else P.out_u[o][c * P.Nu + node] -= acc[o][c];
      }
}

// out_p[o] (=, +=) sum_s wKp[o][s] sum_c B_c u_s,c: one thread per pressure DoF (FE_Q(1) node / FE_DGP(1) cell function)
// (Five threads per FE_Q(1) node, one per z-plane of its 5 x 5 x 5 neighbourhood, with the partial sums added in LDS, measured
// slower: 79 against 62 us on 64^3 cells - the per-thread weight set-up is what one thread per node amortises.)
template <int NS, int NO, bool PDG>
__global__ __launch_bounds__(256, NO <= 2 ? 4 : 2) void stokes_div_kernel(const CouplingParams P, long long Np)
{
  const long long dof = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (dof >= Np) return;
  const int nc[3] = {P.ncx, P.ncy, P.ncz};
  double acc[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) acc[o] = 0.0;
  auto con = [&](int ix, int iy, int iz) {
    return ((P.dmask & 1) && ix == 0) || ((P.dmask & 2) && ix == P.ndu[0] - 1) || ((P.dmask & 4) && iy == 0) ||
           ((P.dmask & 8) && iy == P.ndu[1] - 1) || ((P.dmask & 16) && iz == 0) || ((P.dmask & 32) && iz == P.ndu[2] - 1);
  };
  if constexpr (!PDG) {
    const int j[3] = {int(dof % P.ndp[0]), int((dof / P.ndp[0]) % P.ndp[1]), int(dof / ((long long)P.ndp[0] * P.ndp[1]))};
    // velocity line nodes 2 j - 2 .. 2 j + 2: (cell j - 1: nodes 0, 1, 2 against psi_1), (cell j: nodes 0, 1, 2 against psi_0)
    double wn[3][5], wc[3][5];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const bool lo = j[d] > 0, hi = j[d] < nc[d];
      wn[d][0] = lo ? P.N[0][1] : 0.0; wn[d][1] = lo ? P.N[1][1] : 0.0; wn[d][2] = (lo ? P.N[2][1] : 0.0) + (hi ? P.N[0][0] : 0.0);
      wn[d][3] = hi ? P.N[1][0] : 0.0; wn[d][4] = hi ? P.N[2][0] : 0.0;
      wc[d][0] = lo ? P.C[0][1] : 0.0; wc[d][1] = lo ? P.C[1][1] : 0.0; wc[d][2] = (lo ? P.C[2][1] : 0.0) + (hi ? P.C[0][0] : 0.0);
      wc[d][3] = hi ? P.C[1][0] : 0.0; wc[d][4] = hi ? P.C[2][0] : 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) wn[d][k] *= P.h[d];
    }
    // nodes beyond the lattice and constrained nodes (they read as 0) carry weight 0: the loops are free of branches
    const int lim[3] = {P.ndu[0] - 1, P.ndu[1] - 1, P.ndu[2] - 1};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int i = 2 * j[d] - 2 + k;
        const bool off = i < 0 || i > lim[d] || ((P.dmask >> (2 * d) & 1) && i == 0) || ((P.dmask >> (2 * d + 1) & 1) && i == lim[d]);
        if (off) wn[d][k] = wc[d][k] = 0.0;
      }
    // (the y / z loops stay rolled: their weights are picked with selects on the wave-uniform loop counters, not indexed)
    auto pick = [](const double (&w)[5], int k) { return k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : (k == 3 ? w[3] : w[4]))); };
    int ixs[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) ixs[k] = min(max(2 * j[0] - 2 + k, 0), lim[0]);
    _Pragma("unroll 1") for (int s = 0; s < P.nsrc; ++s) {
      double dv = 0.0;
      const double *us = P.u[s];
      _Pragma("unroll 1") for (int kz = 0; kz < 5; ++kz) {
        const int iz = min(max(2 * j[2] - 2 + kz, 0), lim[2]);
        const double nz = pick(wn[2], kz), cz = pick(wc[2], kz);
        _Pragma("unroll 1") for (int ky = 0; ky < 5; ++ky) {
          const int iy = min(max(2 * j[1] - 2 + ky, 0), lim[1]);
          const double ny = pick(wn[1], ky), cy = pick(wc[1], ky);
          const double *row = us + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz);
          double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
          for (int kx = 0; kx < 5; ++kx) {
            const double *uu = row + ixs[kx];
            sx = fma(wc[0][kx], uu[0], sx);
            sy = fma(wn[0][kx], uu[P.Nu], sy);
            sz = fma(wn[0][kx], uu[2 * P.Nu], sz);
          }
          dv = fma(ny * nz, sx, fma(cy * nz, sy, fma(ny * cz, sz, dv)));
        }
      }
      _Pragma("unroll") for (int o = 0; o < NO; ++o)
        if (o < P.nout) acc[o] = fma(P.wKp[o][s], dv, acc[o]);
    }
  } else {
    const long long cell = dof >> 2;
    const int fn = int(dof & 3);
    const int cx = int(cell % P.ncx), cy = int((cell / P.ncx) % P.ncy), cz = int(cell / ((long long)P.ncx * P.ncy));
    _Pragma("unroll 1") for (int s = 0; s < P.nsrc; ++s) { // (a run-time loop: only the destination loops need compile-time bounds)
      double dv = 0.0;
      for (int az = 0; az < 3; ++az)
        for (int ay = 0; ay < 3; ++ay)
          for (int ax = 0; ax < 3; ++ax) {
            const int ix = 2 * cx + ax, iy = 2 * cy + ay, iz = 2 * cz + az;
            if (con(ix, iy, iz)) continue;
            const double *uu = P.u[s] + (ix + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz));
            // test function fn: 1 / l(xi) / l(eta) / l(zeta): index 1 of N / C in that direction
            const int fx = fn == 1, fy = fn == 2, fz = fn == 3;
            const double Nx = P.h[0] * P.N[ax][fx], Ny = P.h[1] * P.N[ay][fy], Nz = P.h[2] * P.N[az][fz];
            dv = fma(P.C[ax][fx] * Ny * Nz, uu[0], dv);
            dv = fma(Nx * P.C[ay][fy] * Nz, uu[P.Nu], dv);
            dv = fma(Nx * Ny * P.C[az][fz], uu[2 * P.Nu], dv);
          }
      _Pragma("unroll") for (int o = 0; o < NO; ++o)
        if (o < P.nout) acc[o] = fma(P.wKp[o][s], dv, acc[o]);
    }
  }
  _Pragma("unroll") for (int o = 0; o < NO; ++o)
    if (o < P.nout && P.out_p[o]) {
      if (P.store_p[o]) P.out_p[o][dof] = acc[o];
      else P.out_p[o][dof] += acc[o];
    }
}

// FE_DGP(1): one thread per CELL computes the cell's four pressure rows from its 27 x 3 velocity values (the one-thread-per-DoF form
// above reads them four times: 157 us beside the sweep on 64^3 cells)
template <int NS, int NO>
__global__ __launch_bounds__(256, 2) void stokes_div_dgp_cell_kernel(const CouplingParams P, long long ncells)
{
  const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncells) return;
  const int cx = int(cell % P.ncx), cy = int((cell / P.ncx) % P.ncy), cz = int(cell / ((long long)P.ncx * P.ncy));
  double acc[NO][4];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[o][f] = 0.0;
  _Pragma("unroll 1") for (int s = 0; s < P.nsrc; ++s) {
    double dv[4] = {0.0, 0.0, 0.0, 0.0};
    const double *us = P.u[s];
    _Pragma("unroll 1") for (int az = 0; az < 3; ++az) { // (the z and y loops stay rolled: nine loads in flight, a few dozen registers)
      const int iz = 2 * cz + az;
      const bool conz = ((P.dmask & 16) && iz == 0) || ((P.dmask & 32) && iz == P.ndu[2] - 1);
      const double Nz0 = P.h[2] * P.N[az][0], Nz1 = P.h[2] * P.N[az][1], Cz0 = P.C[az][0], Cz1 = P.C[az][1];
      _Pragma("unroll 1") for (int ay = 0; ay < 3; ++ay) {
        const int iy = 2 * cy + ay;
        const bool cony = conz || ((P.dmask & 4) && iy == 0) || ((P.dmask & 8) && iy == P.ndu[1] - 1);
        const double Ny0 = P.h[1] * P.N[ay][0], Ny1 = P.h[1] * P.N[ay][1], Cy0 = P.C[ay][0], Cy1 = P.C[ay][1];
        const double *row = us + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz) + 2 * cx;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          const int ix = 2 * cx + ax;
          const bool con = cony || ((P.dmask & 1) && ix == 0) || ((P.dmask & 2) && ix == P.ndu[0] - 1);
          const double ux = con ? 0.0 : row[ax], uy = con ? 0.0 : row[P.Nu + ax], uz = con ? 0.0 : row[2 * P.Nu + ax];
          const double Nx0 = P.h[0] * P.N[ax][0], Nx1 = P.h[0] * P.N[ax][1], Cx0 = P.C[ax][0], Cx1 = P.C[ax][1];
          // test functions 1, l(xi), l(eta), l(zeta): index 1 of N / C in that direction
          dv[0] += Cx0 * Ny0 * Nz0 * ux + Nx0 * Cy0 * Nz0 * uy + Nx0 * Ny0 * Cz0 * uz;
          dv[1] += Cx1 * Ny0 * Nz0 * ux + Nx1 * Cy0 * Nz0 * uy + Nx1 * Ny0 * Cz0 * uz;
          dv[2] += Cx0 * Ny1 * Nz0 * ux + Nx0 * Cy1 * Nz0 * uy + Nx0 * Ny1 * Cz0 * uz;
          dv[3] += Cx0 * Ny0 * Nz1 * ux + Nx0 * Cy0 * Nz1 * uy + Nx0 * Ny0 * Cz1 * uz;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (o < P.nout)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[o][f] = fma(P.wKp[o][s], dv[f], acc[o][f]);
  }
#pragma unroll
  for (int o = 0; o < NO; ++o)
    if (o < P.nout && P.out_p[o]) {
      double *q = P.out_p[o] + 4 * cell;
#pragma unroll
      for (int f = 0; f < 4; ++f) q[f] = P.store_p[o] ? acc[o][f] : q[f] + acc[o][f];
    }
}

// The same for FE_Q(1) as a MARCH along z: a thread takes DIV_SEG consecutive pressure nodes of a z-line and keeps, per velocity
// z-plane of its 5 x 5 (x, y) neighbourhood, the two partial sums the nodes above and below share (s1 = sum of the in-plane terms of
// the x and y components, s2 = of the z component): two new planes per node instead of five, 2.5 x fewer loads, and a twentieth of
// the threads - the kernel runs beside the velocity sweep, where every instruction it issues competes with the sweep's.
constexpr int DIV_SEG = 4;
template <int NS, int NO>
__global__ __launch_bounds__(256, 2) void stokes_div_march_kernel(const CouplingParams P, int nseg)
{
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long ncol = (long long)P.ndp[0] * P.ndp[1];
  if (t >= ncol * nseg) return;
  const int jx = int(t % P.ndp[0]), jy = int((t / P.ndp[0]) % P.ndp[1]), seg = int(t / ncol);
  const int nc[3] = {P.ncx, P.ncy, P.ncz};
  const int lim[3] = {P.ndu[0] - 1, P.ndu[1] - 1, P.ndu[2] - 1};
  const int jxy[2] = {jx, jy};
  // in-plane weights of this line: velocity line nodes 2 j - 2 .. 2 j + 2 (cell j - 1 against psi_1, cell j against psi_0); nodes beyond
  // the lattice and constrained nodes carry weight 0
  double wn[2][5], wc[2][5];
  int idx[2][5];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const bool lo = jxy[d] > 0, hi = jxy[d] < nc[d];
    wn[d][0] = lo ? P.N[0][1] : 0.0; wn[d][1] = lo ? P.N[1][1] : 0.0; wn[d][2] = (lo ? P.N[2][1] : 0.0) + (hi ? P.N[0][0] : 0.0);
    wn[d][3] = hi ? P.N[1][0] : 0.0; wn[d][4] = hi ? P.N[2][0] : 0.0;
    wc[d][0] = lo ? P.C[0][1] : 0.0; wc[d][1] = lo ? P.C[1][1] : 0.0; wc[d][2] = (lo ? P.C[2][1] : 0.0) + (hi ? P.C[0][0] : 0.0);
    wc[d][3] = hi ? P.C[1][0] : 0.0; wc[d][4] = hi ? P.C[2][0] : 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = 2 * jxy[d] - 2 + k;
      const bool off = i < 0 || i > lim[d] || ((P.dmask >> (2 * d) & 1) && i == 0) || ((P.dmask >> (2 * d + 1) & 1) && i == lim[d]);
      wn[d][k] = off ? 0.0 : wn[d][k] * P.h[d];
      wc[d][k] = off ? 0.0 : wc[d][k];
      idx[d][k] = min(max(i, 0), lim[d]);
    }
  }
  // the two partial sums of velocity plane iz (0 beyond the lattice and on constrained planes)
  auto plane = [&](int s, int iz, double &s1, double &s2) {
    s1 = s2 = 0.0;
    const bool off = iz < 0 || iz > lim[2] || ((P.dmask & 16) && iz == 0) || ((P.dmask & 32) && iz == lim[2]);
    if (off) return; // (wave-uniform for a launch whose threads of a wave share the segment)
    const double *us = P.u[s] + (long long)P.ndu[0] * P.ndu[1] * iz;
    _Pragma("unroll 1") for (int ky = 0; ky < 5; ++ky) {
      const double *row = us + (long long)P.ndu[0] * idx[1][ky];
      const double ny = ky == 0 ? wn[1][0] : (ky == 1 ? wn[1][1] : (ky == 2 ? wn[1][2] : (ky == 3 ? wn[1][3] : wn[1][4])));
      const double cy = ky == 0 ? wc[1][0] : (ky == 1 ? wc[1][1] : (ky == 2 ? wc[1][2] : (ky == 3 ? wc[1][3] : wc[1][4])));
      double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const double *uu = row + idx[0][kx];
        sx = fma(wc[0][kx], uu[0], sx);
        sy = fma(wn[0][kx], uu[P.Nu], sy);
        sz = fma(wn[0][kx], uu[2 * P.Nu], sz);
      }
      s1 = fma(ny, sx, fma(cy, sy, s1));
      s2 = fma(ny, sz, s2);
    }
  };
  const int j0 = int((long long)P.ndp[2] * seg / nseg), j1 = int((long long)P.ndp[2] * (seg + 1) / nseg);
  double s1[NS][5], s2[NS][5]; // planes 2 j - 2 .. 2 j + 2 of the current node
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int k = 0; k < 5; ++k) s1[s][k] = s2[s][k] = 0.0;
  for (int j = j0; j < j1; ++j) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (s < P.nsrc) {
        if (j == j0) {
#pragma unroll
          for (int k = 0; k < 3; ++k) plane(s, 2 * j - 2 + k, s1[s][k], s2[s][k]);
        }
        plane(s, 2 * j + 1, s1[s][3], s2[s][3]);
        plane(s, 2 * j + 2, s1[s][4], s2[s][4]);
      }
    const bool lo = j > 0, hi = j < nc[2];
    const double wnz[5] = {lo ? P.N[0][1] : 0.0, lo ? P.N[1][1] : 0.0, (lo ? P.N[2][1] : 0.0) + (hi ? P.N[0][0] : 0.0), hi ? P.N[1][0] : 0.0, hi ? P.N[2][0] : 0.0};
    const double wcz[5] = {lo ? P.C[0][1] : 0.0, lo ? P.C[1][1] : 0.0, (lo ? P.C[2][1] : 0.0) + (hi ? P.C[0][0] : 0.0), hi ? P.C[1][0] : 0.0, hi ? P.C[2][0] : 0.0};
    double acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (s < P.nsrc) {
        double dv = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) dv = fma(P.h[2] * wnz[k], s1[s][k], fma(wcz[k], s2[s][k], dv));
#pragma unroll
        for (int o = 0; o < NO; ++o)
          if (o < P.nout) acc[o] = fma(P.wKp[o][s], dv, acc[o]);
      }
    const long long dof = jx + (long long)P.ndp[0] * (jy + (long long)P.ndp[1] * j);
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (o < P.nout && P.out_p[o]) {
        if (P.store_p[o]) P.out_p[o][dof] = acc[o];
        else P.out_p[o][dof] += acc[o];
      }
    // the next node shares planes 2 j .. 2 j + 2
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int k = 0; k < 3; ++k) { s1[s][k] = s1[s][k + 2]; s2[s][k] = s2[s][k + 2]; }
  }
}

} // namespace

// The instantiation a launch fits in: shape 0 .. 3 = the compile-time bounds <sources, destinations> <1, 1>, <2, 2>, <MAXSRC, 4>,
// <MAXSRC, MAXOUT>; f is called with the two bounds as integral constants
static int coupling_shape(const CouplingParams &k)
{
  return (k.nsrc == 1 && k.nout == 1) ? 0 : ((k.nsrc <= 2 && k.nout <= 2) ? 1 : (k.nout <= 4 ? 2 : 3));
}
template <class F>
static void with_coupling_bounds(const CouplingParams &k, F f)
{
  std::integral_constant<int, MAXSRC> ns;
  switch (coupling_shape(k)) {
  case 0: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 1>());
  case 1: return f(std::integral_constant<int, 2>(), std::integral_constant<int, 2>());
  case 2: return f(ns, std::integral_constant<int, 4>());
  default: return f(ns, std::integral_constant<int, MAXOUT>());
  }
}

void stokes_grad_launch(const CouplingParams &k, hipStream_t st)
{
  const dim3 grid((unsigned)((k.Nu + 255) / 256)), block(256);
  with_coupling_bounds(k, [&](auto ns, auto no) {
    if (k.pdg) hipLaunchKernelGGL((stokes_grad_kernel<ns(), no(), true>), grid, block, 0, st, k);
    else hipLaunchKernelGGL((stokes_grad_kernel<ns(), no(), false>), grid, block, 0, st, k);
  });
}

void stokes_div_launch(const CouplingParams &k, long long Np, hipStream_t st)
{
  const int shape = coupling_shape(k);
  static const bool div_gather = [] { const char *e = getenv("STFEM_STOKES_DIV_GATHER"); return e && atoi(e) != 0; }();
  if (k.pdg && shape <= 1 && !div_gather) { // FE_DGP(1), up to two time dofs: one thread per cell
    const long long ncells = (long long)k.ncx * k.ncy * k.ncz;
    const unsigned g = (unsigned)((ncells + 255) / 256);
    if (shape == 0) hipLaunchKernelGGL((stokes_div_dgp_cell_kernel<1, 1>), dim3(g), dim3(256), 0, st, k, ncells);
    else hipLaunchKernelGGL((stokes_div_dgp_cell_kernel<2, 2>), dim3(g), dim3(256), 0, st, k, ncells);
    return;
  }
  if (!k.pdg && shape <= 1 && !div_gather) { // FE_Q(1), up to two time dofs: the march along z
    const int nseg = std::max(1, (k.ndp[2] + DIV_SEG - 1) / DIV_SEG);
    const long long nthreads = (long long)k.ndp[0] * k.ndp[1] * nseg;
    const unsigned g = (unsigned)((nthreads + 255) / 256);
    if (shape == 0) hipLaunchKernelGGL((stokes_div_march_kernel<1, 1>), dim3(g), dim3(256), 0, st, k, nseg);
    else hipLaunchKernelGGL((stokes_div_march_kernel<2, 2>), dim3(g), dim3(256), 0, st, k, nseg);
    return;
  }
  const dim3 grid((unsigned)((Np + 255) / 256)), block(256);
  with_coupling_bounds(k, [&](auto ns, auto no) {
    if (k.pdg) hipLaunchKernelGGL((stokes_div_kernel<ns(), no(), true>), grid, block, 0, st, k, Np);
    else hipLaunchKernelGGL((stokes_div_kernel<ns(), no(), false>), grid, block, 0, st, k, Np);
  });
}
