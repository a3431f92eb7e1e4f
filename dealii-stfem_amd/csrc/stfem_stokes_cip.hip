// Stokes two-field operator: the CIP (continuous interior penalty) gradient-jump stabilisation on the interior faces, what
//   StokesMatrixFreeOperator::do_face_integral_local (reference include/operators.h:1605-1633) adds when delta0 != 0:
//   C(w; u)(v) = sum_F int_F delta_F(w) [d_n u] . [d_n v] dA,     [d_n u] = (grad u|_A - grad u|_B) n,
//   delta_F(w) = delta0 h_F^2 / pa (w.n)^2 at each face point,    h_F = sqrt(sum_q JxW_face) (get_h_face, 182-209),  pa = 2^3.5.
// The face rule is QGauss(3)^2, the mapping MappingQ1; entries of u and w on strongly constrained DoFs read as 0, constrained rows
// and the pressure rows receive nothing.  The weight velocity w is an argument of its own (the reference reads it from the source of
// the vmult, 1623; see stfem_stokes_set_cip).
// Cell-centric: a cell computes, for each of its up to six interior faces, the jump at the nine face points - its own normal
// derivative minus the neighbour's, each with its own cell's Jacobian - and adds ONLY its own side's test contribution
//   + delta_F ([d_n u]_own - [d_n u]_other) d_n v_own JxW     (the interior side's + and the exterior side's - of 1628-1629)
// to its own 27 nodes.  n, JxW, h_F and w at the face are those of the cell's own side: the face is one bilinear patch, so both
// sides compute the same surface element |det J| |J^-T e_d| and the same normal up to its sign, which enters squared.  The cell
// reads the neighbour's 81 source values: safe while other colours write, a source is never a destination.  (A face-pair kernel
// would scatter to 45 nodes of two cells and need 12 colours per direction.)
// The launches follow those of the linear operator and of the convection term of the same set: every destination has been written,
// so they read, add and write - eight colour launches (cells of one colour share no DoF), ascending, faces 0..5 and points 0..8 in
// order, no atomics: bitwise reproducible.
// On a z-slab of a partitioned mesh (stfem_stokes_set_cip_neighbours) the same design partitions: the cells next to an interface plane
// treat that face as interior, read the neighbour slab's cell from two ghost DoF planes per source (stfem_stokes_cip_pack on the
// sender) and one ghost vertex plane, and write inside the slab - partial sums in the interface planes, like every other launch.
// Velocity degree 3 (the _space entries of stfem_stokes_cip_space.h): the same design - cell-centric, own side only, eight colour
// launches, no atomics - in a kernel of its own, stokes_cip_q3_kernel below: 64 nodes, the 16 points of QGauss(4)^2 per face,
// pa = 3^3.5, one wave per cell, the normal derivatives from the 1D tables instead of a tabulated sT.  No slabs at degree 3.
// STFEM_STOKES_CIP_WORKGROUPS caps the workgroups of the colour launches at either degree; stfem_stokes_last_cip_plan reports the last
// launch (stfem_stokes_cip_plan.h).
#include "stfem_stokes_internal.h"
#include "stfem_stokes_cip_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>
#include <type_traits>

namespace {

// One half-wave per cell, 256 threads = 8 cells at a time, the cells of one colour dealt round-robin to the half-waves
// (the layout of stokes_inflow_kernel).  The reference-space derivatives of the 27 shape functions at the nine points of the six
// faces are tabulated in LDS once per workgroup (sT[e][f][q][n]; CART keeps d/d xi_d alone: 11.4 KB, otherwise all three: 34 KB).
// Per source and interior face: 27 lanes gather the neighbour's values; the 27 lanes as (face point q, component) evaluate the
// geometry of q (the three component lanes redundantly, rather than idle), the normal derivatives of their component on both sides as
// sums over the table rows, w.n and the flux; the 27 node lanes integrate with the same table rows.
// CART: constant diagonal Jacobian, n = e_d.  MULTI: several sources, each with its own weight velocity; the weighted results
// are summed in registers per destination (up to MAXSRC), one scatter; otherwise one source, the weights applied at scatter time to
// up to MAXOUT destinations.
// SLAB: a z-slab with neighbours (CipSlabParams).  Face 4 of the bottom cell layer / face 5 of the top one is interior where
// `neighbours` names that side; the neighbour cell's 18 nodes beyond the interface plane come from the ghost planes of the source, its
// Jacobian from the two-plane vertex arrays.  The destination writes stay what they are: inside the slab.
template <bool CART, bool MULTI, bool SLAB = false>
__global__ __launch_bounds__(256) void stokes_cip_kernel(const std::conditional_t<SLAB, CipSlabParams, CipParams> prm)
{
  constexpr int NT = CART ? 1 : 3;
  __shared__ double tS[9], tD[9], tE[6], tED[6], tX[3], tW[3];
  __shared__ double sT[NT][6][9][27];                // d phi_n / d xi_e at point q of face f (CART: e = the face's direction)
  __shared__ double sU[8][81], sW[8][81], sN[8][81]; // own source, own weight velocity, the neighbour's source
  __shared__ double sF[8][9][6], sA[8][9];           // per face point: flux[3] and J^-1 n [3]; JxW
  if (threadIdx.x < 9) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < 6) { tE[threadIdx.x] = prm.Eu[threadIdx.x]; tED[threadIdx.x] = prm.EDu[threadIdx.x]; }
  if (threadIdx.x < 3) { tX[threadIdx.x] = prm.xq[threadIdx.x]; tW[threadIdx.x] = prm.wq[threadIdx.x]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 6 * 9 * 27; i += 256) {
    const int n = i % 27, q = (i / 27) % 9, f = i / 243;
    const int d = f >> 1;
    double g0, g1, g2;
    cip_face_gradient(tS, tD, tE, tED, f, q, n, g0, g1, g2);
    if constexpr (CART) {
      sT[0][f][q][n] = d == 0 ? g0 : (d == 1 ? g1 : g2);
    } else {
      sT[0][f][q][n] = g0; sT[NT - 1 > 0 ? 1 : 0][f][q][n] = g1; sT[NT - 1][f][q][n] = g2;
    }
  }
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  const int q = t % 9, comp_q = t / 9, q1 = q % 3, q2 = q / 3; // the point phase: this lane's face point and component
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  double *U = sU[slot], *Wv = sW[slot], *N = sN[slot];
  for (long long item = (long long)blockIdx.x * 8 + slot; item - slot < ncells; item += (long long)gridDim.x * 8) {
    const bool ok = item < ncells;
    const long long cc = ok ? item : 0;
    const int cx = 2 * int(cc % ncxc) + px, cy = 2 * int((cc / ncxc) % ncyc) + py, cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    int faces = 0; // the interior faces of the cell, bit 2 d + s
    if (ok) faces = (cx > 0 ? 1 : 0) | (cx < prm.ncx - 1 ? 2 : 0) | (cy > 0 ? 4 : 0) | (cy < prm.ncy - 1 ? 8 : 0) | (cz > 0 ? 16 : 0) |
                    (cz < prm.ncz - 1 ? 32 : 0);
    if constexpr (SLAB) {
      if (ok) faces |= (cz == 0 ? prm.neighbours & 16 : 0) | (cz == prm.ncz - 1 ? prm.neighbours & 32 : 0);
    }
    if (!__builtin_amdgcn_readfirstlane(__ballot(faces != 0) != 0)) continue; // (wave-uniform skip only: the two half-waves fence together)
    const int ix = 2 * cx + a, iy = 2 * cy + b, iz = 2 * cz + c;
    const bool con = constrained_u(prm, ix, iy, iz);
    const long long gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    double accU[MULTI ? MAXSRC : 1][3];
#pragma unroll
    for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = 0.0;
    const int nsrc = MULTI ? prm.nsrc : 1;
    for (int src = 0; src < nsrc; ++src) {
      const double *us = prm.us[src], *ws = prm.ws[src];
      if (lane27) { // gather (read_dof_values: constrained entries read as 0)
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) {
          U[comp * 27 + t] = (ok && !con) ? us[comp * prm.Nu + gu] : 0.0;
          Wv[comp * 27 + t] = (ok && !con) ? ws[comp * prm.Nu + gu] : 0.0;
        }
      }
      // the source values of the neighbour behind face f (read_dof_values: constrained entries read as 0)
      auto neighbour = [&](int f, double v[3]) {
        const int d = f >> 1, s = f & 1;
        const int jx = 2 * (cx + (d == 0 ? (s ? 1 : -1) : 0)) + a, jy = 2 * (cy + (d == 1 ? (s ? 1 : -1) : 0)) + b,
                  jz = 2 * (cz + (d == 2 ? (s ? 1 : -1) : 0)) + c;
        const bool take = (faces >> f & 1) && lane27 && !constrained_u(prm, jx, jy, jz);
        const long long gn = jx + (long long)prm.ndu[0] * (jy + (long long)prm.ndu[1] * jz);
        if constexpr (SLAB) {
          // Behind an interface face jz = 2 (cz -+ 1) + c leaves the slab.  Face 4 is on only with cz == 0 and bit 4 (see `faces`):
          // jz = c - 2 in {-2, -1, 0}; 0 is the slab's own plane, -2 and -1 are ghost planes jz + 2 in {0, 1} of ghost_lo.  Face 5
          // is on only with cz == ncz - 1 and bit 5: jz = ndu[2] - 1 + c; c == 0 is the slab's own top plane, c in {1, 2} gives
          // ghost planes jz - ndu[2] in {0, 1} of ghost_hi.  With jx in [0, ndu[0]) and jy in [0, ndu[1]) (the x / y faces of the
          // same `take` are on only inside the slab) the index (comp * 2 + plane) ndu[0] ndu[1] + jy ndu[0] + jx lies in
          // [0, 3 * 2 * ndu[0] ndu[1]) = [0, stfem_stokes_cip_ghost_size).  No other face leaves [0, ndu[2]).  The sender has written
          // 0 on the DoFs its z mask constrains; constrained_u below sees the x / y masks, which both slabs share.
          if (d == 2 && (jz < 0 || jz >= prm.ndu[2])) {
            const double *g = jz < 0 ? prm.ghost_lo[MULTI ? src : 0] : prm.ghost_hi[MULTI ? src : 0];
            const long long plane = (long long)prm.ndu[0] * prm.ndu[1];
            const long long gg = (jz < 0 ? jz + 2 : jz - prm.ndu[2]) * plane + jx + (long long)prm.ndu[0] * jy;
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) v[comp] = take ? g[comp * 2 * plane + gg] : 0.0;
            return;
          }
        }
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) v[comp] = take ? us[comp * prm.Nu + gn] : 0.0;
      };
      // CART: all six fetched before the first face is worked on (one memory latency, not six: 1.22 -> 1.16 ms on 64^3 cells); the
      // general kernel has no registers to hold them (with them it ran at one wave per SIMD: 2.9 -> 4.1 ms) and fetches face by face
      double nb[CART ? 6 : 1][3];
      if constexpr (CART) {
#pragma unroll
        for (int f = 0; f < 6; ++f) neighbour(f, nb[f]);
      }
      wave_fence();
      double rU[3] = {0, 0, 0};
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const bool on = faces >> f & 1; // per half-wave
        if (!__builtin_amdgcn_readfirstlane(__ballot(on) != 0)) continue;
        const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0;
        const int ncx_ = cx + (d == 0 ? (s ? 1 : -1) : 0), ncy_ = cy + (d == 1 ? (s ? 1 : -1) : 0), ncz_ = cz + (d == 2 ? (s ? 1 : -1) : 0);
        if constexpr (!CART) neighbour(f, nb[0]);
        if (lane27) {
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) N[comp * 27 + t] = nb[CART ? f : 0][comp];
        }
        wave_fence();
        double go[3] = {0, 0, 0}, wn = 0.0, JxW = 0.0, jump = 0.0;
        if (on && lane27) { // this lane's face point and component: geometry, normal derivatives of both sides, w.n
          double gnb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0};
          if constexpr (CART) {
            nrm[d] = 1.0;
            go[d] = gnb[d] = prm.hinv[d];
            JxW = prm.detJ * prm.hinv[d] * tW[q1] * tW[q2];
          } else {
            double xi[3], Ji[3][3], det;
#pragma unroll
            for (int k = 0; k < 3; ++k) xi[k] = k == d ? double(s) : tX[k == t1 ? q1 : q2];
            det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
            const double len = mapping_q1_face_normal(Ji, d, 0, nrm); // J^-T e_d, unsigned
            JxW = fabs(det) * len * tW[q1] * tW[q2];
#pragma unroll
            for (int e = 0; e < 3; ++e) go[e] = Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2];
            xi[d] = double(1 - s);
            if constexpr (SLAB) {
              // the neighbour cell of an interface face (ncz_ == -1 or ncz, on only with its bit: the array is there) is cell layer
              // 0 of the side's two vertex planes: reads 3 ((cx + i) + (ncx + 1) ((cy + j) + (ncy + 1) k)), k in {0, 1}, inside
              // 2 (ncx + 1) (ncy + 1) * 3
              const bool below = ncz_ < 0, beyond = below || ncz_ >= prm.ncz;
              const double *vertices = beyond ? prm.ghost_vertices[below ? 0 : 1] : prm.vertices;
              det = mapping_q1_inverse(vertices, prm.ncx, prm.ncy, ncx_, ncy_, beyond ? 0 : ncz_, xi, Ji);
            } else {
              det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, ncx_, ncy_, ncz_, xi, Ji);
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) gnb[e] = Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2];
          }
          // reference-space derivatives of this lane's component at the point: this side (face f) and the neighbour's (face f ^ 1)
          const double *Uc = U + comp_q * 27, *Nc = N + comp_q * 27;
#pragma unroll
          for (int e = 0; e < NT; ++e) {
            const double *To = sT[e][f][q], *Tn = sT[e][f ^ 1][q];
            double so = 0.0, sn = 0.0;
#pragma unroll 3
            for (int n = 0; n < 27; ++n) { so = fma(To[n], Uc[n], so); sn = fma(Tn[n], Nc[n], sn); }
            jump += go[CART ? d : e] * so - gnb[CART ? d : e] * sn;
          }
          // w at the point: the nine nodes of the face
          double wval[3] = {0, 0, 0};
#pragma unroll
          for (int j2 = 0; j2 < 3; ++j2)
#pragma unroll
            for (int j1 = 0; j1 < 3; ++j1) {
              const int k0 = d == 0 ? 2 * s : (t1 == 0 ? j1 : j2), k1 = d == 1 ? 2 * s : (t1 == 1 ? j1 : j2), k2 = d == 2 ? 2 * s : j2;
              const double phi = tS[q1 * 3 + j1] * tS[q2 * 3 + j2];
#pragma unroll
              for (int c3 = 0; c3 < 3; ++c3) wval[c3] = fma(phi, Wv[c3 * 27 + k0 + 3 * k1 + 9 * k2], wval[c3]);
            }
          wn = wval[0] * nrm[0] + wval[1] * nrm[1] + wval[2] * nrm[2];
          if (comp_q == 0) sA[slot][q] = JxW;
        }
        wave_fence();
        if (on && lane27) { // h_F^2 = the face's area: the nine JxW in point order
          double area = 0.0;
#pragma unroll
          for (int p = 0; p < 9; ++p) area += sA[slot][p];
          const double delta = prm.scale * area * wn * wn;
          sF[slot][q][comp_q] = delta * jump * JxW;
          if (comp_q == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) sF[slot][q][3 + e] = go[e];
          }
        }
        wave_fence();
        if (on && lane27) { // integrate: the normal derivative of the test function of node (a, b, c), this cell's side
#pragma unroll
          for (int p = 0; p < 9; ++p) {
            const double *F = sF[slot][p];
            double dv;
            if constexpr (CART) dv = F[3 + d] * sT[0][f][p][t];
            else dv = F[3] * sT[0][f][p][t] + F[4] * sT[NT - 1 > 0 ? 1 : 0][f][p][t] + F[5] * sT[NT - 1][f][p][t];
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) rU[comp] = fma(dv, F[comp], rU[comp]);
          }
        }
        wave_fence(); // the next face reuses the neighbour and point buffers
      }
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(prm.wKu[src][o], rU[comp], accU[o][comp]);
          }
      } else {
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) accU[0][comp] = rU[comp];
      }
      wave_fence(); // the next source overwrites U, Wv
    }
    // distribute_local_to_global (add): constrained velocity rows are not written
    if (ok && lane27 && !con) {
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
            double *dptr = prm.out_u[o] + gu;
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += accU[o][comp];
          }
      } else {
        for (int o = 0; o < prm.nout; ++o) {
          double *dptr = prm.out_u[o] + gu;
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += prm.wKu[0][o] * accU[0][comp];
        }
      }
    }
  }
}

// Velocity degree 3: FE_Q(3), 64 nodes, the 4 x 4 Gauss points of a face, pa = 3^3.5.  A kernel beside the degree-2 one, not an
// instantiation of it: that kernel is built on 27 nodes = 9 points x 3 components on one half-wave and on the
// tabulated sT, neither of which exists here, so a shared body would be two bodies under if constexpr and would put the degree-2
// arithmetic, which must not move, at the mercy of every later edit of the degree-3 one.
// One wave per cell and one wave per workgroup (64 threads: nothing is shared between cells but 448 B of 1D tables, so a larger
// workgroup would buy nothing, and a colour of few cells still spreads over the CUs), lane t = a + 4 b + 16 c is node (a, b, c).
// No derivative table: sT[3][6][16][64]
// is 147 KB and leaves no room for the per-wave buffers.  The normal derivative is built from the 1D tables instead (Su, Du at the
// Gauss points, Eu, EDu at the end points: 448 B): d phi_n / d xi_e of node n = (kd, k1, k2) at face point (q1, q2) is a product of
// three 1D entries, so a point sums over kd first (4 fma per derivative and side) and then over the 16 (k1, k2) with the tangential
// 1D values: 16 x (16 + 12) fma per (point, component) in place of 6 x 64 table reads, and the LDS holds the three 192-value
// buffers of a cell and the 16 point records (5.7 KB per workgroup; 13.6 KB on a general mesh with the face geometry sG).
// Per source and interior face: the 64 lanes gather the neighbour's 3 x 64 values; lanes 0..47 as (face point q = t & 15, component
// t >> 4) evaluate the geometry of q (the three component lanes redundantly), the normal derivatives of their component on both sides,
// w.n from the 16 nodes of the face and the flux; the 64 node lanes integrate, again from the 1D tables.  CART / MULTI as at degree 2;
// on a general mesh the geometry of the face points is evaluated once per cell, before the sources (sG, 7.7 KB more).
// No array is indexed at run time: the face loop is unrolled, so directions, strides and end points are constants of each copy.
template <bool CART, bool MULTI>
__global__ __launch_bounds__(64) void stokes_cip_q3_kernel(const CipQ3Params prm)
{
  __shared__ double tS[16], tD[16], tE[8], tED[8], tX[4], tW[4];
  __shared__ double sU[192], sW[192], sN[192]; // own source, own weight velocity, the neighbour's source
  __shared__ double sF[16][6], sA[16];         // per face point: flux[3] and J^-1 n [3]; JxW
  __shared__ double sG[CART ? 1 : 6 * 16 * 10]; // general meshes, per face and point: JxW, n [3], J^-1 n of this side [3] and of the neighbour's [3]
  if (threadIdx.x < 16) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < 8) { tE[threadIdx.x] = prm.Eu[threadIdx.x]; tED[threadIdx.x] = prm.EDu[threadIdx.x]; }
  if (threadIdx.x < 4) { tX[threadIdx.x] = prm.xq[threadIdx.x]; tW[threadIdx.x] = prm.wq[threadIdx.x]; }
  __syncthreads();
  const int t = threadIdx.x;
  const int a = t & 3, b = (t >> 2) & 3, c = t >> 4;
  const bool point = t < 48;                                             // the point phase: 16 points x 3 components
  const int q = t & 15, comp_q = point ? t >> 4 : 0, q1 = q & 3, q2 = q >> 2;
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  double *U = sU, *Wv = sW, *N = sN;
  for (long long item = blockIdx.x; item < ncells; item += gridDim.x) {
    const int cx = 2 * int(item % ncxc) + px, cy = 2 * int((item / ncxc) % ncyc) + py, cz = 2 * int(item / ((long long)ncxc * ncyc)) + pz;
    // the interior faces of the cell, bit 2 d + s: one cell per wave, so a scalar
    const int faces = __builtin_amdgcn_readfirstlane((cx > 0 ? 1 : 0) | (cx < prm.ncx - 1 ? 2 : 0) | (cy > 0 ? 4 : 0) | (cy < prm.ncy - 1 ? 8 : 0) |
                                                     (cz > 0 ? 16 : 0) | (cz < prm.ncz - 1 ? 32 : 0));
    if (faces == 0) continue;
    const int ix = 3 * cx + a, iy = 3 * cy + b, iz = 3 * cz + c;
    const bool con = constrained_u(prm, ix, iy, iz);
    const long long gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    if constexpr (!CART) {
      // The geometry of the 16 points of the interior faces, once per cell and point - not per source and component lane: 96 (face,
      // point) items on the 64 lanes.  The face is a lane's own here, so direction and side are selects (stfem_mapping_q1.h) and the
      // vertices of the two cells come by vector loads; inside the source loop they held the scalar registers of that loop.
#pragma unroll 1
      for (int item = t; item < 96; item += 64) {
        const int f = item >> 4, d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0, g1 = item & 3, g2 = (item >> 2) & 3;
        if (!(faces >> f & 1)) continue;
        double xi[3], Ji[3][3], nrm[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[k] = k == d ? double(s) : tX[k == t1 ? g1 : g2];
        double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
        const double len = mapping_q1_face_normal(Ji, d, 0, nrm); // J^-T e_d, unsigned
        double *G = sG + item * 10;
        G[0] = fabs(det) * len * tW[g1] * tW[g2];
#pragma unroll
        for (int e = 0; e < 3; ++e) { G[1 + e] = nrm[e]; G[4 + e] = Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[k] = k == d ? double(1 - s) : xi[k];
        // (the neighbour behind an interior face exists)
        det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx + (d == 0 ? 2 * s - 1 : 0), cy + (d == 1 ? 2 * s - 1 : 0),
                                 cz + (d == 2 ? 2 * s - 1 : 0), xi, Ji);
#pragma unroll
        for (int e = 0; e < 3; ++e) G[7 + e] = Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2];
      }
    }
    double accU[MULTI ? MAXSRC : 1][3];
#pragma unroll
    for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = 0.0;
    const int nsrc = MULTI ? prm.nsrc : 1;
    for (int src = 0; src < nsrc; ++src) {
      const double *us = prm.us[src], *ws = prm.ws[src];
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) { // gather (read_dof_values: constrained entries read as 0)
        U[comp * 64 + t] = con ? 0.0 : us[comp * prm.Nu + gu];
        Wv[comp * 64 + t] = con ? 0.0 : ws[comp * prm.Nu + gu];
      }
      // the source values of the neighbour behind face f: its node (a, b, c).  Read only behind an interior face, where the cell
      // (cx, cy, cz) -+ e_d exists: jx = 3 (cx -+ 1) + a in [0, ndu[0]), likewise jy, jz
      auto neighbour = [&](int f, double v[3]) {
        const int d = f >> 1, s = f & 1;
        const int jx = 3 * (cx + (d == 0 ? (s ? 1 : -1) : 0)) + a, jy = 3 * (cy + (d == 1 ? (s ? 1 : -1) : 0)) + b,
                  jz = 3 * (cz + (d == 2 ? (s ? 1 : -1) : 0)) + c;
        const bool take = (faces >> f & 1) && !constrained_u(prm, jx, jy, jz);
        const long long gn = jx + (long long)prm.ndu[0] * (jy + (long long)prm.ndu[1] * jz);
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) v[comp] = take ? us[comp * prm.Nu + gn] : 0.0;
      };
      double nb[CART ? 6 : 1][3]; // CART: all six fetched first, one memory latency; the general kernel fetches face by face (as at degree 2)
      if constexpr (CART) {
#pragma unroll
        for (int f = 0; f < 6; ++f) neighbour(f, nb[f]);
      }
      wave_fence();
      double rU[3] = {0, 0, 0};
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        if (!(faces >> f & 1)) continue; // scalar
        const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
        const int sd = d == 0 ? 1 : (d == 1 ? 4 : 16), s1 = t1 == 0 ? 1 : 4, s2 = t2 == 1 ? 4 : 16; // node strides of the three directions
        if constexpr (!CART) neighbour(f, nb[0]);
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) N[comp * 64 + t] = nb[CART ? f : 0][comp];
        wave_fence();
        double go[3] = {0, 0, 0}, wn = 0.0, JxW = 0.0, jump = 0.0;
        if (point) { // this lane's face point and component: geometry, normal derivatives of both sides, w.n
          double gnb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0};
          if constexpr (CART) {
            nrm[d] = 1.0;
            go[d] = gnb[d] = prm.hinv[d];
            JxW = prm.detJ * prm.hinv[d] * tW[q1] * tW[q2];
          } else {
            const double *G = sG + (f * 16 + q) * 10; // the cell's geometry phase
            JxW = G[0];
#pragma unroll
            for (int e = 0; e < 3; ++e) { nrm[e] = G[1 + e]; go[e] = G[4 + e]; gnb[e] = G[7 + e]; }
          }
          // reference-space derivatives of this lane's component at the point, along (d, t1, t2): this side (end point s of direction
          // d) and the neighbour's (end point 1 - s)
          const double *Uc = U + comp_q * 64, *Nc = N + comp_q * 64;
          double od = 0.0, o1 = 0.0, o2 = 0.0, nd = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll 1
          for (int k2 = 0; k2 < 4; ++k2) {
            const double S2 = tS[q2 * 4 + k2], D2 = tD[q2 * 4 + k2];
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) {
              const double S1 = tS[q1 * 4 + k1], D1 = tD[q1 * 4 + k1];
              const double *uo = Uc + k1 * s1 + k2 * s2, *un = Nc + k1 * s1 + k2 * s2;
              double ao = 0.0, bo = 0.0, an = 0.0, bn = 0.0; // the sums over kd: derivative and value along d
#pragma unroll
              for (int kd = 0; kd < 4; ++kd) {
                ao = fma(tED[s * 4 + kd], uo[kd * sd], ao);
                an = fma(tED[(1 - s) * 4 + kd], un[kd * sd], an);
                if constexpr (!CART) {
                  bo = fma(tE[s * 4 + kd], uo[kd * sd], bo);
                  bn = fma(tE[(1 - s) * 4 + kd], un[kd * sd], bn);
                }
              }
              od = fma(S1 * S2, ao, od); nd = fma(S1 * S2, an, nd);
              if constexpr (!CART) {
                o1 = fma(D1 * S2, bo, o1); n1 = fma(D1 * S2, bn, n1);
                o2 = fma(S1 * D2, bo, o2); n2 = fma(S1 * D2, bn, n2);
              }
            }
          }
          jump = go[d] * od - gnb[d] * nd;
          if constexpr (!CART) jump += go[t1] * o1 - gnb[t1] * n1 + go[t2] * o2 - gnb[t2] * n2;
          // w at the point: the 16 nodes of the face
          double wval[3] = {0, 0, 0};
#pragma unroll
          for (int j2 = 0; j2 < 4; ++j2)
#pragma unroll
            for (int j1 = 0; j1 < 4; ++j1) {
              const double phi = tS[q1 * 4 + j1] * tS[q2 * 4 + j2];
#pragma unroll
              for (int c3 = 0; c3 < 3; ++c3) wval[c3] = fma(phi, Wv[c3 * 64 + 3 * s * sd + j1 * s1 + j2 * s2], wval[c3]);
            }
          wn = wval[0] * nrm[0] + wval[1] * nrm[1] + wval[2] * nrm[2];
          if (comp_q == 0) sA[q] = JxW;
        }
        wave_fence();
        if (point) { // h_F^2 = the face's area: the 16 JxW in point order
          double area = 0.0;
#pragma unroll
          for (int p = 0; p < 16; ++p) area += sA[p];
          const double delta = prm.scale * area * wn * wn;
          sF[q][comp_q] = delta * jump * JxW;
          if (comp_q == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) sF[q][3 + e] = go[e];
          }
        }
        wave_fence();
        { // integrate: the normal derivative of the test function of node (a, b, c), this cell's side
          const int kd = d == 0 ? a : (d == 1 ? b : c), k1 = t1 == 0 ? a : b, k2 = t2 == 1 ? b : c;
          const double vd = tE[s * 4 + kd], dd = tED[s * 4 + kd];
#pragma unroll 4
          for (int p = 0; p < 16; ++p) {
            const int p1 = p & 3, p2 = p >> 2;
            const double *F = sF[p];
            const double S1 = tS[p1 * 4 + k1], S2 = tS[p2 * 4 + k2];
            double dv = F[3 + d] * (dd * S1 * S2);
            if constexpr (!CART) dv += F[3 + t1] * (vd * tD[p1 * 4 + k1] * S2) + F[3 + t2] * (vd * S1 * tD[p2 * 4 + k2]);
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) rU[comp] = fma(dv, F[comp], rU[comp]);
          }
        }
        wave_fence(); // the next face reuses the neighbour and point buffers
      }
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(prm.wKu[src][o], rU[comp], accU[o][comp]);
          }
      } else {
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) accU[0][comp] = rU[comp];
      }
      wave_fence(); // the next source overwrites U, Wv
    }
    // distribute_local_to_global (add): constrained velocity rows are not written
    if (!con) {
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
            double *dptr = prm.out_u[o] + gu;
#pragma unroll
            for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += accU[o][comp];
          }
      } else {
        for (int o = 0; o < prm.nout; ++o) {
          double *dptr = prm.out_u[o] + gu;
#pragma unroll
          for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += prm.wKu[0][o] * accU[0][comp];
        }
      }
    }
  }
}

} // namespace

void stokes_cip_end_tables(double Eu[6], double EDu[6])
{
  static const std::vector<double> ends_tables = [] {
    const stfem::ShapeTables tu = stfem::make_shape_tables(2);
    const std::vector<double> ends = {0.0, 1.0};
    stfem::Mat E, ED;
    stfem::lagrange_tables(tu.nodes, ends, E, ED);
    std::vector<double> r(12);
    for (int i = 0; i < 6; ++i) { r[i] = E[i]; r[6 + i] = ED[i]; }
    return r;
  }();
  for (int i = 0; i < 6; ++i) { Eu[i] = ends_tables[i]; EDu[i] = ends_tables[6 + i]; }
}

namespace {

// One plane pair of a velocity source for the neighbour slab (stfem_stokes_cip_pack): out[comp][p][iy][ix] = src[comp][z0 + p][iy][ix],
// 0 on the DoFs this context constrains.  i < 3 * 2 * plane; reads comp * Nu + (z0 + p) * plane + r with z0 + p <= ndu[2] - 2.
__global__ __launch_bounds__(256) void stokes_cip_pack_kernel(const double *__restrict__ src, double *__restrict__ out, int ndx, int ndy,
                                                              int ndz, int z0, long long Nu, int dmask)
{
  const long long plane = (long long)ndx * ndy, n = 6 * plane;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * gridDim.x) {
    const long long r = i % plane;
    const int p = int((i / plane) % 2), comp = int(i / (2 * plane)), ix = int(r % ndx), iy = int(r / ndx), iz = z0 + p;
    const bool con = ((dmask & 1) && ix == 0) || ((dmask & 2) && ix == ndx - 1) || ((dmask & 4) && iy == 0) || ((dmask & 8) && iy == ndy - 1) ||
                     ((dmask & 16) && iz == 0) || ((dmask & 32) && iz == ndz - 1);
    out[i] = con ? 0.0 : src[comp * Nu + iz * plane + r];
  }
}

// the eight colour launches; ghost_lo / ghost_hi: per source the neighbours' planes (read for the sides of c->cip_neighbours only)
int cip_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *weight, double delta0, const double *const *ghost_lo,
               const double *const *ghost_hi, hipStream_t st);

} // namespace

int stokes_cip_source_ready(const stfem_stokes_ctx *c, const double *src_u)
{
  if (!c->cip_neighbours || c->cip_delta0 == 0.0) return STFEM_OK;
  for (const auto &b : c->cip_bindings)
    if (b.src == src_u) {
      if ((c->cip_neighbours & 16) && !b.lower)
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab: the source's binding has no lower ghost planes");
      if ((c->cip_neighbours & 32) && !b.upper)
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab: the source's binding has no upper ghost planes");
      return STFEM_OK;
    }
  return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab with neighbours: no ghost planes bound to the velocity source "
                                                     "(stfem_stokes_cip_bind_ghosts)");
}

int stokes_cip_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *weight, double delta0, hipStream_t st)
{
  if (delta0 == 0.0 || !c->cip_neighbours) return cip_launch(c, set, weight, delta0, nullptr, nullptr, st);
  const double *lo[MAXSRC] = {}, *hi[MAXSRC] = {};
  for (int s = 0; s < set.nsrc && s < MAXSRC; ++s) {
    const int rc = stokes_cip_source_ready(c, set.us[s]);
    if (rc != STFEM_OK) return rc;
    for (const auto &b : c->cip_bindings)
      if (b.src == set.us[s]) { lo[s] = b.lower; hi[s] = b.upper; }
  }
  return cip_launch(c, set, weight, delta0, lo, hi, st);
}

namespace {

// STFEM_STOKES_CIP_WORKGROUPS=<n>, read at every launch: at most n workgroups per CIP colour launch, at either degree
long long cip_workgroup_cap() { return cip_parse_cap(getenv("STFEM_STOKES_CIP_WORKGROUPS")); }

// The eight colour launches at velocity degree 3 (a context without slab neighbours: the slab entries are kept to degree 2)
int cip_q3_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *weight, double delta0, hipStream_t st)
{
  const StokesParamsT<3> &g = c->desc<3>();
  CipQ3Params k;
  k.vertices = g.vertices;
  k.ncx = g.ncx; k.ncy = g.ncy; k.ncz = g.ncz;
  for (int d = 0; d < 3; ++d) { k.ndu[d] = g.ndu[d]; k.hinv[d] = g.hinv[d]; }
  k.Nu = g.Nu;
  k.dmask = g.dmask;
  for (int i = 0; i < 16; ++i) { k.Su[i] = g.Su[i]; k.Du[i] = g.Du[i]; }
  for (int i = 0; i < 4; ++i) { k.xq[i] = g.xq[i]; k.wq[i] = g.wq[i]; }
  static const std::vector<double> ends_tables = [] { // FE_Q(3) values / derivatives at the end points 0 and 1, [s * 4 + a]
    const stfem::ShapeTables tu = stfem::make_shape_tables(3);
    const std::vector<double> ends = {0.0, 1.0};
    stfem::Mat E, ED;
    stfem::lagrange_tables(tu.nodes, ends, E, ED);
    std::vector<double> r(16);
    for (int i = 0; i < 8; ++i) { r[i] = E[i]; r[8 + i] = ED[i]; }
    return r;
  }();
  for (int i = 0; i < 8; ++i) { k.Eu[i] = ends_tables[i]; k.EDu[i] = ends_tables[8 + i]; }
  k.colour = 0; k.cart = g.cart;
  k.detJ = g.detJ;
  k.scale = delta0 / (27.0 * std::sqrt(3.0)); // pa = degree^3.5, degree 3 (operators.h:1614-1615)
  k.nsrc = set.nsrc;
  for (int s = 0; s < MAXSRC; ++s) {
    k.us[s] = s < set.nsrc ? set.us[s] : nullptr;
    k.ws[s] = s < set.nsrc ? weight[s] : nullptr;
    if (s < set.nsrc && (!set.us[s] || !weight[s])) return STFEM_ERR_INVALID_ARGUMENT;
  }
  k.nout = stokes_k_destinations(set, k.out_u, k.wKu);
  if (k.nout == 0) return STFEM_OK;
  const bool multi = set.nsrc > 1;
  const void *kerns[4] = {(const void *)stokes_cip_q3_kernel<false, false>, (const void *)stokes_cip_q3_kernel<true, false>,
                          (const void *)stokes_cip_q3_kernel<false, true>, (const void *)stokes_cip_q3_kernel<true, true>};
  const void *kern = kerns[(multi ? 2 : 0) + (k.cart ? 1 : 0)];
  const long long cap = cip_workgroup_cap();
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) {
    const long long n = cip_colour_cells(c->nc, colour);
    if (n == 0) continue;
    k.colour = colour;
    const CipPlan plan = cip_plan(n, 1, 32ll * c->n_cu, cap); // one wave per cell, one wave per workgroup
    void *args[] = {(void *)&k};
    (void)hipLaunchKernel(kern, dim3((unsigned)plan.grid), dim3(64), args, 0, st);
    c->cip_launched = true;
    c->cip_plan[0] = (int)plan.grid; c->cip_plan[1] = (int)plan.passes;
  }
  return stfem_launch_end("stokes_cip_q3_kernel");
}

int cip_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *weight, double delta0, const double *const *ghost_lo,
               const double *const *ghost_hi, hipStream_t st)
{
  if (delta0 == 0.0) return STFEM_OK;
  const int neighbours = ghost_lo && ghost_hi ? c->cip_neighbours : 0;
  if (c->nc[0] < 2 && c->nc[1] < 2 && c->nc[2] < 2 && !neighbours) return STFEM_OK; // no interior face
  if (set.nsrc < 1 || set.nsrc > MAXSRC || set.nout > (set.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiations' bounds)
  if (c->degree == 3) return cip_q3_launch(c, set, weight, delta0, st);
  const StokesParams &g = c->desc<2>(); // (the slab entries have kept the rest to degree 2)
  CipSlabParams k; // (the instantiations without SLAB read its CipParams part alone)
  k.neighbours = neighbours;
  for (int side = 0; side < 2; ++side) k.ghost_vertices[side] = c->d_cip_vertices[side];
  for (int s = 0; s < MAXSRC; ++s) {
    k.ghost_lo[s] = neighbours && s < set.nsrc ? ghost_lo[s] : nullptr;
    k.ghost_hi[s] = neighbours && s < set.nsrc ? ghost_hi[s] : nullptr;
    if (s < set.nsrc && (((neighbours & 16) && !k.ghost_lo[s]) || ((neighbours & 32) && !k.ghost_hi[s])))
      return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab: ghost planes missing for a side with a neighbour");
  }
  if (neighbours && !g.cart)
    for (int side = 0; side < 2; ++side)
      if ((neighbours >> (4 + side) & 1) && !k.ghost_vertices[side])
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab: no ghost vertex plane on side %d", side);
  k.vertices = g.vertices;
  k.ncx = g.ncx; k.ncy = g.ncy; k.ncz = g.ncz;
  for (int d = 0; d < 3; ++d) { k.ndu[d] = g.ndu[d]; k.xq[d] = g.xq[d]; k.wq[d] = g.wq[d]; k.hinv[d] = g.hinv[d]; }
  k.Nu = g.Nu;
  k.dmask = g.dmask;
  for (int i = 0; i < 9; ++i) { k.Su[i] = g.Su[i]; k.Du[i] = g.Du[i]; }
  stokes_cip_end_tables(k.Eu, k.EDu);
  k.colour = 0; k.cart = g.cart;
  k.detJ = g.detJ;
  k.scale = delta0 / (8.0 * std::sqrt(2.0)); // pa = degree^3.5, degree 2 (operators.h:1614-1615)
  k.nsrc = set.nsrc;
  for (int s = 0; s < MAXSRC; ++s) {
    k.us[s] = s < set.nsrc ? set.us[s] : nullptr;
    k.ws[s] = s < set.nsrc ? weight[s] : nullptr;
    if (s < set.nsrc && (!set.us[s] || !weight[s])) return STFEM_ERR_INVALID_ARGUMENT;
  }
  k.nout = stokes_k_destinations(set, k.out_u, k.wKu); // those with a non-zero weight of the K part receive the term
  if (k.nout == 0) return STFEM_OK;

  const bool multi = set.nsrc > 1;
  const int which = (multi ? 2 : 0) + (k.cart ? 1 : 0);
  const void *kerns[4] = {(const void *)stokes_cip_kernel<false, false>, (const void *)stokes_cip_kernel<true, false>,
                          (const void *)stokes_cip_kernel<false, true>, (const void *)stokes_cip_kernel<true, true>};
  // a slab with neighbours: the SLAB instantiations; without, the four above on the CipParams part of k - today's launches
  const void *slab_kerns[4] = {(const void *)stokes_cip_kernel<false, false, true>, (const void *)stokes_cip_kernel<true, false, true>,
                               (const void *)stokes_cip_kernel<false, true, true>, (const void *)stokes_cip_kernel<true, true, true>};
  const void *kern = neighbours ? slab_kerns[which] : kerns[which];
  const long long cap = cip_workgroup_cap();
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) { // ascending, like every colour sequence of the operator
    const long long n = cip_colour_cells(c->nc, colour);
    if (n == 0) continue; // a colour without cells
    k.colour = colour;
    const CipPlan plan = cip_plan(n, 8, 8ll * c->n_cu, cap); // (without a cap min(ceil(n / 8), 8 n_cu) workgroups, as ever)
    void *args[] = {neighbours ? (void *)&k : (void *)static_cast<CipParams *>(&k)};
    (void)hipLaunchKernel(kern, dim3((unsigned)plan.grid), dim3(256), args, 0, st);
    c->cip_launched = true;
    c->cip_plan[0] = (int)plan.grid; c->cip_plan[1] = (int)plan.passes;
  }
  return stfem_launch_end("stokes_cip_kernel");
}

} // namespace

extern "C" {

// The entries of stfem.h: velocity degree 2.  Their _space forms (stfem_stokes_cip_space.h): the context's degree.
int stfem_stokes_set_cip(stfem_stokes_ctx *c, double delta0, int weight)
{
  if (!c || !std::isfinite(delta0) || weight < STFEM_CIP_WEIGHT_SOURCE || weight > STFEM_CIP_WEIGHT_LINEARISATION)
    return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_set_cip")) return rq;
  c->cip_delta0 = delta0;
  c->cip_weight = weight;
  return STFEM_OK;
}

int stfem_stokes_set_cip_space(stfem_stokes_ctx *c, double delta0, int weight)
{
  if (!c || !std::isfinite(delta0) || weight < STFEM_CIP_WEIGHT_SOURCE || weight > STFEM_CIP_WEIGHT_LINEARISATION)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_set_cip_space: a null context, a non-finite delta0 or a weight outside 0..1");
  c->cip_delta0 = delta0;
  c->cip_weight = weight;
  return STFEM_OK;
}

int stfem_stokes_cip_add(stfem_stokes_ctx *c, double *dst_u, const double *src_u, const double *weight_u, double delta0, void *stream)
{
  if (!c || !dst_u || !src_u || !weight_u || !std::isfinite(delta0)) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst_u == src_u || dst_u == weight_u) return STFEM_ERR_ALIAS;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_add")) return rq;
  STFEM_TRY(hipSetDevice(c->device));
  const StokesSet set = stokes_single_set(src_u, dst_u); // the term by itself
  return cip_launch(c, set, &weight_u, delta0, nullptr, nullptr, static_cast<hipStream_t>(stream)); // (the faces inside the slab alone)
}

int stfem_stokes_cip_add_space(stfem_stokes_ctx *c, double *dst_u, const double *src_u, const double *weight_u, double delta0, void *stream)
{
  if (!c || !dst_u || !src_u || !weight_u || !std::isfinite(delta0))
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_cip_add_space: a null argument or a non-finite delta0");
  if (dst_u == src_u || dst_u == weight_u) return stfem_set_error(STFEM_ERR_ALIAS, "stfem_stokes_cip_add_space: dst_u is src_u or weight_u");
  STFEM_TRY(hipSetDevice(c->device));
  const StokesSet set = stokes_single_set(src_u, dst_u);
  return cip_launch(c, set, &weight_u, delta0, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int stfem_stokes_last_cip_plan(const stfem_stokes_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (!c->cip_launched) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_last_cip_plan: this context has not launched the CIP kernel");
  out[0] = c->cip_plan[0];
  out[1] = c->cip_plan[1];
  return STFEM_OK;
}

int stfem_stokes_set_cip_neighbours(stfem_stokes_ctx *c, int neighbour_mask, const double *lower_vertices, const double *upper_vertices)
{
  if (!c) return STFEM_ERR_INVALID_ARGUMENT;
  if (neighbour_mask & ~48) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "neighbour_mask %d: only bits 4 and 5 name a z neighbour", neighbour_mask);
  if (const int rq = stokes_require_q2(c, "stfem_stokes_set_cip_neighbours")) return rq;
  const double *given[2] = {lower_vertices, upper_vertices};
  if (!c->cart)
    for (int side = 0; side < 2; ++side)
      if ((neighbour_mask >> (4 + side) & 1) && !given[side])
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "general mesh: the %s neighbour needs its vertex plane", side ? "upper" : "lower");
  STFEM_TRY(hipSetDevice(c->device));
  // the new arrays first, then the swap: a failure leaves the context as it was
  double *fresh[2] = {nullptr, nullptr};
  if (!c->cart) {
    const size_t plane = size_t(c->nc[0] + 1) * (c->nc[1] + 1) * 3;
    std::vector<double> two(2 * plane);
    for (int side = 0; side < 2; ++side) {
      if (!(neighbour_mask >> (4 + side) & 1)) continue;
      // [ghost | plane 0] below, [top plane | ghost] above: the neighbour cell layer as a mesh of one layer
      const double *own = c->h_vertices.data() + (side ? size_t(c->nc[2]) * plane : 0);
      std::copy(given[side], given[side] + plane, two.begin() + (side ? plane : 0));
      std::copy(own, own + plane, two.begin() + (side ? 0 : plane));
      hipError_t e = hipMalloc(&fresh[side], 2 * plane * sizeof(double));
      const bool oom = e != hipSuccess;
      if (oom) fresh[side] = nullptr;
      else e = hipMemcpy(fresh[side], two.data(), 2 * plane * sizeof(double), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        for (double *f : fresh)
          if (f) (void)hipFree(f);
        return oom ? STFEM_ERR_OUT_OF_MEMORY : stfem_set_error(STFEM_ERR_HIP, "ghost vertex planes: %s", hipGetErrorString(e));
      }
    }
  }
  for (int side = 0; side < 2; ++side) {
    if (c->d_cip_vertices[side]) (void)hipFree(c->d_cip_vertices[side]); // (synchronises: no launch still reads it)
    c->d_cip_vertices[side] = fresh[side];
  }
  c->cip_neighbours = neighbour_mask;
  return STFEM_OK;
}

int64_t stfem_stokes_cip_ghost_size(const stfem_stokes_ctx *c)
{
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_ghost_size")) return rq;
  return c ? 6ll * c->ndu[0] * c->ndu[1] : 0;
}

int stfem_stokes_cip_ghost_create(stfem_stokes_ctx *c, double **device_out)
{
  if (!c || !device_out) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_ghost_create")) return rq;
  *device_out = nullptr;
  STFEM_TRY(hipSetDevice(c->device));
  const size_t bytes = size_t(stfem_stokes_cip_ghost_size(c)) * sizeof(double);
  double *d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  const hipError_t e = hipMemset(d, 0, bytes);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return stfem_set_error(STFEM_ERR_HIP, "hipMemset(ghost planes): %s", hipGetErrorString(e));
  }
  *device_out = d;
  return STFEM_OK;
}

void stfem_stokes_cip_ghost_destroy(stfem_stokes_ctx *c, double *ghost)
{
  if (!c || !ghost) return;
  (void)hipSetDevice(c->device);
  // bindings that name the array go with it: a later launch must not read freed memory
  auto &b = c->cip_bindings;
  b.erase(std::remove_if(b.begin(), b.end(), [&](const stfem_stokes_ctx::CipBinding &e) { return e.lower == ghost || e.upper == ghost; }), b.end());
  (void)hipFree(ghost);
}

int stfem_stokes_cip_pack(stfem_stokes_ctx *c, const double *src_u, int side, double *out, void *stream)
{
  if (!c || !src_u || !out || side < 0 || side > 1) return STFEM_ERR_INVALID_ARGUMENT;
  if (out == src_u) return STFEM_ERR_ALIAS;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_pack")) return rq;
  STFEM_TRY(hipSetDevice(c->device));
  const long long n = 6ll * c->ndu[0] * c->ndu[1];
  const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 8ll * c->n_cu);
  stfem_launch_begin();
  stokes_cip_pack_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(src_u, out, c->ndu[0], c->ndu[1], c->ndu[2],
                                                                             side ? c->ndu[2] - 3 : 1, c->Nu, c->dmask);
  return stfem_launch_end("stokes_cip_pack_kernel");
}

int stfem_stokes_cip_add_slab(stfem_stokes_ctx *c, double *dst_u, const double *src_u, const double *weight_u, double delta0,
                              const double *lower_ghost, const double *upper_ghost, void *stream)
{
  if (!c || !dst_u || !src_u || !weight_u || !std::isfinite(delta0)) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_add_slab")) return rq;
  if (((c->cip_neighbours & 16) && !lower_ghost) || ((c->cip_neighbours & 32) && !upper_ghost))
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "CIP term on a slab: ghost planes missing for a side with a neighbour (mask %d)",
                           c->cip_neighbours);
  if (dst_u == src_u || dst_u == weight_u || dst_u == lower_ghost || dst_u == upper_ghost) return STFEM_ERR_ALIAS;
  STFEM_TRY(hipSetDevice(c->device));
  const StokesSet set = stokes_single_set(src_u, dst_u); // the term by itself
  return cip_launch(c, set, &weight_u, delta0, &lower_ghost, &upper_ghost, static_cast<hipStream_t>(stream));
}

int stfem_stokes_cip_bind_ghosts(stfem_stokes_ctx *c, const double *src_u, const double *lower_ghost, const double *upper_ghost)
{
  if (!c || !src_u) return STFEM_ERR_INVALID_ARGUMENT;
  if (src_u == lower_ghost || src_u == upper_ghost) return STFEM_ERR_ALIAS;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_cip_bind_ghosts")) return rq;
  auto &b = c->cip_bindings;
  b.erase(std::remove_if(b.begin(), b.end(), [&](const stfem_stokes_ctx::CipBinding &e) { return e.src == src_u; }), b.end());
  if (lower_ghost || upper_ghost) b.push_back({src_u, lower_ghost, upper_ghost});
  return STFEM_OK;
}

} // extern "C"
