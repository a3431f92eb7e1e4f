// Stokes two-field operator: the cell kernel, for velocity degree DEG = 2 (FE_Q(2)^3 x FE_Q(1) / FE_DGP(1), QGauss(3)) and DEG = 3
// (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), QGauss(4), the pair the reference builds for time degree 2, tests/tp_03stokes.cc:79-86).  It
// replaces, for the cell loop (LoopType::Cell: no weak boundary ids, delta0 = 0):
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
// stores: no atomics, no zeroing, bitwise reproducible.  No CPU fallback.  At degree 2 it serves general meshes (boxes take the
// Kronecker path of stfem_stokes.hip unless STFEM_STOKES_CELL=1), at degree 3 every mesh.
//
// Thread layout: lane t = a + (DEG + 1) b + (DEG + 1)^2 c of a cell is its velocity node (a, b, c) and its quadrature point (a, b, c).
// Degree 2: 27 of 32 lanes, one wave owns two cells; degree 3: 64 lanes, one wave is one cell.  Evaluation and integration are
// sum-factorised (three 1D stages each, see stokes_cell_kernel); the MappingQ1 Jacobian is evaluated on the fly from the eight cell
// vertices (24 doubles per cell instead of a stored metric), or is a constant diagonal on axis-aligned boxes.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// 256 threads = 8 (degree 2) or 4 (degree 3) cells at a time; the workgroups walk over the cells.
// Sum-factorised: evaluation and integration are three 1D stages each (x, y, z), handed from lane to lane through two wave-private
// LDS regions per cell that alternate as source and destination, ordered with wave_fence() (a cell never leaves its wave: no
// workgroup barrier inside the cell loop).
//   evaluate : lane (a, b, c) = (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point (q_x, q_y, q_z)
//   integrate: lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node (n_x, n_y, n_z)
// The FE_Q(DEG - 1) pressure rides on the lanes with a, b, c < DEG (node (a, b, c)); the other lanes compute on clamped indices and
// their results are not used.  The FE_DGP(DEG - 1) functions are evaluated directly at the lane's point and integrated by the first
// lanes of the cell, one function each, as sums over the quadrature points in ascending order.
// CART: axis-aligned uniform cells (the context was created without vertices): constant diagonal Jacobian.
// MULTI: several sources per cell, weighted sums in registers (one set per destination pair, up to MAXSRC), one scatter; otherwise
//        one source (index 0), no sums, the weights applied at scatter time to up to MAXOUT destination pairs (see StokesParams)
// PDG: FE_DGP pressure (a template parameter: the FE_Q instantiations carry none of it, and the other way round)
template <int DEG, bool CART, bool MULTI, bool PDG>
__global__ __launch_bounds__(256) void stokes_cell_kernel(const StokesParamsT<DEG> prm)
{
  constexpr int N1 = DEG + 1, N2 = N1 * N1, NN = N1 * N2; // nodes = quadrature points per direction, per cell: 27 or 64
  constexpr int LANES = NN <= 32 ? 32 : 64, CELLS = 256 / LANES;
  constexpr int NDGP = DEG * (DEG + 1) * (DEG + 2) / 6; // 4 or 10
  constexpr int R = 13 * NN;                            // doubles per cell of each region (largest stage: 13 arrays of NN)
  constexpr int XP = 3 * NN;                            // the cell's pressure values in the gather: X[XP ..] (nodes or functions)
  constexpr bool HELD = COLUMNS_HELD<DEG>;
  // the 1D tables behind the regions, in the same array: [q*N1+a], [q*N1+a], and the pressure's, N1 * DEG doubles either way: FE_Q
  // [q*DEG+a], FE_DGP the Legendre functions at the Gauss points [degree*N1+q], degree 0 = 1
  __shared__ double smem[CELLS * 2 * R + 2 * N2 + N1 * DEG];
  double *const tS = smem + CELLS * 2 * R, *const tD = tS + N2, *const tP = tD + N2, *const tL = tP;
  if (threadIdx.x < N2) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < N1 * DEG) tP[threadIdx.x] = !PDG ? prm.Sp[threadIdx.x] : (threadIdx.x < N1 ? 1.0 : prm.lq[threadIdx.x / N1 - 1][threadIdx.x % N1]);
  __syncthreads();
  const int slot = threadIdx.x / LANES, tl = threadIdx.x % LANES;
  const bool lane_on = NN == LANES || tl < NN;
  const int t = lane_on ? tl : 0;
  const int a = t % N1, b = (t / N1) % N1, c = t / N2;
  const int ap = a < DEG ? a : DEG - 1, bp = b < DEG ? b : DEG - 1, cp = c < DEG ? c : DEG - 1; // (pressure stages: clamped, unused where DEG)
  double *X = smem + slot * (2 * R), *Y = X + R;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  const Coef<N1, 1, true> Sa(tS + N1 * a), Da(tD + N1 * a), Sb(tS + N1 * b), Db(tD + N1 * b), Sc(tS + N1 * c), Dc(tD + N1 * c);
  const Coef<N1, N1, HELD> SaT(tS + a), DaT(tD + a), SbT(tS + b), DbT(tD + b), ScT(tS + c), DcT(tD + c);
  const Coef<DEG, 1, HELD> Pa(tP + DEG * a), Pb(tP + DEG * b), Pc(tP + DEG * c);
  const Coef<N1, DEG, HELD> PaT(tP + ap), PbT(tP + bp), PcT(tP + cp);
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  // this lane also carries a pressure DoF of the cell: FE_Q node (a, b, c), or FE_DGP function tl
  const bool pnode = PDG ? tl < NDGP : (lane_on && a < DEG && b < DEG && c < DEG);
  const int pslot = PDG ? (tl < NDGP ? tl : NDGP - 1) : ap + DEG * bp + DEG * DEG * cp; // its slot in the cell's pressure values X[XP ..]
  // FE_DGP: the functions at this lane's quadrature point, and the degrees of the function this lane integrates
  auto legendre = [&](int degree, int q) { return degree == 0 ? 1.0 : tL[degree * N1 + q]; }; // (a constant degree 0 folds)
  double phi[PDG ? NDGP : 1];
  int ei = 0, ej = 0, ek = 0;
  if constexpr (PDG) {
    constexpr DgpDegrees<DEG> dgp = dgp_degrees<DEG>();
#pragma unroll
    for (int f = 0; f < NDGP; ++f) {
      phi[f] = legendre(dgp.d[f][0], a) * legendre(dgp.d[f][1], b) * legendre(dgp.d[f][2], c);
      if (tl == f) { ei = dgp.d[f][0]; ej = dgp.d[f][1]; ek = dgp.d[f][2]; }
    }
  } else {
    phi[0] = 0.0;
  }
  // the cells of one colour share no DoF: the eight colours run as eight launches, lowest first, and
  // scatter with plain loads and stores (no atomics, no zeroing of the destinations, deterministic)
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;

  // every cell slot (half-wave or wave) walks through its own contiguous run of cells: cells sharing nodes are handled one after the
  // other by the same lanes instead of at the same time by neighbouring ones.  Degree 2 with prm.interleave: the eight half-waves of
  // the workgroup take eight consecutive cells of the workgroup's run at a time (their rows are 32 bytes apart: denser sectors per
  // gather / scatter instruction); degree 3 keeps the contiguous runs
  const long long nslot = (long long)gridDim.x * CELLS, run = (ncells + nslot - 1) / nslot;
  const long long wg_first = (long long)blockIdx.x * CELLS * run, wg_end = wg_first + CELLS * run;
  const bool interleave = DEG == 2 && prm.interleave;
  const int STRIDE = interleave ? CELLS : 1;
  const long long first = interleave ? wg_first + slot : ((long long)blockIdx.x * CELLS + slot) * run;
  // the DoFs of a cell are fetched while the previous cell is being computed
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu, gp;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && (interleave ? cell < wg_end : cell < first + run);
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = DEG * q.cx + a, iy = DEG * q.cy + b, iz = DEG * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    q.gp = PDG ? (q.cx + (long long)prm.ncx * (q.cy + (long long)prm.ncy * q.cz)) * NDGP + pslot
               : ((DEG - 1) * q.cx + ap) + (long long)prm.ndp[0] * (((DEG - 1) * q.cy + bp) + (long long)prm.ndp[1] * ((DEG - 1) * q.cz + cp));
    return q;
  };
  double un[3] = {0, 0, 0}, pn = 0.0;
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained velocity entries read as 0
    const double *us = prm.us[MULTI ? s : 0], *ps = prm.ps[MULTI ? s : 0];
    if (q.ok && lane_on && !q.con) {
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
    const int cx = cur.cx, cy = cur.cy, cz = cur.cz;
    const bool con = cur.con;
    const long long gu = cur.gu, gp = cur.gp;
    const bool active = cur.ok && lane_on;

    // ---- gather: X = u[3][NN], p[nodes or functions]
    if (lane_on) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) X[comp * NN + t] = un[comp];
    }
    if (pnode) X[XP + pslot] = pn;
    nxt = ids(first + STRIDE * ((it2 + 1) / nsrc));
    fetch(nxt, int((it2 + 1) % nsrc));
    wave_fence();
    double pval = 0.0;
    if constexpr (PDG) {
#pragma unroll
      for (int j = 0; j < NDGP; ++j) pval = fma(phi[j], X[XP + j], pval);
    }

    // ---- evaluate, x: (n_x, n_y, n_z) -> (q_x, n_y, n_z): values and x derivatives -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *up = X + comp * NN + N1 * b + N2 * c;
      double u[N1];
#pragma unroll
      for (int n = 0; n < N1; ++n) u[n] = up[n];
      Y[(comp * 2) * NN + t] = dot<N1>(Sa, u);
      Y[(comp * 2 + 1) * NN + t] = dot<N1>(Da, u);
    }
    if constexpr (!PDG) Y[6 * NN + t] = dot<DEG>(Pa, X + XP + DEG * bp + DEG * DEG * cp); // pressure (n_y, n_z < DEG)
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z): value, d/dx, d/dy -> X
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *vp = Y + (comp * 2) * NN + a + N2 * c, *dp = vp + NN;
      double v[N1], d[N1];
#pragma unroll
      for (int n = 0; n < N1; ++n) v[n] = vp[N1 * n];
#pragma unroll
      for (int n = 0; n < N1; ++n) d[n] = dp[N1 * n];
      X[(comp * 3) * NN + t] = dot<N1>(Sb, v);
      X[(comp * 3 + 1) * NN + t] = dot<N1>(Sb, d);
      X[(comp * 3 + 2) * NN + t] = dot<N1>(Db, v);
    }
    if constexpr (!PDG) X[9 * NN + t] = dot<DEG>(Pb, Y + 6 * NN + a + N2 * cp, N1);
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): value and reference gradient in registers
    double uval[3], gref[3][3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *vp = X + (comp * 3) * NN + a + N1 * b;
      double v[N1];
#pragma unroll
      for (int n = 0; n < N1; ++n) v[n] = vp[N2 * n];
      uval[comp] = dot<N1>(Sc, v);
      gref[comp][0] = dot<N1>(Sc, vp + NN, N2);
      gref[comp][1] = dot<N1>(Sc, vp + 2 * NN, N2);
      gref[comp][2] = dot<N1>(Dc, v);
    }
    if constexpr (!PDG) pval = dot<DEG>(Pc, X + 9 * NN + a + N1 * b, N2);

    // ---- quadrature-point operation (operators.h:1547-1553, 1570; weights applied at scatter time) -> Y:
    // arrays comp * 3 + e: the flux in reference coordinates, 9: div u, 10 + comp: the mass term
    if (CART) {
      const double JxW = prm.detJ * wabc;
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const double g = gref[comp][e] * prm.hinv[e];
          Y[(comp * 3 + e) * NN + t] = (prm.nu * g - (comp == e ? pval : 0.0)) * JxW * prm.hinv[e];
        }
        Y[(10 + comp) * NN + t] = uval[comp] * JxW;
      }
      Y[9 * NN + t] = (gref[0][0] * prm.hinv[0] + gref[1][1] * prm.hinv[1] + gref[2][2] * prm.hinv[2]) * JxW;
    } else {
      const double xi[3] = {prm.xq[a], prm.xq[b], prm.xq[c]};
      double Ji[3][3];
      const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji); // (at this lane's point)
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
        for (int e = 0; e < 3; ++e) Y[(comp * 3 + e) * NN + t] = Ji[e][0] * F[0] + Ji[e][1] * F[1] + Ji[e][2] * F[2];
        Y[(10 + comp) * NN + t] = uval[comp] * JxW;
      }
      Y[9 * NN + t] = divu * JxW;
    }
    wave_fence();
    double rP = 0.0;
    if constexpr (PDG) { // (q_j, div u): the cell's own test functions, each summed over the quadrature points in ascending order
      if (tl < NDGP) {
        const double *fd = Y + 9 * NN;
        for (int qc = 0; qc < N1; ++qc)
          for (int qb = 0; qb < N1; ++qb) {
            const double lbc = tL[ej * N1 + qb] * tL[ek * N1 + qc]; // (the lane's degrees: the row of ones where 0, no select)
#pragma unroll
            for (int qa = 0; qa < N1; ++qa) rP = fma(tL[ei * N1 + qa] * lbc, fd[qa + N1 * qb + N2 * qc], rP);
          }
      }
    }

    // ---- integrate, z: quadrature point -> (q_x, q_y, n_z) -> X: per component flux_x, flux_y (values in z), flux_z (derivative), mass
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *f0 = Y + (comp * 3) * NN + a + N1 * b, *fm = Y + (10 + comp) * NN + a + N1 * b;
      X[(comp * 4) * NN + t] = dot<N1>(ScT, f0, N2);
      X[(comp * 4 + 1) * NN + t] = dot<N1>(ScT, f0 + NN, N2);
      X[(comp * 4 + 2) * NN + t] = dot<N1>(DcT, f0 + 2 * NN, N2);
      X[(comp * 4 + 3) * NN + t] = dot<N1>(ScT, fm, N2);
    }
    if constexpr (!PDG) X[12 * NN + t] = dot<N1>(PcT, Y + 9 * NN + a + N1 * b, N2);
    wave_fence();
    // ---- y: -> (q_x, n_y, n_z) -> Y
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *g0 = X + (comp * 4) * NN + a + N2 * c;
      Y[(comp * 3) * NN + t] = dot<N1>(SbT, g0, N1);
      Y[(comp * 3 + 1) * NN + t] = dot<N1>(DbT, g0 + NN, N1) + dot<N1>(SbT, g0 + 2 * NN, N1);
      Y[(comp * 3 + 2) * NN + t] = dot<N1>(SbT, g0 + 3 * NN, N1);
    }
    if constexpr (!PDG) Y[9 * NN + t] = dot<N1>(PbT, X + 12 * NN + a + N2 * c, N1);
    wave_fence();
    // ---- x: -> node (a, b, c)
    double rK[3], rM[3];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      const double *h0 = Y + (comp * 3) * NN + N1 * b + N2 * c;
      rK[comp] = dot<N1>(DaT, h0) + dot<N1>(SaT, h0 + NN);
      rM[comp] = dot<N1>(SaT, h0 + 2 * NN);
    }
    if constexpr (!PDG) rP = dot<N1>(PaT, Y + 9 * NN + N1 * b + N2 * c);

    // ---- distribute_local_to_global: constrained velocity rows stay 0.  A DoF on a face shared with a neighbouring cell is first
    // touched by the cell whose colour bits are 0 in all shared directions (last node index: DEG velocity, DEG - 1 FE_Q pressure).
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
      const bool fu = !((a == 0 && cx > 0 && px) || (a == DEG && cx < prm.ncx - 1 && px) ||
                        (b == 0 && cy > 0 && py) || (b == DEG && cy < prm.ncy - 1 && py) ||
                        (c == 0 && cz > 0 && pz) || (c == DEG && cz < prm.ncz - 1 && pz));
      const bool fp = PDG || !((a == 0 && cx > 0 && px) || (a == DEG - 1 && cx < prm.ncx - 1 && px) ||
                                    (b == 0 && cy > 0 && py) || (b == DEG - 1 && cy < prm.ncy - 1 && py) ||
                                    (c == 0 && cz > 0 && pz) || (c == DEG - 1 && cz < prm.ncz - 1 && pz));
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

template <int DEG> const void *cell_kernel(int which) // which = 4 PDG + 2 MULTI + CART
{
  const void *const kerns[8] = {
    (const void *)stokes_cell_kernel<DEG, false, false, false>, (const void *)stokes_cell_kernel<DEG, true, false, false>,
    (const void *)stokes_cell_kernel<DEG, false, true, false>,  (const void *)stokes_cell_kernel<DEG, true, true, false>,
    (const void *)stokes_cell_kernel<DEG, false, false, true>,  (const void *)stokes_cell_kernel<DEG, true, false, true>,
    (const void *)stokes_cell_kernel<DEG, false, true, true>,   (const void *)stokes_cell_kernel<DEG, true, true, true>};
  return kerns[which];
}

template <int DEG> int cell_launch(stfem_stokes_ctx *c, const StokesSet &set, hipStream_t st)
{
  if (set.nsrc < 1 || set.nsrc > MAXSRC || set.nout > (set.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiation's bounds)
  StokesParamsT<DEG> prm = stokes_params<DEG>(c, set);
  void *args[] = {&prm};
  const int which = (prm.pdg ? 4 : 0) + (set.nsrc > 1 ? 2 : 0) + (prm.cart ? 1 : 0), cells = DEG == 3 ? 4 : 8; // (cells per workgroup)
  const void *kern = cell_kernel<DEG>(which);
  // persistent workgroups: exactly as many as stay resident, asked once per instantiation, not on the launch path (measured at degree
  // 2 on 64^3 cells, cG(1): 2 per CU 0.41 ms, 3: 0.50, 4: 0.43, 8: 0.45, one workgroup per 8 cells: 0.52 - long runs keep the prefetch
  // of the next cell's DoFs going and leave no partial round)
  static int resident_of[8] = {};
  const int resident = stokes_resident(resident_of[which], kern);
  static const int grid_env = [] {
    const char *e = getenv("STFEM_STOKES_GRID"); // workgroups per CU of a colour launch at degree 2 (experiments)
    return e ? std::max(1, atoi(e)) : 0;
  }();
  stfem_launch_begin();
  stokes_colour_launches(c, cells, grid_env && DEG == 2 ? grid_env : resident, c->cell_plan, [&](int colour, unsigned grid) {
    prm.colour = colour; // (ascending: see store_u / store_p)
    (void)hipLaunchKernel(kern, dim3(grid), dim3(256), args, 0, st);
    c->cell_launched = true;
  });
  return stfem_launch_end("stokes_cell_kernel");
}

} // namespace

int stokes_cell_launch(stfem_stokes_ctx *c, const StokesSet &set, hipStream_t st)
{
  return stokes_with_degree(c, [&](auto deg) { return cell_launch<deg()>(c, set, st); });
}
