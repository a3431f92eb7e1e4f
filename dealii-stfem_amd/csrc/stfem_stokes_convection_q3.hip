// Stokes two-field operator at velocity degree 3 (FE_Q(3)^3, QGauss(4)): the convection term of the Navier-Stokes modes, the degree-3
// counterpart of stokes_convection_kernel.  The meaning is that of the header comment of stfem_stokes_convection.hip, without the
// weak-face part (a degree-3 context has no weak faces): with the linearisation velocity b and the source velocity u, both read as
// read_dof_values reads them, at the operator's own 4 x 4 x 4 Gauss points
//   form     : out_u += - int (u (x) b) : grad v
//   jacobian : out_u += - int (b (x) u + u (x) b) : grad v
// Pressure rows and constrained velocity rows receive nothing.  The launches follow the linear cell launches of the same set, which
// have written every destination: read, add, write - eight colour launches (cells of one colour share no DoF), ascending, no atomics,
// no zeroing, a fixed summation order, bitwise reproducible.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

// The layout of stokes_cell_kernel<3, ...> (stfem_stokes_cell.hip): one wave per cell, lane t = a + 4 b + 16 c its velocity node and its
// Gauss point (a, b, c), 256 threads = 4 cells at a time, persistent workgroups that walk contiguous runs of cells, the next cell's DoFs
// (6 doubles per lane and source: u and b) fetched while this one is computed, two wave-private LDS regions per cell handed between the
// sum-factorised 1D stages and ordered with wave_fence(): no workgroup barrier inside the cell loop.
//   evaluate  (values only, six fields u_0..2, b_0..2): lane (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point
//   integrate (gradients only, nine fields F[i][e]):    lane (q_x, q_y, n_z) -> (q_x, n_y, n_z) -> velocity node
// The rows of the lane's quadrature index (evaluation) are held in registers, the columns of its node index (integration) are read from
// LDS where they are used, as the cell kernel has them at this degree (COLUMNS_HELD there).
// CART: constant diagonal Jacobian (the context was created without vertices); otherwise MappingQ1 from the eight cell vertices.
// MULTI: every source s has its own b_s; the weighted results are summed in registers per destination (up to MAXSRC), one scatter;
// otherwise one source, the weights applied at scatter time to up to MAXOUT destinations.
// JACOBIAN: the flux of the jacobian mode, otherwise that of the form mode.
template <bool CART, bool MULTI, bool JACOBIAN>
__global__ __launch_bounds__(256) void stokes_convection_q3_kernel(const ConvectionQ3Params prm)
{
  constexpr int N1 = 4, N2 = N1 * N1, NN = N1 * N2, CELLS = 256 / NN;
  constexpr int R = 9 * NN; // doubles per cell of each region (largest stage: 9 x 64)
  __shared__ double smem[CELLS * 2 * R + 2 * N2];
  double *const tS = smem + CELLS * 2 * R, *const tD = tS + N2; // 1D tables [q*4+a]
  if (threadIdx.x < N2) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x / NN, t = threadIdx.x % NN;
  const int a = t % N1, b = (t / N1) % N1, c = t / N2;
  double *X = smem + slot * (2 * R), *Y = X + R;
  // evaluation: row of this lane's quadrature index; integration: column of this lane's node index
  const Coef<N1, 1, true> Sa(tS + N1 * a), Sb(tS + N1 * b), Sc(tS + N1 * c);
  const Coef<N1, N1, false> SaT(tS + a), DaT(tD + a), SbT(tS + b), DbT(tD + b), ScT(tS + c), DcT(tD + c);
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  const int px = prm.colour & 1, py = (prm.colour >> 1) & 1, pz = prm.colour >> 2;
  const int ncxc = (prm.ncx - px + 1) / 2, ncyc = (prm.ncy - py + 1) / 2, nczc = (prm.ncz - pz + 1) / 2;
  const long long ncells = (long long)ncxc * ncyc * nczc;
  // every wave walks through its own contiguous run of the colour's cells
  const long long nslot = (long long)gridDim.x * CELLS, run = (ncells + nslot - 1) / nslot;
  const long long first = ((long long)blockIdx.x * CELLS + slot) * run;
  struct CellIds {
    int cx, cy, cz;
    bool ok, con;
    long long gu;
  };
  auto ids = [&](long long cell) {
    CellIds q;
    q.ok = cell < ncells && cell < first + run;
    const long long cc = q.ok ? cell : 0;
    q.cx = 2 * int(cc % ncxc) + px; q.cy = 2 * int((cc / ncxc) % ncyc) + py; q.cz = 2 * int(cc / ((long long)ncxc * ncyc)) + pz;
    const int ix = 3 * q.cx + a, iy = 3 * q.cy + b, iz = 3 * q.cz + c;
    q.con = constrained_u(prm, ix, iy, iz);
    q.gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    return q;
  };
  double un[3] = {0, 0, 0}, bn[3] = {0, 0, 0};
  const int nsrc = MULTI ? prm.nsrc : 1;
  auto fetch = [&](const CellIds &q, int s) { // read_dof_values: constrained entries of u and of b read as 0
    const double *us = prm.us[MULTI ? s : 0], *bs = prm.bs[MULTI ? s : 0];
    if (q.ok && !q.con) {
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

    // ---- gather: X = u[3][64], b[3][64]
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) { X[comp * NN + t] = un[comp]; X[(3 + comp) * NN + t] = bn[comp]; }
    nxt = ids(first + (it2 + 1) / nsrc);
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

    // ---- quadrature-point operation (operators.h:1554-1567): F[i][j] = - u_i b_j (- b_i u_j), pulled back -> Y[(i*3+e)*64 + t]
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
      double Ji[3][3], det;
      cip_jacobian(prm, cx, cy, cz, xi, Ji, det); // (J^-1 and det J of the trilinear mapping at this lane's point)
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
    if (cur.ok && !con && src == nsrc - 1) {
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

} // namespace

int stokes_convection_q3_launch(stfem_stokes_ctx *c, const StokesParams &prm, const double *const *lin, int mode, hipStream_t st)
{
  if (mode != STFEM_CONVECTION_FORM && mode != STFEM_CONVECTION_JACOBIAN) return STFEM_ERR_INVALID_ARGUMENT;
  if (c->degree != 3) return STFEM_ERR_UNSUPPORTED;
  if (prm.nsrc < 1 || prm.nsrc > MAXSRC || prm.nout > (prm.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiations' bounds)
  const StokesParamsT<3> &g = c->base3; // geometry and tables: `prm` carries the set alone on a degree-3 context
  ConvectionQ3Params k;
  k.vertices = g.vertices;
  k.ncx = g.ncx; k.ncy = g.ncy; k.ncz = g.ncz;
  for (int d = 0; d < 3; ++d) { k.ndu[d] = g.ndu[d]; k.hinv[d] = g.hinv[d]; }
  k.Nu = g.Nu;
  k.dmask = g.dmask;
  for (int i = 0; i < 16; ++i) { k.Su[i] = g.Su[i]; k.Du[i] = g.Du[i]; }
  for (int i = 0; i < 4; ++i) { k.xq[i] = g.xq[i]; k.wq[i] = g.wq[i]; }
  k.colour = 0; k.cart = g.cart;
  k.detJ = g.detJ;
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

  const bool multi = prm.nsrc > 1, jac = mode == STFEM_CONVECTION_JACOBIAN;
  const int which = (jac ? 4 : 0) + (multi ? 2 : 0) + (k.cart ? 1 : 0);
  const void *kerns[8] = {(const void *)stokes_convection_q3_kernel<false, false, false>, (const void *)stokes_convection_q3_kernel<true, false, false>,
                          (const void *)stokes_convection_q3_kernel<false, true, false>,  (const void *)stokes_convection_q3_kernel<true, true, false>,
                          (const void *)stokes_convection_q3_kernel<false, false, true>,  (const void *)stokes_convection_q3_kernel<true, false, true>,
                          (const void *)stokes_convection_q3_kernel<false, true, true>,   (const void *)stokes_convection_q3_kernel<true, true, true>};
  const void *kern = kerns[which];
  // resident workgroups per CU of the instantiations, asked once (not on the launch path); persistent workgroups as in stokes_cell_launch
  static int resident_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int &resident = resident_of[which];
  if (resident < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, 256, 0) != hipSuccess || resident < 1)) resident = 2;
  // STFEM_STOKES_Q3_WORKGROUPS=<n>, read at every launch: at most n workgroups per colour launch (tests: several cells per wave)
  long long cap = 0;
  if (const char *e = getenv("STFEM_STOKES_Q3_WORKGROUPS")) cap = std::max(1ll, atoll(e));
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) { // ascending, like every colour sequence of the operator
    const long long n = (long long)((c->nc[0] - (colour & 1) + 1) / 2) * ((c->nc[1] - ((colour >> 1) & 1) + 1) / 2) *
                        ((c->nc[2] - (colour >> 2) + 1) / 2);
    if (n == 0) continue;
    k.colour = colour;
    long long grid = std::min<long long>((n + 3) / 4, (long long)c->n_cu * resident);
    if (cap) grid = std::min(grid, cap);
    void *args[] = {(void *)&k};
    (void)hipLaunchKernel(kern, dim3((unsigned)grid), dim3(256), args, 0, st);
    c->convection_launched = true;
    c->convection_plan[0] = (int)grid;
    c->convection_plan[1] = (int)((n + grid * 4 - 1) / (grid * 4));
  }
  return stfem_launch_end("stokes_convection_q3_kernel");
}
