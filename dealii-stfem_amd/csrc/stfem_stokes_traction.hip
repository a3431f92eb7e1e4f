// Stokes two-field operator: the force on boundary faces,
//   StokesMatrixFreeOperator::compute_drag_lift (reference include/operators.h:1344-1389):
//   f = scale sum_{faces of obstacle_id} sum_q ( p n - nu (grad u + grad u^T) n ) JxW_face   (tau of 1372-1377, integrate_value 1379)
// at the operator's 3 x 3 face Gauss points, n the outward unit normal (J^-T e_d normalised, signed by the side), JxW_face and the
// normal from stfem_mapping_q1.h, as the weak-face kernel takes them (stfem_stokes_boundary.hip).  The full physical gradient at a
// face point: tangential derivatives from Su / Du, the normal one from the end-point derivative table EDu, all with the cell's own
// Jacobian.
// Work items are the pairs (selected face, boundary cell of that face) in the order of stfem_stokes_face_points; nothing is scattered,
// so there are no colours: one launch over all items, every item writes its three sums, then one workgroup sums the items in a fixed
// order - no atomics, bitwise reproducible.  Up to MAXSRC (u, p) pairs ride in one launch of each stage: the geometry of an item is
// computed once for all of them, the arithmetic of a pair does not depend on how many ride along.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cmath>

namespace {

struct TractionParams {
  const double *vertices; // device, (nc+1)^3 * 3
  int ncx, ncy, ncz;
  int ndu[3], ndp[3];
  long long Nu;
  int dmask, pdg;
  int read_plain;          // 0: velocity entries on strongly constrained DoFs read as 0 (read_dof_values); 1: as stored
  double nu;
  int foff[7];             // first item (cell of a face, lower tangential axis fastest) of every selected face, [6] = total
  int nsrc;
  const double *us[MAXSRC], *ps[MAXSRC];
  double *items;           // [source][item][3], the unscaled force of every item
  double Su[9], Du[9], Sp[6];  // [q*3+a], [q*3+a], [q*2+a] at the Gauss points
  double Eu[6], EDu[6], Ep[4]; // [s*n+a] at the end points 0 and 1
  double xq[3], wq[3];
};

// The item layout of stokes_boundary_kernel: one half-wave per item, 256 threads = 8 items at a time, the cell's velocity and
// pressure values staged through a wave-private LDS region, lanes 0..8 own the face points (q = q1 + 3 q2), lane 0 sums them.
__global__ __launch_bounds__(256) void stokes_traction_kernel(const TractionParams prm)
{
  __shared__ double tS[9], tD[9], tP[6], tE[6], tED[6], tEP[4], tX[3], tW[3];
  __shared__ double sX[8][89], sT[8][9][3];
  if (threadIdx.x < 9) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < 6) { tP[threadIdx.x] = prm.Sp[threadIdx.x]; tE[threadIdx.x] = prm.Eu[threadIdx.x]; tED[threadIdx.x] = prm.EDu[threadIdx.x]; }
  if (threadIdx.x < 4) tEP[threadIdx.x] = prm.Ep[threadIdx.x];
  if (threadIdx.x < 3) { tX[threadIdx.x] = prm.xq[threadIdx.x]; tW[threadIdx.x] = prm.wq[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  const bool pnode = prm.pdg ? t32 < 4 : (lane27 && a < 2 && b < 2 && c < 2);
  const int pslot = prm.pdg ? (t32 & 3) : a + 2 * b + 4 * c;
  const long long nitems = prm.foff[6];
  double *X = sX[slot];
  // (the trip count is the same for the eight items of a workgroup: the two half-waves of a wave fence together)
  for (long long first = (long long)blockIdx.x * 8; first < nitems; first += (long long)gridDim.x * 8) {
    const long long item = first + slot;
    const bool ok = item < nitems;
    int f0 = 0, base = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f)
      if (ok && item >= prm.foff[f] && item < prm.foff[f + 1]) { f0 = f; base = prm.foff[f]; }
    const int d = f0 >> 1, s = f0 & 1; // (tangential axes: t1 = d == 0 ? 1 : 0 < t2 = d == 2 ? 1 : 2)
    // (selects, not indexed arrays: the cell and the face point stay in registers)
    const int n1 = d == 0 ? prm.ncy : prm.ncx, nd = d == 0 ? prm.ncx : (d == 1 ? prm.ncy : prm.ncz);
    const long long e = ok ? item - base : 0;
    const int c1 = int(e % n1), c2 = int(e / n1), cd = s ? nd - 1 : 0;
    const int cx = d == 0 ? cd : c1, cy = d == 1 ? cd : (d == 0 ? c1 : c2), cz = d == 2 ? cd : c2;
    const int ix = 2 * cx + a, iy = 2 * cy + b, iz = 2 * cz + c;
    const bool zero = !prm.read_plain && constrained_u(prm, ix, iy, iz);
    const long long gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    const long long gp = prm.pdg ? (cx + (long long)prm.ncx * (cy + (long long)prm.ncy * cz)) * 4 + (t32 & 3)
                                 : (cx + (a < 2 ? a : 1)) + (long long)prm.ndp[0] * ((cy + (b < 2 ? b : 1)) + (long long)prm.ndp[1] * (cz + (c < 2 ? c : 1)));
    const int q1 = t32 % 3, q2 = (t32 / 3) % 3;
    const bool point = ok && t32 < 9;
    // 1D tables of face point (q1, q2), per direction: values and derivatives of the three FE_Q(2) nodes, values of the two FE_Q(1)
    // nodes - the end-point tables along the face's direction d, the Gauss-point tables along the tangential ones (t1 < t2)
    const int qx = q1, qy = d == 0 ? q1 : q2, qz = q2; // the Gauss index along x, y, z where that direction is tangential
    double vx[3], dx[3], vy[3], dy[3], vz[3], dz[3], px[2], py[2], pz[2];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      vx[n] = d == 0 ? tE[s * 3 + n] : tS[qx * 3 + n]; dx[n] = d == 0 ? tED[s * 3 + n] : tD[qx * 3 + n];
      vy[n] = d == 1 ? tE[s * 3 + n] : tS[qy * 3 + n]; dy[n] = d == 1 ? tED[s * 3 + n] : tD[qy * 3 + n];
      vz[n] = d == 2 ? tE[s * 3 + n] : tS[qz * 3 + n]; dz[n] = d == 2 ? tED[s * 3 + n] : tD[qz * 3 + n];
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      px[n] = d == 0 ? tEP[s * 2 + n] : tP[qx * 2 + n];
      py[n] = d == 1 ? tEP[s * 2 + n] : tP[qy * 2 + n];
      pz[n] = d == 2 ? tEP[s * 2 + n] : tP[qz * 2 + n];
    }
    // FE_DGP(1) functions 1, l(xi), l(eta), l(zeta) at the face point, l(x) = sqrt 3 (2 x - 1)
    const double lx = 1.7320508075688772 * (2.0 * (d == 0 ? double(s) : tX[qx]) - 1.0);
    const double ly = 1.7320508075688772 * (2.0 * (d == 1 ? double(s) : tX[qy]) - 1.0);
    const double lz = 1.7320508075688772 * (2.0 * (d == 2 ? double(s) : tX[qz]) - 1.0);

    // ---- geometry of this lane's face point, once for all sources
    double Ji[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, nrm[3] = {0, 0, 0}, JxW = 0.0;
    if (point) {
      const double x1 = tX[q1], x2 = tX[q2], xd = s;
      const double xi0 = d == 0 ? xd : x1, xi1 = d == 1 ? xd : (d == 0 ? x1 : x2), xi2 = d == 2 ? xd : x2;
      const double xi[3] = {xi0, xi1, xi2};
      const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
      const double len = mapping_q1_face_normal(Ji, d, s ? 1 : -1, nrm);
      JxW = fabs(det) * len * tW[q1] * tW[q2];
    }

    for (int src = 0; src < prm.nsrc; ++src) {
      // ---- gather: X = u[3][27], p[8 or 4]
      const double *us = prm.us[0], *ps = prm.ps[0];
#pragma unroll
      for (int o = 1; o < MAXSRC; ++o)
        if (src == o) { us = prm.us[o]; ps = prm.ps[o]; } // (a select: no indexed copy of the argument)
      if (lane27)
        for (int comp = 0; comp < 3; ++comp) X[comp * 27 + t] = (ok && !zero) ? us[comp * prm.Nu + gu] : 0.0;
      if (pnode) X[81 + pslot] = ok ? ps[gp] : 0.0;
      wave_fence();
      if (point) { // operators.h:1370-1378
        double gref[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, pval = 0.0; // d u_comp / d xi_e
#pragma unroll
        for (int comp = 0; comp < 3; ++comp)
#pragma unroll
          for (int kc = 0; kc < 3; ++kc)
#pragma unroll
            for (int kb = 0; kb < 3; ++kb) {
              const double *w = X + comp * 27 + 3 * kb + 9 * kc; // an x-line of the cell
              const double v = w[0] * vx[0] + w[1] * vx[1] + w[2] * vx[2], g = w[0] * dx[0] + w[1] * dx[1] + w[2] * dx[2];
              gref[comp][0] += g * (vy[kb] * vz[kc]);
              gref[comp][1] += v * (dy[kb] * vz[kc]);
              gref[comp][2] += v * (vy[kb] * dz[kc]);
            }
        if (prm.pdg) {
          pval = X[81] + X[82] * lx + X[83] * ly + X[84] * lz;
        } else {
#pragma unroll
          for (int kc = 0; kc < 2; ++kc)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) pval += (X[81 + 2 * kb + 4 * kc] * px[0] + X[82 + 2 * kb + 4 * kc] * px[1]) * (py[kb] * pz[kc]);
        }
        double grad[3][3]; // d u_comp / d x_k
        for (int comp = 0; comp < 3; ++comp)
          for (int k = 0; k < 3; ++k) grad[comp][k] = gref[comp][0] * Ji[0][k] + gref[comp][1] * Ji[1][k] + gref[comp][2] * Ji[2][k];
        for (int comp = 0; comp < 3; ++comp) {
          double sn = 0.0;
          for (int k = 0; k < 3; ++k) sn += (grad[comp][k] + grad[k][comp]) * nrm[k];
          sT[slot][t32][comp] = (pval * nrm[comp] - prm.nu * sn) * JxW;
        }
      }
      wave_fence();
      // ---- the item's sum over its nine points, in point order
      if (ok && t32 == 0) {
        double *o = prm.items + ((long long)src * nitems + item) * 3;
        for (int comp = 0; comp < 3; ++comp) {
          double sum = 0.0;
          for (int q = 0; q < 9; ++q) sum += sT[slot][q][comp];
          o[comp] = sum;
        }
      }
      wave_fence(); // the next source, or the next item, overwrites X and the point buffer
    }
  }
}

// stage 2: out[i][comp] = sum of the item values of source i - strided partial sums in item order, then a tree with fixed shape
// (stokes_divergence_finish), one sum after the other in ONE workgroup
__global__ __launch_bounds__(256) void stokes_traction_finish(long long nitems, int nsrc, const double *__restrict__ items, double *__restrict__ out)
{
  __shared__ double red[256];
  for (int k = 0; k < 3 * nsrc; ++k) {
    const double *v = items + (long long)(k / 3) * nitems * 3 + k % 3;
    double s = 0.0;
    for (long long i = threadIdx.x; i < nitems; i += 256) s += v[3 * i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (int(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = red[0];
    __syncthreads(); // red is reused by the next sum
  }
}

// first item of every face of the mask (stfem_stokes_face_points' order), [6] = the count
long long traction_offsets(const stfem_stokes_ctx *c, int face_mask, int foff[7])
{
  long long off = 0;
  for (int f = 0; f < 6; ++f) {
    foff[f] = int(off);
    const int d = f / 2, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    if (face_mask >> f & 1) off += (long long)c->nc[t1] * c->nc[t2];
  }
  foff[6] = int(off);
  return off;
}

} // namespace

extern "C" {

int64_t stfem_stokes_drag_lift_n_items(const stfem_stokes_ctx *c, int face_mask)
{
  if (!c) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift_n_items: null context");
  if (face_mask < 1 || face_mask > 63) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift_n_items: face_mask %d outside 1..63", face_mask);
  if (const int rq = stokes_require_q2(c, "stfem_stokes_drag_lift_n_items")) return rq;
  int foff[7];
  return traction_offsets(c, face_mask, foff);
}

int stfem_stokes_drag_lift(stfem_stokes_ctx *c, int face_mask, double scale, int read_plain, int n, const double *const *u,
                           const double *const *p, double *item_out, double *out, void *stream)
{
  // (all refusals before anything touches the device)
  if (!c || !u || !p || !out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift: null %s", !c ? "context" : !u ? "u" : !p ? "p" : "out");
  if (n < 1) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift: n = %d pairs", n);
  if (face_mask < 1 || face_mask > 63) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift: face_mask %d outside 1..63", face_mask);
  if (!std::isfinite(scale)) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift: scale is not finite");
  if (const int rq = stokes_require_q2(c, "stfem_stokes_drag_lift")) return rq;
  for (int i = 0; i < n; ++i)
    if (!u[i] || !p[i]) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_drag_lift: null %s[%d]", !u[i] ? "u" : "p", i);
  TractionParams k;
  const long long nitems = traction_offsets(c, face_mask, k.foff);
  if (nitems > 0x7fffffffll) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_drag_lift: %lld items", nitems);
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // scratch: [n][items][3] item values, then [n][3] sums
  const size_t need = (size_t(nitems) * 3 + 3) * size_t(n);
  if (c->trac_cap < need) {
    if (c->d_trac) STFEM_TRY(hipFree(c->d_trac));
    c->d_trac = nullptr;
    c->trac_cap = 0;
    if (hipMalloc(&c->d_trac, need * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      c->d_trac = nullptr;
      return stfem_set_error(STFEM_ERR_OUT_OF_MEMORY, "stfem_stokes_drag_lift: %zu doubles of scratch", need);
    }
    c->trac_cap = need;
  }
  double *items = item_out ? item_out : c->d_trac, *sums = c->d_trac + size_t(nitems) * 3 * size_t(n);
  const StokesParams &b = c->desc<2>();
  k.vertices = c->d_vertices;
  k.ncx = c->nc[0]; k.ncy = c->nc[1]; k.ncz = c->nc[2];
  for (int d = 0; d < 3; ++d) { k.ndu[d] = c->ndu[d]; k.ndp[d] = c->ndp[d]; k.xq[d] = b.xq[d]; k.wq[d] = b.wq[d]; }
  k.Nu = c->Nu;
  k.dmask = c->dmask; k.pdg = c->pspace;
  k.read_plain = read_plain != 0;
  k.nu = c->nu;
  for (int i = 0; i < 9; ++i) { k.Su[i] = b.Su[i]; k.Du[i] = b.Du[i]; }
  for (int i = 0; i < 6; ++i) k.Sp[i] = b.Sp[i];
  { // FE_Q(2) values / derivatives and FE_Q(1) values at the end points 0 and 1, [s * n + a]
    const stfem::ShapeTables tu = stfem::make_shape_tables(2), tp = stfem::make_shape_tables(1);
    const std::vector<double> ends = {0.0, 1.0};
    stfem::Mat Eu, EDu, Ep, EDp;
    stfem::lagrange_tables(tu.nodes, ends, Eu, EDu);
    stfem::lagrange_tables(tp.nodes, ends, Ep, EDp);
    for (int i = 0; i < 6; ++i) { k.Eu[i] = Eu[i]; k.EDu[i] = EDu[i]; }
    for (int i = 0; i < 4; ++i) k.Ep[i] = Ep[i];
  }
  const unsigned grid = (unsigned)std::min<long long>((nitems + 7) / 8, 4ll * c->n_cu);
  stfem_launch_begin();
  for (int g0 = 0; g0 < n; g0 += MAXSRC) { // one launch of each stage per group of MAXSRC pairs
    k.nsrc = std::min(MAXSRC, n - g0);
    for (int s = 0; s < MAXSRC; ++s) {
      k.us[s] = s < k.nsrc ? u[g0 + s] : nullptr;
      k.ps[s] = s < k.nsrc ? p[g0 + s] : nullptr;
    }
    k.items = items + size_t(g0) * size_t(nitems) * 3;
    hipLaunchKernelGGL(stokes_traction_kernel, dim3(grid), dim3(256), 0, st, k);
    hipLaunchKernelGGL(stokes_traction_finish, dim3(1), dim3(256), 0, st, nitems, k.nsrc, (const double *)k.items, sums + 3 * size_t(g0));
  }
  if (const int rc = stfem_launch_end("stokes_traction_kernel")) return rc;
  std::vector<double> h(3 * size_t(n));
  STFEM_TRY(hipMemcpyAsync(h.data(), sums, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < h.size(); ++i) out[i] = scale * h[i];
  return STFEM_OK;
}

} // extern "C"
