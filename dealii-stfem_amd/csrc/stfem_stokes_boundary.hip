// Stokes two-field operator: the weak (Nitsche) boundary faces, for velocity degree DEG = 2 and 3.
// The boundary faces of the linear operator (LoopType::Full, reference include/operators.h:1640-1741)
// Weak (Nitsche) faces: v <- -nu grad u n + p n + gamma1/h u + gamma2/h n (u.n), dv/dn <- -nu u, q <- -u.n with
// gamma1 = nu penalty1, gamma2 = penalty2 (1220-1221) and h = sqrt(face area) (get_h_face, 184-209); outflow faces add
// nothing to the linear operator (1680-1711: the back-flow term carries a factor 0.0, the rest is nonlinear-only).
// The same kernel evaluates StokesNitscheMatrixFreeOperator::vmult (1898-1940): the functional of the Dirichlet data g.
// One half-wave (degree 2: 27 of 32 lanes) or wave (degree 3: 64 lanes) per boundary CELL - a cell on several weak faces is handled
// once, by its lowest face, for all of them; eight colour launches after the cell loop's, plain read-add-write: no atomics,
// reproducible.  Lane t = a + (DEG + 1) b + (DEG + 1)^2 c is velocity node (a, b, c); the first (DEG + 1)^2 lanes are the face's Gauss
// points q1 + (DEG + 1) q2, lower tangential direction fastest; the FE_Q(DEG - 1) pressure rides on the lanes with a, b, c < DEG, the
// FE_DGP(DEG - 1) functions on the first 4 or 10 lanes.  A face point is evaluated as a direct sum over the cell's nodes, c slowest, a
// fastest, on its own lane (the work scales with the surface); the integration sums over the face points in ascending order.
// Face geometry: stfem_mapping_q1.h.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {


// MULTI: several sources, their weighted sums in registers (operator mode only); otherwise one source, or the data g (rhs mode:
// no source is read), with the weights applied at scatter time
template <int DEG, bool MULTI>
__global__ __launch_bounds__(256) void stokes_boundary_kernel(const StokesParamsT<DEG> prm, const BoundaryParams bp)
{
  constexpr int N1 = DEG + 1, N2 = N1 * N1, NN = N1 * N2; // nodes per direction, face points, nodes per cell
  constexpr int LANES = NN <= 32 ? 32 : 64, SLOTS = 256 / LANES;
  constexpr int NPQ = DEG * DEG * DEG, NDGP = DEG * (DEG + 1) * (DEG + 2) / 6; // pressure DoFs of a cell: FE_Q(DEG - 1), FE_DGP(DEG - 1)
  constexpr int XP = 3 * NN;                                                   // the cell's pressure values: X[XP ..]
  __shared__ double tS[N2], tD[N2], tP[N1 * DEG], tE[2 * N1], tED[2 * N1], tEP[2 * DEG], tX[N1], tW[N1], tL[DEG == 2 ? 1 : (DEG - 1) * N1];
  __shared__ double sX[SLOTS][XP + (NPQ > NDGP ? NPQ : NDGP)], sF[SLOTS][N2][7], sG[SLOTS][N2][12], sJ[SLOTS][N2];
  if (threadIdx.x < N2) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  if (threadIdx.x < N1 * DEG) tP[threadIdx.x] = prm.Sp[threadIdx.x];
  if (threadIdx.x < 2 * N1) { tE[threadIdx.x] = bp.Eu[threadIdx.x]; tED[threadIdx.x] = bp.EDu[threadIdx.x]; }
  if (threadIdx.x < 2 * DEG) tEP[threadIdx.x] = bp.Ep[threadIdx.x];
  if (threadIdx.x < N1) { tX[threadIdx.x] = prm.xq[threadIdx.x]; tW[threadIdx.x] = prm.wq[threadIdx.x]; }
  if constexpr (DEG > 2) {
    if (threadIdx.x < (DEG - 1) * N1) tL[threadIdx.x] = prm.lq[threadIdx.x / N1][threadIdx.x % N1]; // l_1, l_2 at the Gauss points
  }
  __syncthreads();
  const int slot = threadIdx.x / LANES, tl = threadIdx.x % LANES;
  const bool lane_on = NN == LANES || tl < NN;
  const int t = lane_on ? tl : 0;
  const int a = t % N1, b = (t / N1) % N1, c = t / N2;
  const bool pnode = prm.pdg ? tl < NDGP : (lane_on && a < DEG && b < DEG && c < DEG);
  const int pslot = prm.pdg ? tl : a + DEG * b + DEG * DEG * c;
  // FE_DGP: the degrees (i, j, k) of the function this lane integrates
  int ei = 0, ej = 0, ek = 0;
  {
    constexpr DgpDegrees<DEG> dgp = dgp_degrees<DEG>();
#pragma unroll
    for (int f = 0; f < NDGP; ++f)
      if (tl == f) { ei = dgp.d[f][0]; ej = dgp.d[f][1]; ek = dgp.d[f][2]; }
  }
  const int nc[3] = {prm.ncx, prm.ncy, prm.ncz};
  double *X = sX[slot];
  for (long long item = (long long)blockIdx.x * SLOTS + slot; item - slot < bp.foff[6]; item += (long long)gridDim.x * SLOTS) {
    // (all slots of the workgroup run the same number of rounds: nothing below is a workgroup barrier, but keep it uniform)
    bool ok = item < bp.foff[6];
    int f0 = 0;
    for (int f = 0; f < 6; ++f)
      if (ok && item >= bp.foff[f] && item < bp.foff[f + 1]) f0 = f;
    int cc[3] = {0, 0, 0};
    {
      const int d = f0 >> 1, s = f0 & 1, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
      const long long e = ok ? item - bp.foff[f0] : 0;
      cc[d] = s ? nc[d] - 1 : 0;
      cc[t1] = int(e % nc[t1]);
      cc[t2] = int(e / nc[t1]);
    }
    const int cx = cc[0], cy = cc[1], cz = cc[2];
    ok = ok && ((cx & 1) + 2 * (cy & 1) + 4 * (cz & 1)) == prm.colour;
    // the cell's weak faces; it is handled by the lowest of them
    int faces = 0;
    for (int f = 0; f < 6; ++f) {
      const int d = f >> 1, s = f & 1;
      if ((bp.weak_mask >> f & 1) && cc[d] == (s ? nc[d] - 1 : 0)) faces |= 1 << f;
    }
    ok = ok && (faces & ((1 << f0) - 1)) == 0;
    if (!__builtin_amdgcn_readfirstlane(__ballot(ok) != 0)) continue; // (wave-uniform skip only: the half-waves of a wave fence together)
    const int ix = DEG * cx + a, iy = DEG * cy + b, iz = DEG * cz + c;
    const bool con = constrained_u(prm, ix, iy, iz);
    const long long gu = ix + (long long)prm.ndu[0] * (iy + (long long)prm.ndu[1] * iz);
    const long long gp = prm.pdg ? (cx + (long long)prm.ncx * (cy + (long long)prm.ncy * cz)) * NDGP + (tl < NDGP ? tl : 0)
                                 : ((DEG - 1) * cx + (a < DEG ? a : DEG - 1)) +
                                       (long long)prm.ndp[0] * (((DEG - 1) * cy + (b < DEG ? b : DEG - 1)) + (long long)prm.ndp[1] * ((DEG - 1) * cz + (c < DEG ? c : DEG - 1)));
    double accU[MULTI ? MAXSRC : 1][3], accP[MULTI ? MAXSRC : 1];
#pragma unroll
    for (int o = 0; o < (MULTI ? MAXSRC : 1); ++o) accU[o][0] = accU[o][1] = accU[o][2] = accP[o] = 0.0;
    const int nsrc = MULTI ? prm.nsrc : 1;
    for (int src = 0; src < nsrc; ++src) {
      if (!bp.g) { // gather (read_dof_values: constrained velocity entries read as 0)
        const double *us = prm.us[src], *ps = prm.ps[src];
        if (lane_on)
          for (int comp = 0; comp < 3; ++comp) X[comp * NN + t] = (ok && !con) ? us[comp * prm.Nu + gu] : 0.0;
        if (pnode) X[XP + pslot] = (ok && ps) ? ps[gp] : 0.0;
      }
      double rU[3] = {0, 0, 0}, rP = 0.0;
      for (int f = 0; f < 6; ++f) {
        if (!__builtin_amdgcn_readfirstlane(__ballot(ok && (faces >> f & 1)) != 0)) continue;
        const bool on = ok && (faces >> f & 1); // per slot
        const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
        const int q1 = tl % N1, q2 = (tl / N1) % N1;
        // 1D tables of face point (q1, q2) / of any point q: value and derivative of node n along direction dir
        auto tv = [&](int dir, int qa, int qb, int n) { return dir == d ? tE[s * N1 + n] : tS[(dir == t1 ? qa : qb) * N1 + n]; };
        auto td = [&](int dir, int qa, int qb, int n) { return dir == d ? tED[s * N1 + n] : tD[(dir == t1 ? qa : qb) * N1 + n]; };
        auto tp = [&](int dir, int qa, int qb, int n) { return dir == d ? tEP[s * DEG + n] : tP[(dir == t1 ? qa : qb) * DEG + n]; };
        // FE_DGP(DEG - 1) at face point (qa, qb).  Degree 2, function j: 1, l(xi), l(eta), l(zeta), l(x) = sqrt 3 (2 x - 1); degree 3,
        // degrees (i, j, k): l_i(xi) l_j(eta) l_k(zeta) from the tables of the cell kernel, at the end points l_1 = -+ sqrt 3, l_2 = sqrt 5
        auto dg = [&](int j, int qa, int qb) {
          if (j == 0) return 1.0;
          const int dir = j - 1;
          const double x = dir == d ? double(s) : tX[dir == t1 ? qa : qb];
          return 1.7320508075688772 * (2.0 * x - 1.0);
        };
        auto leg = [&](int n, int dir, int qa, int qb) {
          if (n == 0) return 1.0;
          if (dir == d) return n == 1 ? (s ? 1.7320508075688772 : -1.7320508075688772) : 2.23606797749979;
          return tL[(n - 1) * N1 + (dir == t1 ? qa : qb)];
        };
        auto dg3 = [&](int i, int j, int k, int qa, int qb) { return leg(i, 0, qa, qb) * leg(j, 1, qa, qb) * leg(k, 2, qa, qb); };
        double Ji[3][3], nrm[3], JxW = 0.0;
        if (on && tl < N2) { // geometry of this lane's face point
          double xi[3];
          xi[d] = s; xi[t1] = tX[q1]; xi[t2] = tX[q2];
          const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
          const double len = mapping_q1_face_normal(Ji, d, s ? 1 : -1, nrm);
          JxW = fabs(det) * len * tW[q1] * tW[q2];
          sJ[slot][tl] = JxW;
        }
        wave_fence();
        if (on && tl < N2) {
          double area = 0.0;
          for (int q = 0; q < N2; ++q) area += sJ[slot][q];
          const double h = sqrt(area); // get_h_face: area^(1 / (dim - 1))
          double val[3], nd[3], pq;
          if (bp.g) { // operators.h:1921-1932
            const int c1 = cc[t1], c2 = cc[t2];
            long long pt = 0;
            for (int ff = 0; ff < f; ++ff)
              if (bp.weak_mask >> ff & 1) pt += (long long)N2 * (bp.foff[ff + 1] - bp.foff[ff]);
            pt += (long long)N2 * (c1 + (long long)nc[t1] * c2) + tl;
            const double g0 = bp.g[3 * pt], g1 = bp.g[3 * pt + 1], g2 = bp.g[3 * pt + 2];
            const double gq[3] = {g0, g1, g2};
            const double gn = g0 * nrm[0] + g1 * nrm[1] + g2 * nrm[2];
            for (int comp = 0; comp < 3; ++comp) {
              val[comp] = ((bp.gamma1 / h) * gq[comp] + (bp.gamma2 / h) * nrm[comp] * gn) * JxW;
              nd[comp] = -prm.nu * gq[comp] * JxW;
            }
            pq = -gn * JxW;
          } else { // operators.h:1720-1739
            double uval[3] = {0, 0, 0}, gref[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, pval = 0.0;
            for (int kc = 0; kc < N1; ++kc)
              for (int kb = 0; kb < N1; ++kb)
                for (int ka = 0; ka < N1; ++ka) {
                  const double sx = tv(0, q1, q2, ka), sy = tv(1, q1, q2, kb), sz = tv(2, q1, q2, kc);
                  const double dx = td(0, q1, q2, ka) * sy * sz, dy = sx * td(1, q1, q2, kb) * sz, dz = sx * sy * td(2, q1, q2, kc);
                  for (int comp = 0; comp < 3; ++comp) {
                    const double w = X[comp * NN + ka + N1 * kb + N2 * kc];
                    gref[comp][0] += w * dx; gref[comp][1] += w * dy; gref[comp][2] += w * dz;
                    uval[comp] += w * sx * sy * sz;
                  }
                }
            if (prm.pdg) {
              if constexpr (DEG == 2) {
                for (int j = 0; j < 4; ++j) pval += X[XP + j] * dg(j, q1, q2);
              } else {
                constexpr DgpDegrees<DEG> dgp = dgp_degrees<DEG>();
#pragma unroll
                for (int j = 0; j < NDGP; ++j) pval += X[XP + j] * dg3(dgp.d[j][0], dgp.d[j][1], dgp.d[j][2], q1, q2);
              }
            } else
            for (int kc = 0; kc < DEG; ++kc)
              for (int kb = 0; kb < DEG; ++kb)
                for (int ka = 0; ka < DEG; ++ka)
                  pval += X[XP + ka + DEG * kb + DEG * DEG * kc] * tp(0, q1, q2, ka) * tp(1, q1, q2, kb) * tp(2, q1, q2, kc);
            double un = 0.0, gn[3];
            for (int comp = 0; comp < 3; ++comp) {
              gn[comp] = 0.0;
              for (int k = 0; k < 3; ++k)
                gn[comp] += (gref[comp][0] * Ji[0][k] + gref[comp][1] * Ji[1][k] + gref[comp][2] * Ji[2][k]) * nrm[k];
              un += uval[comp] * nrm[comp];
            }
            for (int comp = 0; comp < 3; ++comp) {
              val[comp] = (-prm.nu * gn[comp] + pval * nrm[comp] + (bp.gamma1 / h) * uval[comp] + (bp.gamma2 / h) * nrm[comp] * un) * JxW;
              nd[comp] = -prm.nu * uval[comp] * JxW;
            }
            pq = -un * JxW;
          }
          double *F = sF[slot][tl], *G = sG[slot][tl];
          for (int comp = 0; comp < 3; ++comp) { F[comp] = val[comp]; F[3 + comp] = nd[comp]; }
          F[6] = pq;
          for (int e = 0; e < 3; ++e)
            for (int k = 0; k < 3; ++k) G[3 * e + k] = Ji[e][k];
          for (int k = 0; k < 3; ++k) G[9 + k] = nrm[k];
        }
        wave_fence();
        if (on && lane_on) { // integrate: test values and test normal derivatives of node (a, b, c)
          for (int q = 0; q < N2; ++q) {
            const int qa = q % N1, qb = q / N1;
            const double *F = sF[slot][q], *G = sG[slot][q];
            const double sx = tv(0, qa, qb, a), sy = tv(1, qa, qb, b), sz = tv(2, qa, qb, c);
            const double gr[3] = {td(0, qa, qb, a) * sy * sz, sx * td(1, qa, qb, b) * sz, sx * sy * td(2, qa, qb, c)};
            double dn = 0.0;
            for (int k = 0; k < 3; ++k) dn += (gr[0] * G[k] + gr[1] * G[3 + k] + gr[2] * G[6 + k]) * G[9 + k];
            const double v = sx * sy * sz;
            for (int comp = 0; comp < 3; ++comp) rU[comp] += v * F[comp] + dn * F[3 + comp];
            if (pnode) {
              if constexpr (DEG == 2) rP += (prm.pdg ? dg(tl & 3, qa, qb) : tp(0, qa, qb, a) * tp(1, qa, qb, b) * tp(2, qa, qb, c)) * F[6];
              else rP += (prm.pdg ? dg3(ei, ej, ek, qa, qb) : tp(0, qa, qb, a) * tp(1, qa, qb, b) * tp(2, qa, qb, c)) * F[6];
            }
          }
        }
        wave_fence(); // the next face reuses the point buffers
      }
      if constexpr (MULTI) {
#pragma unroll
        for (int o = 0; o < MAXSRC; ++o)
          if (o < prm.nout) {
            for (int comp = 0; comp < 3; ++comp) accU[o][comp] = fma(prm.wKu[src][o], rU[comp], accU[o][comp]);
            accP[o] = fma(prm.wKp[src][o], rP, accP[o]);
          }
      } else {
        for (int comp = 0; comp < 3; ++comp) accU[0][comp] = rU[comp];
        accP[0] = rP;
      }
      wave_fence(); // the next source overwrites X
    }
    // distribute_local_to_global (add): constrained velocity rows are not written
    if (ok && lane_on) {
      for (int o = 0; o < prm.nout; ++o) {
        const double kU = MULTI ? 1.0 : prm.wKu[0][o], kP = MULTI ? 1.0 : prm.wKp[0][o]; // (several sources: the weights are in the sums)
        const int oa = MULTI ? o : 0;
        if (prm.out_u[o] && !con && kU != 0.0) {
          double *dptr = prm.out_u[o] + gu;
          for (int comp = 0; comp < 3; ++comp) dptr[comp * prm.Nu] += kU * accU[oa][comp];
        }
        if (pnode && prm.out_p[o] && kP != 0.0) prm.out_p[o][gp] += kP * accP[oa];
      }
    }
  }
}

template <int DEG> int boundary_launch(stfem_stokes_ctx *c, const StokesSet &set, const BoundaryParams &bp, hipStream_t st)
{
  constexpr int SLOTS = DEG == 2 ? 8 : 4; // boundary cells of a workgroup at a time
  const long long items = bp.foff[6];
  StokesParamsT<DEG> prm = stokes_params<DEG>(c, set);
  long long grid = std::min<long long>((items + SLOTS - 1) / SLOTS, 4ll * c->n_cu);
  if (const char *e = getenv("STFEM_STOKES_FACE_WORKGROUPS")) grid = std::min(grid, std::max(1ll, atoll(e)));
  stfem_launch_begin();
  for (int colour = 0; colour < 8; ++colour) {
    prm.colour = colour;
    if (prm.nsrc > 1) hipLaunchKernelGGL((stokes_boundary_kernel<DEG, true>), dim3((unsigned)grid), dim3(256), 0, st, prm, bp);
    else hipLaunchKernelGGL((stokes_boundary_kernel<DEG, false>), dim3((unsigned)grid), dim3(256), 0, st, prm, bp);
  }
  c->face_launched = true;
  c->face_plan[0] = (int)grid;
  c->face_plan[1] = (int)((items + grid * SLOTS - 1) / (grid * SLOTS));
  return stfem_launch_end("stokes_boundary_kernel");
}

// What the setter and its _space form share: masks, penalties, work items and the end-point tables of the context's degree
int set_weak_boundaries(stfem_stokes_ctx *c, int weak_mask, int outflow_mask, double penalty1, double penalty2)
{
  // a face in both sets takes the outflow branch in the reference (1680: checked first), i.e. no term in the linear operator
  c->outflow_mask = outflow_mask;
  c->weak_mask = weak_mask & ~outflow_mask;
  c->penalty1 = penalty1;
  c->penalty2 = penalty2;
  BoundaryParams &b = c->bnd;
  std::memset(&b, 0, sizeof(b));
  b.weak_mask = c->weak_mask;
  b.gamma1 = c->nu * penalty1;
  b.gamma2 = penalty2;
  int off = 0;
  for (int f = 0; f < 6; ++f) {
    b.foff[f] = off;
    const int d = f / 2, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    if (c->weak_mask >> f & 1) off += c->nc[t1] * c->nc[t2];
  }
  b.foff[6] = off;
  const int nu1 = c->degree + 1, np1 = c->degree;
  const stfem::ShapeTables tu = stfem::make_shape_tables(c->degree), tp = stfem::make_shape_tables(c->degree - 1);
  const std::vector<double> ends = {0.0, 1.0};
  stfem::Mat Eu, EDu, Ep, EDp;
  stfem::lagrange_tables(tu.nodes, ends, Eu, EDu);
  stfem::lagrange_tables(tp.nodes, ends, Ep, EDp);
  for (int i = 0; i < 2 * nu1; ++i) { b.Eu[i] = Eu[i]; b.EDu[i] = EDu[i]; }
  for (int i = 0; i < 2 * np1; ++i) b.Ep[i] = Ep[i];
  return STFEM_OK;
}

int64_t n_face_points(const stfem_stokes_ctx *c) { return (long long)(c->degree + 1) * (c->degree + 1) * c->bnd.foff[6]; }

int face_points(const stfem_stokes_ctx *c, double *out)
{
  const int nq = c->degree + 1;
  std::vector<double> xq, wq;
  stfem::gauss_rule(nq, xq, wq);
  size_t pt = 0;
  for (int f = 0; f < 6; ++f) {
    if (!(c->weak_mask >> f & 1)) continue;
    const int d = f / 2, s = f % 2, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    for (int c2 = 0; c2 < c->nc[t2]; ++c2)
      for (int c1 = 0; c1 < c->nc[t1]; ++c1) {
        int cc[3];
        cc[d] = s ? c->nc[d] - 1 : 0; cc[t1] = c1; cc[t2] = c2;
        for (int q2 = 0; q2 < nq; ++q2)
          for (int q1 = 0; q1 < nq; ++q1, ++pt) {
            double xi[3];
            xi[d] = s; xi[t1] = xq[q1]; xi[t2] = xq[q2];
            mapping_q1_point(c->h_vertices.data(), c->nc[0], c->nc[1], cc[0], cc[1], cc[2], xi, out + 3 * pt);
          }
      }
  }
  return STFEM_OK;
}

int nitsche_rhs(stfem_stokes_ctx *c, const double *g_at_face_points, double *dst_u, double *dst_p, void *stream)
{
  const size_t npts = size_t(n_face_points(c));
  if (npts == 0) return STFEM_OK; // no Dirichlet functions: vmult does nothing (operators.h:1836)
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (c->g_points < npts) {
    if (c->d_g) STFEM_TRY(hipFree(c->d_g));
    c->d_g = nullptr;
    c->g_points = 0;
    if (hipMalloc(&c->d_g, npts * 3 * sizeof(double)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    c->g_points = npts;
  }
  STFEM_TRY(hipMemcpyAsync(c->d_g, g_at_face_points, npts * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  STFEM_TRY(hipStreamSynchronize(st)); // (the caller's host array may go away)
  StokesSet set = stokes_single_set(nullptr, dst_u); // no source: the data takes its place
  set.out_p[0] = dst_p;
  set.wKp[0][0] = 1.0;
  return stokes_boundary_launch(c, set, c->d_g, st);
}

} // namespace

int stokes_boundary_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *d_g, hipStream_t st)
{
  if (set.nsrc < 1 || set.nsrc > MAXSRC || set.nout > (set.nsrc > 1 ? MAXSRC : MAXOUT)) return STFEM_ERR_UNSUPPORTED; // (the instantiation's bounds)
  BoundaryParams bp = c->bnd;
  bp.g = d_g;
  if (bp.foff[6] == 0) return STFEM_OK;
  return stokes_with_degree(c, [&](auto deg) { return boundary_launch<deg()>(c, set, bp, st); });
}

extern "C" {

// ---- weak boundary conditions (operators.h:1206-1211, 1220-1221; StokesNitscheMatrixFreeOperator 1768-1951) ----
// The entries of stfem.h: velocity degree 2.  Their _space forms (stfem_stokes_boundary_space.h): the context's degree.
int stfem_stokes_set_weak_boundaries(stfem_stokes_ctx *c, int weak_mask, int outflow_mask, double penalty1, double penalty2)
{
  if (!c || weak_mask < 0 || weak_mask > 63 || outflow_mask < 0 || outflow_mask > 63) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_set_weak_boundaries")) return rq;
  return set_weak_boundaries(c, weak_mask, outflow_mask, penalty1, penalty2);
}

int stfem_stokes_set_weak_boundaries_space(stfem_stokes_ctx *c, int weak_mask, int outflow_mask, double penalty1, double penalty2)
{
  if (!c || weak_mask < 0 || weak_mask > 63 || outflow_mask < 0 || outflow_mask > 63)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_set_weak_boundaries_space: a null context or a mask outside 0..63");
  return set_weak_boundaries(c, weak_mask, outflow_mask, penalty1, penalty2);
}

int64_t stfem_stokes_n_face_points(const stfem_stokes_ctx *c)
{
  if (const int rq = stokes_require_q2(c, "stfem_stokes_n_face_points")) return rq;
  return c ? n_face_points(c) : 0;
}

int64_t stfem_stokes_n_face_points_space(const stfem_stokes_ctx *c) { return c ? n_face_points(c) : 0; }

int stfem_stokes_face_points(const stfem_stokes_ctx *c, double *out)
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_face_points")) return rq;
  return face_points(c, out);
}

int stfem_stokes_face_points_space(const stfem_stokes_ctx *c, double *out)
{
  if (!c || !out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_face_points_space: a null argument");
  return face_points(c, out);
}

int stfem_stokes_nitsche_rhs(stfem_stokes_ctx *c, const double *g_at_face_points, double *dst_u, double *dst_p, void *stream)
{
  if (!c || !g_at_face_points || !dst_u || !dst_p) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_nitsche_rhs")) return rq;
  return nitsche_rhs(c, g_at_face_points, dst_u, dst_p, stream);
}

int stfem_stokes_nitsche_rhs_space(stfem_stokes_ctx *c, const double *g_at_face_points, double *dst_u, double *dst_p, void *stream)
{
  if (!c || !g_at_face_points || !dst_u || !dst_p) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_nitsche_rhs_space: a null argument");
  return nitsche_rhs(c, g_at_face_points, dst_u, dst_p, stream);
}

int stfem_stokes_last_face_plan(const stfem_stokes_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (!c->face_launched) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_last_face_plan: this context has not launched the boundary kernel");
  out[0] = c->face_plan[0];
  out[1] = c->face_plan[1];
  return STFEM_OK;
}

} // extern "C"
