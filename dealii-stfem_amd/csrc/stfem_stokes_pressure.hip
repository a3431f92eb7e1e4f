// Stokes two-field operator: the pressure space by itself - what the solver around the operator needs of it (tests/tp_03stokes.cc:
// 404-425, 1047-1062, include/exact_solution.h:503-649, the pressure transfer of the Stokes multigrid levels).  The entries of
// include/stfem.h serve velocity degree 2 (FE_Q(1) / FE_DGP(1)); their _space forms (include/stfem_stokes_pressure_space.h) serve
// degree 3 too (FE_Q(2) / FE_DGP(2)) and are, at degree 2, the same code path.
#include "stfem_stokes_internal.h"

#include <cstring>

namespace {
// sum JxW (p_h - p)^2 and max |p_h - p| over QGauss(nq)^3 of the cells; blockIdx.x = cell (axis-aligned uniform cells).  DEG: the
// velocity degree.  At DEG = 3 the three 1D functions of the pressure space at the nq points, [j][q], follow the weights in the buffer
// of the rule: the Lagrange functions of FE_Q(2) on 0, 1/2, 1, or the Legendre functions of FE_DGP(2), whose ten products stand in
// the order of include/stfem_stokes_space.h.
template <bool PDG, int DEG>
__global__ __launch_bounds__(64) void pressure_difference_kernel(int ncx, int ncy, int ncz, int nq, double vol, const double *__restrict__ xq,
                                                                 const double *__restrict__ wq, const double *__restrict__ p,
                                                                 const double *__restrict__ exact, double *__restrict__ out)
{
  const long long cell = blockIdx.x;
  const int cx = int(cell % ncx), cy = int((cell / ncx) % ncy), cz = int(cell / ((long long)ncx * ncy));
  const int nq3 = nq * nq * nq;
  double l2 = 0.0, l8 = 0.0;
  for (int q = threadIdx.x; q < nq3; q += 64) {
    const int qx = q % nq, qy = (q / nq) % nq, qz = q / (nq * nq);
    const double x = xq[qx], y = xq[qy], z = xq[qz];
    double ph;
    if constexpr (DEG == 3) {
      const double *L = wq + nq;
      const double ax[3] = {L[qx], L[nq + qx], L[2 * nq + qx]}, ay[3] = {L[qy], L[nq + qy], L[2 * nq + qy]},
                   az[3] = {L[qz], L[nq + qz], L[2 * nq + qz]};
      if (PDG) {
        const double *c = p + 10 * cell;
        ph = c[0] + c[1] * ax[1] + c[2] * ax[2] + c[3] * ay[1] + c[4] * ax[1] * ay[1] + c[5] * ay[2] + c[6] * az[1] + c[7] * ax[1] * az[1] +
             c[8] * ay[1] * az[1] + c[9] * az[2];
      } else {
        const int npx = 2 * ncx + 1, npy = 2 * ncy + 1;
        ph = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i)
              ph += ax[i] * ay[j] * az[k] * p[(2 * cx + i) + (long long)npx * ((2 * cy + j) + (long long)npy * (2 * cz + k))];
      }
    } else if (PDG) {
      const double *c = p + 4 * cell;
      const double s3 = 1.7320508075688772;
      ph = c[0] + s3 * (c[1] * (2 * x - 1) + c[2] * (2 * y - 1) + c[3] * (2 * z - 1));
    } else {
      const int npx = ncx + 1, npy = ncy + 1;
      ph = 0.0;
      for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 2; ++j)
          for (int i = 0; i < 2; ++i)
            ph += (i ? x : 1 - x) * (j ? y : 1 - y) * (k ? z : 1 - z) * p[(cx + i) + (long long)npx * ((cy + j) + (long long)npy * (cz + k))];
    }
    const double e = ph - exact[cell * nq3 + q];
    l2 += vol * wq[qx] * wq[qy] * wq[qz] * e * e;
    l8 = fmax(l8, fabs(e));
  }
  __shared__ double s2[64], s8[64];
  s2[threadIdx.x] = l2; s8[threadIdx.x] = l8;
  __syncthreads();
  if (threadIdx.x == 0) { // fixed order: reproducible
    double a = 0.0, b = 0.0;
    for (int t = 0; t < 64; ++t) { a += s2[t]; b = fmax(b, s8[t]); }
    out[2 * cell] = a;
    out[2 * cell + 1] = b;
  }
}
__global__ __launch_bounds__(256) void pressure_difference_finish(long long ncells, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double s2[256], s8[256];
  double a = 0.0, b = 0.0;
  for (long long c = threadIdx.x; c < ncells; c += 256) { a += part[2 * c]; b = fmax(b, part[2 * c + 1]); }
  s2[threadIdx.x] = a; s8[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    double x = 0.0, y = 0.0;
    for (int t = 0; t < 256; ++t) { x += s2[t]; y = fmax(y, s8[t]); }
    out[0] = x; out[1] = y;
  }
}
// FE_DGP(1) between a mesh and the mesh of its 2 x 2 x 2 children: the parent's function on child (sx, sy, sz) has the coefficients
// c0 + sqrt 3 ((sx - 1/2) c1 + (sy - 1/2) c2 + (sz - 1/2) c3), c1 / 2, c2 / 2, c3 / 2 (the embedding MGTwoLevelTransfer prolongates
// with; its restriction is the transpose).  One thread per coarse cell.
template <bool RESTRICT>
__global__ __launch_bounds__(256) void dgp_transfer_kernel(int ncx, int ncy, int ncz, double *__restrict__ dst, const double *__restrict__ src, int add)
{
  const long long cc = (long long)blockIdx.x * 256 + threadIdx.x; // coarse cell
  if (cc >= (long long)ncx * ncy * ncz) return;
  const int cx = int(cc % ncx), cy = int((cc / ncx) % ncy), cz = int(cc / ((long long)ncx * ncy));
  const int fx = 2 * ncx, fy = 2 * ncy;
  const double s3h = 0.8660254037844386; // sqrt 3 / 2
  double acc[4] = {0, 0, 0, 0};
  double pc[4] = {0, 0, 0, 0};
  if (!RESTRICT)
    for (int j = 0; j < 4; ++j) pc[j] = src[4 * cc + j];
  for (int sz = 0; sz < 2; ++sz)
    for (int sy = 0; sy < 2; ++sy)
      for (int sx = 0; sx < 2; ++sx) {
        const long long fc = (2 * cx + sx) + (long long)fx * ((2 * cy + sy) + (long long)fy * (2 * cz + sz));
        const double ox = sx ? s3h : -s3h, oy = sy ? s3h : -s3h, oz = sz ? s3h : -s3h;
        if (RESTRICT) {
          const double *f = src + 4 * fc;
          acc[0] += f[0];
          acc[1] += ox * f[0] + 0.5 * f[1];
          acc[2] += oy * f[0] + 0.5 * f[2];
          acc[3] += oz * f[0] + 0.5 * f[3];
        } else {
          double *f = dst + 4 * fc;
          const double v[4] = {pc[0] + ox * pc[1] + oy * pc[2] + oz * pc[3], 0.5 * pc[1], 0.5 * pc[2], 0.5 * pc[3]};
          for (int j = 0; j < 4; ++j) f[j] = add ? f[j] + v[j] : v[j];
        }
      }
  if (RESTRICT)
    for (int j = 0; j < 4; ++j) dst[4 * cc + j] = add ? dst[4 * cc + j] + acc[j] : acc[j];
}
// FE_DGP(2) between the same two meshes.  The parent's 1D Legendre functions on child s are l_i = sum_j T[s][i][j] l_j (lower
// triangular: stfem::dgp_child_tables, passed by value), so the products of total degree <= 2 map into themselves and the 10 x 10
// matrix of child (sx, sy, sz) is M[m'][m] = Tx[i][i'] Ty[j][j'] Tz[k][k'] for m = (i, j, k), m' = (i', j', k') in the order of
// include/stfem_stokes_space.h.  One thread per coarse cell, a fixed order of the sums.
struct DgpTables {
  double T[2][3][3];
};
__host__ __device__ constexpr int dgp2_i(int m) { return (m == 1 || m == 4 || m == 7) ? 1 : (m == 2 ? 2 : 0); }
__host__ __device__ constexpr int dgp2_j(int m) { return (m == 3 || m == 4 || m == 8) ? 1 : (m == 5 ? 2 : 0); }
__host__ __device__ constexpr int dgp2_k(int m) { return (m == 6 || m == 7 || m == 8) ? 1 : (m == 9 ? 2 : 0); }
// (T[s][i][j] is non-zero for j == i and j == i - 1 alone)
__host__ __device__ constexpr bool dgp2_entry(int i, int j) { return j == i || j == i - 1; }
template <bool RESTRICT>
__global__ __launch_bounds__(256) void dgp2_transfer_kernel(int ncx, int ncy, int ncz, double *__restrict__ dst, const double *__restrict__ src, int add,
                                                            const DgpTables tab)
{
  const long long cc = (long long)blockIdx.x * 256 + threadIdx.x; // coarse cell
  if (cc >= (long long)ncx * ncy * ncz) return;
  const int cx = int(cc % ncx), cy = int((cc / ncx) % ncy), cz = int(cc / ((long long)ncx * ncy));
  const int fx = 2 * ncx, fy = 2 * ncy;
  double acc[10], pc[10];
#pragma unroll
  for (int m = 0; m < 10; ++m) { acc[m] = 0.0; pc[m] = RESTRICT ? 0.0 : src[10 * cc + m]; }
#pragma unroll
  for (int sz = 0; sz < 2; ++sz)
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const long long fc = (2 * cx + sx) + (long long)fx * ((2 * cy + sy) + (long long)fy * (2 * cz + sz));
        double fv[10], v[10];
#pragma unroll
        for (int n = 0; n < 10; ++n) { fv[n] = RESTRICT ? src[10 * fc + n] : 0.0; v[n] = 0.0; }
#pragma unroll
        for (int m = 0; m < 10; ++m)
#pragma unroll
          for (int n = 0; n < 10; ++n) { // m: the parent's function, n: the child's
            if (!dgp2_entry(dgp2_i(m), dgp2_i(n)) || !dgp2_entry(dgp2_j(m), dgp2_j(n)) || !dgp2_entry(dgp2_k(m), dgp2_k(n))) continue;
            const double M = tab.T[sx][dgp2_i(m)][dgp2_i(n)] * tab.T[sy][dgp2_j(m)][dgp2_j(n)] * tab.T[sz][dgp2_k(m)][dgp2_k(n)];
            if (RESTRICT) acc[m] += M * fv[n];
            else v[n] += M * pc[m];
          }
        if (!RESTRICT) {
          double *f = dst + 10 * fc;
#pragma unroll
          for (int n = 0; n < 10; ++n) f[n] = add ? f[n] + v[n] : v[n];
        }
      }
  if (RESTRICT) {
#pragma unroll
    for (int m = 0; m < 10; ++m) dst[10 * cc + m] = add ? dst[10 * cc + m] + acc[m] : acc[m];
  }
}

// ---- the entries, for a context of the degree their caller has admitted
int pressure_ctx(stfem_stokes_ctx *c, stfem_ctx **out)
{
  *out = nullptr;
  if (!c->pressure_space) {
    stfem_mesh_desc md;
    std::memset(&md, 0, sizeof(md));
    md.device = c->device;
    md.dirichlet_mask = 0;
    const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
    if (c->pspace) {
      if (ncells < 2 || ncells - 1 > 0x7fffffffll)
        return stfem_set_error(STFEM_ERR_UNSUPPORTED, "the carrier of a FE_DGP pressure needs 2 <= n_cells <= 2^31 (%lld cells)", ncells);
      // FE_DGP(1): 2 x 2 x n_cells DoFs; FE_DGP(2): 2 x 5 x n_cells
      md.ncell[0] = 1;
      md.ncell[1] = c->degree == 3 ? 4 : 1;
      md.ncell[2] = int32_t(ncells - 1);
      for (int d = 0; d < 3; ++d) { md.lower[d] = 0.0; md.upper[d] = 1.0; }
    } else {
      for (int d = 0; d < 3; ++d) {
        md.ncell[d] = c->nc[d];
        md.lower[d] = c->h_vertices[d];
        md.upper[d] = c->h_vertices[c->h_vertices.size() - 3 + d];
      }
      if (!c->cart) md.vertices = c->h_vertices.data();
    }
    stfem_space_desc sd{1, 2, 1, 0}; // (the carrier is a degree-1 context whatever the pressure degree)
    if (!c->pspace) { sd.degree = c->degree - 1; sd.n_q_points_1d = c->degree; }
    const int rc = stfem_ctx_create(&md, &sd, &c->pressure_space);
    if (rc != STFEM_OK) return rc;
  }
  *out = c->pressure_space;
  return STFEM_OK;
}

int pressure_mean_vectors(stfem_stokes_ctx *c, double *ones, double *weights, double *volume)
{
  if (!c->cart) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "the pressure mean vectors are built for axis-aligned uniform meshes");
  const double cell = c->detJ;
  const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
  *volume = cell * double(ncells);
  if (c->pspace) { // psi_0 = 1, the others have zero mean on a box
    const long long per = c->degree == 3 ? 10 : 4;
    for (long long i = 0; i < c->Np; ++i) { ones[i] = i % per == 0 ? 1.0 : 0.0; weights[i] = i % per == 0 ? cell : 0.0; }
  } else if (c->degree == 3) { // FE_Q(2): the assembled 1D integrals (1/6, 4/6, 1/6) per cell on the 2 nc + 1 lattice
    auto w1 = [](int i, int n) { return (i & 1) ? 4.0 / 6.0 : ((i == 0 || i == n - 1) ? 1.0 / 6.0 : 2.0 / 6.0); };
    for (int k = 0; k < c->ndp[2]; ++k)
      for (int j = 0; j < c->ndp[1]; ++j)
        for (int i = 0; i < c->ndp[0]; ++i) {
          const long long o = i + (long long)c->ndp[0] * (j + (long long)c->ndp[1] * k);
          ones[o] = 1.0;
          weights[o] = cell * w1(i, c->ndp[0]) * w1(j, c->ndp[1]) * w1(k, c->ndp[2]);
        }
  } else {
    for (int k = 0; k < c->ndp[2]; ++k)
      for (int j = 0; j < c->ndp[1]; ++j)
        for (int i = 0; i < c->ndp[0]; ++i) {
          const double wx = (i == 0 || i == c->ndp[0] - 1) ? 0.5 : 1.0, wy = (j == 0 || j == c->ndp[1] - 1) ? 0.5 : 1.0,
                       wz = (k == 0 || k == c->ndp[2] - 1) ? 0.5 : 1.0;
          const long long o = i + (long long)c->ndp[0] * (j + (long long)c->ndp[1] * k);
          ones[o] = 1.0;
          weights[o] = cell * wx * wy * wz;
        }
  }
  return STFEM_OK;
}

int pressure_quadrature_points(const stfem_stokes_ctx *c, int nq, double *out)
{
  if (!c->cart) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "the pressure quadrature points are built for axis-aligned uniform meshes");
  std::vector<double> xq, wq;
  stfem::gauss_rule(nq, xq, wq);
  double lo[3], h[3];
  for (int d = 0; d < 3; ++d) { lo[d] = c->h_vertices[d]; h[d] = 1.0 / c->hinv[d]; }
  size_t o = 0;
  for (int cz = 0; cz < c->nc[2]; ++cz)
    for (int cy = 0; cy < c->nc[1]; ++cy)
      for (int cx = 0; cx < c->nc[0]; ++cx)
        for (int qz = 0; qz < nq; ++qz)
          for (int qy = 0; qy < nq; ++qy)
            for (int qx = 0; qx < nq; ++qx, o += 3) {
              out[o] = lo[0] + h[0] * (cx + xq[qx]);
              out[o + 1] = lo[1] + h[1] * (cy + xq[qy]);
              out[o + 2] = lo[2] + h[2] * (cz + xq[qz]);
            }
  return STFEM_OK;
}

int pressure_difference(stfem_stokes_ctx *c, int nq, const double *p, const double *exact_at_points, double out[2], void *stream)
{
  if (!c->cart) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "the pressure difference is built for axis-aligned uniform meshes");
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
  const size_t npts = size_t(ncells) * nq * nq * nq;
  if (c->pq_points < npts) {
    if (c->d_pq) STFEM_TRY(hipFree(c->d_pq));
    if (c->d_pred) STFEM_TRY(hipFree(c->d_pred));
    c->d_pq = c->d_pred = nullptr;
    c->pq_points = 0;
    // (behind the values: the rule, 2 nq, and at degree 3 the three 1D functions of the pressure space at its points, 3 nq; nq <= 8)
    if (hipMalloc(&c->d_pq, (npts + 40) * sizeof(double)) != hipSuccess || hipMalloc(&c->d_pred, (2 * size_t(ncells) + 2) * sizeof(double)) != hipSuccess)
      return STFEM_ERR_OUT_OF_MEMORY;
    c->pq_points = npts;
  }
  std::vector<double> xq, wq;
  stfem::gauss_rule(nq, xq, wq);
  std::vector<double> rule(xq);
  rule.insert(rule.end(), wq.begin(), wq.end());
  if (c->degree == 3) {
    rule.resize(size_t(5 * nq));
    for (int q = 0; q < nq; ++q) {
      double l[3];
      if (c->pspace) stfem::legendre01(xq[q], l);
      else stfem::lagrange_q2_01(xq[q], l);
      for (int j = 0; j < 3; ++j) rule[size_t((2 + j) * nq + q)] = l[j];
    }
  }
  STFEM_TRY(hipMemcpyAsync(c->d_pq, exact_at_points, npts * sizeof(double), hipMemcpyHostToDevice, st));
  STFEM_TRY(hipMemcpyAsync(c->d_pq + npts, rule.data(), rule.size() * sizeof(double), hipMemcpyHostToDevice, st));
  stfem_launch_begin();
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)ncells), dim3(64), 0, st, c->nc[0], c->nc[1], c->nc[2], nq, c->detJ, (const double *)(c->d_pq + npts),
                       (const double *)(c->d_pq + npts + nq), p, (const double *)c->d_pq, c->d_pred);
  };
  stokes_with_degree(c, [&](auto deg) {
    if (c->pspace) launch(pressure_difference_kernel<true, deg()>);
    else launch(pressure_difference_kernel<false, deg()>);
  });
  hipLaunchKernelGGL(pressure_difference_finish, dim3(1), dim3(256), 0, st, ncells, c->d_pred, c->d_pred + 2 * ncells);
  if (const int rc = stfem_launch_end("pressure_difference_kernel")) return rc;
  STFEM_TRY(hipMemcpyAsync(out, c->d_pred + 2 * ncells, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  return STFEM_OK;
}

template <bool RESTRICT>
int dgp_transfer(const char *me, stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst, const double *src, int add, void *stream)
{
  if (fine->degree != coarse->degree)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "%s: the two contexts have velocity degrees %d and %d, must be the same", me, fine->degree, coarse->degree);
  if (!fine->pspace || !coarse->pspace) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "%s: both contexts must have a FE_DGP pressure", me);
  for (int d = 0; d < 3; ++d)
    if (fine->nc[d] != 2 * coarse->nc[d]) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(fine->device));
  const long long nc = (long long)coarse->nc[0] * coarse->nc[1] * coarse->nc[2];
  const dim3 grid((unsigned)((nc + 255) / 256));
  hipStream_t st = static_cast<hipStream_t>(stream);
  return stokes_with_degree(fine, [&](auto deg) {
    if constexpr (deg() == 3) {
      DgpTables tab;
      stfem::dgp_child_tables(tab.T);
      hipLaunchKernelGGL(dgp2_transfer_kernel<RESTRICT>, grid, dim3(256), 0, st, coarse->nc[0], coarse->nc[1], coarse->nc[2], dst, src, add, tab);
      return stfem_launch_end(RESTRICT ? "dgp2_transfer_kernel<true>" : "dgp2_transfer_kernel<false>");
    } else {
      hipLaunchKernelGGL(dgp_transfer_kernel<RESTRICT>, grid, dim3(256), 0, st, coarse->nc[0], coarse->nc[1], coarse->nc[2], dst, src, add);
      return stfem_launch_end(RESTRICT ? "dgp_transfer_kernel<true>" : "dgp_transfer_kernel<false>");
    }
  });
}
} // namespace

extern "C" {

// The scalar context behind the pressure vectors, for their vector arithmetic (stfem_vector_wrap + stfem_vector_axpby / stfem_dot /
// stfem_multi_dot ...) and, for FE_Q(1), for everything a FE_Q(1) function has in this library (load vectors, transfers, error norms).
// FE_Q(1): a degree-1 context on the mesh, no constraints.  FE_DGP(1): the arrays have 4 n_cells entries, which no mesh of this
// library's continuous elements has in general: the context is a CARRIER - a degree-1 context on 1 x 1 x (n_cells - 1) cells, i.e. with
// 2 x 2 x n_cells DoFs - good for the vector arithmetic only.  Owned by the Stokes context.
// (_space, velocity degree 3: FE_Q(2): a degree-2 context on the mesh; FE_DGP(2): a degree-1 carrier on 1 x 4 x (n_cells - 1) cells.)
int stfem_stokes_pressure_ctx(stfem_stokes_ctx *c, stfem_ctx **out)
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_pressure_ctx")) return rq;
  return pressure_ctx(c, out);
}
int stfem_stokes_pressure_ctx_space(stfem_stokes_ctx *c, stfem_ctx **out)
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  return pressure_ctx(c, out);
}

// The constant function and the mean-value functional of the pressure space (host arrays of n_pressure_dofs entries): ones = the
// coefficients of p = 1, weights = (1, psi_j) so that mean(p) = weights . p / volume (VectorTools::compute_mean_value /
// add_constant, tests/tp_03stokes.cc:1047-1062).  Axis-aligned uniform meshes.
int stfem_stokes_pressure_mean_vectors(stfem_stokes_ctx *c, double *ones, double *weights, double *volume)
{
  if (!c || !ones || !weights || !volume) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_pressure_mean_vectors")) return rq;
  return pressure_mean_vectors(c, ones, weights, volume);
}
int stfem_stokes_pressure_mean_vectors_space(stfem_stokes_ctx *c, double *ones, double *weights, double *volume)
{
  if (!c || !ones || !weights || !volume) return STFEM_ERR_INVALID_ARGUMENT;
  return pressure_mean_vectors(c, ones, weights, volume);
}

// quadrature points of QGauss(nq)^3 on the cells, out[cell][q][3], q = qx + nq (qy + nq qz) (axis-aligned uniform meshes)
int stfem_stokes_pressure_quadrature_points(const stfem_stokes_ctx *c, int nq, double *out)
{
  if (!c || !out || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_pressure_quadrature_points")) return rq;
  return pressure_quadrature_points(c, nq, out);
}
int stfem_stokes_pressure_quadrature_points_space(const stfem_stokes_ctx *c, int nq, double *out)
{
  if (!c || !out || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  return pressure_quadrature_points(c, nq, out);
}

// out = { sum JxW (p_h - p)^2, max |p_h - p| } over those points (VectorTools::integrate_difference, L2_norm squared and Linfty_norm);
// p: device, exact_at_points: host [cell][q].  Synchronous.
int stfem_stokes_pressure_difference(stfem_stokes_ctx *c, int nq, const double *p, const double *exact_at_points, double out[2], void *stream)
{
  if (!c || !p || !exact_at_points || !out || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_pressure_difference")) return rq;
  return pressure_difference(c, nq, p, exact_at_points, out, stream);
}
int stfem_stokes_pressure_difference_space(stfem_stokes_ctx *c, int nq, const double *p, const double *exact_at_points, double out[2], void *stream)
{
  if (!c || !p || !exact_at_points || !out || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  return pressure_difference(c, nq, p, exact_at_points, out, stream);
}

// The FE_DGP(1) pressure between a mesh and the mesh with twice the cells per direction (the pressure variable's MGTwoLevelTransfer
// of the Stokes multigrid levels, include/stmg.h:557-600): prolongate: fine (=, +=) embedding of coarse; restrict: coarse (=, +=) its
// transpose applied to fine.  FE_Q(1) pressures use stfem_transfer_* on stfem_stokes_pressure_ctx.
// (_space: FE_DGP(2) between two contexts of velocity degree 3 as well.)
int stfem_stokes_dgp_prolongate(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_fine, const double *src_coarse, int add, void *stream)
{
  if (!fine || !coarse || !dst_fine || !src_coarse) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(fine, "stfem_stokes_dgp_prolongate")) return rq;
  if (const int rq = stokes_require_q2(coarse, "stfem_stokes_dgp_prolongate")) return rq;
  return dgp_transfer<false>("stfem_stokes_dgp_prolongate", fine, coarse, dst_fine, src_coarse, add, stream);
}
int stfem_stokes_dgp_prolongate_space(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_fine, const double *src_coarse, int add, void *stream)
{
  if (!fine || !coarse || !dst_fine || !src_coarse) return STFEM_ERR_INVALID_ARGUMENT;
  return dgp_transfer<false>("stfem_stokes_dgp_prolongate_space", fine, coarse, dst_fine, src_coarse, add, stream);
}
int stfem_stokes_dgp_restrict(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_coarse, const double *src_fine, int add, void *stream)
{
  if (!fine || !coarse || !dst_coarse || !src_fine) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(fine, "stfem_stokes_dgp_restrict")) return rq;
  if (const int rq = stokes_require_q2(coarse, "stfem_stokes_dgp_restrict")) return rq;
  return dgp_transfer<true>("stfem_stokes_dgp_restrict", fine, coarse, dst_coarse, src_fine, add, stream);
}
int stfem_stokes_dgp_restrict_space(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_coarse, const double *src_fine, int add, void *stream)
{
  if (!fine || !coarse || !dst_coarse || !src_fine) return STFEM_ERR_INVALID_ARGUMENT;
  return dgp_transfer<true>("stfem_stokes_dgp_restrict_space", fine, coarse, dst_coarse, src_fine, add, stream);
}

// What the context was made with (include/stfem_stokes_pressure_space.h); no device array, no device call
int stfem_stokes_get_space(const stfem_stokes_ctx *c, stfem_stokes_space_desc *out)
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->velocity_degree = c->degree;
  out->pressure_space = c->pspace;
  out->viscosity = c->nu;
  return STFEM_OK;
}

} // extern "C"
