// What the slab driver needs around the operator: load vectors, nodal interpolation points
// and error norms.  None of it is on the vmult hot path; the kernels are plain (one workgroup
// per cell, the MappingQ1 Jacobian and the mapped points from the eight cell vertices on the fly: stfem_mapping_q1.h).
//
// Replaces, for the structured meshes of this library:
//   VectorTools::create_right_hand_side(mapping, dof_handler, quad, f, rhs, constraints)  (tests/tp_01.cc:382-392)
//       -> stfem_quadrature_points + stfem_integrate_rhs (the caller evaluates f at the points)
//   VectorTools::interpolate(mapping, dof_handler, u, vec)                                (tests/tp_01.cc:393-400)
//       -> stfem_support_points + stfem_vector_upload
//   VectorTools::integrate_difference (L2, Linfty, H1-seminorm) of ErrorCalculator::evaluate_error
//       (include/exact_solution.h:534-600)                                                -> stfem_integrate_difference
//   the vector arithmetic of SolverFGMRES / TimeIntegrator (add, sadd, equ)               -> stfem_vector_axpby (stfem_vector.hip)
#include "stfem_internal.h"
#include "stfem_mapping_q1.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

// vertices of the structured block on the host (the context keeps them for general meshes only)
std::vector<double> host_vertices(const stfem_ctx *c)
{
  if (!c->vertices.empty()) return c->vertices;
  std::vector<double> v(size_t(c->nc[0] + 1) * (c->nc[1] + 1) * (c->nc[2] + 1) * 3);
  size_t o = 0;
  for (int k = 0; k <= c->nc[2]; ++k)
    for (int j = 0; j <= c->nc[1]; ++j)
      for (int i = 0; i <= c->nc[0]; ++i, ++o) {
        v[3 * o] = c->lower[0] + c->h[0] * i;
        v[3 * o + 1] = c->lower[1] + c->h[1] * j;
        v[3 * o + 2] = c->lower[2] + c->h[2] * k;
      }
  return v;
}

struct CellGeomParams {
  const double *vertices; // device
  int ncx, ncy, ncz, nx, ny, p, nq, dmask;
  const double *S, *D;    // [nq][n]: nodal basis and its reference derivative at the quadrature points (device)
  const double *xq, *wq;  // [nq] (device)
};

// f(x) = amplitude * prod_d sin(2 pi frequency x_d): the separable functions of the reference's convergence tests (exact solutions and
// right-hand sides of include/exact_solution.h:27-81, 147-197 at a fixed time), evaluated on the device instead of handed in point by point
struct ProductFn {
  int on;
  double amplitude, frequency;
};
__device__ double product_value(const ProductFn &f, const double x[3], double grad[3])
{
  const double w = 6.283185307179586476925286766559 * f.frequency;
  const double s[3] = {sin(w * x[0]), sin(w * x[1]), sin(w * x[2])}, c[3] = {cos(w * x[0]), cos(w * x[1]), cos(w * x[2])};
  if (grad) {
    grad[0] = f.amplitude * w * c[0] * s[1] * s[2];
    grad[1] = f.amplitude * w * s[0] * c[1] * s[2];
    grad[2] = f.amplitude * w * s[0] * s[1] * c[2];
  }
  return f.amplitude * s[0] * s[1] * s[2];
}

// rhs_a += sum_q JxW_q f_q phi_a(x_q); one workgroup per cell; constrained rows stay 0.  One launch covers the cells of ONE
// parity (cx & 1, cy & 1, cz & 1) = (par & 1, par >> 1 & 1, par >> 2): two of them share no DoF, so the plain `+=` below has no
// race, and the eight launches in a fixed sequence give every shared DoF a fixed order of its up-to-eight contributions - the
// load vector repeats bitwise (a global atomicAdd here made it depend on timing).
template <typename T>
__global__ __launch_bounds__(256) void integrate_rhs_kernel(const CellGeomParams g, const double *__restrict__ fq, T *__restrict__ dst, const ProductFn pf,
                                                            const int par)
{
  extern __shared__ double sm[]; // [nq^3] JxW f
  const int n = g.p + 1, nq = g.nq, nq3 = nq * nq * nq, nloc = n * n * n;
  const int px = par & 1, py = (par >> 1) & 1, pz = par >> 2;
  const int hx = (g.ncx - px + 1) / 2, hy = (g.ncy - py + 1) / 2; // cells of this parity per direction
  const long long b = blockIdx.x;
  const int cx = 2 * int(b % hx) + px, cy = 2 * int((b / hx) % hy) + py, cz = 2 * int(b / ((long long)hx * hy)) + pz;
  const long long cell = cx + (long long)g.ncx * (cy + (long long)g.ncy * cz);
  for (int q = threadIdx.x; q < nq3; q += 256) {
    const int qx = q % nq, qy = (q / nq) % nq, qz = q / (nq * nq);
    const double xi[3] = {g.xq[qx], g.xq[qy], g.xq[qz]};
    double J[3][3];
    mapping_q1_jacobian(g.vertices, g.ncx, g.ncy, cx, cy, cz, xi, J);
    double fv;
    if (pf.on) {
      double x[3];
      mapping_q1_point(g.vertices, g.ncx, g.ncy, cx, cy, cz, xi, x);
      fv = product_value(pf, x, nullptr);
    } else fv = fq[cell * nq3 + q];
    sm[q] = mapping_q1_det(J) * g.wq[qx] * g.wq[qy] * g.wq[qz] * fv;
  }
  __syncthreads();
  for (int a = threadIdx.x; a < nloc; a += 256) {
    const int ax = a % n, ay = (a / n) % n, az = a / (n * n);
    const int ix = g.p * cx + ax, iy = g.p * cy + ay, iz = g.p * cz + az;
    const bool con = ((g.dmask & 1) && ix == 0) || ((g.dmask & 2) && ix == g.nx - 1) || ((g.dmask & 4) && iy == 0) ||
                     ((g.dmask & 8) && iy == g.ny - 1) || ((g.dmask & 16) && iz == 0) || ((g.dmask & 32) && iz == g.p * g.ncz);
    if (con) continue;
    double s = 0.0;
    for (int qz = 0; qz < nq; ++qz)
      for (int qy = 0; qy < nq; ++qy) {
        const double syz = g.S[qy * n + ay] * g.S[qz * n + az];
        for (int qx = 0; qx < nq; ++qx) s += sm[qx + nq * (qy + nq * qz)] * g.S[qx * n + ax] * syz;
      }
    dst[ix + (long long)g.nx * (iy + (long long)g.ny * iz)] += T(s);
  }
}

// per cell: sum_q JxW (u_h - u)^2, max_q |u_h - u|, sum_q JxW |grad u_h - grad u|^2  -> out[cell][3]
template <typename T>
__global__ __launch_bounds__(256) void integrate_difference_kernel(const CellGeomParams g, const T *__restrict__ u,
                                                                   const double *__restrict__ exact, const double *__restrict__ exact_grad,
                                                                   double *__restrict__ out, const ProductFn pf)
{
  extern __shared__ double sm[]; // [nloc] cell values, then 3 x 256 reduction
  const int n = g.p + 1, nq = g.nq, nq3 = nq * nq * nq, nloc = n * n * n;
  double *ul = sm, *red = sm + nloc;
  const long long cell = blockIdx.x;
  const int cx = int(cell % g.ncx), cy = int((cell / g.ncx) % g.ncy), cz = int(cell / ((long long)g.ncx * g.ncy));
  for (int a = threadIdx.x; a < nloc; a += 256) {
    const int ax = a % n, ay = (a / n) % n, az = a / (n * n);
    ul[a] = double(u[(g.p * cx + ax) + (long long)g.nx * ((g.p * cy + ay) + (long long)g.ny * (g.p * cz + az))]);
  }
  __syncthreads();
  double l2 = 0.0, l8 = 0.0, h1 = 0.0;
  for (int q = threadIdx.x; q < nq3; q += 256) {
    const int qx = q % nq, qy = (q / nq) % nq, qz = q / (nq * nq);
    const double xi[3] = {g.xq[qx], g.xq[qy], g.xq[qz]};
    double J[3][3];
    mapping_q1_jacobian(g.vertices, g.ncx, g.ncy, cx, cy, cz, xi, J);
    const double det = mapping_q1_det(J), JxW = det * g.wq[qx] * g.wq[qy] * g.wq[qz];
    double val = 0.0, gr[3] = {0, 0, 0};
    for (int az = 0; az < n; ++az)
      for (int ay = 0; ay < n; ++ay)
        for (int ax = 0; ax < n; ++ax) {
          const double w = ul[ax + n * (ay + n * az)];
          const double sx = g.S[qx * n + ax], sy = g.S[qy * n + ay], sz = g.S[qz * n + az];
          val += w * sx * sy * sz;
          gr[0] += w * g.D[qx * n + ax] * sy * sz;
          gr[1] += w * sx * g.D[qy * n + ay] * sz;
          gr[2] += w * sx * sy * g.D[qz * n + az];
        }
    double ex, exg[3] = {0, 0, 0};
    if (pf.on) {
      double x[3];
      mapping_q1_point(g.vertices, g.ncx, g.ncy, cx, cy, cz, xi, x);
      ex = product_value(pf, x, exg);
    } else {
      ex = exact[cell * nq3 + q];
      if (exact_grad)
        for (int d = 0; d < 3; ++d) exg[d] = exact_grad[(cell * nq3 + q) * 3 + d];
    }
    const double e = val - ex;
    l2 += JxW * e * e;
    l8 = fmax(l8, fabs(e));
    if (exact_grad || pf.on) {
      // physical gradient = J^-T reference gradient
      double Ji[3][3];
      mapping_q1_inverse(J, Ji);
      for (int d = 0; d < 3; ++d) {
        const double gd = gr[0] * Ji[0][d] + gr[1] * Ji[1][d] + gr[2] * Ji[2][d] - exg[d];
        h1 += JxW * gd * gd;
      }
    }
  }
  red[threadIdx.x] = l2; red[256 + threadIdx.x] = l8; red[512 + threadIdx.x] = h1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (int(threadIdx.x) < s) {
      red[threadIdx.x] += red[threadIdx.x + s];
      red[256 + threadIdx.x] = fmax(red[256 + threadIdx.x], red[256 + threadIdx.x + s]);
      red[512 + threadIdx.x] += red[512 + threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[cell * 3] = red[0]; out[cell * 3 + 1] = red[256]; out[cell * 3 + 2] = red[512]; }
}

// device copies of the geometry and of the tables of QGauss(nq) against the context's nodal basis
struct GeomUpload {
  double *d = nullptr;
  CellGeomParams g{};
  int build(const stfem_ctx *c, int nq)
  {
    const int n = c->p + 1;
    const std::vector<double> v = host_vertices(c);
    std::vector<double> xq, wq;
    stfem::gauss_rule(nq, xq, wq);
    stfem::Mat S, D;
    stfem::lagrange_tables(c->tab.nodes, xq, S, D);
    std::vector<double> all(v);
    const size_t oS = all.size();
    all.insert(all.end(), S.begin(), S.end());
    const size_t oD = all.size();
    all.insert(all.end(), D.begin(), D.end());
    const size_t ox = all.size();
    all.insert(all.end(), xq.begin(), xq.end());
    const size_t ow = all.size();
    all.insert(all.end(), wq.begin(), wq.end());
    if (hipMalloc(&d, all.size() * sizeof(double)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    STFEM_TRY(hipMemcpy(d, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
    g.vertices = d; g.S = d + oS; g.D = d + oD; g.xq = d + ox; g.wq = d + ow;
    g.ncx = c->nc[0]; g.ncy = c->nc[1]; g.ncz = c->nc[2]; g.nx = c->nd[0]; g.ny = c->nd[1];
    g.p = c->p; g.nq = nq; g.dmask = c->dmask;
    (void)n;
    return STFEM_OK;
  }
  ~GeomUpload()
  {
    if (d) (void)hipFree(d);
  }
};

} // namespace

extern "C" {

int stfem_support_points(const stfem_ctx *c, double *out)
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  const std::vector<double> v = host_vertices(c);
  const int p = c->p;
  for (int iz = 0; iz < c->nd[2]; ++iz)
    for (int iy = 0; iy < c->nd[1]; ++iy)
      for (int ix = 0; ix < c->nd[0]; ++ix) {
        const int cx = std::min(ix / p, c->nc[0] - 1), cy = std::min(iy / p, c->nc[1] - 1), cz = std::min(iz / p, c->nc[2] - 1);
        const double xi[3] = {c->tab.nodes[ix - p * cx], c->tab.nodes[iy - p * cy], c->tab.nodes[iz - p * cz]};
        mapping_q1_point(v.data(), c->nc[0], c->nc[1], cx, cy, cz, xi, out + 3 * (ix + size_t(c->nd[0]) * (iy + size_t(c->nd[1]) * iz)));
      }
  return STFEM_OK;
}

int stfem_quadrature_points(const stfem_ctx *c, int nq, double *out)
{
  if (!c || !out || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  const std::vector<double> v = host_vertices(c);
  std::vector<double> xq, wq;
  stfem::gauss_rule(nq, xq, wq);
  size_t o = 0;
  for (int cz = 0; cz < c->nc[2]; ++cz)
    for (int cy = 0; cy < c->nc[1]; ++cy)
      for (int cx = 0; cx < c->nc[0]; ++cx)
        for (int qz = 0; qz < nq; ++qz)
          for (int qy = 0; qy < nq; ++qy)
            for (int qx = 0; qx < nq; ++qx, ++o) {
              const double xi[3] = {xq[qx], xq[qy], xq[qz]};
              mapping_q1_point(v.data(), c->nc[0], c->nc[1], cx, cy, cz, xi, out + 3 * o);
            }
  return STFEM_OK;
}

static int integrate_rhs_impl(stfem_ctx *c, int nq, const double *f_at_points, const ProductFn pf, stfem_vec *dst, int block, void *stream)
{
  if (!c || (!f_at_points && !pf.on) || !dst || dst->ctx != c || block < 0 || block >= dst->nb || nq < 1 || nq > 8) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  GeomUpload geo;
  int rc = geo.build(c, nq);
  if (rc != STFEM_OK) return rc;
  const size_t nf = size_t(c->ncells) * nq * nq * nq;
  double *d_f = nullptr;
  hipError_t e = hipSuccess;
  if (!pf.on) {
    if (hipMalloc(&d_f, nf * sizeof(double)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    e = hipMemcpyAsync(d_f, f_at_points, nf * sizeof(double), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess) e = hipMemsetAsync(dst->blk[block], 0, size_t(c->ndofs) * c->es, st);
  const size_t lds = size_t(nq) * nq * nq * sizeof(double);
  stfem_launch_begin();
  for (int par = 0; par < 8 && e == hipSuccess && rc == STFEM_OK; ++par) { // fixed sequence on one stream: see the kernel
    const long long nblk = (long long)((c->nc[0] - (par & 1) + 1) / 2) * ((c->nc[1] - ((par >> 1) & 1) + 1) / 2) * ((c->nc[2] - (par >> 2) + 1) / 2);
    if (nblk == 0) continue;
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(integrate_rhs_kernel<T>, dim3((unsigned)nblk), dim3(256), lds, st, geo.g, d_f, static_cast<T *>(dst->blk[block]), pf, par);
    });
    rc = stfem_launch_end("integrate_rhs_kernel");
  }
  if (e == hipSuccess && rc == STFEM_OK) e = hipStreamSynchronize(st);
  if (d_f) (void)hipFree(d_f);
  if (e != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "stfem_integrate_rhs: %s", hipGetErrorString(e));
  return rc;
}

int stfem_integrate_rhs(stfem_ctx *c, int nq, const double *f_at_points, stfem_vec *dst, int block, void *stream)
{
  return integrate_rhs_impl(c, nq, f_at_points, ProductFn{0, 0.0, 0.0}, dst, block, stream);
}
int stfem_integrate_rhs_product(stfem_ctx *c, int nq, double amplitude, double frequency, stfem_vec *dst, int block, void *stream)
{
  return integrate_rhs_impl(c, nq, nullptr, ProductFn{1, amplitude, frequency}, dst, block, stream);
}

static int integrate_difference_impl(stfem_ctx *c, int nq, const stfem_vec *u, int block, const double *exact_at_points,
                                     const double *exact_grad_at_points, const ProductFn pf, double out[3], void *stream)
{
  if (!c || !u || u->ctx != c || block < 0 || block >= u->nb || (!exact_at_points && !pf.on) || !out || nq < 1 || nq > 8)
    return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  GeomUpload geo;
  int rc = geo.build(c, nq);
  if (rc != STFEM_OK) return rc;
  const size_t npts = size_t(c->ncells) * nq * nq * nq;
  double *d_e = nullptr, *d_g = nullptr, *d_out = nullptr;
  auto cleanup = [&]() {
    if (d_e) (void)hipFree(d_e);
    if (d_g) (void)hipFree(d_g);
    if (d_out) (void)hipFree(d_out);
  };
  if ((!pf.on && hipMalloc(&d_e, npts * sizeof(double)) != hipSuccess) || hipMalloc(&d_out, size_t(c->ncells) * 3 * sizeof(double)) != hipSuccess ||
      (!pf.on && exact_grad_at_points && hipMalloc(&d_g, npts * 3 * sizeof(double)) != hipSuccess)) {
    cleanup();
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  hipError_t e = hipSuccess;
  if (!pf.on) e = hipMemcpyAsync(d_e, exact_at_points, npts * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !pf.on && exact_grad_at_points) e = hipMemcpyAsync(d_g, exact_grad_at_points, npts * 3 * sizeof(double), hipMemcpyHostToDevice, st);
  std::vector<double> part(size_t(c->ncells) * 3);
  if (e == hipSuccess) {
    const int n = c->p + 1;
    const size_t lds = (size_t(n) * n * n + 3 * 256) * sizeof(double);
    stfem_launch_begin();
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(integrate_difference_kernel<T>, dim3((unsigned)c->ncells), dim3(256), lds, st, geo.g,
                         static_cast<const T *>(u->blk[block]), d_e, d_g, d_out, pf);
    });
    rc = stfem_launch_end("integrate_difference_kernel");
  }
  if (e == hipSuccess && rc == STFEM_OK) e = hipMemcpyAsync(part.data(), d_out, part.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == STFEM_OK) e = hipStreamSynchronize(st);
  cleanup();
  if (e != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "stfem_integrate_difference: %s", hipGetErrorString(e));
  if (rc != STFEM_OK) return rc;
  out[0] = out[1] = out[2] = 0.0;
  for (int64_t cell = 0; cell < c->ncells; ++cell) {
    out[0] += part[cell * 3];
    out[1] = std::max(out[1], part[cell * 3 + 1]);
    out[2] += part[cell * 3 + 2];
  }
  return STFEM_OK;
}

int stfem_integrate_difference(stfem_ctx *c, int nq, const stfem_vec *u, int block, const double *exact_at_points,
                               const double *exact_grad_at_points, double out[3], void *stream)
{
  return integrate_difference_impl(c, nq, u, block, exact_at_points, exact_grad_at_points, ProductFn{0, 0.0, 0.0}, out, stream);
}
int stfem_integrate_difference_product(stfem_ctx *c, int nq, const stfem_vec *u, int block, double amplitude, double frequency, double out[3],
                                       void *stream)
{
  return integrate_difference_impl(c, nq, u, block, nullptr, nullptr, ProductFn{1, amplitude, frequency}, out, stream);
}

} // extern "C"
