// Stokes two-field operator: the divergence functional of a velocity,
//   StokesMatrixFreeOperator::compute_divergence / divergence_cell_loop (reference include/operators.h:1391-1439):
//   cell_vector[cell] = sum_q (div u_h)^2 JxW at the operator's 3 x 3 x 3 Gauss points, the return value sqrt(sum_cell cell_vector[cell]).
// The velocity is read PLAIN (read_dof_values_plain, 1430): entries on strongly constrained DoFs count as stored, not as zero.
// Nothing is scattered, so there are no colours: one launch over all cells, every cell writes its own entry, then one workgroup
// sums the entries in a fixed order - no atomics, bitwise reproducible.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cmath>

namespace {

struct DivergenceParams {
  const double *vertices; // device, (nc+1)^3 * 3
  const double *u;        // [3][Nu]
  double *cell_out;       // [n_cells], cell = cx + ncx (cy + ncy cz)
  int ncx, ncy, ncz;
  int ndu[2];
  long long Nu;
  double Su[9], Du[9]; // [q*3+a]
  double xq[3], wq[3];
};

// The cell layout of stokes_convection_kernel (stfem_stokes_convection.hip): one half-wave per cell, 27 active lanes, 256 threads =
// 8 cells at a time, two wave-private LDS regions per cell handed between the sum-factorised 1D stages, the MappingQ1 metric from the
// eight vertices at this lane's quadrature point (boxes take the same path: their metric is the diagonal one up to rounding).
//   evaluate (gradients only, three fields): lane (n_x, n_y, n_z) -> (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point
__global__ __launch_bounds__(256) void stokes_divergence_kernel(const DivergenceParams prm)
{
  constexpr int RX = 243, RY = 162; // doubles per cell of the two regions: 9 x 27 after the y stage, 6 x 27 after the x stage
  __shared__ double smem[8 * (RX + RY)];
  __shared__ double tS[9], tD[9];
  if (threadIdx.x < 9) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x >> 5, t32 = threadIdx.x & 31;
  const bool lane27 = t32 < 27;
  const int t = lane27 ? t32 : 0;
  const int a = t % 3, b = (t / 3) % 3, c = t / 9;
  double *X = smem + slot * (RX + RY), *Y = X + RX;
  double Sa[3], Da[3], Sb[3], Db[3], Sc[3], Dc[3]; // rows of this lane's quadrature indices
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    Sa[n] = tS[a * 3 + n]; Da[n] = tD[a * 3 + n];
    Sb[n] = tS[b * 3 + n]; Db[n] = tD[b * 3 + n];
    Sc[n] = tS[c * 3 + n]; Dc[n] = tD[c * 3 + n];
  }
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  const long long ncells = (long long)prm.ncx * prm.ncy * prm.ncz;
  // (the trip count is the same for the eight cells of a workgroup: the two half-waves of a wave fence together)
  for (long long first = (long long)blockIdx.x * 8; first < ncells; first += (long long)gridDim.x * 8) {
    const long long cell = first + slot;
    const bool ok = cell < ncells;
    const long long cc = ok ? cell : 0;
    const int cx = int(cc % prm.ncx), cy = int((cc / prm.ncx) % prm.ncy), cz = int(cc / ((long long)prm.ncx * prm.ncy));
    const long long gu = (2 * cx + a) + (long long)prm.ndu[0] * ((2 * cy + b) + (long long)prm.ndu[1] * (2 * cz + c));

    // ---- gather (plain): X = u[3][27]
    if (lane27) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) X[comp * 27 + t] = ok ? prm.u[comp * prm.Nu + gu] : 0.0;
    }
    wave_fence();
    // ---- x: (n_x, n_y, n_z) -> (q_x, n_y, n_z): value and x derivative -> Y[(2 f + {0, 1}) * 27 + t]
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *u = X + f * 27 + 3 * b + 9 * c;
      Y[(2 * f) * 27 + t] = fma(Sa[2], u[2], fma(Sa[1], u[1], Sa[0] * u[0]));
      Y[(2 * f + 1) * 27 + t] = fma(Da[2], u[2], fma(Da[1], u[1], Da[0] * u[0]));
    }
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z): d/dx, d/dy and the value -> X[(3 f + {0, 1, 2}) * 27 + t]
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *v = Y + (2 * f) * 27 + a + 9 * c, *vx = v + 27;
      X[(3 * f) * 27 + t] = fma(Sb[2], vx[6], fma(Sb[1], vx[3], Sb[0] * vx[0]));
      X[(3 * f + 1) * 27 + t] = fma(Db[2], v[6], fma(Db[1], v[3], Db[0] * v[0]));
      X[(3 * f + 2) * 27 + t] = fma(Sb[2], v[6], fma(Sb[1], v[3], Sb[0] * v[0]));
    }
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): the reference gradients g[f][e] = d u_f / d xi_e in registers
    double g[3][3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *w0 = X + (3 * f) * 27 + a + 3 * b, *w1 = w0 + 27, *w2 = w0 + 54;
      g[f][0] = fma(Sc[2], w0[18], fma(Sc[1], w0[9], Sc[0] * w0[0]));
      g[f][1] = fma(Sc[2], w1[18], fma(Sc[1], w1[9], Sc[0] * w1[0]));
      g[f][2] = fma(Dc[2], w2[18], fma(Dc[1], w2[9], Dc[0] * w2[0]));
    }

    // ---- quadrature-point operation (operators.h:1432-1436): div u = sum_f sum_e (dxi_e / dx_f) g[f][e]
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
    double div = 0.0;
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
      for (int e = 0; e < 3; ++e) div = fma(Ji[e][f], g[f][e], div);
    if (lane27) Y[t] = div * div * (det * wabc);
    wave_fence();
    // ---- the cell's sum over its 27 points, in point order
    if (ok && t32 == 0) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 27; ++q) s += Y[q];
      prm.cell_out[cell] = s;
    }
    wave_fence(); // the next cell's gather and x stage overwrite X and Y
  }
}

// stage 2: out[0] = sum of the cell values - strided partial sums in index order, then a tree with fixed shape (dot_finish_kernel)
__global__ __launch_bounds__(256) void stokes_divergence_finish(long long ncells, const double *__restrict__ cells, double *__restrict__ out)
{
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < ncells; i += 256) s += cells[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

} // namespace

extern "C" {

// cell_out: device, n_cells entries (cell = cx + ncx (cy + ncy cz)), or NULL; total: host.  Synchronous.
int stfem_stokes_divergence(stfem_stokes_ctx *c, const double *u, double *cell_out, double *total, void *stream)
{
  if (!c || !u || !total) return STFEM_ERR_INVALID_ARGUMENT; // (before anything touches the device)
  if (const int rq = stokes_require_q2(c, "stfem_stokes_divergence")) return rq;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
  if (!c->d_div) {
    if (hipMalloc(&c->d_div, (size_t(ncells) + 1) * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      c->d_div = nullptr;
      return STFEM_ERR_OUT_OF_MEMORY;
    }
  }
  DivergenceParams k;
  k.vertices = c->d_vertices;
  k.u = u;
  k.cell_out = cell_out ? cell_out : c->d_div;
  k.ncx = c->nc[0]; k.ncy = c->nc[1]; k.ncz = c->nc[2];
  k.ndu[0] = c->ndu[0]; k.ndu[1] = c->ndu[1];
  k.Nu = c->Nu;
  for (int i = 0; i < 9; ++i) { k.Su[i] = c->base.Su[i]; k.Du[i] = c->base.Du[i]; }
  for (int i = 0; i < 3; ++i) { k.xq[i] = c->base.xq[i]; k.wq[i] = c->base.wq[i]; }
  stfem_launch_begin();
  const unsigned grid = (unsigned)std::min<long long>((ncells + 7) / 8, 4ll * c->n_cu);
  hipLaunchKernelGGL(stokes_divergence_kernel, dim3(grid), dim3(256), 0, st, k);
  hipLaunchKernelGGL(stokes_divergence_finish, dim3(1), dim3(256), 0, st, ncells, (const double *)k.cell_out, c->d_div + ncells);
  if (const int rc = stfem_launch_end("stokes_divergence_kernel")) return rc;
  double sum = 0.0;
  STFEM_TRY(hipMemcpyAsync(&sum, c->d_div + ncells, sizeof(double), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  *total = std::sqrt(sum);
  return STFEM_OK;
}

} // extern "C"
