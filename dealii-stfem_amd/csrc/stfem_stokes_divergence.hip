// Stokes two-field operator: the divergence functional of a velocity, for velocity degree DEG = 2 (FE_Q(2)^3, QGauss(3)) and DEG = 3
// (FE_Q(3)^3, QGauss(4), reached through stfem_stokes_divergence_space of include/stfem_stokes_pressure_space.h),
//   StokesMatrixFreeOperator::compute_divergence / divergence_cell_loop (reference include/operators.h:1391-1439):
//   cell_vector[cell] = sum_q (div u_h)^2 JxW at the operator's (DEG + 1)^3 Gauss points, the return value sqrt(sum_cell cell_vector[cell]).
// The velocity is read PLAIN (read_dof_values_plain, 1430): entries on strongly constrained DoFs count as stored, not as zero.
// Nothing is scattered, so there are no colours: one launch over all cells, every cell writes its own entry, then one workgroup
// sums the entries in a fixed order - no atomics, bitwise reproducible.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cmath>

namespace {

template <int DEG> struct DivergenceParamsT {
  const double *vertices; // device, (nc+1)^3 * 3
  const double *u;        // [3][Nu]
  double *cell_out;       // [n_cells], cell = cx + ncx (cy + ncy cz)
  int ncx, ncy, ncz;
  int ndu[2];
  long long Nu;
  double Su[(DEG + 1) * (DEG + 1)], Du[(DEG + 1) * (DEG + 1)]; // [q*(DEG+1)+a]
  double xq[DEG + 1], wq[DEG + 1];
};

// The cell layout of stokes_cell_kernel and stokes_convection_kernel: lane t = a + (DEG + 1) b + (DEG + 1)^2 c of a cell is its
// velocity node and its Gauss point - degree 2: one half-wave per cell, 27 active lanes, 256 threads = 8 cells at a time; degree 3: one
// wave per cell, 64 lanes = 64 nodes = 64 points, 4 cells at a time -, persistent workgroups striding over the cells, two wave-private
// LDS regions per cell handed between the sum-factorised 1D stages behind wave_fence() (6 x NN doubles after the x stage, 9 x NN after
// the y stage), the MappingQ1 metric from the eight vertices at this lane's quadrature point (boxes take the same path: their metric
// is the diagonal one up to rounding).
//   evaluate (gradients only, three fields): lane (n_x, n_y, n_z) -> (q_x, n_y, n_z) -> (q_x, q_y, n_z) -> quadrature point
template <int DEG>
__global__ __launch_bounds__(256) void stokes_divergence_kernel(const DivergenceParamsT<DEG> prm)
{
  constexpr int N1 = DEG + 1, N2 = N1 * N1, NN = N1 * N2; // nodes = quadrature points per direction, per cell: 27 or 64
  constexpr int LANES = NN <= 32 ? 32 : 64, CELLS = 256 / LANES;
  constexpr int RX = 9 * NN, RY = 6 * NN; // doubles per cell of the two regions: 9 x NN after the y stage, 6 x NN after the x stage
  __shared__ double smem[CELLS * (RX + RY)];
  __shared__ double tS[N2], tD[N2];
  if (threadIdx.x < N2) { tS[threadIdx.x] = prm.Su[threadIdx.x]; tD[threadIdx.x] = prm.Du[threadIdx.x]; }
  __syncthreads();
  const int slot = threadIdx.x / LANES, tl = threadIdx.x % LANES;
  const bool lane_on = NN == LANES || tl < NN;
  const int t = lane_on ? tl : 0;
  const int a = t % N1, b = (t / N1) % N1, c = t / N2;
  double *X = smem + slot * (RX + RY), *Y = X + RX;
  double Sa[N1], Da[N1], Sb[N1], Db[N1], Sc[N1], Dc[N1]; // rows of this lane's quadrature indices
#pragma unroll
  for (int n = 0; n < N1; ++n) {
    Sa[n] = tS[a * N1 + n]; Da[n] = tD[a * N1 + n];
    Sb[n] = tS[b * N1 + n]; Db[n] = tD[b * N1 + n];
    Sc[n] = tS[c * N1 + n]; Dc[n] = tD[c * N1 + n];
  }
  const double wabc = prm.wq[a] * prm.wq[b] * prm.wq[c];
  const long long ncells = (long long)prm.ncx * prm.ncy * prm.ncz;
  // (the trip count is the same for all cells of a workgroup: the two half-waves of a wave at degree 2 fence together)
  for (long long first = (long long)blockIdx.x * CELLS; first < ncells; first += (long long)gridDim.x * CELLS) {
    const long long cell = first + slot;
    const bool ok = cell < ncells;
    const long long cc = ok ? cell : 0;
    const int cx = int(cc % prm.ncx), cy = int((cc / prm.ncx) % prm.ncy), cz = int(cc / ((long long)prm.ncx * prm.ncy));
    const long long gu = (DEG * cx + a) + (long long)prm.ndu[0] * ((DEG * cy + b) + (long long)prm.ndu[1] * (DEG * cz + c));

    // ---- gather (plain): X = u[3][NN]
    if (lane_on) {
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) X[comp * NN + t] = ok ? prm.u[comp * prm.Nu + gu] : 0.0;
    }
    wave_fence();
    // ---- x: (n_x, n_y, n_z) -> (q_x, n_y, n_z): value and x derivative -> Y[(2 f + {0, 1}) * NN + t]
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *u = X + f * NN + N1 * b + N2 * c;
      Y[(2 * f) * NN + t] = dot<N1>(Sa, u);
      Y[(2 * f + 1) * NN + t] = dot<N1>(Da, u);
    }
    wave_fence();
    // ---- y: -> (q_x, q_y, n_z): d/dx, d/dy and the value -> X[(3 f + {0, 1, 2}) * NN + t]
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *v = Y + (2 * f) * NN + a + N2 * c, *vx = v + NN;
      X[(3 * f) * NN + t] = dot<N1>(Sb, vx, N1);
      X[(3 * f + 1) * NN + t] = dot<N1>(Db, v, N1);
      X[(3 * f + 2) * NN + t] = dot<N1>(Sb, v, N1);
    }
    wave_fence();
    // ---- z: -> quadrature point (a, b, c): the reference gradients g[f][e] = d u_f / d xi_e in registers
    double g[3][3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double *w0 = X + (3 * f) * NN + a + N1 * b, *w1 = w0 + NN, *w2 = w0 + 2 * NN;
      g[f][0] = dot<N1>(Sc, w0, N2);
      g[f][1] = dot<N1>(Sc, w1, N2);
      g[f][2] = dot<N1>(Dc, w2, N2);
    }

    // ---- quadrature-point operation (operators.h:1432-1436): div u = sum_f sum_e (dxi_e / dx_f) g[f][e]
    const double xi[3] = {prm.xq[a], prm.xq[b], prm.xq[c]};
    double Ji[3][3];
    const double det = mapping_q1_inverse(prm.vertices, prm.ncx, prm.ncy, cx, cy, cz, xi, Ji);
    double div = 0.0;
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
      for (int e = 0; e < 3; ++e) div = fma(Ji[e][f], g[f][e], div);
    if (lane_on) Y[t] = div * div * (det * wabc);
    wave_fence();
    // ---- the cell's sum over its NN points, in point order, by one lane
    if (ok && tl == 0) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NN; ++q) s += Y[q];
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

// The cell launch at degree DEG, with its plan (stfem_stokes_last_divergence_plan).  Degree 2: four workgroups of eight cells at a time
// per CU.  Degree 3: persistent workgroups of four waves, as many as stay resident; STFEM_STOKES_Q3_WORKGROUPS=<n>, read at every
// launch, caps them (tests: several cells per wave on a small mesh)
template <int DEG> void divergence_launch(stfem_stokes_ctx *c, const double *u, double *cells, long long ncells, hipStream_t st)
{
  constexpr int per = DEG == 3 ? 4 : 8; // cells of a workgroup at a time
  const StokesParamsT<DEG> &g = c->desc<DEG>();
  DivergenceParamsT<DEG> k;
  k.vertices = c->d_vertices;
  k.u = u;
  k.cell_out = cells;
  k.ncx = c->nc[0]; k.ncy = c->nc[1]; k.ncz = c->nc[2];
  k.ndu[0] = c->ndu[0]; k.ndu[1] = c->ndu[1];
  k.Nu = c->Nu;
  for (int i = 0; i < (DEG + 1) * (DEG + 1); ++i) { k.Su[i] = g.Su[i]; k.Du[i] = g.Du[i]; }
  for (int i = 0; i < DEG + 1; ++i) { k.xq[i] = g.xq[i]; k.wq[i] = g.wq[i]; }
  long long grid = std::min<long long>((ncells + per - 1) / per, 4ll * c->n_cu);
  if constexpr (DEG == 3) {
    static int resident = 0;
    grid = std::min<long long>((ncells + per - 1) / per, (long long)c->n_cu * stokes_resident(resident, (const void *)stokes_divergence_kernel<3>));
    if (const char *e = getenv("STFEM_STOKES_Q3_WORKGROUPS")) grid = std::min(grid, std::max(1ll, atoll(e)));
  }
  hipLaunchKernelGGL(stokes_divergence_kernel<DEG>, dim3((unsigned)grid), dim3(256), 0, st, k);
  c->divergence_plan[0] = (int)grid;
  c->divergence_plan[1] = (int)((ncells + grid * per - 1) / (grid * per));
}

// The functional at the context's degree (the entry points have checked their arguments)
int stokes_divergence(stfem_stokes_ctx *c, const double *u, double *cell_out, double *total, void *stream)
{
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
  double *cells = cell_out ? cell_out : c->d_div;
  stfem_launch_begin();
  stokes_with_degree(c, [&](auto deg) { divergence_launch<deg()>(c, u, cells, ncells, st); });
  c->divergence_launched = true; // (stfem_stokes_last_divergence_plan)
  hipLaunchKernelGGL(stokes_divergence_finish, dim3(1), dim3(256), 0, st, ncells, (const double *)cells, c->d_div + ncells);
  if (const int rc = stfem_launch_end("stokes_divergence_kernel")) return rc;
  double sum = 0.0;
  STFEM_TRY(hipMemcpyAsync(&sum, c->d_div + ncells, sizeof(double), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  *total = std::sqrt(sum);
  return STFEM_OK;
}

} // namespace

extern "C" {

// cell_out: device, n_cells entries (cell = cx + ncx (cy + ncy cz)), or NULL; total: host.  Synchronous.
int stfem_stokes_divergence(stfem_stokes_ctx *c, const double *u, double *cell_out, double *total, void *stream)
{
  if (!c || !u || !total) return STFEM_ERR_INVALID_ARGUMENT; // (before anything touches the device)
  if (const int rq = stokes_require_q2(c, "stfem_stokes_divergence")) return rq;
  return stokes_divergence(c, u, cell_out, total, stream);
}

// The same for a context of either degree (include/stfem_stokes_pressure_space.h): degree 2 is the entry above, launch for launch
int stfem_stokes_divergence_space(stfem_stokes_ctx *c, const double *u, double *cell_out, double *total, void *stream)
{
  if (!c || !u || !total) return STFEM_ERR_INVALID_ARGUMENT;
  return stokes_divergence(c, u, cell_out, total, stream);
}

int stfem_stokes_last_divergence_plan(const stfem_stokes_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (!c->divergence_launched)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_last_divergence_plan: this context has not launched the divergence kernel");
  out[0] = c->divergence_plan[0];
  out[1] = c->divergence_plan[1];
  return STFEM_OK;
}

} // extern "C"
