// Cell-patch Vanka / additive-Schwarz smoother of the space-time system.
//
// Replaces PreconditionVanka (reference include/stmg.h:619-907) for the scalar system
// A = Alpha (x) K + Beta (x) M on one rank:
//   set-up (stmg.h:786-829, compute_block_matrix.h:50-139): per cell the block
//       B_c(k + i n, l + j n) = valence(k) * (Beta(i,j) M(k,l) + Alpha(i,j) K(k,l)),   k, l = DoFs of the cell,
//     K, M = the ASSEMBLED matrices with the zero-boundary constraints (tests/tp_01.cc:283-299), inverted by
//     Gauss-Jordan;
//   vmult (stmg.h:832-872): dst = sum over cells of scatter(B_c^-1 gather(src)).
// On the axis-aligned uniform meshes this path serves (cfg 1), the restriction of an assembled Kronecker
// matrix to a cell is the Kronecker product of restricted 1D matrices, and it only depends on which
// neighbours the cell has: at most 27 different blocks per mesh instead of one 250 x 250 block per cell
// (250 kB per Q4 x cG(2) cell in fp32).  The apply is then a GEMM per block class,
//       Y[250 x cells] = B^-1[250 x 250] X[250 x cells],
// with the gather and the scatter fused in: MFMA work (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32,
// 125 kflop against 4 kB of DoF traffic per cell).  Cells are processed in eight colours (cells of one
// colour share no DoF), so the scatter is plain load-add-store: no atomics, bitwise reproducible.
// General meshes and coefficient tables get one block per cell (the reference's layout): set-up on the device (or, for
// comparison, on the host from device-computed cell matrices), apply = one HBM-bound block-times-vector per cell
// (vanka_apply_percell_kernel).  Meshes of up to 50 000 cells take two launches instead of eight: all cells at once, then
// vanka_collect_kernel.
// The host steps of the set-up - block classes, cell lists, tile plan, constrain / scale / invert / store - are in
// stfem_vanka_setup.h, shared with the Stokes smoother; uploads and launches go through the helpers of stfem_vanka_kernel.h.
#include "stfem_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "stfem_vanka_kernel.h"
#include "stfem_vanka_setup.h"

namespace vanka = stfem::vanka;

namespace {

// ---- general meshes / coefficient tables: one block per cell ----
// Cell matrices from the stored metric: K_c(a,b) = sum_q grad phi_a^T G_q grad phi_b, M_c(a,b) = sum_q Mq phi_a phi_b
// (what MatrixFreeTools::compute_matrix gets from do_cell_integral_local on unit vectors, operators.h:1021-1033).
// One workgroup per cell; a thread takes entries (a, b).  Set-up code: plain, not tuned.
template <typename T>
__global__ __launch_bounds__(256) void vanka_cell_matrices_kernel(int n, const T *__restrict__ metric,
                                                                   const double *__restrict__ S1, const double *__restrict__ D1,
                                                                   double *__restrict__ Kc, double *__restrict__ Mc)
{
  const int nloc = n * n * n;
  extern __shared__ double sm[]; // [nloc][7] metric of the cell, [n*n] S, [n*n] D
  double *met = sm, *S = sm + nloc * 7, *D = S + n * n;
  const long long cell = blockIdx.x;
  for (int i = threadIdx.x; i < nloc * 7; i += 256) met[i] = double(metric[(cell * nloc + i / 7) * 8 + i % 7]);
  for (int i = threadIdx.x; i < n * n; i += 256) { S[i] = S1[i]; D[i] = D1[i]; }
  __syncthreads();
  for (int e = threadIdx.x; e < nloc * nloc; e += 256) {
    const int a = e / nloc, b = e % nloc;
    const int ax = a % n, ay = (a / n) % n, az = a / (n * n), bx = b % n, by = (b / n) % n, bz = b / (n * n);
    double k = 0.0, mm = 0.0;
    for (int qz = 0; qz < n; ++qz)
      for (int qy = 0; qy < n; ++qy)
        for (int qx = 0; qx < n; ++qx) {
          const double *g = met + (qx + n * (qy + n * qz)) * 7;
          const double sax = S[qx * n + ax], say = S[qy * n + ay], saz = S[qz * n + az];
          const double sbx = S[qx * n + bx], sby = S[qy * n + by], sbz = S[qz * n + bz];
          const double ga[3] = {D[qx * n + ax] * say * saz, sax * D[qy * n + ay] * saz, sax * say * D[qz * n + az]};
          const double gb[3] = {D[qx * n + bx] * sby * sbz, sbx * D[qy * n + by] * sbz, sbx * sby * D[qz * n + bz]};
          k += ga[0] * (g[0] * gb[0] + g[1] * gb[1] + g[2] * gb[2]) + ga[1] * (g[1] * gb[0] + g[3] * gb[1] + g[4] * gb[2]) +
               ga[2] * (g[2] * gb[0] + g[4] * gb[1] + g[5] * gb[2]);
          mm += g[6] * sax * say * saz * sbx * sby * sbz;
        }
    Kc[cell * nloc * nloc + e] = k;
    Mc[cell * nloc * nloc + e] = mm;
  }
}

struct VankaCellParams {
  const void *src[VK_MAX_BLOCKS];
  void *dst[VK_MAX_BLOCKS];
  const void *blocks; // [cell][kpad][mpad], element (row r, column k) of the cell's inverse at [k][r]
  const int *off;
  const int *cell;    // [ncell of this colour]: cell number
  int m, mpad, kpad, nloc, p, colour;
  int ncx, ncy, ncz, nx, ny;
  void *flat;         // two-phase apply (small meshes): Y[cell][mpad]; nullptr: colour launches
  double omega;
  int accumulate;
};

// y = B_c^-1 x per cell, the block streamed from HBM once (the reference's apply: stmg.h:845-867): one workgroup per
// cell, thread r = row r; x in LDS.  HBM-bound: kpad * mpad elements per cell against 2 m of DoF traffic.
template <typename T>
__global__ __launch_bounds__(256) void vanka_apply_percell_kernel(const VankaCellParams prm)
{
  __shared__ T xs[VK_MAX_ROWS];
  const int cell = prm.flat ? int(blockIdx.x) : prm.cell[blockIdx.x];
  const int cx = cell % prm.ncx, cy = (cell / prm.ncx) % prm.ncy, cz = cell / (prm.ncx * prm.ncy);
  const long long base = (long long)prm.p * cx + (long long)prm.nx * ((long long)prm.p * cy + (long long)prm.ny * prm.p * cz);
  for (int r = threadIdx.x; r < prm.kpad; r += 256) {
    T v = T(0);
    if (r < prm.m) {
      const int blk = r / prm.nloc, n = r - blk * prm.nloc;
      const T *sp = static_cast<const T *>(prm.src[0]);
#pragma unroll
      for (int b = 1; b < VK_MAX_BLOCKS; ++b)
        if (b == blk) sp = static_cast<const T *>(prm.src[b]);
      v = sp[base + prm.off[n]];
    }
    xs[r] = v;
  }
  __syncthreads();
  const T *B = static_cast<const T *>(prm.blocks) + (size_t)cell * prm.kpad * prm.mpad;
  for (int r = threadIdx.x; r < prm.m; r += 256) {
    T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
    const T *col = B + r;
    int k = 0;
    for (; k + 3 < prm.kpad; k += 4) {
      a0 = fma(col[(size_t)k * prm.mpad], xs[k], a0);
      a1 = fma(col[(size_t)(k + 1) * prm.mpad], xs[k + 1], a1);
      a2 = fma(col[(size_t)(k + 2) * prm.mpad], xs[k + 2], a2);
      a3 = fma(col[(size_t)(k + 3) * prm.mpad], xs[k + 3], a3);
    }
    for (; k < prm.kpad; ++k) a0 = fma(col[(size_t)k * prm.mpad], xs[k], a0);
    const T y = (a0 + a1) + (a2 + a3);
    if (prm.flat) {
      static_cast<T *>(prm.flat)[size_t(cell) * prm.mpad + r] = y;
      continue;
    }
    const int blk = r / prm.nloc, n = r - blk * prm.nloc;
    T *dp = static_cast<T *>(prm.dst[0]);
#pragma unroll
    for (int b = 1; b < VK_MAX_BLOCKS; ++b)
      if (b == blk) dp = static_cast<T *>(prm.dst[b]);
    // first touch (lowest colour among the cells sharing the DoF) stores, the others add
    const int np = prm.p + 1;
    const int idx[3] = {n % np, (n / np) % np, n / (np * np)};
    const int cc[3] = {cx, cy, cz}, nc[3] = {prm.ncx, prm.ncy, prm.ncz};
    bool first = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const bool shared = (idx[d] == 0 && cc[d] > 0) || (idx[d] == prm.p && cc[d] < nc[d] - 1);
      if (shared && ((prm.colour >> d) & 1)) first = false;
    }
    T *q = dp + base + prm.off[n];
    const T oy = T(prm.omega) * y;
    *q = (first && !prm.accumulate) ? oy : *q + oy;
  }
}


// Second phase of the two-phase apply (small meshes, where eight colour launches of ~20 us each are all latency): every DoF sums
// the rows its (up to eight) cells left in the scratch array, in a fixed order (z, y, x of the cells) - reproducible - and
// stores: dst = sum over cells of scatter(B_c^-1 gather(src)) (stmg.h:836-867) in two launches instead of eight.
struct VankaCollectParams {
  void *dst[VK_MAX_BLOCKS];
  const void *y;    // [slot][mpad]
  const int *slot;  // cell -> slot (nullptr: slot = cell)
  int nb, nloc, p, mpad;
  int ncx, ncy, ncz, nx, ny, nz;
  double omega;
  int accumulate;
};
template <typename T> __global__ __launch_bounds__(256) void vanka_collect_kernel(const VankaCollectParams prm)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)prm.nx * prm.ny * prm.nz) return;
  const int ix = int(i % prm.nx), iy = int((i / prm.nx) % prm.ny), iz = int(i / ((long long)prm.nx * prm.ny));
  const int p = prm.p, np = p + 1;
  int cc[3][2], ll[3][2], cnt[3];
  const int idx[3] = {ix, iy, iz}, nc[3] = {prm.ncx, prm.ncy, prm.ncz};
  node_cells(idx, p, nc, cc, ll, cnt);
  T acc[VK_MAX_BLOCKS];
#pragma unroll
  for (int b = 0; b < VK_MAX_BLOCKS; ++b) acc[b] = T(0);
  const T *Y = static_cast<const T *>(prm.y);
  for (int kz = 0; kz < cnt[2]; ++kz)
    for (int ky = 0; ky < cnt[1]; ++ky)
      for (int kx = 0; kx < cnt[0]; ++kx) {
        const int cell = cc[0][kx] + prm.ncx * (cc[1][ky] + prm.ncy * cc[2][kz]);
        const int n = ll[0][kx] + np * (ll[1][ky] + np * ll[2][kz]);
        const T *row = Y + size_t(prm.slot ? prm.slot[cell] : cell) * prm.mpad + n;
#pragma unroll
        for (int b = 0; b < VK_MAX_BLOCKS; ++b)
          if (b < prm.nb) acc[b] += row[b * prm.nloc];
      }
#pragma unroll
  for (int b = 0; b < VK_MAX_BLOCKS; ++b)
    if (b < prm.nb) {
      T *d = static_cast<T *>(prm.dst[b]) + i;
      *d = prm.accumulate ? *d + T(prm.omega) * acc[b] : T(prm.omega) * acc[b];
    }
}

// ---- device-side set-up of the per-cell blocks (large general meshes: MI355X holds the reference's one-block-per-cell layout of
// a whole configs[2] / configs[3] mesh in HBM; the set-up must then not go through the host either) ----
struct VankaAssembleParams {
  const double *Kc, *Mc; // cell matrices of the cell layers [zw0, zw1)
  double *B;             // [cell of the batch][m][m]
  int ncx, ncy, ncz, p, nb, dmask;
  int zw0;               // first cell layer held in Kc / Mc
  int z0, ncells_batch;  // the batch: cell layers from z0, ncells_batch cells
  double Alpha[VK_MAX_BLOCKS * VK_MAX_BLOCKS], Beta[VK_MAX_BLOCKS * VK_MAX_BLOCKS];
};

// One workgroup per cell: the restriction of the ASSEMBLED K, M to the cell's DoFs (own cell matrix + what the neighbours add on
// shared faces, edges and vertices: compute_block_matrix.h:50-139), zero-boundary rows / columns with the diagonal kept, valence
// scaling of the rows, Kronecker with Alpha / Beta (stmg.h:806-829).  Same steps as vanka_create_per_cell_host.
__global__ __launch_bounds__(256) void vanka_assemble_kernel(const VankaAssembleParams prm)
{
  const int n = prm.p + 1, nloc = n * n * n, m = prm.nb * nloc;
  const int lc = blockIdx.x; // cell of the batch
  const int cpl = prm.ncx * prm.ncy;
  const int cz = prm.z0 + lc / cpl, cy = (lc % cpl) / prm.ncx, cx = lc % prm.ncx;
  const int cc[3] = {cx, cy, cz}, nc[3] = {prm.ncx, prm.ncy, prm.ncz};
  double *B = prm.B + (size_t)lc * m * m;
  for (int e = threadIdx.x; e < nloc * nloc; e += blockDim.x) {
    const int a = e / nloc, b = e % nloc;
    const int ia[3] = {a % n, (a / n) % n, a / (n * n)}, ib[3] = {b % n, (b / n) % n, b / (n * n)};
    double val = 1.0;
    bool con_a = false, con_b = false;
    int lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if ((ia[d] == 0 && cc[d] > 0) || (ia[d] == prm.p && cc[d] < nc[d] - 1)) val *= 2.0;
      const bool lo_face = cc[d] == 0 && (prm.dmask & (1 << (2 * d))), hi_face = cc[d] == nc[d] - 1 && (prm.dmask & (2 << (2 * d)));
      con_a = con_a || (ia[d] == 0 && lo_face) || (ia[d] == prm.p && hi_face);
      con_b = con_b || (ib[d] == 0 && lo_face) || (ib[d] == prm.p && hi_face);
      lo[d] = (ia[d] == 0 && ib[d] == 0 && cc[d] > 0) ? -1 : 0;
      hi[d] = (ia[d] == prm.p && ib[d] == prm.p && cc[d] < nc[d] - 1) ? 1 : 0;
    }
    double ks = 0.0, ms = 0.0;
    if (a == b || !(con_a || con_b)) {
      for (int sz = lo[2]; sz <= hi[2]; ++sz)
        for (int sy = lo[1]; sy <= hi[1]; ++sy)
          for (int sx = lo[0]; sx <= hi[0]; ++sx) {
            const int sh[3] = {sx, sy, sz};
            int a2 = 0, b2 = 0, mul = 1;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              a2 += (sh[d] == -1 ? prm.p : (sh[d] == 1 ? 0 : ia[d])) * mul;
              b2 += (sh[d] == -1 ? prm.p : (sh[d] == 1 ? 0 : ib[d])) * mul;
              mul *= n;
            }
            const size_t c2 = (size_t)(cx + sx) + (size_t)prm.ncx * ((cy + sy) + (size_t)prm.ncy * (cz + sz - prm.zw0));
            ks += prm.Kc[(c2 * nloc + a2) * nloc + b2];
            ms += prm.Mc[(c2 * nloc + a2) * nloc + b2];
          }
    }
    for (int i = 0; i < prm.nb; ++i)
      for (int j = 0; j < prm.nb; ++j)
        B[(size_t)(i * nloc + a) * m + j * nloc + b] = val * (prm.Beta[i * prm.nb + j] * ms + prm.Alpha[i * prm.nb + j] * ks);
  }
}

// In-place Gauss-Jordan inverse with partial pivoting (FullMatrix::gauss_jordan, stmg.h:828; the steps of vanka::invert, stfem_vanka_setup.h), one
// workgroup per m x m matrix in global memory, then the block in the apply's layout: out[k][r] = T(inverse(r, k)), row stride mpad.
template <typename T>
__global__ __launch_bounds__(256) void vanka_invert_kernel(double *__restrict__ Ball, T *__restrict__ out_all, int m, int mpad, int kpad,
                                                            long long cell0, int *__restrict__ singular)
{
  __shared__ double rowc[VK_MAX_ROWS];
  __shared__ int piv[VK_MAX_ROWS];
  __shared__ double rbest[256];
  __shared__ int rarg[256];
  double *A = Ball + (size_t)blockIdx.x * m * m;
  const int t = threadIdx.x;
  for (int c = 0; c < m; ++c) {
    double best = -1.0;
    int arg = c;
    for (int r = c + t; r < m; r += 256) {
      const double v = fabs(A[(size_t)r * m + c]);
      if (v > best) { best = v; arg = r; }
    }
    rbest[t] = best;
    rarg[t] = arg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) {
        // the first (lowest) row among equal magnitudes, as the sequential search picks it
        if (rbest[t + s] > rbest[t] || (rbest[t + s] == rbest[t] && rarg[t + s] < rarg[t])) { rbest[t] = rbest[t + s]; rarg[t] = rarg[t + s]; }
      }
      __syncthreads();
    }
    const int p = rarg[0];
    const double pv = rbest[0];
    if (pv <= 0.0) {
      if (t == 0) *singular = 1;
      return;
    }
    if (t == 0) piv[c] = p;
    // swap rows c and p, scale the pivot row, keep it in LDS
    const double inv = 1.0 / A[(size_t)p * m + c];
    __syncthreads(); // (every thread has read the pivot before the row is rewritten)
    for (int k = t; k < m; k += 256) {
      const double up = A[(size_t)p * m + k], uc = A[(size_t)c * m + k];
      if (p != c) A[(size_t)p * m + k] = uc;
      const double v = (k == c ? 1.0 : up) * inv;
      A[(size_t)c * m + k] = v;
      rowc[k] = v;
    }
    __syncthreads();
    // eliminate column c from every other row: a wave takes a row at a time, lanes along the row
    const int wave = t >> 6, lane = t & 63;
    for (int r = wave; r < m; r += 4) {
      if (r == c) continue;
      const double f = A[(size_t)r * m + c];
      if (f == 0.0) continue;
      for (int k = lane; k < m; k += 64) {
        const double v = (k == c ? 0.0 : A[(size_t)r * m + k]) - f * rowc[k];
        A[(size_t)r * m + k] = v;
      }
    }
    __syncthreads();
  }
  // undo the row exchanges on the columns, last first
  for (int c = m - 1; c >= 0; --c) {
    const int p = piv[c];
    if (p != c) {
      for (int r = t; r < m; r += 256) {
        const double a = A[(size_t)r * m + c];
        A[(size_t)r * m + c] = A[(size_t)r * m + p];
        A[(size_t)r * m + p] = a;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  T *out = out_all + (size_t)(cell0 + blockIdx.x) * kpad * mpad;
  for (int e = t; e < kpad * mpad; e += 256) {
    const int k = e / mpad, r = e % mpad;
    out[e] = (k < m && r < m) ? T(A[(size_t)r * m + k]) : T(0);
  }
}

} // namespace

// vanka_invert_kernel<double> for the other translation units (the per-cell Stokes blocks, stfem_stokes_vanka_cell.hip)
int stfem_vanka_invert_launch(double *B, double *out, int m, int mpad, int kpad, long long cell0, unsigned count, int *singular, void *stream)
{
  if (m < 1 || m > VK_MAX_ROWS || count == 0) return STFEM_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(vanka_invert_kernel<double>, dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream), B, out, m, mpad, kpad, cell0, singular);
  return stfem_launch_end("vanka_invert_kernel");
}

constexpr int VK_FLAT = 8; // the launch after the eight colours: all cells at once (two-phase apply)

struct stfem_vanka {
  stfem_ctx *ctx = nullptr;
  int nb = 0, nloc = 0, m = 0, mt = 0, mtw = 0, parts = 0, mpad = 0, kpad = 0, nclasses = 0;
  int setup_batches = 0; // batches of cell layers the device set-up of the per-cell blocks took (stfem_vanka_setup_batches)
  void *d_blocks = nullptr;
  void *d_blocks_base = nullptr; // allocation d_blocks points into (blocks built on an extended context: the ghost layers' come first)
  int *d_off = nullptr;
  bool per_cell = false; // one block per cell (general meshes, coefficient tables): d_blocks is [cell][kpad][mpad]
  // the launches of an apply: colours 0 - 7, or VK_FLAT alone.  Class blocks: d_cell = first DoF per list entry, d_cls per quad
  // of 64 entries, ngrid quads; per-cell blocks: d_cell = cell numbers (VK_FLAT: every cell, no list), ngrid cells.
  int *d_cell[VK_FLAT + 1] = {}, *d_cls[VK_FLAT + 1] = {};
  int ngrid[VK_FLAT + 1] = {};
  // two-phase apply (meshes of up to VK_FLAT_CELLS cells): all cells in ONE launch, rows to d_flat, then vanka_collect_kernel
  bool flat = false;
  void *d_flat = nullptr;
  int *d_slot = nullptr;
};
using VankaPtr = std::unique_ptr<stfem_vanka, void (*)(stfem_vanka *)>; // (released only into *out)

constexpr long long VK_FLAT_CELLS = 50000; // (36^3 cells: 45 us instead of 8 x 23; at 72^3 the scratch traffic costs more than the launches)
static bool vanka_wants_flat(const stfem_ctx *c)
{
  if (const char *e = getenv("STFEM_VANKA_COLOURS")) // (tests and measurements: the colour launches on small meshes too)
    if (atoi(e)) return false;
  return c->ncells <= VK_FLAT_CELLS;
}

// the float or double instantiation of kernel template K, by the context's Number type
#define VK_TYPED(c, K) ((c)->prec ? reinterpret_cast<const void *>(&K<float>) : reinterpret_cast<const void *>(&K<double>))

template <typename T, int NLOC> static const void *vanka_kernel(int mtw)
{
  switch (mtw) {
#define VK_CASE(MT) case MT: return reinterpret_cast<const void *>(&vanka_apply_kernel<T, NLOC, MT>);
    VK_CASE(1) VK_CASE(2) VK_CASE(3) VK_CASE(4) VK_CASE(6) VK_CASE(8)
#undef VK_CASE
    default: return nullptr;
  }
}
template <typename T> static const void *vanka_kernel(int p, int mtw)
{
  switch (p) {
    case 1: return vanka_kernel<T, 8>(mtw);
    case 2: return vanka_kernel<T, 27>(mtw);
    case 3: return vanka_kernel<T, 64>(mtw);
    case 4: return vanka_kernel<T, 125>(mtw);
    case 5: return vanka_kernel<T, 216>(mtw);
    default: return nullptr;
  }
}
static const void *vanka_kernel(const stfem_ctx *c, int mtw) { return stfem_by_prec(c, [&](auto t) { return vanka_kernel<decltype(t)>(c->p, mtw); }); }

static int vanka_collect(const stfem_vanka *v, stfem_vec *dst, double omega, int accumulate, hipStream_t st)
{
  const stfem_ctx *c = v->ctx;
  VankaCollectParams cp;
  std::memset(&cp, 0, sizeof(cp));
  for (int i = 0; i < v->nb; ++i) cp.dst[i] = dst->blk[i];
  cp.y = v->d_flat;
  cp.slot = v->d_slot;
  cp.nb = v->nb; cp.nloc = v->nloc; cp.p = c->p; cp.mpad = v->mpad;
  cp.ncx = c->nc[0]; cp.ncy = c->nc[1]; cp.ncz = c->nc[2]; cp.nx = c->nd[0]; cp.ny = c->nd[1]; cp.nz = c->nd[2];
  cp.omega = omega; cp.accumulate = accumulate;
  return vk_launch(VK_TYPED(c, vanka_collect_kernel), dim3((unsigned)((c->ndofs + 255) / 256)), &cp, st, "vanka_collect_kernel");
}

// a new smoother on context c, nothing built yet
static VankaPtr vanka_new(stfem_ctx *c, int nb)
{
  VankaPtr v(new (std::nothrow) stfem_vanka, stfem_vanka_destroy);
  if (v) {
    const int n = c->p + 1;
    v->ctx = c; v->nb = nb; v->nloc = n * n * n; v->m = nb * v->nloc;
  }
  return v;
}

// local node -> DoF offset from the cell's first node
static int vanka_offset_table(stfem_vanka *v)
{
  const stfem_ctx *c = v->ctx;
  const int n = c->p + 1;
  std::vector<int> off(v->nloc);
  for (int kz = 0; kz < n; ++kz)
    for (int jy = 0; jy < n; ++jy)
      for (int ix = 0; ix < n; ++ix) off[ix + n * (jy + n * kz)] = ix + c->nd[0] * (jy + c->nd[1] * kz);
  return vk_upload(&v->d_off, off);
}

// per-cell variant: one block of mt row tiles per cell
static void vanka_per_cell_shape(stfem_vanka *v)
{
  v->per_cell = true;
  v->mt = (v->m + 15) / 16;
  v->mpad = 16 * v->mt;
  v->kpad = ((v->m + 3) / 4) * 4;
}

// The blocks on the host, in the context's Number type and the apply's layout [block][kpad][mpad], filled block by block from the
// restricted assembled matrices K, M of a cell with its constrained nodes (con) and node valences (val): stmg.h:806-829
namespace {
struct VankaHostBlocks {
  const stfem_vanka *v;
  const double *Alpha, *Beta;
  std::vector<float> f32;
  std::vector<double> f64, B;
  std::vector<int> dof; // row -> node
  VankaHostBlocks(const stfem_vanka *v_, size_t count, const double *Alpha_, const double *Beta_) : v(v_), Alpha(Alpha_), Beta(Beta_), dof(v_->m)
  {
    if (v->ctx->prec) f32.resize(count * v->kpad * v->mpad);
    else f64.resize(count * v->kpad * v->mpad);
    for (int r = 0; r < v->m; ++r) dof[r] = r % v->nloc;
  }
  bool add(size_t index, const std::vector<double> &K, const std::vector<double> &M, const std::vector<char> &con, const std::vector<double> &val) // false: singular
  {
    const size_t at = index * v->kpad * v->mpad;
    vanka::combine_scalar(v->nb, v->nloc, Alpha, Beta, K, M, B);
    return v->ctx->prec ? vanka::finish_block(v->m, B, dof, con, val, f32.data() + at, v->mpad, v->kpad)
                        : vanka::finish_block(v->m, B, dof, con, val, f64.data() + at, v->mpad, v->kpad);
  }
  int upload(stfem_vanka *to) const { return v->ctx->prec ? vk_upload(&to->d_blocks, f32) : vk_upload(&to->d_blocks, f64); }
};
} // namespace

// per-cell variant: DoF offsets, the cells of every colour and, for the two-phase apply, the scratch array (slot = cell)
static int vanka_per_cell_tables(stfem_vanka *v)
{
  stfem_ctx *c = v->ctx;
  const int ncx = c->nc[0], ncy = c->nc[1], ncz = c->nc[2];
  int rc = vanka_offset_table(v);
  for (int colour = 0; colour < 8 && rc == STFEM_OK; ++colour) {
    std::vector<int> cells;
    for (int cz = colour >> 2; cz < ncz; cz += 2)
      for (int cy = (colour >> 1) & 1; cy < ncy; cy += 2)
        for (int cx = colour & 1; cx < ncx; cx += 2) cells.push_back(cx + ncx * (cy + ncy * cz));
    v->ngrid[colour] = int(cells.size());
    if (!cells.empty()) rc = vk_upload(&v->d_cell[colour], cells);
  }
  if (rc != STFEM_OK || !vanka_wants_flat(c)) return rc;
  v->ngrid[VK_FLAT] = int(c->ncells);
  v->flat = true;
  return vk_alloc(&v->d_flat, size_t(c->ncells) * v->mpad * c->es);
}

// Set-up of the per-cell blocks (general meshes, coefficient tables): cell matrices on the device from the stored
// metric, then on the host the reference's steps one by one (stmg.h:786-829, compute_block_matrix.h:50-139):
// restriction of the assembled matrices to the cell's DoFs (= the cell's own matrix + what the neighbours add on
// shared faces, edges and vertices), zero-boundary rows / columns, valence scaling, Kronecker with Alpha / Beta,
// Gauss-Jordan.  Meant for the mesh sizes the reference can hold too (one (n_blocks nloc)^2 block per cell).
static int vanka_create_per_cell_host(stfem_vanka *v, const double *Alpha, const double *Beta)
{
  stfem_ctx *c = v->ctx;
  const int p = c->p, n = p + 1, nloc = v->nloc;
  vanka_per_cell_shape(v);
  const size_t bsz = size_t(v->kpad) * v->mpad;
  if (double(c->ncells) * double(bsz) * double(c->es) > 64e9) {
    return stfem_set_error(STFEM_ERR_OUT_OF_MEMORY, "per-cell blocks of %lld cells need %.1f GB", (long long)c->ncells,
                           double(c->ncells) * double(bsz) * double(c->es) * 1e-9);
  }
  // ---- cell matrices
  const void *metric = nullptr;
  int rc = stfem_internal_metric(c, &metric, nullptr);
  if (rc != STFEM_OK) return rc;
  const size_t nmat = size_t(c->ncells) * nloc * nloc;
  double *d_tab = nullptr, *d_K = nullptr, *d_M = nullptr;
  std::vector<double> tabs(2 * n * n);
  for (int i = 0; i < n * n; ++i) { tabs[i] = c->tab.S[i]; tabs[n * n + i] = c->tab.D[i]; }
  auto cleanup = [&]() {
    if (d_tab) (void)hipFree(d_tab);
    if (d_K) (void)hipFree(d_K);
    if (d_M) (void)hipFree(d_M);
  };
  if (hipMalloc(&d_tab, tabs.size() * sizeof(double)) != hipSuccess || hipMalloc(&d_K, nmat * sizeof(double)) != hipSuccess ||
      hipMalloc(&d_M, nmat * sizeof(double)) != hipSuccess) {
    cleanup();
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  std::vector<double> Kc(nmat), Mc(nmat);
  {
    hipError_t e = hipMemcpy(d_tab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice);
    const size_t lds = (size_t(nloc) * 7 + 2 * n * n) * sizeof(double);
    int launched = STFEM_OK;
    if (e == hipSuccess) {
      stfem_by_prec(c, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(vanka_cell_matrices_kernel<T>, dim3((unsigned)c->ncells), dim3(256), lds, 0, n, static_cast<const T *>(metric), d_tab,
                           d_tab + n * n, d_K, d_M);
      });
      launched = stfem_launch_end("vanka_cell_matrices_kernel");
    }
    if (e == hipSuccess && launched == STFEM_OK) e = hipMemcpy(Kc.data(), d_K, nmat * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && launched == STFEM_OK) e = hipMemcpy(Mc.data(), d_M, nmat * sizeof(double), hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "cell matrices: %s", hipGetErrorString(e));
    if (launched != STFEM_OK) return launched;
  }
  // ---- blocks
  const int ncx = c->nc[0], ncy = c->nc[1], ncz = c->nc[2];
  std::vector<double> Kr(size_t(nloc) * nloc), Mr(size_t(nloc) * nloc), val(nloc);
  std::vector<char> cn(nloc);
  VankaHostBlocks blocks(v, size_t(c->ncells), Alpha, Beta);
  for (int cz = 0; cz < ncz; ++cz)
    for (int cy = 0; cy < ncy; ++cy)
      for (int cx = 0; cx < ncx; ++cx) {
        const int cc[3] = {cx, cy, cz};
        const size_t cell = cx + size_t(ncx) * (cy + size_t(ncy) * cz);
        for (int a = 0; a < nloc; ++a) {
          const int ia[3] = {a % n, (a / n) % n, a / (n * n)};
          double vv = 1.0;
          bool con = false;
          for (int d = 0; d < 3; ++d) {
            if ((ia[d] == 0 && cc[d] > 0) || (ia[d] == p && cc[d] < c->nc[d] - 1)) vv *= 2.0;
            if ((ia[d] == 0 && cc[d] == 0 && (c->dmask & (1 << (2 * d)))) || (ia[d] == p && cc[d] == c->nc[d] - 1 && (c->dmask & (2 << (2 * d)))))
              con = true;
          }
          val[a] = vv;
          cn[a] = con;
          for (int b = 0; b < nloc; ++b) {
            const int ib[3] = {b % n, (b / n) % n, b / (n * n)};
            // cells holding both DoFs: per direction the cell itself, and the neighbour across a face both lie on
            int lo[3], hi[3];
            for (int d = 0; d < 3; ++d) {
              lo[d] = (ia[d] == 0 && ib[d] == 0 && cc[d] > 0) ? -1 : 0;
              hi[d] = (ia[d] == p && ib[d] == p && cc[d] < c->nc[d] - 1) ? 1 : 0;
            }
            double ks = 0.0, ms = 0.0;
            for (int sz = lo[2]; sz <= hi[2]; ++sz)
              for (int sy = lo[1]; sy <= hi[1]; ++sy)
                for (int sx = lo[0]; sx <= hi[0]; ++sx) {
                  const int sh[3] = {sx, sy, sz};
                  int a2 = 0, b2 = 0, mul = 1;
                  for (int d = 0; d < 3; ++d) {
                    const int ja = sh[d] == -1 ? p : (sh[d] == 1 ? 0 : ia[d]), jb = sh[d] == -1 ? p : (sh[d] == 1 ? 0 : ib[d]);
                    a2 += ja * mul;
                    b2 += jb * mul;
                    mul *= n;
                  }
                  const size_t c2 = (cx + sx) + size_t(ncx) * ((cy + sy) + size_t(ncy) * (cz + sz));
                  ks += Kc[(c2 * nloc + a2) * nloc + b2];
                  ms += Mc[(c2 * nloc + a2) * nloc + b2];
                }
            Kr[size_t(a) * nloc + b] = ks;
            Mr[size_t(a) * nloc + b] = ms;
          }
        }
        // from here on as for the class blocks: constraints, valence, Kronecker with Alpha / Beta, Gauss-Jordan
        if (!blocks.add(cell, Kr, Mr, cn, val)) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "singular cell block (cell %zu)", cell);
      }
  rc = blocks.upload(v);
  if (rc != STFEM_OK) return rc;
  v->nclasses = int(c->ncells);
  return vanka_per_cell_tables(v);
}

// The per-cell blocks built on the device, a few cell layers at a time: cell matrices of the layers and their neighbours
// (vanka_cell_matrices_kernel), assembly of the restricted, weighted, Kronecker-combined block (vanka_assemble_kernel), batched
// Gauss-Jordan (vanka_invert_kernel) straight into the apply's layout.  Nothing but Alpha / Beta crosses the host.
static int vanka_create_per_cell_device(stfem_vanka *v, const double *Alpha, const double *Beta)
{
  stfem_ctx *c = v->ctx;
  const int p = c->p, n = p + 1, nloc = v->nloc, m = v->m, nb = v->nb;
  vanka_per_cell_shape(v);
  const size_t bsz = size_t(v->kpad) * v->mpad;
  const int ncx = c->nc[0], ncy = c->nc[1], ncz = c->nc[2];
  const size_t cpl = size_t(ncx) * ncy;
  const size_t km_layer = 2 * cpl * nloc * nloc * sizeof(double), b_layer = cpl * size_t(m) * m * sizeof(double);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
  const double need = double(c->ncells) * double(bsz) * double(c->es);
  // scratch of one batch of L cell layers: (L + 2) layers of cell matrices + L layers of fp64 blocks; at most 6 GB,
  // and never more than what is left beside the blocks themselves
  const double budget = std::min(6e9, 0.9 * double(free_b) - need);
  if (budget < 3.0 * double(km_layer) + double(b_layer)) {
    return stfem_set_error(STFEM_ERR_OUT_OF_MEMORY, "per-cell blocks of %lld cells need %.1f GB (%.1f GB free)", (long long)c->ncells, need * 1e-9, double(free_b) * 1e-9);
  }
  int L = int((budget - 2.0 * double(km_layer)) / double(km_layer + b_layer));
  L = std::max(1, std::min(L, ncz));
  if (const char *e = getenv("STFEM_VANKA_SETUP_LAYERS")) // at most this many cell layers per batch (tests: the batch loop on small meshes)
    if (atoi(e) > 0) L = std::min(L, atoi(e));
  const void *metric = nullptr;
  int rc = stfem_internal_metric(c, &metric, nullptr);
  if (rc != STFEM_OK) return rc;
  double *d_tab = nullptr, *d_K = nullptr, *d_M = nullptr, *d_B = nullptr;
  int *d_flag = nullptr;
  auto cleanup = [&]() {
    (void)hipFree(d_tab);
    (void)hipFree(d_K);
    (void)hipFree(d_M);
    (void)hipFree(d_B);
    (void)hipFree(d_flag);
  };
  std::vector<double> tabs(2 * n * n);
  for (int i = 0; i < n * n; ++i) { tabs[i] = c->tab.S[i]; tabs[n * n + i] = c->tab.D[i]; }
  const size_t win_cells = cpl * size_t(std::min(ncz, L + 2));
  rc = vk_alloc(&v->d_blocks, size_t(c->ncells) * bsz * c->es);
  if (rc != STFEM_OK) return rc;
  if (hipMalloc(&d_tab, tabs.size() * sizeof(double)) != hipSuccess || hipMalloc(&d_K, win_cells * nloc * nloc * sizeof(double)) != hipSuccess ||
      hipMalloc(&d_M, win_cells * nloc * nloc * sizeof(double)) != hipSuccess || hipMalloc(&d_B, cpl * L * size_t(m) * m * sizeof(double)) != hipSuccess ||
      hipMalloc(&d_flag, sizeof(int)) != hipSuccess) {
    cleanup();
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  hipError_t e = hipMemcpy(d_tab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_flag, 0, sizeof(int));
  VankaAssembleParams ap;
  ap.Kc = d_K; ap.Mc = d_M; ap.B = d_B;
  ap.ncx = ncx; ap.ncy = ncy; ap.ncz = ncz; ap.p = p; ap.nb = nb; ap.dmask = c->dmask;
  for (int i = 0; i < nb * nb; ++i) { ap.Alpha[i] = Alpha[i]; ap.Beta[i] = Beta[i]; }
  const size_t lds = (size_t(nloc) * 7 + 2 * n * n) * sizeof(double);
  v->setup_batches = 0;
  int launched = STFEM_OK;
  for (int z0 = 0; z0 < ncz && e == hipSuccess && launched == STFEM_OK; z0 += L) {
    ++v->setup_batches;
    const int z1 = std::min(ncz, z0 + L), zw0 = std::max(0, z0 - 1), zw1 = std::min(ncz, z1 + 1);
    const size_t wcells = cpl * size_t(zw1 - zw0), bcells = cpl * size_t(z1 - z0);
    const size_t moff = cpl * size_t(zw0) * nloc * 8; // metric records [cell][q][8]
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(vanka_cell_matrices_kernel<T>, dim3((unsigned)wcells), dim3(256), lds, 0, n, static_cast<const T *>(metric) + moff, d_tab,
                         d_tab + n * n, d_K, d_M);
    });
    ap.zw0 = zw0; ap.z0 = z0; ap.ncells_batch = int(bcells);
    hipLaunchKernelGGL(vanka_assemble_kernel, dim3((unsigned)bcells), dim3(256), 0, 0, ap);
    const long long cell0 = (long long)cpl * z0;
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(vanka_invert_kernel<T>, dim3((unsigned)bcells), dim3(256), 0, 0, d_B, static_cast<T *>(v->d_blocks), m, v->mpad, v->kpad, cell0, d_flag);
    });
    launched = stfem_launch_end("per-cell block set-up kernels");
    if (launched == STFEM_OK) e = hipDeviceSynchronize(); // (the next batch reuses the scratch)
  }
  int flag = 0;
  if (e == hipSuccess && launched == STFEM_OK) e = hipMemcpy(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "per-cell block set-up: %s", hipGetErrorString(e));
  if (launched != STFEM_OK) return launched;
  if (flag) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "singular cell block");
  v->nclasses = int(c->ncells);
  return vanka_per_cell_tables(v);
}

static int vanka_create_per_cell(stfem_vanka *v, const double *Alpha, const double *Beta)
{
  const char *e = getenv("STFEM_VANKA_HOST_SETUP"); // the same steps on the host, block by block (for comparison; small meshes only)
  return (e && atoi(e) != 0) ? vanka_create_per_cell_host(v, Alpha, Beta) : vanka_create_per_cell_device(v, Alpha, Beta);
}

// Class variant: the block of every class from Kronecker products of restricted 1D matrices, inverted on the host in double
static int build_class_blocks(stfem_vanka *v, const vanka::ClassTable &t, const double *Alpha, const double *Beta)
{
  const stfem_ctx *c = v->ctx;
  const int p = c->p, n = p + 1, nloc = v->nloc;
  const vanka::TilePlan plan = vanka::scalar_tile_plan((v->m + 15) / 16, c->prec != 0);
  if (plan.mtw == 0 || !vanka_kernel(c, plan.mtw)) return STFEM_ERR_UNSUPPORTED;
  v->mtw = plan.mtw; v->parts = plan.parts; v->mt = plan.parts * plan.mtw;
  v->mpad = 16 * v->mt;
  v->kpad = ((v->m + KS - 1) / KS) * KS;
  v->nclasses = int(t.key.size());
  // 1D nodal matrices of the reference cell: Mhat = S^T W S, Khat = D^T W D
  const stfem::ShapeTables &tab = c->tab;
  std::vector<double> Mh(n * n, 0.0), Kh(n * n, 0.0);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      for (int q = 0; q < n; ++q) {
        Mh[a * n + b] += tab.wq[q] * tab.S[q * n + a] * tab.S[q * n + b];
        Kh[a * n + b] += tab.wq[q] * tab.D[q * n + a] * tab.D[q * n + b];
      }
  VankaHostBlocks blocks(v, t.key.size(), Alpha, Beta);
  std::vector<double> Kr(size_t(nloc) * nloc), Mr(size_t(nloc) * nloc), val(nloc);
  std::vector<char> cn(nloc);
  for (int ci = 0; ci < v->nclasses; ++ci) {
    const int key = t.key[ci];
    // restricted assembled 1D matrices: the end nodes also carry the neighbour's diagonal entry
    std::vector<double> M1[3], K1[3];
    bool con[3][8], shared[3][8];
    for (int d = 0; d < 3; ++d) {
      const int k = (key >> (2 * d)) & 3;
      const double h = c->h[d];
      M1[d].assign(n * n, 0.0);
      K1[d].assign(n * n, 0.0);
      for (int e = 0; e < n * n; ++e) {
        M1[d][e] = h * Mh[e];
        K1[d][e] = Kh[e] / h;
      }
      if (k & 1) { M1[d][0] += h * Mh[p * n + p]; K1[d][0] += Kh[p * n + p] / h; }
      if (k & 2) { M1[d][p * n + p] += h * Mh[0]; K1[d][p * n + p] += Kh[0] / h; }
      for (int a = 0; a < n; ++a) {
        shared[d][a] = (a == 0 && (k & 1)) || (a == p && (k & 2));
        con[d][a] = (a == 0 && !(k & 1) && (c->dmask & (1 << (2 * d)))) || (a == p && !(k & 2) && (c->dmask & (2 << (2 * d))));
      }
    }
    for (int kz = 0; kz < n; ++kz)
      for (int jy = 0; jy < n; ++jy)
        for (int ix = 0; ix < n; ++ix) {
          const int r = ix + n * (jy + n * kz);
          val[r] = (shared[0][ix] ? 2.0 : 1.0) * (shared[1][jy] ? 2.0 : 1.0) * (shared[2][kz] ? 2.0 : 1.0);
          cn[r] = con[0][ix] || con[1][jy] || con[2][kz];
          for (int kz2 = 0; kz2 < n; ++kz2)
            for (int jy2 = 0; jy2 < n; ++jy2)
              for (int ix2 = 0; ix2 < n; ++ix2) {
                const int s = ix2 + n * (jy2 + n * kz2);
                const double mx = M1[0][ix * n + ix2], my = M1[1][jy * n + jy2], mz = M1[2][kz * n + kz2];
                const double kx = K1[0][ix * n + ix2], ky = K1[1][jy * n + jy2], kz1 = K1[2][kz * n + kz2];
                Mr[size_t(r) * nloc + s] = mz * my * mx;
                Kr[size_t(r) * nloc + s] = mz * my * kx + mz * ky * mx + kz1 * my * mx;
              }
        }
    if (!blocks.add(ci, Kr, Mr, cn, val)) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "singular cell block (class %d)", key);
  }
  return blocks.upload(v);
}

// Class variant: DoF offsets and the cell lists of the eight colour launches and, on small meshes, of the two-phase apply
static int build_cell_lists(stfem_vanka *v, const vanka::ClassTable &t)
{
  const stfem_ctx *c = v->ctx;
  const int p = c->p;
  std::vector<int> first(size_t(c->ncells)); // first DoF of every cell
  for (int cz = 0; cz < c->nc[2]; ++cz)
    for (int cy = 0; cy < c->nc[1]; ++cy)
      for (int cx = 0; cx < c->nc[0]; ++cx) first[cx + c->nc[0] * (cy + c->nc[1] * cz)] = p * cx + c->nd[0] * (p * cy + c->nd[1] * p * cz);
  int rc = vanka_offset_table(v);
  v->flat = vanka_wants_flat(c);
  for (int l = 0; l <= (v->flat ? VK_FLAT : 7) && rc == STFEM_OK; ++l) {
    const vanka::CellList list = vanka::cell_list(t, l == VK_FLAT ? -1 : l);
    v->ngrid[l] = int(list.cls.size());
    if (list.cls.empty()) continue;
    rc = vk_upload(&v->d_cell[l], vanka::gather_cells(list.order, first, -1));
    if (rc == STFEM_OK) rc = vk_upload(&v->d_cls[l], list.cls);
    if (l != VK_FLAT) continue; // cell -> slot for the second phase, and the rows between the two
    if (rc == STFEM_OK) rc = vk_upload(&v->d_slot, list.slot);
    if (rc == STFEM_OK) rc = vk_alloc(&v->d_flat, list.order.size() * v->mpad * c->es);
  }
  return rc;
}

extern "C" {

int stfem_vanka_create(stfem_ctx *c, int nb, const double *Alpha, const double *Beta, stfem_vanka **out)
{
  return stfem_vanka_create_partitioned(c, nb, Alpha, Beta, 0, out);
}

int stfem_vanka_create_partitioned(stfem_ctx *c, int nb, const double *Alpha, const double *Beta, int neighbour_mask, stfem_vanka **out)
{
  if (!c || !Alpha || !Beta || !out || nb < 1 || nb > VK_MAX_BLOCKS || (neighbour_mask & ~63) || (neighbour_mask & c->dmask))
    return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const int n = c->p + 1;
  if (nb * n * n * n > VK_MAX_ROWS) return STFEM_ERR_UNSUPPORTED; // Q4 with more than 4 temporal blocks, Q5 with more than 2
  STFEM_TRY(hipSetDevice(c->device));
  VankaPtr v = vanka_new(c, nb);
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  int rc;
  // one block per neighbour pattern needs identical cells: axis-aligned uniform mesh, no coefficient tables;
  // everything else gets one block per cell
  if (!c->cartesian || c->coef_layout[0] != 0 || c->coef_layout[1] != 0) {
    if (neighbour_mask) return STFEM_ERR_UNSUPPORTED; // (the blocks of the interface cells need the cell matrices of the neighbour rank's cells)
    rc = vanka_create_per_cell(v.get(), Alpha, Beta);
  } else {
    const vanka::ClassTable t = vanka::class_table(c->nc, neighbour_mask);
    rc = build_class_blocks(v.get(), t, Alpha, Beta);
    if (rc == STFEM_OK) rc = build_cell_lists(v.get(), t);
  }
  if (rc == STFEM_OK) *out = v.release();
  return rc;
}

// One block per cell on a z-slab of a partitioned GENERAL mesh (perturbed cells, coefficient tables: BASELINE configs[2] on more
// than one rank).  The block of a cell next to the interface needs the cell matrices of the neighbour rank's cells
// (stmg.h:688-689, 795-796 and compute_block_matrix.h:68-73: the reference builds the blocks on locally owned AND ghost cells):
// the caller hands over a second context, `extended`, of the same slab plus one ghost cell layer on every side that has a
// neighbour (the vertices of those layers are all that crosses the ranks, once).  The blocks are built on it as on any mesh and
// the ones of the slab's own cells are kept; the apply runs on the slab and leaves PARTIAL sums in the interface planes like
// the uniform-mesh variant (stfem_vanka_create_partitioned).
int stfem_vanka_create_partitioned_general(stfem_ctx *slab, stfem_ctx *extended, int nb, const double *Alpha, const double *Beta,
                                           int neighbour_mask, stfem_vanka **out)
{
  if (!slab || !extended || !Alpha || !Beta || !out || nb < 1) return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (neighbour_mask & ~(16 | 32)) return STFEM_ERR_UNSUPPORTED; // z-slabs
  const int glo = (neighbour_mask & 16) ? 1 : 0, ghi = (neighbour_mask & 32) ? 1 : 0;
  if (extended->p != slab->p || extended->prec != slab->prec || extended->device != slab->device || extended->nc[0] != slab->nc[0] ||
      extended->nc[1] != slab->nc[1] || extended->nc[2] != slab->nc[2] + glo + ghi)
    return STFEM_ERR_SHAPE_MISMATCH;
  // the extended context carries the domain's constraints: none on a z face with a ghost layer, the slab's elsewhere
  if ((extended->dmask & 15) != (slab->dmask & 15) || (glo && (extended->dmask & 16)) || (ghi && (extended->dmask & 32)) ||
      (!glo && (extended->dmask & 16) != (slab->dmask & 16)) || (!ghi && (extended->dmask & 32) != (slab->dmask & 32)))
    return STFEM_ERR_INVALID_ARGUMENT;
  stfem_vanka *built = nullptr;
  int rc = stfem_vanka_create_partitioned(extended, nb, Alpha, Beta, 0, &built);
  if (rc != STFEM_OK) return rc;
  VankaPtr ve(built, stfem_vanka_destroy);
  if (!ve->per_cell) // an axis-aligned uniform mesh: the class variant handles the partition by itself
    return stfem_vanka_create_partitioned(slab, nb, Alpha, Beta, neighbour_mask, out);
  VankaPtr v = vanka_new(slab, nb);
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->mt = ve->mt; v->mtw = ve->mtw; v->parts = ve->parts; v->mpad = ve->mpad; v->kpad = ve->kpad;
  v->per_cell = true;
  v->nclasses = int(slab->ncells);
  // take the allocation over; the slab's cells start behind the lower ghost layer
  v->d_blocks_base = ve->d_blocks;
  ve->d_blocks = nullptr;
  const size_t bsz = size_t(v->kpad) * v->mpad;
  v->d_blocks = static_cast<char *>(v->d_blocks_base) + size_t(glo) * size_t(slab->nc[0]) * slab->nc[1] * bsz * slab->es;
  ve.reset();
  STFEM_TRY(hipSetDevice(slab->device));
  rc = vanka_per_cell_tables(v.get());
  if (rc == STFEM_OK) *out = v.release();
  return rc;
}

void stfem_vanka_destroy(stfem_vanka *v)
{
  if (!v) return;
  (void)hipSetDevice(v->ctx->device);
  (void)hipFree(v->d_blocks_base ? v->d_blocks_base : v->d_blocks);
  (void)hipFree(v->d_off);
  (void)hipFree(v->d_flat);
  (void)hipFree(v->d_slot);
  for (int l = 0; l <= VK_FLAT; ++l) {
    (void)hipFree(v->d_cell[l]);
    (void)hipFree(v->d_cls[l]);
  }
  delete v;
}

int stfem_vanka_n_classes(const stfem_vanka *v) { return v ? v->nclasses : 0; }
int stfem_vanka_plan(const stfem_vanka *v, int32_t out[2])
{
  if (!v || !out) return STFEM_ERR_INVALID_ARGUMENT;
  out[0] = v->mtw; out[1] = v->parts;
  return STFEM_OK;
}

int stfem_vanka_setup_batches(const stfem_vanka *v) { return v ? v->setup_batches : 0; }

int stfem_vanka_vmult(stfem_vanka *v, stfem_vec *dst, const stfem_vec *src, void *stream) { return stfem_vanka_step(v, dst, 1.0, 0, src, stream); }

// dst = (accumulate ? dst : 0) + omega * V src: the relaxation step x <- x + omega P^-1 r of the multigrid smoothers
// (PreconditionRelaxation around the Vanka smoother, stmg.h:1199-1238) without a temporary vector and a separate update pass
int stfem_vanka_step(stfem_vanka *v, stfem_vec *dst, double omega, int accumulate, const stfem_vec *src, void *stream)
{
  if (!v || !dst || !src) return STFEM_ERR_INVALID_ARGUMENT;
  TraceScope scope("vanka"); // the reference's TimerOutput scope "vanka" (stmg.h:835)
  if (dst->ctx != v->ctx || src->ctx != v->ctx || dst->nb != v->nb || src->nb != v->nb) return STFEM_ERR_SHAPE_MISMATCH;
  for (int i = 0; i < v->nb; ++i)
    for (int j = 0; j < v->nb; ++j)
      if (dst->blk[i] == src->blk[j]) return STFEM_ERR_ALIAS;
  stfem_ctx *c = v->ctx;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the parameters of both kernels; a launch changes the cell list and the colour only
  VankaParams prm;
  VankaCellParams cp;
  std::memset(&prm, 0, sizeof(prm));
  std::memset(&cp, 0, sizeof(cp));
  for (int i = 0; i < v->nb; ++i) {
    prm.src[i] = cp.src[i] = src->blk[i];
    prm.dst[i] = cp.dst[i] = dst->blk[i];
  }
  prm.blocks = cp.blocks = v->d_blocks;
  prm.off = cp.off = v->d_off;
  prm.m = cp.m = v->m; prm.mpad = cp.mpad = v->mpad; prm.kpad = cp.kpad = v->kpad; prm.p = cp.p = c->p;
  cp.nloc = v->nloc; cp.ncx = c->nc[0]; cp.ncy = c->nc[1]; cp.ncz = c->nc[2]; cp.nx = c->nd[0]; cp.ny = c->nd[1];
  prm.flat = cp.flat = v->flat ? v->d_flat : nullptr;
  prm.omega = cp.omega = omega; prm.accumulate = cp.accumulate = accumulate;
  const void *kernel = v->per_cell ? VK_TYPED(c, vanka_apply_percell_kernel) : vanka_kernel(c, v->mtw);
  if (!kernel) return STFEM_ERR_UNSUPPORTED;
  stfem_launch_begin();
  // dst = 0 (stmg.h:836) is not a pass of its own: the first cell to touch a DoF stores (every DoF has one)
  for (int l = v->flat ? VK_FLAT : 0; l <= (v->flat ? VK_FLAT : 7); ++l) {
    if (v->ngrid[l] == 0) continue;
    prm.cell = cp.cell = v->d_cell[l];
    prm.cls = v->d_cls[l];
    prm.nquad = v->ngrid[l];
    prm.colour = cp.colour = l & 7;
    const int rc = v->per_cell ? vk_launch(kernel, dim3(v->ngrid[l]), &cp, st, "vanka_apply_percell_kernel")
                               : vk_launch(kernel, dim3(v->ngrid[l], v->parts), &prm, st, "vanka_apply_kernel");
    if (rc != STFEM_OK) return rc;
  }
  return v->flat ? vanka_collect(v, dst, omega, accumulate, st) : STFEM_OK;
}

} // extern "C"
