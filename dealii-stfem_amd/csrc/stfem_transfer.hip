// Space transfers of the space-time multigrid: what the reference gets from deal.II's
// MGTwoLevelTransfer<dim, VectorT<Number>> (reinit / prolongate_and_add / restrict_and_add / interpolate as used by
// MGTwoLevelBlockTransfer, include/stmg.h:38-110, built in build_stmg_transfers, stmg.h:580-600) for the
// structured meshes of this library: h-transfer (twice the cells per direction, same degree) and p-transfer (same
// cells, lower degree), with the zero-boundary constraints of both levels.
//
// MI355X design: on a structured block with lexicographic numbering the embedding of the coarse space is the
// Kronecker product Pz (x) Py (x) Px of banded 1D matrices (the transfer is defined on the reference cell, so this
// holds for MappingQ1-perturbed meshes too; a DoF is constrained iff one of its three line indices is, so the
// constraints factorise as well).  A transfer is therefore three passes of one kernel, a banded 1D mat-vec along
// one axis of the array with the x index on the lanes: every load and store is a coalesced full line, there is no
// scatter, no atomics and no colouring, and the result is reproducible.  HBM traffic of an h-prolongation:
// 29 coarse-vector sizes against the 17 a single fused pass would need (read coarse, read + write fine).
// Which kernel each pass of each operation takes is decided once, when the transfer is created (TransferPlan).
// (The 1D factors themselves: host_tables.cpp; the precision change between the solver's vectors and the multigrid's:
// stfem_vector.hip; the level schedule: stfem_host_helpers.cpp.)
#include "stfem_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

namespace {

// one banded 1D matrix in row-compressed form: row o = sum_k w[off[o] + k] * in[first[o] + k], k < off[o+1] - off[o]
struct Band {
  int n_out = 0, n_in = 0;
  std::vector<int> first, off;
  std::vector<double> w;
  int *d_first = nullptr, *d_off = nullptr;
  double *d_w = nullptr;
};

// dense n_out x n_in -> Band (the nonzeros of a row are contiguous up to exact zeros in between)
Band make_band(int n_out, int n_in, const std::vector<double> &A)
{
  Band b;
  b.n_out = n_out;
  b.n_in = n_in;
  b.off.push_back(0);
  for (int o = 0; o < n_out; ++o) {
    int lo = n_in, hi = -1;
    for (int i = 0; i < n_in; ++i)
      if (A[size_t(o) * n_in + i] != 0.0) {
        lo = std::min(lo, i);
        hi = std::max(hi, i);
      }
    b.first.push_back(hi < 0 ? 0 : lo);
    for (int i = lo; i <= hi; ++i) b.w.push_back(A[size_t(o) * n_in + i]);
    b.off.push_back(int(b.w.size()));
  }
  if (b.w.empty()) b.w.push_back(0.0);
  return b;
}

// The table-driven pass: serves the x axis, `interpolate`, the z restriction of a slab with a ghost plane on top, shapes
// without a cell instantiation (FE_Q(5)) and axes that are a copy.
template <typename T>
__global__ void __launch_bounds__(256)
axis_apply_kernel(T *__restrict__ out, const T *__restrict__ in, int d0, int d1, int d2, int axis, int n_in, const int *__restrict__ first,
                  const int *__restrict__ off, const double *__restrict__ w, int add)
{
  const long long total = (long long)d0 * d1 * d2;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int i0 = int(t % d0), i1 = int((t / d0) % d1), i2 = int(t / ((long long)d0 * d1));
    const int o = axis == 0 ? i0 : axis == 1 ? i1 : i2;
    const int k0 = off[o], k1 = off[o + 1], f = first[o];
    long long base, stride;
    if (axis == 0) {
      base = f + (long long)n_in * (i1 + (long long)d1 * i2);
      stride = 1;
    } else if (axis == 1) {
      base = i0 + (long long)d0 * (f + (long long)n_in * i2);
      stride = d0;
    } else {
      base = i0 + (long long)d0 * (i1 + (long long)d1 * f);
      stride = (long long)d0 * d1;
    }
    T acc = add ? out[t] : T(0);
    for (int k = k0; k < k1; ++k) acc += T(w[k]) * in[base + (k - k0) * stride];
    out[t] = acc;
  }
}


// Cell form of the 1D passes along y and z (the bulk of the traffic): a thread takes one COARSE cell of a line - the local
// embedding matrix L [(R + 1) x (PC + 1)] is the same for every cell, so the weights are kernel arguments (scalar registers),
// the PC + 1 coarse values are loaded once for the R (+ 1) fine values they produce, and no index table is read.
// Addressing: element (inner, i, outer) of an array with n entries along the axis at inner + S (i + n outer), inner < S contiguous.
template <typename T> struct CellMat {
  T L[9 * 5]; // L[j * (PC + 1) + a]
};
constexpr int CF_LO_C = 1, CF_HI_C = 2, CF_LO_F = 4, CF_HI_F = 8; // constrained ends of the coarse / fine line

// the end of the cell kernels: an adding pass leaves a constrained row alone, an overwriting pass gives it an exact zero
template <typename T> __device__ __forceinline__ void store_row(T *q, T v, bool constrained, int add)
{
  if (add) {
    if (!constrained) *q += v;
  } else *q = constrained ? T(0) : v;
}

template <typename T, int PC, int R>
__global__ void __launch_bounds__(256)
cell_prolongate_kernel(T *__restrict__ out, const T *__restrict__ in, long long S, int ncell, long long total, const CellMat<T> m, int flags, int add)
{
  const long long n_c = (long long)PC * ncell + 1, n_f = (long long)R * ncell + 1;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long inner = t % S, rest = t / S;
    const int c = int(rest % ncell);
    const long long outer = rest / ncell;
    const bool first = c == 0, last = c == ncell - 1;
    T u[PC + 1];
#pragma unroll
    for (int a = 0; a <= PC; ++a) u[a] = in[inner + S * (c * (long long)PC + a + n_c * outer)];
    if (first && (flags & CF_LO_C)) u[0] = T(0);
    if (last && (flags & CF_HI_C)) u[PC] = T(0);
    T *o = out + inner + S * (c * (long long)R + n_f * outer);
#pragma unroll
    for (int j = 0; j <= R; ++j) {
      if (j == R && !last) break; // the upper end belongs to the next cell
      T v = T(0);
#pragma unroll
      for (int a = 0; a <= PC; ++a) v += m.L[j * (PC + 1) + a] * u[a];
      const bool constrained = (first && j == 0 && (flags & CF_LO_F)) || (last && j == R && (flags & CF_HI_F));
      // (store_row written out: with the address formed ahead of the branch the compiler packs other fp32 products of the rows
      // above into v_pk_mul_f32 + v_add_f32 instead of fused multiply-adds, and the float results move by an ulp)
      if (add) {
        if (!constrained) o[S * j] += v;
      } else o[S * j] = constrained ? T(0) : v;
    }
  }
}

// The passes along y and z of the prolongation in ONE kernel (same embedding matrix along both axes): a thread takes one coarse cell of
// the (y, z) plane at its x index, loads its (PC + 1)^2 coarse values once and writes the R^2 (+ the upper ends at the mesh boundary)
// fine values they produce - the (fine x, fine y, coarse z) intermediate of the three-pass form (4 coarse-vector sizes written and
// read again for an h-transfer) never exists: 21 instead of 29 coarse-vector sizes of traffic.
// in: [nx][PC ncy + 1][PC ncz + 1], out: [nx][R ncy + 1][R ncz + 1], x contiguous.
template <typename T, int PC, int R>
__global__ void __launch_bounds__(256)
cell_prolongate_yz_kernel(T *__restrict__ out, const T *__restrict__ in, int nx, int ncy, int ncz, long long total, const CellMat<T> m, int flags_y,
                          int flags_z, int add)
{
  const long long n_cy = (long long)PC * ncy + 1, n_fy = (long long)R * ncy + 1;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = int(t % nx);
    const long long rest = t / nx;
    const int cy = int(rest % ncy), cz = int(rest / ncy);
    const bool first_y = cy == 0, last_y = cy == ncy - 1, first_z = cz == 0, last_z = cz == ncz - 1;
    T u[PC + 1][PC + 1]; // [az][ay]
#pragma unroll
    for (int az = 0; az <= PC; ++az)
#pragma unroll
      for (int ay = 0; ay <= PC; ++ay) u[az][ay] = in[x + (long long)nx * ((cy * (long long)PC + ay) + n_cy * (cz * (long long)PC + az))];
    if (first_y && (flags_y & CF_LO_C)) {
#pragma unroll
      for (int az = 0; az <= PC; ++az) u[az][0] = T(0);
    }
    if (last_y && (flags_y & CF_HI_C)) {
#pragma unroll
      for (int az = 0; az <= PC; ++az) u[az][PC] = T(0);
    }
    if (first_z && (flags_z & CF_LO_C)) {
#pragma unroll
      for (int ay = 0; ay <= PC; ++ay) u[0][ay] = T(0);
    }
    if (last_z && (flags_z & CF_HI_C)) {
#pragma unroll
      for (int ay = 0; ay <= PC; ++ay) u[PC][ay] = T(0);
    }
    T *o = out + x + (long long)nx * (cy * (long long)R + n_fy * (cz * (long long)R));
#pragma unroll
    for (int jz = 0; jz <= R; ++jz) {
      if (jz == R && !last_z) break; // the upper ends belong to the next cells
      T tz[PC + 1];
#pragma unroll
      for (int ay = 0; ay <= PC; ++ay) {
        T v = T(0);
#pragma unroll
        for (int az = 0; az <= PC; ++az) v += m.L[jz * (PC + 1) + az] * u[az][ay];
        tz[ay] = v;
      }
      const bool con_z = (first_z && jz == 0 && (flags_z & CF_LO_F)) || (last_z && jz == R && (flags_z & CF_HI_F));
#pragma unroll
      for (int jy = 0; jy <= R; ++jy) {
        if (jy == R && !last_y) break;
        T v = T(0);
#pragma unroll
        for (int ay = 0; ay <= PC; ++ay) v += m.L[jy * (PC + 1) + ay] * tz[ay];
        const bool constrained = con_z || (first_y && jy == 0 && (flags_y & CF_LO_F)) || (last_y && jy == R && (flags_y & CF_HI_F));
        store_row(o + (long long)nx * (jy + n_fy * jz), v, constrained, add);
      }
    }
  }
}

// The transpose: coarse node a of cell c collects the fine values of its own cell and, for a = 0, of the interior of the cell before.
// A march: a thread walks along the axis through the coarse cells [c0, c1) of its segment and keeps the interior fine values of the
// cell before in registers, so every fine value is loaded once (with one thread per coarse cell the previous cell's rows come from
// HBM again: the planes of one coarse cell exceed the L2 along z, 2 x the reads).
template <typename T, int PC, int R>
__global__ void __launch_bounds__(256)
cell_restrict_march_kernel(T *__restrict__ out, const T *__restrict__ in, long long S, int ncell, int nseg, long long total, const CellMat<T> m, int flags,
                           int add)
{
  const long long n_c = (long long)PC * ncell + 1, n_f = (long long)R * ncell + 1;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long inner = t % S, rest = t / S;
    const int seg = int(rest % nseg);
    const long long outer = rest / nseg;
    const int c0 = int((long long)ncell * seg / nseg), c1 = int((long long)ncell * (seg + 1) / nseg);
    const T *f = in + inner + S * (n_f * outer);
    T *o = out + inner + S * (n_c * outer);
    T w[R > 1 ? R - 1 : 1], u0;
#pragma unroll
    for (int j = 1; j < R; ++j) w[j - 1] = c0 > 0 ? f[S * ((long long)(c0 - 1) * R + j)] : T(0);
    u0 = f[S * ((long long)c0 * R)];
    if (c0 == 0 && (flags & CF_LO_F)) u0 = T(0);
    for (int c = c0; c < c1; ++c) {
      const bool first = c == 0, last = c == ncell - 1;
      T u[R + 1];
      u[0] = u0;
#pragma unroll
      for (int j = 1; j <= R; ++j) u[j] = f[S * ((long long)c * R + j)];
      if (last && (flags & CF_HI_F)) u[R] = T(0);
#pragma unroll
      for (int a = 0; a <= PC; ++a) {
        if (a == PC && !last) break;
        T v = T(0);
#pragma unroll
        for (int j = (a == PC ? 1 : 0); j <= (a == 0 ? R - 1 : R); ++j) v += m.L[j * (PC + 1) + a] * u[j];
        if (a == 0) {
#pragma unroll
          for (int j = 1; j < R; ++j) v += m.L[j * (PC + 1) + PC] * w[j - 1];
        }
        const bool constrained = (first && a == 0 && (flags & CF_LO_C)) || (last && a == PC && (flags & CF_HI_C));
        store_row(o + S * ((long long)c * PC + a), v, constrained, add);
      }
#pragma unroll
      for (int j = 1; j < R; ++j) w[j - 1] = u[j];
      u0 = u[R];
    }
  }
}

// the (coarse degree, fine nodes per coarse cell) shapes the cell kernels are instantiated for: along one axis, and along y and z at once
#define STFEM_CELL_SHAPES(X) X(1, 2) X(1, 3) X(1, 4) X(1, 6) X(1, 8) X(2, 3) X(2, 4) X(2, 6) X(2, 8) X(3, 4) X(3, 6) X(3, 8) X(4, 8)
#define STFEM_CELL_YZ_SHAPES(X)                                                                                       \
  X(1, 2) X(2, 4) X(3, 6) X(4, 8) /* h-transfers */ X(1, 3) X(1, 4) X(2, 3) X(3, 4) /* (p-transfers on the same cells) */
#define STFEM_IS_SHAPE(PC_, R_) || (pc == PC_ && R == R_)
constexpr bool has_cell(int pc, int R) { return false STFEM_CELL_SHAPES(STFEM_IS_SHAPE); }
constexpr bool has_cell_yz(int pc, int R) { return false STFEM_CELL_YZ_SHAPES(STFEM_IS_SHAPE); }
#undef STFEM_IS_SHAPE

// the restriction marches with at most this many segments per line
constexpr int MARCH_MAX_SEGMENTS = 64;

// What one operation runs, fixed when the transfer is created.  The x pass is always table-driven.
struct TransferPlan {
  bool fuse_yz = false; // prolongation only: x pass, then y and z in one kernel (two launches instead of three)
  bool cell[3] = {};    // the pass along this axis takes the cell kernel (else axis_apply_kernel)
  int nseg[3] = {};     // restriction in cell form: segments per line of the march
};

} // namespace

struct stfem_transfer {
  stfem_ctx *fine = nullptr, *coarse = nullptr;
  Band P[3], R[3], I[3]; // per direction: prolongation rows, its transpose, nodal interpolation (all with the constraints)
  // cell form of P / R along y and z: local embedding matrix, coarse degree, fine nodes per coarse cell, coarse cells, constrained ends
  // (up to FE_Q(5) on both levels with two fine cells per coarse one: 11 x 6 entries; the cell kernels are instantiated up to
  // FE_Q(4): 9 x 5, larger blocks take the table-driven passes)
  double L[3][11 * 6] = {};
  int pc[3] = {0, 0, 0}, Rn[3] = {0, 0, 0}, ncc[3] = {0, 0, 0}, flags[3] = {0, 0, 0};
  TransferPlan plan_p, plan_r, plan_i; // prolongation, restriction, interpolation (tables along every axis)
  void *d_tmp[2] = {nullptr, nullptr};
  size_t tmp_elems = 0;
  // diagnostics (stfem_transfer_last_path): fused y-z kernel in the last prolongation; most coarse cells one thread marched through in
  // the last restriction along y and z (0: table-driven pass)
  int last_path[3] = {0, 0, 0};
};

namespace {

int upload(Band &b)
{
  STFEM_TRY(hipMalloc(&b.d_first, b.first.size() * sizeof(int)));
  STFEM_TRY(hipMalloc(&b.d_off, b.off.size() * sizeof(int)));
  STFEM_TRY(hipMalloc(&b.d_w, b.w.size() * sizeof(double)));
  STFEM_TRY(hipMemcpy(b.d_first, b.first.data(), b.first.size() * sizeof(int), hipMemcpyHostToDevice));
  STFEM_TRY(hipMemcpy(b.d_off, b.off.data(), b.off.size() * sizeof(int), hipMemcpyHostToDevice));
  STFEM_TRY(hipMemcpy(b.d_w, b.w.data(), b.w.size() * sizeof(double), hipMemcpyHostToDevice));
  return STFEM_OK;
}
void release(Band &b)
{
  (void)hipFree(b.d_first);
  (void)hipFree(b.d_off);
  (void)hipFree(b.d_w);
}

// The passes of the three operations, from what is fixed at creation.  ghost_top: the top fine plane of a slab is restricted by the
// neighbour above, and the cell form of the restriction has no such mask: table-driven pass along z.
void make_plan(stfem_transfer *t, bool ghost_top)
{
  const stfem_ctx *fine = t->fine, *coarse = t->coarse;
  for (int ax = 1; ax < 3; ++ax) { // (an axis with the same cells and degree on both levels is a copy: table-driven)
    const bool cell = t->Rn[ax] > t->pc[ax] && has_cell(t->pc[ax], t->Rn[ax]);
    t->plan_p.cell[ax] = cell;
    t->plan_r.cell[ax] = cell && !(ax == 2 && ghost_top);
  }
  // the y and z passes of the prolongation can run as one kernel: same coarse degree, refinement and embedding matrix along both
  // (measured on the cfg-1 levels, two Q4 blocks: fp32 h 0.231 -> 0.153 ms, fp32 / fp64 p 0.208 -> 0.172 / 0.315 -> 0.253 ms; fp64 h with 81 weights in
  // scalar registers 0.332 -> 0.340 ms, and below ~150 000 threads the one-cell-per-thread form has too few of them: both keep the three passes)
  const long long yz_threads = (long long)fine->nd[0] * t->ncc[1] * t->ncc[2];
  const bool heavy = fine->prec == 0 && t->pc[1] == 4 && t->Rn[1] == 8;
  t->plan_p.fuse_yz = t->pc[1] == t->pc[2] && t->Rn[1] == t->Rn[2] && t->Rn[1] > t->pc[1] && yz_threads >= 150000 && !heavy &&
                      std::equal(t->L[1], t->L[1] + 11 * 6, t->L[2]) && has_cell_yz(t->pc[1], t->Rn[1]);
  // the restriction runs z, y, x: lines of the z pass (fine x, fine y), of the y pass (fine x, coarse z).  Enough threads to fill the
  // chip: lines x segments >= ~2^18
  const long long lines[3] = {0, (long long)fine->nd[0] * coarse->nd[2], (long long)fine->nd[0] * fine->nd[1]};
  for (int ax = 1; ax < 3; ++ax)
    if (t->plan_r.cell[ax]) {
      const int nseg = int(std::min<long long>(t->ncc[ax], std::max<long long>(1, (262144 + lines[ax] - 1) / lines[ax])));
      t->plan_r.nseg[ax] = std::min(nseg, MARCH_MAX_SEGMENTS);
    }
}

template <typename T>
int launch_axis(T *out, const T *in, const int dims[3], int axis, const Band &b, int add, hipStream_t s)
{
  const long long total = (long long)dims[0] * dims[1] * dims[2];
  const int blocks = int(std::min<long long>((total + 255) / 256, 1 << 20));
  axis_apply_kernel<T><<<blocks, 256, 0, s>>>(out, in, dims[0], dims[1], dims[2], axis, b.n_in, b.d_first, b.d_off, b.d_w, add);
  return stfem_launch_end("axis_apply_kernel");
}

template <typename T> CellMat<T> cell_mat(const double *L)
{
  CellMat<T> m;
  for (int i = 0; i < 9 * 5; ++i) m.L[i] = T(L[i]);
  return m;
}

// one pass in cell form over `lines` lines of ncell coarse cells: the prolongation (nseg = 0, a thread per coarse cell) or the
// restriction as a march with nseg segments per line
template <typename T>
int launch_cell(int pc, int R, int nseg, T *out, const T *in, long long S, int ncell, long long lines, const double *L, int flags, int add, hipStream_t s)
{
  const CellMat<T> m = cell_mat<T>(L);
  const long long total = lines * (nseg ? nseg : ncell);
  const int blocks = int(std::min<long long>((total + 255) / 256, 1 << 20));
#define STFEM_CELL_CASE(PC_, R_)                                                                                              \
  if (pc == PC_ && R == R_) {                                                                                                 \
    if (nseg) cell_restrict_march_kernel<T, PC_, R_><<<blocks, 256, 0, s>>>(out, in, S, ncell, nseg, total, m, flags, add);   \
    else cell_prolongate_kernel<T, PC_, R_><<<blocks, 256, 0, s>>>(out, in, S, ncell, total, m, flags, add);                  \
    return stfem_launch_end(nseg ? "cell_restrict_march_kernel" : "cell_prolongate_kernel");                                  \
  }
  STFEM_CELL_SHAPES(STFEM_CELL_CASE)
#undef STFEM_CELL_CASE
  return STFEM_ERR_UNSUPPORTED; // (not reached: make_plan asks has_cell)
}

template <typename T>
int launch_cell_yz(int pc, int R, T *out, const T *in, int nx, int ncy, int ncz, const double *L, int flags_y, int flags_z, int add, hipStream_t s)
{
  const CellMat<T> m = cell_mat<T>(L);
  const long long total = (long long)nx * ncy * ncz;
  const int blocks = int(std::min<long long>((total + 255) / 256, 1 << 20));
#define STFEM_CELL_CASE(PC_, R_)                                                                                              \
  if (pc == PC_ && R == R_) {                                                                                                 \
    cell_prolongate_yz_kernel<T, PC_, R_><<<blocks, 256, 0, s>>>(out, in, nx, ncy, ncz, total, m, flags_y, flags_z, add);     \
    return stfem_launch_end("cell_prolongate_yz_kernel");                                                                     \
  }
  STFEM_CELL_YZ_SHAPES(STFEM_CELL_CASE)
#undef STFEM_CELL_CASE
  return STFEM_ERR_UNSUPPORTED; // (not reached: make_plan asks has_cell_yz)
}

// out (dims of `to`) (+)= (B2 (x) B1 (x) B0) in, the passes of `plan`; expanding (prolongation): x, y, z keeps the intermediates
// small; contracting: z, y, x.  The last pass takes `add`, the others overwrite their intermediate.
template <typename T>
int apply3(stfem_transfer *t, const Band B[3], const TransferPlan &plan, bool expanding, void *out, const void *in, int add, hipStream_t s)
{
  int dims[3] = {B[0].n_in, B[1].n_in, B[2].n_in};
  const T *cur = static_cast<const T *>(in);
  const int npass = plan.fuse_yz ? 2 : 3;
  for (int step = 0; step < npass; ++step) {
    const int ax = expanding ? step : 2 - step;
    const bool final = step == npass - 1;
    T *dst = final ? static_cast<T *>(out) : static_cast<T *>(t->d_tmp[step]);
    const int a = final ? add : 0;
    int st;
    if (plan.fuse_yz && step == 1)
      st = launch_cell_yz<T>(t->pc[1], t->Rn[1], dst, cur, dims[0], t->ncc[1], t->ncc[2], t->L[1], t->flags[1], t->flags[2], a, s);
    else {
      dims[ax] = B[ax].n_out;
      if (plan.cell[ax]) {
        const long long S = ax == 1 ? dims[0] : (long long)dims[0] * dims[1];
        st = launch_cell<T>(t->pc[ax], t->Rn[ax], plan.nseg[ax], dst, cur, S, t->ncc[ax], S * (ax == 1 ? dims[2] : 1), t->L[ax], t->flags[ax], a, s);
      } else st = launch_axis<T>(dst, cur, dims, ax, B[ax], a, s);
    }
    if (st != STFEM_OK) return st;
    cur = dst;
  }
  return STFEM_OK;
}

int run(stfem_transfer *t, const Band B[3], const TransferPlan &plan, stfem_ctx *to, stfem_ctx *from, stfem_vec *dst, const stfem_vec *src, bool expanding,
        int add, void *stream)
{
  if (!t || !dst || !src) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst->ctx != to || src->ctx != from || dst->nb != src->nb) return STFEM_ERR_SHAPE_MISMATCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int b = 0; b < dst->nb; ++b) {
    const int st = stfem_by_prec(to, [&](auto n) { return apply3<decltype(n)>(t, B, plan, expanding, dst->blk[b], src->blk[b], add, s); });
    if (st != STFEM_OK) return st;
  }
  return STFEM_OK;
}

} // namespace

extern "C" {

int stfem_transfer_create(stfem_ctx *fine, stfem_ctx *coarse, stfem_transfer **out)
{
  return stfem_transfer_create_partitioned(fine, coarse, 0, out);
}

int stfem_transfer_create_partitioned(stfem_ctx *fine, stfem_ctx *coarse, int neighbour_mask, stfem_transfer **out)
{
  if (!fine || !coarse || !out || (neighbour_mask & ~48) || (neighbour_mask & (fine->dmask | coarse->dmask))) return STFEM_ERR_INVALID_ARGUMENT;
  if (fine->prec != coarse->prec || fine->device != coarse->device) return STFEM_ERR_SHAPE_MISMATCH;
  for (int d = 0; d < 3; ++d) {
    const bool same = fine->nc[d] == coarse->nc[d], twice = fine->nc[d] == 2 * coarse->nc[d];
    if (!same && !twice) return STFEM_ERR_SHAPE_MISMATCH;
  }
  if (coarse->p > fine->p) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(fine->device));
  stfem_transfer *t = new stfem_transfer;
  t->fine = fine;
  t->coarse = coarse;
  // a slab with a neighbour above: its top fine plane is the ghost copy of the neighbour's bottom plane (stfem.h: halo support) and
  // is restricted THERE; here it does not contribute, and the add-exchange of the coarse interface planes completes the sums
  const bool ghost_top = neighbour_mask & 32;
  for (int d = 0; d < 3; ++d) {
    std::vector<double> P, I;
    stfem::line_matrices(fine->nc[d], fine->p, coarse->nc[d], coarse->p, P, I);
    const std::vector<double> P0 = P;
    const int n_f = fine->nd[d], n_c = coarse->nd[d];
    // zero-boundary constraints of both levels: constrained rows are not written, constrained columns read as 0
    auto constrained = [&](const stfem_ctx *c, int i, int n) { return (i == 0 && (c->dmask >> (2 * d) & 1)) || (i == n - 1 && (c->dmask >> (2 * d + 1) & 1)); };
    std::vector<double> R(size_t(n_c) * n_f);
    for (int f = 0; f < n_f; ++f)
      for (int c = 0; c < n_c; ++c) {
        if (constrained(fine, f, n_f) || constrained(coarse, c, n_c)) P[size_t(f) * n_c + c] = 0.0, I[size_t(c) * n_f + f] = 0.0;
        R[size_t(c) * n_f + f] = (d == 2 && ghost_top && f == n_f - 1) ? 0.0 : P[size_t(f) * n_c + c];
      }
    // cell form: the block of cell 0 of the unconstrained embedding (the same in every cell)
    t->pc[d] = coarse->p;
    t->Rn[d] = (fine->nc[d] / coarse->nc[d]) * fine->p;
    t->ncc[d] = coarse->nc[d];
    t->flags[d] = (constrained(coarse, 0, n_c) ? CF_LO_C : 0) | (constrained(coarse, n_c - 1, n_c) ? CF_HI_C : 0) |
                  (constrained(fine, 0, n_f) ? CF_LO_F : 0) | (constrained(fine, n_f - 1, n_f) ? CF_HI_F : 0);
    for (int j = 0; j <= t->Rn[d]; ++j)
      for (int a = 0; a <= t->pc[d]; ++a) t->L[d][j * (t->pc[d] + 1) + a] = P0[size_t(j) * n_c + a];
    t->P[d] = make_band(n_f, n_c, P);
    t->R[d] = make_band(n_c, n_f, R);
    t->I[d] = make_band(n_c, n_f, I);
    for (Band *b : {&t->P[d], &t->R[d], &t->I[d]}) {
      const int st = upload(*b);
      if (st != STFEM_OK) {
        stfem_transfer_destroy(t);
        return st;
      }
    }
  }
  make_plan(t, ghost_top);
  // intermediates: (fine x, coarse y, coarse z) and (fine x, fine y, coarse z); the contracting order needs
  // (fine x, fine y, coarse z) and (fine x, coarse y, coarse z): the larger of the two fits both roles
  t->tmp_elems = size_t(fine->nd[0]) * fine->nd[1] * coarse->nd[2];
  for (int k = 0; k < 2; ++k)
    if (hipMalloc(&t->d_tmp[k], t->tmp_elems * fine->es) != hipSuccess) {
      stfem_transfer_destroy(t);
      return STFEM_ERR_OUT_OF_MEMORY;
    }
  *out = t;
  return STFEM_OK;
}

void stfem_transfer_destroy(stfem_transfer *t)
{
  if (!t) return;
  for (int d = 0; d < 3; ++d) {
    release(t->P[d]);
    release(t->R[d]);
    release(t->I[d]);
  }
  (void)hipFree(t->d_tmp[0]);
  (void)hipFree(t->d_tmp[1]);
  delete t;
}

int stfem_transfer_prolongate(stfem_transfer *t, stfem_vec *dst_fine, const stfem_vec *src_coarse, int add, void *stream)
{
  if (!t) return STFEM_ERR_INVALID_ARGUMENT;
  t->last_path[0] = 0;
  const int st = run(t, t->P, t->plan_p, t->fine, t->coarse, dst_fine, src_coarse, true, add, stream);
  if (st == STFEM_OK) t->last_path[0] = t->plan_p.fuse_yz;
  return st;
}
int stfem_transfer_restrict(stfem_transfer *t, stfem_vec *dst_coarse, const stfem_vec *src_fine, int add, void *stream)
{
  if (!t) return STFEM_ERR_INVALID_ARGUMENT;
  t->last_path[1] = t->last_path[2] = 0;
  const int st = run(t, t->R, t->plan_r, t->coarse, t->fine, dst_coarse, src_fine, false, add, stream);
  if (st == STFEM_OK)
    for (int ax = 1; ax < 3; ++ax) // the longest segment [ncell seg / nseg, ncell (seg + 1) / nseg) of the march
      if (t->plan_r.cell[ax]) t->last_path[ax] = (t->ncc[ax] + t->plan_r.nseg[ax] - 1) / t->plan_r.nseg[ax];
  return st;
}
int stfem_transfer_interpolate(stfem_transfer *t, stfem_vec *dst_coarse, const stfem_vec *src_fine, void *stream)
{
  return t ? run(t, t->I, t->plan_i, t->coarse, t->fine, dst_coarse, src_fine, false, 0, stream) : STFEM_ERR_INVALID_ARGUMENT;
}

int stfem_transfer_last_path(const stfem_transfer *t, int32_t out[3])
{
  if (!t || !out) return STFEM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 3; ++i) out[i] = t->last_path[i];
  return STFEM_OK;
}

} // extern "C"
