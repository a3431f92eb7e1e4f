// Vectors of the space-time operator (include/stfem.h): storage, the block arithmetic of the Krylov solvers and the
// time integrators (tensorproduct_add, axpby, inner products, Gram-Schmidt), the precision change of the multigrid and the
// DoF-plane copies of the z-slab exchange.
// (The entry points have C linkage through their declarations in the header.)
#include "stfem_internal.h"
#include "stfem_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

using namespace stfem;

int stfem_vector_create(stfem_ctx *c, int nb, stfem_vec **out)
{
  if (!c || !out || nb < 1) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  stfem_vec *v = new (std::nothrow) stfem_vec;
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->ctx = c;
  v->device = c->device;
  v->nb = nb;
  v->owns = true;
  v->blk.assign(nb, nullptr);
  for (int b = 0; b < nb; ++b) {
    if (hipMalloc(&v->blk[b], size_t(c->ndofs) * c->es) != hipSuccess) {
      stfem_vector_destroy(v);
      return STFEM_ERR_OUT_OF_MEMORY;
    }
    const hipError_t e = hipMemset(v->blk[b], 0, size_t(c->ndofs) * c->es);
    if (e != hipSuccess) {
      stfem_vector_destroy(v);
      return stfem_set_error(STFEM_ERR_HIP, "hipMemset(new vector): %s", hipGetErrorString(e));
    }
  }
  *out = v;
  return STFEM_OK;
}

int stfem_vector_wrap(stfem_ctx *c, int nb, void *const *blocks, stfem_vec **out)
{
  if (!c || !out || nb < 1 || !blocks) return STFEM_ERR_INVALID_ARGUMENT;
  stfem_vec *v = new (std::nothrow) stfem_vec;
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->ctx = c;
  v->device = c->device;
  v->nb = nb;
  v->owns = false;
  for (int b = 0; b < nb; ++b) {
    if (!blocks[b]) {
      delete v;
      return STFEM_ERR_INVALID_ARGUMENT;
    }
    v->blk.push_back(blocks[b]);
  }
  *out = v;
  return STFEM_OK;
}

int stfem_vector_rebind(stfem_vec *v, int nb, void *const *blocks)
{
  if (!v || v->owns || nb < 1 || !blocks) return STFEM_ERR_INVALID_ARGUMENT;
  for (int b = 0; b < nb; ++b)
    if (!blocks[b]) return STFEM_ERR_INVALID_ARGUMENT;
  try {
    v->blk.assign(blocks, blocks + nb); // no allocation while the block count does not grow
  } catch (...) {
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  v->nb = nb;
  return STFEM_OK;
}

void stfem_vector_destroy(stfem_vec *v)
{
  if (!v) return;
  if (v->owns) {
    (void)hipSetDevice(v->device);
    for (void *p : v->blk)
      if (p) (void)hipFree(p);
  }
  delete v;
}

int stfem_vector_n_blocks(const stfem_vec *v) { return v ? v->nb : 0; }
void *stfem_vector_block(const stfem_vec *v, int b)
{
  return (v && b >= 0 && b < v->nb) ? v->blk[b] : nullptr;
}

int stfem_vector_upload(stfem_vec *v, const double *const *host)
{
  if (!v || !host) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(v->ctx->device));
  const size_t n = size_t(v->ctx->ndofs);
  std::vector<float> tmp(v->ctx->prec ? n : 0);
  for (int b = 0; b < v->nb; ++b) {
    if (v->ctx->prec) { // host side is always double; fp32 contexts convert here
      for (size_t i = 0; i < n; ++i) tmp[i] = float(host[b][i]);
      STFEM_TRY(hipMemcpy(v->blk[b], tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    } else {
      STFEM_TRY(hipMemcpy(v->blk[b], host[b], n * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  return STFEM_OK;
}

int stfem_vector_download(const stfem_vec *v, double *const *host)
{
  if (!v || !host) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(v->ctx->device));
  STFEM_TRY(hipDeviceSynchronize());
  const size_t n = size_t(v->ctx->ndofs);
  std::vector<float> tmp(v->ctx->prec ? n : 0);
  for (int b = 0; b < v->nb; ++b) {
    if (v->ctx->prec) {
      STFEM_TRY(hipMemcpy(tmp.data(), v->blk[b], n * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) host[b][i] = tmp[i];
    } else {
      STFEM_TRY(hipMemcpy(host[b], v->blk[b], n * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return STFEM_OK;
}

// ------------------------------------------------------------------------------------ BLAS-1

template <typename T> struct AxpyArgs {
  const T *x[MAX_BLOCKS];
  T coef[MAX_BLOCKS];
  int n;
};
template <typename T> __global__ __launch_bounds__(256) void axpy_kernel(int64_t n, AxpyArgs<T> a, T *y)
{
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    T acc = y[i];
    for (int t = 0; t < a.n; ++t) acc = fma(a.coef[t], a.x[t][i], acc);
    y[i] = acc;
  }
}

template <typename T>
static int tensorproduct_add_t(stfem_ctx *c, int nrows, int ncols, const double *A, stfem_vec *cv, const stfem_vec *b,
                               hipStream_t st)
{
  for (int i = 0; i < nrows; ++i) // a refused call modifies nothing: every row is checked before the first launch
    for (int j = 0; j < ncols; ++j)
      if (A[size_t(i) * ncols + j] != 0.0 && cv->blk[i] == b->blk[j]) return STFEM_ERR_ALIAS;
  for (int i = 0; i < nrows; ++i)
    for (int j0 = 0; j0 < ncols; j0 += MAX_BLOCKS) {
      AxpyArgs<T> a;
      a.n = 0;
      for (int j = j0; j < std::min(ncols, j0 + MAX_BLOCKS); ++j)
        if (A[size_t(i) * ncols + j] != 0.0) { // operators.h:246
          a.x[a.n] = static_cast<const T *>(b->blk[j]);
          a.coef[a.n++] = T(A[size_t(i) * ncols + j]);
        }
      if (a.n == 0) continue;
      const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 256 * 16);
      hipLaunchKernelGGL(axpy_kernel<T>, dim3(grid), dim3(256), 0, st, c->ndofs, a, static_cast<T *>(cv->blk[i]));
    }
  return STFEM_OK;
}

int stfem_tensorproduct_add(stfem_ctx *c, int nrows, int ncols, const double *A, stfem_vec *cv,
                            const stfem_vec *b, void *stream)
{
  if (!c || !A || !cv || !b || cv->ctx != c || b->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (cv->nb != nrows || b->nb != ncols) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  return stfem_by_prec(c, [&](auto t) { return tensorproduct_add_t<decltype(t)>(c, nrows, ncols, A, cv, b, st); });
}

// Local inner products, accumulated in double for both precisions, in TWO STAGES with a fixed summation order (bitwise
// reproducible: round 2 finished with a device atomic): every workgroup of stage 1 writes its partial sums, one
// workgroup of stage 2 adds them in index order.  One launch pair handles up to DOT_VECS left-hand vectors against the
// same right-hand vector over all spatial blocks (the Gram-Schmidt step of the Krylov solvers: k inner products, one pass
// over w per group of eight, one read-back).
struct DotArgs {
  const void *a[DOT_VECS][MAX_BLOCKS];
  const void *b[MAX_BLOCKS];
  int nvec, nblk;
};
template <typename T>
__global__ __launch_bounds__(256) void multi_dot_kernel(int64_t n, const DotArgs args, double *partial /* [nvec][gridDim.x] */)
{
  __shared__ double red[DOT_VECS][4];
  double s[DOT_VECS];
#pragma unroll
  for (int v = 0; v < DOT_VECS; ++v) s[v] = 0.0;
  for (int blk = 0; blk < args.nblk; ++blk) {
    const T *b = static_cast<const T *>(args.b[blk]);
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
      const double w = double(b[i]);
#pragma unroll
      for (int v = 0; v < DOT_VECS; ++v)
        if (v < args.nvec) s[v] = fma(double(static_cast<const T *>(args.a[v][blk])[i]), w, s[v]);
    }
  }
#pragma unroll
  for (int v = 0; v < DOT_VECS; ++v) {
    for (int off = 32; off > 0; off >>= 1) s[v] += __shfl_down(s[v], off, 64);
    if ((threadIdx.x & 63) == 0) red[v][threadIdx.x >> 6] = s[v];
  }
  __syncthreads();
  if (threadIdx.x < unsigned(args.nvec)) {
    const int v = threadIdx.x;
    partial[v * gridDim.x + blockIdx.x] = (red[v][0] + red[v][1]) + (red[v][2] + red[v][3]);
  }
}
// stage 2: out[v] = sum of the partials of vector v in index order (a tree with fixed shape)
__global__ __launch_bounds__(256) void dot_finish_kernel(int nvec, int nparts, const double *partial, double *out)
{
  __shared__ double red[256];
  for (int v = 0; v < nvec; ++v) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partial[v * nparts + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (int(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[v] = red[0];
    __syncthreads();
  }
}
struct MultiAxpyArgs {
  const void *x[DOT_VECS][MAX_BLOCKS];
  void *y[MAX_BLOCKS];
  double coef[DOT_VECS];
  const double *dcoef; // coefficients on the device (sign applied below), or nullptr: coef
  double sign;
  int nvec;
};
// y += sign * sum_v coef_v x_v on every spatial block (blockIdx.y)
template <typename T> __global__ __launch_bounds__(256) void multi_axpy_kernel(int64_t n, const MultiAxpyArgs args)
{
  const int blk = blockIdx.y;
  T *y = static_cast<T *>(args.y[blk]);
  double c[DOT_VECS];
#pragma unroll
  for (int v = 0; v < DOT_VECS; ++v) c[v] = v < args.nvec ? args.sign * (args.dcoef ? args.dcoef[v] : args.coef[v]) : 0.0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    double acc = double(y[i]);
#pragma unroll
    for (int v = 0; v < DOT_VECS; ++v)
      if (v < args.nvec) acc = fma(c[v], double(static_cast<const T *>(args.x[v][blk])[i]), acc);
    y[i] = T(acc);
  }
}

// d_out[0 .. k): <a_i, b> over the first n_own entries of every block; stays on the device
static int multi_dot_device(stfem_ctx *c, int k, const stfem_vec *const *as, const stfem_vec *b, int64_t n_own, double *d_out, hipStream_t st)
{
  if (b->nb > MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  for (int i = 0; i < k; ++i)
    if (!as[i] || as[i]->nb != b->nb || as[i]->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  const int grid = (int)std::min<int64_t>((n_own + 255) / 256, DOT_GRID);
  double *partial = c->d_scratch + DOT_RESULTS; // [DOT_VECS][DOT_GRID]
  stfem_launch_begin();
  for (int k0 = 0; k0 < k; k0 += DOT_VECS) {
    DotArgs args;
    std::memset(&args, 0, sizeof(args));
    args.nvec = std::min(DOT_VECS, k - k0);
    args.nblk = b->nb;
    for (int j = 0; j < b->nb; ++j) args.b[j] = b->blk[j];
    for (int v = 0; v < args.nvec; ++v)
      for (int j = 0; j < b->nb; ++j) args.a[v][j] = as[k0 + v]->blk[j];
    stfem_by_prec(c, [&](auto t) { hipLaunchKernelGGL(multi_dot_kernel<decltype(t)>, dim3(grid), dim3(256), 0, st, n_own, args, partial); });
    hipLaunchKernelGGL(dot_finish_kernel, dim3(1), dim3(256), 0, st, args.nvec, grid, partial, d_out + k0);
  }
  return stfem_launch_end("multi_dot_kernel");
}

int stfem_dot(stfem_ctx *c, const stfem_vec *a, const stfem_vec *b, int64_t n_own, double *out, void *stream)
{
  if (!c || !a || !b || !out || a->nb != b->nb || a->ctx != c || b->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (n_own <= 0 || n_own > c->ndofs) n_own = c->ndofs;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a->nb > MAX_BLOCKS) { // (vectors of more than eight blocks: eight at a time)
    double sum = 0.0;
    for (int j0 = 0; j0 < a->nb; j0 += MAX_BLOCKS) {
      stfem_vec va = *a, vb = *b;
      va.nb = vb.nb = std::min(MAX_BLOCKS, a->nb - j0);
      va.blk.assign(a->blk.begin() + j0, a->blk.begin() + j0 + va.nb);
      vb.blk.assign(b->blk.begin() + j0, b->blk.begin() + j0 + vb.nb);
      double part = 0.0;
      const int rc = stfem_dot(c, &va, &vb, n_own, &part, stream);
      if (rc != STFEM_OK) return rc;
      sum += part;
    }
    *out = sum;
    return STFEM_OK;
  }
  const stfem_vec *as[1] = {a};
  const int rc = multi_dot_device(c, 1, as, b, n_own, c->d_scratch, st);
  if (rc != STFEM_OK) return rc;
  STFEM_TRY(hipMemcpyAsync(out, c->d_scratch, sizeof(double), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  return STFEM_OK;
}

int stfem_multi_dot(stfem_ctx *c, int k, const stfem_vec *const *as, const stfem_vec *b, int64_t n_own, double *out, void *stream)
{
  if (!c || !as || !b || !out || k < 1 || k > DOT_RESULTS - 8 || b->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (n_own <= 0 || n_own > c->ndofs) n_own = c->ndofs;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = multi_dot_device(c, k, as, b, n_own, c->d_scratch, st);
  if (rc != STFEM_OK) return rc;
  STFEM_TRY(hipMemcpyAsync(out, c->d_scratch, sizeof(double) * k, hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  return STFEM_OK;
}

int stfem_multi_axpy(stfem_ctx *c, int k, const double *coef, const stfem_vec *const *xs, stfem_vec *y, void *stream)
{
  if (!c || !coef || !xs || !y || k < 1 || y->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (y->nb > MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  for (int i = 0; i < k; ++i) // a refused call modifies nothing: every vector is checked before the first launch
    if (!xs[i] || xs[i]->nb != y->nb || xs[i]->ctx != c || xs[i] == y) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 2048);
  stfem_launch_begin();
  for (int k0 = 0; k0 < k; k0 += DOT_VECS) {
    MultiAxpyArgs args;
    std::memset(&args, 0, sizeof(args));
    args.nvec = std::min(DOT_VECS, k - k0);
    args.sign = 1.0;
    for (int j = 0; j < y->nb; ++j) args.y[j] = y->blk[j];
    for (int v = 0; v < args.nvec; ++v) {
      args.coef[v] = coef[k0 + v];
      for (int j = 0; j < y->nb; ++j) args.x[v][j] = xs[k0 + v]->blk[j];
    }
    stfem_by_prec(c, [&](auto t) { hipLaunchKernelGGL(multi_axpy_kernel<decltype(t)>, dim3(grid, y->nb), dim3(256), 0, st, c->ndofs, args); });
  }
  return stfem_launch_end("multi_axpy_kernel");
}

// One classical Gram-Schmidt pass of w against v_0 .. v_{k-1} entirely on the device: h = V^T w (two-stage reduction),
// w -= V h with the coefficients read from device memory, h copied to the host at the end (one synchronisation).
int stfem_orthogonalize(stfem_ctx *c, int k, const stfem_vec *const *vs, stfem_vec *w, int64_t n_own, double *h_out, double *norm2_before,
                        double *norm2_out, void *stream)
{
  if (!c || !vs || !w || !h_out || k < 1 || k > DOT_RESULTS - 9 || w->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (w->nb > MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  for (int i = 0; i < k; ++i) { // a refused call modifies nothing: every vector is checked before the first launch
    if (!vs[i] || vs[i]->nb != w->nb || vs[i]->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
    if (vs[i] == w) return STFEM_ERR_ALIAS;
  }
  if (n_own <= 0 || n_own > c->ndofs) n_own = c->ndofs;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // slots of the scratch array: [0, k) coefficients, k: <w, w> before (rides in the same launch as the coefficients), k + 1: after
  std::vector<const stfem_vec *> all(vs, vs + k);
  if (norm2_before) all.push_back(w);
  int rc = multi_dot_device(c, int(all.size()), all.data(), w, n_own, c->d_scratch, st);
  if (rc != STFEM_OK) return rc;
  const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 2048);
  for (int k0 = 0; k0 < k; k0 += DOT_VECS) {
    MultiAxpyArgs args;
    std::memset(&args, 0, sizeof(args));
    args.nvec = std::min(DOT_VECS, k - k0);
    args.sign = -1.0;
    args.dcoef = c->d_scratch + k0;
    for (int j = 0; j < w->nb; ++j) args.y[j] = w->blk[j];
    for (int v = 0; v < args.nvec; ++v)
      for (int j = 0; j < w->nb; ++j) args.x[v][j] = vs[k0 + v]->blk[j];
    stfem_by_prec(c, [&](auto t) { hipLaunchKernelGGL(multi_axpy_kernel<decltype(t)>, dim3(grid, w->nb), dim3(256), 0, st, c->ndofs, args); });
  }
  if ((rc = stfem_launch_end("multi_axpy_kernel")) != STFEM_OK) return rc; // (before multi_dot_device begins a sequence of its own)
  if (norm2_out) { // <w, w> after the projection, in the slot behind the coefficients
    const stfem_vec *ws[1] = {w};
    rc = multi_dot_device(c, 1, ws, w, n_own, c->d_scratch + k + 1, st);
    if (rc != STFEM_OK) return rc;
  }
  std::vector<double> host(size_t(k) + 2);
  STFEM_TRY(hipMemcpyAsync(host.data(), c->d_scratch, sizeof(double) * (k + 2), hipMemcpyDeviceToHost, st));
  STFEM_TRY(hipStreamSynchronize(st));
  for (int i = 0; i < k; ++i) h_out[i] = host[i];
  if (norm2_before) *norm2_before = host[k];
  if (norm2_out) *norm2_out = host[k + 1];
  return STFEM_OK;
}

// y = a x + b y on up to eight blocks per launch (blockIdx.y = block).  A zero factor means "not read": a = 0 never
// touches x, b = 0 never touches y's old content (0 * NaN and 0 * Inf would survive otherwise, where deal.II's
// `dst = 0.` / equ() assign); x and y may be the same vector (no __restrict__).
struct AxpbyBlocks {
  const void *x[8];
  void *y[8];
};
template <typename T>
__global__ __launch_bounds__(256) void axpby_kernel(int64_t n, T a, T b, const AxpbyBlocks blocks)
{
  const T *x = static_cast<const T *>(blocks.x[blockIdx.y]);
  T *y = static_cast<T *>(blocks.y[blockIdx.y]);
  const int64_t i0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
  if (a == T(0) && b == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = T(0);
  else if (a == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = b * y[i];
  else if (b == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = a * x[i];
  else
    for (int64_t i = i0; i < n; i += stride) y[i] = a * x[i] + b * y[i];
}

// the same on arrays of different lengths in one launch (the blocks of a two-variable vector: velocity and pressure blocks)
struct AxpbyMany {
  const void *x[8];
  void *y[8];
  long long len[8];
};
template <typename T>
__global__ __launch_bounds__(256) void axpby_many_kernel(T a, T b, const AxpbyMany v)
{
  const T *x = static_cast<const T *>(v.x[blockIdx.y]);
  T *y = static_cast<T *>(v.y[blockIdx.y]);
  const int64_t n = v.len[blockIdx.y];
  const int64_t i0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
  if (a == T(0) && b == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = T(0);
  else if (a == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = b * y[i];
  else if (b == T(0))
    for (int64_t i = i0; i < n; i += stride) y[i] = a * x[i];
  else
    for (int64_t i = i0; i < n; i += stride) y[i] = a * x[i] + b * y[i];
}

int stfem_vector_axpby(stfem_ctx *c, double a, const stfem_vec *x, double b, stfem_vec *y, void *stream)
{
  if (!c || !x || !y || x->ctx != c || y->ctx != c || x->nb != y->nb) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 4096);
  stfem_launch_begin();
  for (int b0 = 0; b0 < x->nb; b0 += 8) {
    const int nb = std::min(8, x->nb - b0);
    AxpbyBlocks bl{};
    for (int j = 0; j < nb; ++j) {
      bl.x[j] = x->blk[b0 + j];
      bl.y[j] = y->blk[b0 + j];
    }
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(axpby_kernel<T>, dim3(grid, nb), dim3(256), 0, st, c->ndofs, T(a), T(b), bl);
    });
  }
  return stfem_launch_end("axpby_kernel");
}

int stfem_axpby_many(stfem_ctx *c, int n_arrays, const int64_t *len, double a, const void *const *x, double b, void *const *y, void *stream)
{
  if (!c || n_arrays < 0 || (n_arrays > 0 && (!len || !y || (a != 0.0 && !x)))) return STFEM_ERR_INVALID_ARGUMENT;
  for (int j = 0; j < n_arrays; ++j)
    if (len[j] < 0 || !y[j] || (a != 0.0 && !x[j])) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  stfem_launch_begin();
  for (int b0 = 0; b0 < n_arrays; b0 += 8) {
    const int nb = std::min(8, n_arrays - b0);
    AxpbyMany v{};
    long long longest = 0;
    for (int j = 0; j < nb; ++j) {
      v.x[j] = a != 0.0 ? x[b0 + j] : nullptr;
      v.y[j] = y[b0 + j];
      v.len[j] = len[b0 + j];
      longest = std::max<long long>(longest, len[b0 + j]);
    }
    if (longest == 0) continue;
    const unsigned grid = (unsigned)std::min<long long>((longest + 255) / 256, 4096);
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(axpby_many_kernel<T>, dim3(grid, nb), dim3(256), 0, st, T(a), T(b), v);
    });
  }
  return stfem_launch_end("axpby_many_kernel");
}

int stfem_vector_set_zero(stfem_ctx *c, stfem_vec *y, void *stream)
{
  if (!c || !y || y->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  const size_t bytes = size_t(c->ndofs) * c->es;
  for (int j = 0; j < y->nb; ++j) STFEM_TRY(hipMemsetAsync(y->blk[j], 0, bytes, static_cast<hipStream_t>(stream)));
  return STFEM_OK;
}

// the precision change between the solver's vectors and the multigrid's (GMG::vmult, stmg.h:1330-1343: copy_locally_owned_data_from)
namespace {
template <typename TD, typename TS> __global__ void convert_kernel(TD *__restrict__ d, const TS *__restrict__ s, long long n)
{
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) d[t] = TD(s[t]);
}
} // namespace

int stfem_vector_convert(stfem_vec *dst, const stfem_vec *src, void *stream)
{
  if (!dst || !src) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst->nb != src->nb || dst->ctx->ndofs != src->ctx->ndofs) return STFEM_ERR_SHAPE_MISMATCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n = dst->ctx->ndofs;
  const int blocks = int(std::min<long long>((n + 255) / 256, 1 << 16));
  for (int b = 0; b < dst->nb; ++b) {
    const int pd = dst->ctx->prec, ps = src->ctx->prec;
    if (pd == ps) STFEM_TRY(hipMemcpyAsync(dst->blk[b], src->blk[b], size_t(n) * dst->ctx->es, hipMemcpyDeviceToDevice, s));
    else if (pd == 1) convert_kernel<float, double><<<blocks, 256, 0, s>>>(static_cast<float *>(dst->blk[b]), static_cast<const double *>(src->blk[b]), n);
    else convert_kernel<double, float><<<blocks, 256, 0, s>>>(static_cast<double *>(dst->blk[b]), static_cast<const float *>(src->blk[b]), n);
  }
  return stfem_launch_end("convert_kernel");
}

// ------------------------------------------------------------------------------------ plane exchange

template <typename T>
__global__ __launch_bounds__(256) void plane_copy_kernel(int64_t n, const T *src, T *dst, int add)
{
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    dst[i] = add ? dst[i] + src[i] : src[i];
}

int stfem_plane_pack(stfem_ctx *c, const stfem_vec *v, int iz, void *buf, void *stream)
{
  if (!c || !v || !buf || iz < 0 || iz >= c->nd[2]) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  const int64_t plane = int64_t(c->nd[0]) * c->nd[1];
  for (int b = 0; b < v->nb; ++b)
    STFEM_TRY(hipMemcpyAsync(static_cast<char *>(buf) + size_t(b) * plane * c->es,
                           static_cast<const char *>(v->blk[b]) + size_t(plane) * iz * c->es, plane * c->es,
                           hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return STFEM_OK;
}

int stfem_plane_unpack(stfem_ctx *c, stfem_vec *v, int iz, const void *buf, int add, void *stream)
{
  if (!c || !v || !buf || iz < 0 || iz >= c->nd[2]) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  const int64_t plane = int64_t(c->nd[0]) * c->nd[1];
  const unsigned grid = (unsigned)std::min<int64_t>((plane + 255) / 256, 4096);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int b = 0; b < v->nb; ++b) {
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(plane_copy_kernel<T>, dim3(grid), dim3(256), 0, st, plane, static_cast<const T *>(buf) + b * plane,
                         static_cast<T *>(v->blk[b]) + plane * iz, add);
    });
  }
  return STFEM_OK;
}

struct PlanesMoveArgs {
  const void *src[MAX_BLOCKS];
  void *dst[MAX_BLOCKS];
};
// blockIdx.y = plane, blockIdx.z = block; the first / last plane of the range may be added to the destination instead of copied
template <typename T>
__global__ __launch_bounds__(256) void planes_move_kernel(int64_t plane, int nplanes, int add_mask, const PlanesMoveArgs a)
{
  const int q = blockIdx.y;
  const bool add = (q == 0 && (add_mask & 1)) || (q == nplanes - 1 && (add_mask & 2));
  const T *s = static_cast<const T *>(a.src[blockIdx.z]) + plane * q;
  T *d = static_cast<T *>(a.dst[blockIdx.z]) + plane * q;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < plane; i += int64_t(gridDim.x) * blockDim.x) d[i] = add ? d[i] + s[i] : s[i];
}

// nplanes consecutive DoF planes of src (from plane iz_src, context cs) to dst (from plane iz_dst, context cd: the same plane size and
// Number); add_mask bit 0: the first plane is ADDED to the destination's, bit 1: the last one.  One launch for all blocks.
int stfem_planes_move(stfem_ctx *cs, const stfem_vec *src, int iz_src, stfem_ctx *cd, stfem_vec *dst, int iz_dst, int nplanes, int add_mask,
                      void *stream)
{
  if (!cs || !cd || !src || !dst || src->ctx != cs || dst->ctx != cd || nplanes < 1 || iz_src < 0 || iz_dst < 0 || iz_src + nplanes > cs->nd[2] ||
      iz_dst + nplanes > cd->nd[2])
    return STFEM_ERR_INVALID_ARGUMENT;
  if (cs->nd[0] != cd->nd[0] || cs->nd[1] != cd->nd[1] || cs->prec != cd->prec || cs->device != cd->device || src->nb != dst->nb)
    return STFEM_ERR_SHAPE_MISMATCH;
  if (src->nb > MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  STFEM_TRY(hipSetDevice(cd->device));
  const int64_t plane = int64_t(cd->nd[0]) * cd->nd[1];
  PlanesMoveArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int b = 0; b < src->nb; ++b) {
    a.src[b] = static_cast<const char *>(src->blk[b]) + size_t(plane) * iz_src * cs->es;
    a.dst[b] = static_cast<char *>(dst->blk[b]) + size_t(plane) * iz_dst * cd->es;
  }
  const dim3 grid((unsigned)std::min<int64_t>((plane + 255) / 256, 1024), nplanes, src->nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  stfem_by_prec(cd, [&](auto t) { hipLaunchKernelGGL(planes_move_kernel<decltype(t)>, grid, dim3(256), 0, st, plane, nplanes, add_mask, a); });
  return stfem_launch_end("planes_move_kernel");
}
