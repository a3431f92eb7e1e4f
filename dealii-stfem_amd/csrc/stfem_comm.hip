// RCCL inside the boundary: the z-slab partition's interface-plane exchange and the
// reducing inner product, behind the C-ABI, so that a C++ caller (the deal.II side) runs sharded
// without any Python.
//
// Replaces, around the cell loop of MatrixFreeOperator::vmult (reference include/operators.h:1016-1017,
// MatrixFree::cell_loop): src.update_ghost_values() -> stfem_ghost_update, dst.compress(VectorOperation::add)
// followed by the next update_ghost_values -> stfem_halo_begin / stfem_halo_end (one packed exchange of
// all temporal blocks per space-time vmult instead of the reference's 2 * n_blocks), and the MPI_Allreduce
// inside LinearAlgebra::distributed::Vector::operator* / l2_norm -> stfem_dot_global.
//
// One process per GPU; a communicator is one RCCL communicator + one private HIP stream + two events.
// Ring neighbours only (z-slabs): each message rides one xGMI link; the four transfers of a rank are
// fused in one ncclGroupStart/End.  RCCL is bound at run time (dlopen): the library also loads on a
// box without RCCL, where stfem_comm_create reports STFEM_ERR_UNSUPPORTED.  If the process already
// carries an RCCL (e.g. PyTorch's) that copy is used, so that one process never runs two of them.
#include "stfem_internal.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types and enums only: no link-time dependency

#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <new>

namespace {

struct Rccl {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr; // optional
  bool ok = false;
};

template <class F> bool bind(void *h, const char *name, F &f)
{
  f = reinterpret_cast<F>(dlsym(h, name));
  return f != nullptr;
}

const Rccl &rccl()
{
  static Rccl r = [] {
    Rccl q;
    // a copy already in the process first (RTLD_DEFAULT sees it if it was loaded globally), then
    // the known file names without loading a second copy, then a fresh load
    void *h = nullptr;
    if (dlsym(RTLD_DEFAULT, "ncclCommInitRank")) h = RTLD_DEFAULT;
    const char *names[] = {"librccl.so", "librccl.so.1"};
    for (int pass = 0; pass < 2 && !h; ++pass)
      for (const char *n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
        if (h) break;
      }
    if (!h) return q;
    q.handle = h;
    q.ok = bind(h, "ncclGetUniqueId", q.GetUniqueId) && bind(h, "ncclCommInitRank", q.CommInitRank) &&
           bind(h, "ncclCommDestroy", q.CommDestroy) && bind(h, "ncclSend", q.Send) && bind(h, "ncclRecv", q.Recv) &&
           bind(h, "ncclGroupStart", q.GroupStart) && bind(h, "ncclGroupEnd", q.GroupEnd) &&
           bind(h, "ncclAllReduce", q.AllReduce) && bind(h, "ncclGetErrorString", q.GetErrorString);
    (void)bind(h, "ncclCommCount", q.CommCount);
    return q;
  }();
  return r;
}

} // namespace

struct stfem_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1, device = 0;
  hipStream_t stream = nullptr;     // the transfers run here, beside the caller's stream
  hipEvent_t packed = nullptr, arrived = nullptr;
  // packed planes [top send | bottom send | top recv | bottom recv], grown on demand
  void *buf = nullptr;
  size_t buf_bytes = 0;
  double *d_red = nullptr; // all-reduce operand
  // the exchange in flight between halo_begin and halo_end
  bool pending = false;
  int lower = -1, upper = -1;
  size_t plane_bytes = 0; // of all blocks
};

#define COMM_NCCL(call)                                                                                               \
  do {                                                                                                                \
    ncclResult_t r_ = (call);                                                                                         \
    if (r_ != ncclSuccess) return stfem_set_error(STFEM_ERR_COMM, "%s: %s", #call, rccl().GetErrorString(r_));        \
  } while (0)

// inside ncclGroupStart / GroupEnd: a failed call still closes the group (an open group would swallow every later
// RCCL call of this thread) before the error is returned
#define COMM_NCCL_IN_GROUP(call)                                                                                      \
  do {                                                                                                                \
    ncclResult_t r_ = (call);                                                                                         \
    if (r_ != ncclSuccess) {                                                                                          \
      (void)rccl().GroupEnd();                                                                                        \
      return stfem_set_error(STFEM_ERR_COMM, "%s: %s", #call, rccl().GetErrorString(r_));                             \
    }                                                                                                                 \
  } while (0)

extern "C" {


int stfem_comm_get_unique_id(void *id)
{
  if (!id) return STFEM_ERR_INVALID_ARGUMENT;
  static_assert(STFEM_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (!rccl().ok) {
    const char *why = dlerror(); // (a second call returns NULL)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "librccl.so not found: %s", why ? why : "");
  }
  ncclUniqueId u;
  COMM_NCCL(rccl().GetUniqueId(&u));
  std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return STFEM_OK;
}

int stfem_comm_create(const void *id, int rank, int world, int device, stfem_comm **out)
{
  if (!id || !out || world < 1 || rank < 0 || rank >= world) return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!rccl().ok) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "librccl.so not found");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return STFEM_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(device));
  stfem_comm *c = new (std::nothrow) stfem_comm;
  if (!c) return STFEM_ERR_OUT_OF_MEMORY;
  c->rank = rank; c->world = world; c->device = device;
  ncclUniqueId u;
  std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclResult_t r = rccl().CommInitRank(&c->comm, world, u, rank);
  if (r != ncclSuccess) {
    delete c;
    return stfem_set_error(STFEM_ERR_COMM, "ncclCommInitRank: %s", rccl().GetErrorString(r));
  }
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->packed, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->arrived, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&c->d_red, sizeof(double));
  if (e != hipSuccess) {
    stfem_comm_destroy(c);
    return stfem_set_error(STFEM_ERR_HIP, "communicator stream, events and buffer: %s", hipGetErrorString(e));
  }
  *out = c;
  return STFEM_OK;
}

void stfem_comm_destroy(stfem_comm *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)rccl().CommDestroy(c->comm);
  if (c->buf) (void)hipFree(c->buf);
  if (c->d_red) (void)hipFree(c->d_red);
  if (c->packed) (void)hipEventDestroy(c->packed);
  if (c->arrived) (void)hipEventDestroy(c->arrived);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int stfem_comm_available(void) { return rccl().ok ? 1 : 0; }
int stfem_comm_rccl_count(const stfem_comm *c)
{
  int n = 0;
  if (!c || !c->comm || !rccl().CommCount || rccl().CommCount(c->comm, &n) != ncclSuccess) return 0;
  return n;
}
int stfem_comm_rank(const stfem_comm *c) { return c ? c->rank : -1; }
int stfem_comm_size(const stfem_comm *c) { return c ? c->world : 0; }

static int plane_geometry(stfem_ctx *ctx, const stfem_vec *v, size_t &plane_bytes, int &nz)
{
  int32_t nd[3];
  if (stfem_n_dofs_1d(ctx, nd) != STFEM_OK) return STFEM_ERR_INVALID_ARGUMENT;
  const size_t es = stfem_ctx_precision(ctx) ? sizeof(float) : sizeof(double);
  plane_bytes = size_t(nd[0]) * nd[1] * es * stfem_vector_n_blocks(v);
  nz = nd[2];
  return STFEM_OK;
}

static int ensure_buffers(stfem_comm *c, size_t plane_bytes)
{
  if (c->buf_bytes >= 4 * plane_bytes) return STFEM_OK;
  STFEM_TRY(hipStreamSynchronize(c->stream));
  if (c->buf) STFEM_TRY(hipFree(c->buf));
  c->buf = nullptr;
  c->buf_bytes = 0;
  if (hipMalloc(&c->buf, 4 * plane_bytes) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
  c->buf_bytes = 4 * plane_bytes;
  return STFEM_OK;
}

static int check_neighbours(const stfem_comm *c, int lower, int upper)
{
  return (lower >= -1 && lower < c->world && upper >= -1 && upper < c->world) ? STFEM_OK : STFEM_ERR_INVALID_ARGUMENT;
}

int stfem_halo_begin(stfem_ctx *ctx, stfem_comm *c, stfem_vec *v, int lower, int upper, void *stream)
{
  return stfem_halo_begin_split(c, ctx, v, ctx, v, lower, upper, stream);
}

// The same with the two interface planes taken from two vectors: plane 0 of v_lo (context ctx_lo) goes to the lower neighbour, the
// top plane of v_hi (context ctx_hi) to the upper one.  A rank that sweeps its interface cell layers first (into vectors of their
// own) starts the exchange with this before it sweeps its interior cells; stfem_halo_end then adds what arrived into the assembled
// destination vector as usual.
int stfem_halo_begin_split(stfem_comm *c, stfem_ctx *ctx_lo, stfem_vec *v_lo, stfem_ctx *ctx_hi, stfem_vec *v_hi, int lower, int upper, void *stream)
{
  if (!ctx_lo || !ctx_hi || !c || !v_lo || !v_hi || check_neighbours(c, lower, upper) != STFEM_OK || c->pending)
    return STFEM_ERR_INVALID_ARGUMENT;
  size_t pb, pb_hi;
  int nz_lo, nz;
  int rc = plane_geometry(ctx_lo, v_lo, pb, nz_lo);
  if (rc == STFEM_OK) rc = plane_geometry(ctx_hi, v_hi, pb_hi, nz);
  if (rc != STFEM_OK) return rc;
  if (pb != pb_hi || stfem_ctx_precision(ctx_lo) != stfem_ctx_precision(ctx_hi)) return STFEM_ERR_SHAPE_MISMATCH;
  stfem_ctx *ctx = ctx_hi;
  if (lower < 0 && upper < 0) {
    c->lower = lower; c->upper = upper; c->plane_bytes = pb;
    c->pending = true;
    return STFEM_OK;
  }
  STFEM_TRY(hipSetDevice(c->device));
  if ((rc = ensure_buffers(c, pb)) != STFEM_OK) return rc;
  char *ts = static_cast<char *>(c->buf), *bs = ts + pb, *tr = bs + pb, *br = tr + pb;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // this rank's partial sums of its two interface planes
  if (upper >= 0 && (rc = stfem_plane_pack(ctx_hi, v_hi, nz - 1, ts, st)) != STFEM_OK) return rc;
  if (lower >= 0 && (rc = stfem_plane_pack(ctx_lo, v_lo, 0, bs, st)) != STFEM_OK) return rc;
  STFEM_TRY(hipEventRecord(c->packed, st));
  STFEM_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
  const ncclDataType_t dt = stfem_ctx_precision(ctx) ? ncclFloat : ncclDouble;
  const size_t count = pb / (stfem_ctx_precision(ctx) ? sizeof(float) : sizeof(double));
  COMM_NCCL(rccl().GroupStart());
  if (upper >= 0) {
    COMM_NCCL_IN_GROUP(rccl().Send(ts, count, dt, upper, c->comm, c->stream));
    COMM_NCCL_IN_GROUP(rccl().Recv(tr, count, dt, upper, c->comm, c->stream));
  }
  if (lower >= 0) {
    COMM_NCCL_IN_GROUP(rccl().Send(bs, count, dt, lower, c->comm, c->stream));
    COMM_NCCL_IN_GROUP(rccl().Recv(br, count, dt, lower, c->comm, c->stream));
  }
  COMM_NCCL(rccl().GroupEnd());
  STFEM_TRY(hipEventRecord(c->arrived, c->stream));
  c->lower = lower; c->upper = upper; c->plane_bytes = pb; // (only a successful begin leaves an exchange pending)
  c->pending = true;
  return STFEM_OK;
}

int stfem_halo_end(stfem_ctx *ctx, stfem_comm *c, stfem_vec *v, void *stream)
{
  if (!ctx || !c || !v || !c->pending) return STFEM_ERR_INVALID_ARGUMENT;
  c->pending = false;
  if (c->lower < 0 && c->upper < 0) return STFEM_OK;
  size_t pb;
  int nz;
  int rc = plane_geometry(ctx, v, pb, nz);
  if (rc != STFEM_OK || pb != c->plane_bytes) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  STFEM_TRY(hipStreamWaitEvent(st, c->arrived, 0));
  char *tr = static_cast<char *>(c->buf) + 2 * pb, *br = tr + pb;
  if (c->upper >= 0 && (rc = stfem_plane_unpack(ctx, v, nz - 1, tr, 1, st)) != STFEM_OK) return rc;
  if (c->lower >= 0 && (rc = stfem_plane_unpack(ctx, v, 0, br, 1, st)) != STFEM_OK) return rc;
  // the buffers are reused by the next exchange: it must not start before these adds have read them
  STFEM_TRY(hipEventRecord(c->packed, st));
  STFEM_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
  return STFEM_OK;
}

int stfem_ghost_update(stfem_ctx *ctx, stfem_comm *c, stfem_vec *v, int lower, int upper, void *stream)
{
  if (!ctx || !c || !v || check_neighbours(c, lower, upper) != STFEM_OK || c->pending)
    return STFEM_ERR_INVALID_ARGUMENT;
  if (lower < 0 && upper < 0) return STFEM_OK;
  size_t pb;
  int nz;
  int rc = plane_geometry(ctx, v, pb, nz);
  if (rc != STFEM_OK) return rc;
  STFEM_TRY(hipSetDevice(c->device));
  if ((rc = ensure_buffers(c, pb)) != STFEM_OK) return rc;
  char *bs = static_cast<char *>(c->buf) + pb, *tr = bs + pb;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the owner of an interface plane is the upper rank (its bottom plane); the lower rank's top plane is the ghost
  if (lower >= 0 && (rc = stfem_plane_pack(ctx, v, 0, bs, st)) != STFEM_OK) return rc;
  STFEM_TRY(hipEventRecord(c->packed, st));
  STFEM_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
  const ncclDataType_t dt = stfem_ctx_precision(ctx) ? ncclFloat : ncclDouble;
  const size_t count = pb / (stfem_ctx_precision(ctx) ? sizeof(float) : sizeof(double));
  COMM_NCCL(rccl().GroupStart());
  if (lower >= 0) COMM_NCCL_IN_GROUP(rccl().Send(bs, count, dt, lower, c->comm, c->stream));
  if (upper >= 0) COMM_NCCL_IN_GROUP(rccl().Recv(tr, count, dt, upper, c->comm, c->stream));
  COMM_NCCL(rccl().GroupEnd());
  STFEM_TRY(hipEventRecord(c->arrived, c->stream));
  STFEM_TRY(hipStreamWaitEvent(st, c->arrived, 0));
  if (upper >= 0 && (rc = stfem_plane_unpack(ctx, v, nz - 1, tr, 0, st)) != STFEM_OK) return rc;
  STFEM_TRY(hipEventRecord(c->packed, st));
  STFEM_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
  return STFEM_OK;
}

// Caller's buffers, no packing.  Each send is followed by the receive it meets on the self-loop communicator, where the pairs match in
// the order they are issued: up -> below, down -> above.
int stfem_neighbour_exchange(stfem_comm *c, int lower, int upper, int64_t count, const double *send_down, const double *send_up,
                             double *recv_below, double *recv_above, void *stream)
{
  if (!c || count < 0 || check_neighbours(c, lower, upper) != STFEM_OK || c->pending) return STFEM_ERR_INVALID_ARGUMENT;
  if ((lower >= 0 && (!send_down || !recv_below)) || (upper >= 0 && (!send_up || !recv_above))) return STFEM_ERR_INVALID_ARGUMENT;
  if ((lower < 0 && upper < 0) || count == 0) return STFEM_OK;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  STFEM_TRY(hipEventRecord(c->packed, st));
  STFEM_TRY(hipStreamWaitEvent(c->stream, c->packed, 0));
  COMM_NCCL(rccl().GroupStart());
  if (upper >= 0) COMM_NCCL_IN_GROUP(rccl().Send(send_up, size_t(count), ncclDouble, upper, c->comm, c->stream));
  if (lower >= 0) COMM_NCCL_IN_GROUP(rccl().Recv(recv_below, size_t(count), ncclDouble, lower, c->comm, c->stream));
  if (lower >= 0) COMM_NCCL_IN_GROUP(rccl().Send(send_down, size_t(count), ncclDouble, lower, c->comm, c->stream));
  if (upper >= 0) COMM_NCCL_IN_GROUP(rccl().Recv(recv_above, size_t(count), ncclDouble, upper, c->comm, c->stream));
  COMM_NCCL(rccl().GroupEnd());
  STFEM_TRY(hipEventRecord(c->arrived, c->stream));
  STFEM_TRY(hipStreamWaitEvent(st, c->arrived, 0));
  return STFEM_OK;
}

int stfem_dot_global(stfem_ctx *ctx, stfem_comm *c, const stfem_vec *a, const stfem_vec *b, int64_t n_own,
                     double *out, void *stream)
{
  if (!ctx || !c || !a || !b || !out) return STFEM_ERR_INVALID_ARGUMENT;
  double local = 0.0;
  const int rc = stfem_dot(ctx, a, b, n_own, &local, stream); // synchronous
  if (rc != STFEM_OK) return rc;
  if (c->world == 1) {
    *out = local;
    return STFEM_OK;
  }
  STFEM_TRY(hipSetDevice(c->device));
  STFEM_TRY(hipMemcpyAsync(c->d_red, &local, sizeof(double), hipMemcpyHostToDevice, c->stream));
  COMM_NCCL(rccl().AllReduce(c->d_red, c->d_red, 1, ncclDouble, ncclSum, c->comm, c->stream));
  STFEM_TRY(hipMemcpyAsync(out, c->d_red, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  STFEM_TRY(hipStreamSynchronize(c->stream));
  return STFEM_OK;
}

} // extern "C"
