// Stokes two-field operator on MI355X (BASELINE configs[4]): the context, its vectors and the vmult entry points.
//
// Two implementations of the cell loop.  Axis-aligned uniform meshes: the Kronecker form (stokes_cart_launch below) - the velocity
// components as the blocks of the scalar FE_Q(2) pencil sweep (csrc/stfem_pencil.hip), for one time dof with the pressure gradient
// term folded into that sweep, and the coupling kernels of stfem_stokes_coupling.hip, the divergence as a marching gather kernel.
// General meshes: the cell kernel (stfem_stokes_cell.hip).  On top of either: the weak (Nitsche) boundary faces
// (stfem_stokes_boundary.hip), and with a convection mode (form / jacobian of the Navier-Stokes operator) the convection launches
// (stfem_stokes_convection.hip), and with delta0 != 0 the CIP interior-face launches (stfem_stokes_cip.hip).  The helpers of the pressure space the solver around the operator needs: stfem_stokes_pressure.hip.
// Every entry point describes its launches in ONE form, a StokesSet (stfem_stokes_set.h: sources, destinations, weights, store flags -
// nothing of the mesh or the degree), put together by the builder of stokes_set_builder below.  A launcher writes the set into the
// context's description of its degree (stokes_params<DEG>, stfem_stokes_internal.h); the degree becomes a template parameter in
// stokes_with_degree alone.
// A context of velocity degree 3 (stfem_stokes_create_space) has one implementation of the linear cell operator, the same cell kernel
// at DEG = 3 (stfem_stokes_cell.hip), and on top of it either the boundary launches of the weak faces (the boundary kernel at DEG = 3,
// set through stfem_stokes_set_weak_boundaries_space of stfem_stokes_boundary_space.h) or the convection launches of the
// Navier-Stokes modes (the same kernel at DEG = 3, stfem_stokes_convection.hip), reached through the _space entries of
// stfem_stokes_convection_space.h - not both: a mode on a context with weak faces is refused (stokes_refuse_inflow_q3) - and last,
// with delta0 != 0, the CIP launches of the degree-3 kernel (stfem_stokes_set_cip_space of stfem_stokes_cip_space.h).
// stokes_require_q2 refuses the rest, so that stokes_launch finds nothing else to launch there
// (beside the operator such a context has its per-cell Vanka smoother, stfem_stokes_vanka_create_space in stfem_stokes_vanka.hip).
#include "stfem_stokes_internal.h"

#include <mutex>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

static int stokes_lowest_priority()
{
  int lo = 0, hi = 0; // (numerically highest value = lowest priority)
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return lo;
}
// One side stream per device for all Stokes contexts (a multigrid has one context per level: a stream each would outnumber the
// hardware queues, and dependencies between streams that share a queue are resolved on the host).  Never destroyed.
static hipStream_t stokes_side_stream(int device)
{
  static std::mutex mu;
  static hipStream_t streams[64] = {};
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!streams[device] && hipStreamCreateWithPriority(&streams[device], hipStreamNonBlocking, stokes_lowest_priority()) != hipSuccess) {
    (void)hipGetLastError();
    streams[device] = nullptr;
  }
  return streams[device];
}

// Geometry and 1D tables of a context, in the launch description of its degree; what does not depend on the degree on the context too
template <int DEG, class Table>
static void stokes_describe(stfem_stokes_ctx *c, const stfem_mesh_desc *mesh, const Table &Su, const Table &Du, const stfem::Mat &Sp,
                            const std::vector<double> &xq, const std::vector<double> &wq, StokesParamsT<DEG> &b)
{
  for (int i = 0; i < (DEG + 1) * (DEG + 1); ++i) { b.Su[i] = Su[i]; b.Du[i] = Du[i]; }
  for (int i = 0; i < (DEG + 1) * DEG; ++i) b.Sp[i] = Sp[i];
  for (int i = 0; i <= DEG; ++i) {
    b.xq[i] = xq[i]; b.wq[i] = wq[i];
    b.lq[0][i] = std::sqrt(3.0) * (2.0 * xq[i] - 1.0);
    if (DEG > 2) b.lq[DEG - 2][i] = std::sqrt(5.0) * (6.0 * xq[i] * xq[i] - 6.0 * xq[i] + 1.0);
  }
  b.vertices = c->d_vertices;
  b.ncx = c->nc[0]; b.ncy = c->nc[1]; b.ncz = c->nc[2];
  for (int d = 0; d < 3; ++d) { b.ndu[d] = c->ndu[d]; b.ndp[d] = c->ndp[d]; }
  b.Nu = c->Nu; b.Np = c->Np;
  b.dmask = c->dmask;
  b.nu = c->nu;
  b.cart = mesh->vertices ? 0 : 1;
  b.pdg = c->pspace;
  b.interleave = 1;
  if (const char *e = getenv("STFEM_STOKES_INTERLEAVE")) b.interleave = atoi(e) != 0;
  b.detJ = 1.0;
  for (int d = 0; d < 3; ++d) {
    const double h = (mesh->upper[d] - mesh->lower[d]) / c->nc[d];
    b.hinv[d] = 1.0 / h;
    b.detJ *= h;
  }
  c->cart = b.cart != 0; c->detJ = b.detJ;
  for (int d = 0; d < 3; ++d) c->hinv[d] = b.hinv[d];
}

extern "C" {

int stfem_stokes_last_cell_plan(const stfem_stokes_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (!c->cell_launched) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_last_cell_plan: this context has not launched the cell kernel");
  out[0] = c->cell_plan[0];
  out[1] = c->cell_plan[1];
  return STFEM_OK;
}

int stfem_stokes_last_convection_plan(const stfem_stokes_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  if (!c->convection_launched)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_last_convection_plan: this context has not launched a convection kernel");
  out[0] = c->convection_plan[0];
  out[1] = c->convection_plan[1];
  return STFEM_OK;
}

int stfem_stokes_last_sweep_plan(const stfem_stokes_ctx *c, int32_t out[3])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  out[2] = c->last_grad_in_sweep ? 1 : 0;
  return stfem_last_sweep_plan(c->scalar, out); // the velocity sweeps run on the scalar FE_Q(2) context
}

int stfem_stokes_create(const stfem_mesh_desc *mesh, int velocity_degree, double viscosity, stfem_stokes_ctx **out)
{
  return stfem_stokes_create_ex(mesh, velocity_degree, 0, viscosity, out);
}

// The context of velocity degree 2 or 3 behind the three constructors
static int stokes_create_degree(const stfem_mesh_desc *mesh, int velocity_degree, int pressure_space, double viscosity, stfem_stokes_ctx **out);

int stfem_stokes_create_ex(const stfem_mesh_desc *mesh, int velocity_degree, int pressure_space, double viscosity, stfem_stokes_ctx **out)
{
  if (!mesh || !out || pressure_space < 0 || pressure_space > 1) return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (velocity_degree != 2) return STFEM_ERR_UNSUPPORTED; // this constructor: Q2/Q1 (BASELINE configs[4]) only; degree 3: stfem_stokes_create_space
  return stokes_create_degree(mesh, velocity_degree, pressure_space, viscosity, out);
}

int stfem_stokes_create_space(const stfem_mesh_desc *mesh, const stfem_stokes_space_desc *space, stfem_stokes_ctx **out)
{
  if (!mesh || !space || !out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_create_space: a null argument");
  *out = nullptr;
  for (int i = 0; i < 4; ++i)
    if (space->reserved[i] != 0)
      return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_create_space: reserved[%d] = %d, must be 0", i, (int)space->reserved[i]);
  if (space->pressure_space < 0 || space->pressure_space > 1)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_create_space: pressure_space %d, must be 0 (FE_Q) or 1 (FE_DGP)",
                           (int)space->pressure_space);
  if (space->velocity_degree == 2) return stfem_stokes_create_ex(mesh, 2, space->pressure_space, space->viscosity, out);
  if (space->velocity_degree != 3)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stfem_stokes_create_space: velocity degree %d is not built (2 and 3 are)",
                           (int)space->velocity_degree);
  return stokes_create_degree(mesh, 3, space->pressure_space, space->viscosity, out);
}

static int stokes_create_degree(const stfem_mesh_desc *mesh, int velocity_degree, int pressure_space, double viscosity, stfem_stokes_ctx **out)
{
  for (int d = 0; d < 3; ++d)
    if (mesh->ncell[d] < 1) return STFEM_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  {
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return stfem_set_error(STFEM_ERR_NO_DEVICE, "hipGetDeviceCount: %s (%d devices)", hipGetErrorString(e), ndev);
  }
  if (mesh->device < 0 || mesh->device >= ndev) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(mesh->device));
  stfem_stokes_ctx *c = new (std::nothrow) stfem_stokes_ctx;
  if (!c) return STFEM_ERR_OUT_OF_MEMORY;
  c->device = mesh->device;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, mesh->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
  }
  c->dmask = mesh->dirichlet_mask;
  c->nu = viscosity;
  for (int d = 0; d < 3; ++d) {
    c->nc[d] = mesh->ncell[d];
    c->ndu[d] = velocity_degree * mesh->ncell[d] + 1;
    c->ndp[d] = (velocity_degree - 1) * mesh->ncell[d] + 1;
  }
  c->degree = velocity_degree;
  c->Nu = (long long)c->ndu[0] * c->ndu[1] * c->ndu[2];
  c->Np = (long long)c->ndp[0] * c->ndp[1] * c->ndp[2];
  c->pspace = pressure_space;
  // FE_DGP(1): 1, x, y, z per cell; FE_DGP(2): the ten Legendre products of total degree <= 2
  if (pressure_space == 1) c->Np = (velocity_degree == 2 ? 4ll : 10ll) * c->nc[0] * c->nc[1] * c->nc[2];
  const size_t nv = size_t(c->nc[0] + 1) * (c->nc[1] + 1) * (c->nc[2] + 1);
  std::vector<double> v(nv * 3);
  if (mesh->vertices) {
    std::memcpy(v.data(), mesh->vertices, nv * 3 * sizeof(double));
  } else {
    size_t o = 0;
    for (int k = 0; k <= c->nc[2]; ++k)
      for (int j = 0; j <= c->nc[1]; ++j)
        for (int i = 0; i <= c->nc[0]; ++i, ++o) {
          v[3 * o] = mesh->lower[0] + (mesh->upper[0] - mesh->lower[0]) * i / c->nc[0];
          v[3 * o + 1] = mesh->lower[1] + (mesh->upper[1] - mesh->lower[1]) * j / c->nc[1];
          v[3 * o + 2] = mesh->lower[2] + (mesh->upper[2] - mesh->lower[2]) * k / c->nc[2];
        }
  }
  if (hipMalloc(&c->d_vertices, nv * 3 * sizeof(double)) != hipSuccess) {
    delete c;
    return STFEM_ERR_OUT_OF_MEMORY;
  }
  const hipError_t up = hipMemcpy(c->d_vertices, v.data(), nv * 3 * sizeof(double), hipMemcpyHostToDevice);
  if (up != hipSuccess) {
    (void)hipFree(c->d_vertices);
    delete c;
    return stfem_set_error(STFEM_ERR_HIP, "vertex upload: %s", hipGetErrorString(up));
  }
  c->h_vertices = v;
  std::memset(&c->bnd, 0, sizeof(c->bnd));
  // 1D tables: FE_Q(degree) and FE_Q(degree - 1) on Gauss-Lobatto nodes at the degree + 1 Gauss points
  const stfem::ShapeTables tu = stfem::make_shape_tables(velocity_degree), tp = stfem::make_shape_tables(velocity_degree - 1);
  std::vector<double> xq, wq;
  stfem::gauss_rule(velocity_degree + 1, xq, wq);
  stfem::Mat Sp, Gp;
  stfem::lagrange_tables(tp.nodes, xq, Sp, Gp);
  std::memset(&c->coupling, 0, sizeof(c->coupling));
  if (velocity_degree == 3) stokes_describe(c, mesh, tu.S, tu.D, Sp, xq, wq, c->base3);
  else stokes_describe(c, mesh, tu.S, tu.D, Sp, xq, wq, c->base);
  if (c->cart && velocity_degree == 2) { // (degree 3: no scalar pencil context, the cell kernel serves boxes too)
    const char *e = getenv("STFEM_STOKES_CELL"); // 1: keep the cell kernel on boxes too (cross-checks, measurements)
    if (!(e && atoi(e) != 0)) {
      stfem_mesh_desc md = *mesh;
      md.vertices = nullptr;
      stfem_space_desc sd{2, 3, 1, 0};
      const int rc = stfem_ctx_create(&md, &sd, &c->scalar);
      if (rc != STFEM_OK) c->scalar = nullptr; // (the cell kernel serves then)
      else if (!(c->side = stokes_side_stream(c->device)) || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
               hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        c->side = nullptr; // (the divergence kernel then follows the sweep on the caller's stream)
      }
    }
    CouplingParams &k = c->coupling;
    k.ncx = c->nc[0]; k.ncy = c->nc[1]; k.ncz = c->nc[2];
    for (int d = 0; d < 3; ++d) {
      k.ndu[d] = c->ndu[d]; k.ndp[d] = c->ndp[d];
      k.h[d] = (mesh->upper[d] - mesh->lower[d]) / c->nc[d];
    }
    k.Nu = c->Nu; k.dmask = c->dmask; k.pdg = c->pspace;
    // 1D integrals on the reference cell with the operator's Gauss rule (exact for these polynomials)
    for (int a = 0; a < 3; ++a)
      for (int j = 0; j < 2; ++j) {
        double n = 0.0, cc = 0.0;
        for (int q = 0; q < 3; ++q) {
          const double psi = c->pspace ? (j == 0 ? 1.0 : std::sqrt(3.0) * (2.0 * xq[q] - 1.0)) : Sp[q * 2 + j];
          n += wq[q] * tu.S[q * 3 + a] * psi;
          cc += wq[q] * tu.D[q * 3 + a] * psi;
        }
        k.N[a][j] = n;
        k.C[a][j] = cc;
      }
  }
  *out = c;
  return STFEM_OK;
}

void stfem_stokes_destroy(stfem_stokes_ctx *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->d_vertices) (void)hipFree(c->d_vertices);
  if (c->d_g) (void)hipFree(c->d_g);
  if (c->scalar) stfem_ctx_destroy(c->scalar);
  if (c->pressure_space) stfem_ctx_destroy(c->pressure_space);
  if (c->d_pq) (void)hipFree(c->d_pq);
  if (c->d_pred) (void)hipFree(c->d_pred);
  if (c->d_div) (void)hipFree(c->d_div);
  if (c->d_trac) (void)hipFree(c->d_trac);
  for (double *v : c->d_cip_vertices)
    if (v) (void)hipFree(v);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  delete c;
}

} // extern "C"
int stokes_require_q2(const stfem_stokes_ctx *c, const char *entry)
{
  if (c && c->degree != 2)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "%s is built for velocity degree 2 only (this context has degree %d)", entry, c->degree);
  return STFEM_OK;
}
int stfem_stokes_internal_desc(const stfem_stokes_ctx *c, stfem_stokes_desc *d)
{
  if (!c || !d) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(c, "stfem_stokes_internal_desc")) return rq;
  return stokes_desc_any_degree(c, d);
}
int stokes_velocity_degree(const stfem_stokes_ctx *c) { return c->degree; }
int stokes_refuse_inflow_q3(const stfem_stokes_ctx *c, const char *entry)
{
  if (c && c->degree == 3 && c->weak_mask)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "%s on a context of velocity degree 3 with weak faces (mask %d): the inflow term - min(b.n, 0) u of the "
                           "faces is not built at degree 3", entry, c->weak_mask);
  return STFEM_OK;
}
int stokes_desc_any_degree(const stfem_stokes_ctx *c, stfem_stokes_desc *d)
{
  d->device = c->device; d->cart = c->cart; d->pspace = c->pspace; d->dmask = c->dmask;
  d->weak_mask = c->weak_mask; d->outflow_mask = c->outflow_mask;
  for (int k = 0; k < 3; ++k) {
    d->nc[k] = c->nc[k]; d->ndu[k] = c->ndu[k]; d->ndp[k] = c->ndp[k];
    d->lower[k] = c->h_vertices[k];
    d->upper[k] = c->h_vertices[c->h_vertices.size() - 3 + k];
  }
  d->Nu = c->Nu; d->Np = c->Np; d->nu = c->nu; d->penalty1 = c->penalty1; d->penalty2 = c->penalty2;
  return STFEM_OK;
}
extern "C" {

int64_t stfem_stokes_n_velocity_dofs(const stfem_stokes_ctx *c) { return c ? c->Nu : 0; }
int64_t stfem_stokes_n_pressure_dofs(const stfem_stokes_ctx *c) { return c ? c->Np : 0; }

static size_t stokes_len(const stfem_stokes_ctx *c, int variable) { return variable == 0 ? size_t(3 * c->Nu) : size_t(c->Np); }

int stfem_stokes_vector_create(stfem_stokes_ctx *c, int variable, double **device_out)
{
  if (!c || !device_out || variable < 0 || variable > 1) return STFEM_ERR_INVALID_ARGUMENT;
  *device_out = nullptr;
  STFEM_TRY(hipSetDevice(c->device));
  double *d = nullptr;
  if (hipMalloc(&d, stokes_len(c, variable) * sizeof(double)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
  const hipError_t e = hipMemset(d, 0, stokes_len(c, variable) * sizeof(double));
  if (e != hipSuccess) {
    (void)hipFree(d);
    return stfem_set_error(STFEM_ERR_HIP, "hipMemset(new vector): %s", hipGetErrorString(e));
  }
  *device_out = d;
  return STFEM_OK;
}

void stfem_stokes_vector_destroy(stfem_stokes_ctx *c, double *device_vec)
{
  if (!c || !device_vec) return;
  (void)hipSetDevice(c->device);
  (void)hipFree(device_vec);
}

int stfem_stokes_vector_upload(stfem_stokes_ctx *c, int variable, double *device_vec, const double *host)
{
  if (!c || !device_vec || !host || variable < 0 || variable > 1) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  STFEM_TRY(hipMemcpy(device_vec, host, stokes_len(c, variable) * sizeof(double), hipMemcpyHostToDevice));
  return STFEM_OK;
}

int stfem_stokes_vector_download(stfem_stokes_ctx *c, int variable, const double *device_vec, double *host)
{
  if (!c || !device_vec || !host || variable < 0 || variable > 1) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  STFEM_TRY(hipMemcpy(host, device_vec, stokes_len(c, variable) * sizeof(double), hipMemcpyDeviceToHost));
  return STFEM_OK;
}

} // extern "C"

namespace {

int stokes_launch(stfem_stokes_ctx *c, const StokesSet &set, int mode, const double *const *lin, hipStream_t st);

// One set of launches in the making (StokesSetBuilder, stfem_stokes_set.h), bound to stokes_launch on a context and a stream.
// mode: STFEM_CONVECTION_*, what follows the launches of the linear operator.
auto stokes_set_builder(stfem_stokes_ctx *c, hipStream_t st, int mode = STFEM_CONVECTION_NONE)
{
  return StokesSetBuilder([=](const StokesSet &set, const double *const *lin) { return stokes_launch(c, set, mode, lin, st); });
}

// The Kronecker path of stokes_launch (axis-aligned uniform meshes, see stfem_stokes_coupling.hip): the same arguments, three steps.
int stokes_cart_launch(stfem_stokes_ctx *c, const StokesSet &set, hipStream_t st)
{
  const int nsrc = set.nsrc, nout = set.nout;
  if (nsrc < 1 || nsrc > MAXSRC || nout > MAXOUT) return STFEM_ERR_UNSUPPORTED;
  // ---- the coupling, in gather form: parameters
  CouplingParams k = c->coupling;
  k.nsrc = nsrc; k.nout = nout;
  for (int q = 0; q < nsrc; ++q) { k.u[q] = set.us[q]; k.p[q] = set.ps[q]; }
  bool k_u = false, any_p = false; // (any_p: a destination that is overwritten is written even with zero weights)
  int n_store_u = 0, n_add_u = 0;
  for (int o = 0; o < nout; ++o) {
    k.out_u[o] = set.out_u[o]; k.out_p[o] = set.out_p[o];
    k.store_p[o] = set.store_p[o];
    if (set.out_u[o]) (set.store_u[o] ? n_store_u : n_add_u)++;
    any_p = any_p || set.out_p[o];
    for (int q = 0; q < nsrc; ++q) {
      k.wKu[o][q] = set.ps[q] ? set.wKu[q][o] : 0.0;
      k.wKp[o][q] = set.wKp[q][o];
      k_u = k_u || (set.out_u[o] && k.wKu[o][q] != 0.0);
    }
  }
  stfem_launch_begin();
  // ---- 2. out_p (=, +=) sum_q wKp B u_q, beside the velocity sweep (STFEM_STOKES_SERIAL=1: on the caller's stream, after it)
  static const bool serial = [] { const char *e = getenv("STFEM_STOKES_SERIAL"); return e && atoi(e) != 0; }();
  // The fork onto the side stream - ONE per device, shared by every Stokes context: with a stream per context (a multigrid has one
  // context per level) the streams outnumbered the hardware queues, and the multigrid-preconditioned solve ran three times slower
  // than on one stream (profiles/r3/experiments.txt Z: 64^3 cells, 47 against 16 ms per FGMRES iteration).  No fork where the
  // gradient term rides in the sweep: that sweep leaves no registers for a second kernel on the CU.
  // STFEM_STOKES_FORK_MIN_CELLS=<n>: fork on meshes of at least n cells only (measurements).
  static const long long fork_min_cells = [] {
    const char *e = getenv("STFEM_STOKES_FORK_MIN_CELLS");
    return e ? atoll(e) : 0ll;
  }();
  // One time dof, FE_Q(1) pressure, the only velocity destination overwritten: the sweep adds - wKu B^T p to what it stores
  // (SweepParams::gp) and the gradient kernel of step 3 is not needed (it read and wrote the whole velocity destination again).  With
  // any further velocity destination the gradient kernel serves them all.  STFEM_STOKES_GRAD_KERNEL=1: always the gradient kernel.
  static const bool unfused_grad = [] { const char *e = getenv("STFEM_STOKES_GRAD_KERNEL"); return e && atoi(e) != 0; }();
  const bool grad_in_sweep = nsrc == 1 && n_store_u == 1 && n_add_u == 0 && !c->pspace && k_u && !unfused_grad;
  const bool forked = any_p && !serial && c->side && !grad_in_sweep && (long long)k.ncx * k.ncy * k.ncz >= fork_min_cells;
  // (the fork point is here, before the sweep; the side stream's commands are enqueued after the sweep's so that the sweep's
  // persistent workgroups - exactly the resident number - are placed first and the divergence kernel fills what is left)
  if (forked) STFEM_TRY(hipEventRecord(c->ev_fork, st));
  bool grad_done = false; // (a sweep that has no gradient hook leaves the term to step 3)
  // ---- 1. velocity blocks: out_u[o] (=, +=) sum_q (nu wKu K + wM M) u_q, component by component as scalar FE_Q(2) systems
  // (one launch with the three components as blocks when there is a single source and destination)
  for (int pass = 0; pass < 2; ++pass) { // destinations that are overwritten, then those that are accumulated into
    int rows[MAXOUT], nr = 0;
    for (int o = 0; o < nout; ++o)
      if (set.out_u[o] && (set.store_u[o] != 0) == (pass == 0)) rows[nr++] = o;
    if (nr == 0) continue;
    const int ncomp_blocks = (nr == 1 && nsrc == 1) ? 3 : 1; // components as blocks of one launch, or one launch per component
    for (int c0 = 0; c0 < 3; c0 += ncomp_blocks) {
      const int nbo = nr * ncomp_blocks, nbi = nsrc * ncomp_blocks;
      std::vector<void *> dptr(nbo), sptr(nbi);
      std::vector<double> a(size_t(nbo) * nbi, 0.0), b(size_t(nbo) * nbi, 0.0);
      for (int cc = 0; cc < ncomp_blocks; ++cc) {
        for (int r = 0; r < nr; ++r) dptr[cc * nr + r] = set.out_u[rows[r]] + (c0 + cc) * c->Nu;
        for (int q = 0; q < nsrc; ++q) sptr[cc * nsrc + q] = const_cast<double *>(set.us[q]) + (c0 + cc) * c->Nu;
        for (int r = 0; r < nr; ++r)
          for (int q = 0; q < nsrc; ++q) {
            a[size_t(cc * nr + r) * nbi + cc * nsrc + q] = c->nu * set.wKu[q][rows[r]];
            b[size_t(cc * nr + r) * nbi + cc * nsrc + q] = set.wM[q][rows[r]];
          }
      }
      stfem_vec *vd = nullptr, *vs = nullptr;
      int rc = stfem_vector_wrap(c->scalar, nbo, dptr.data(), &vd);
      if (rc == STFEM_OK) rc = stfem_vector_wrap(c->scalar, nbi, sptr.data(), &vs);
      if (grad_in_sweep && rc == STFEM_OK) {
        double w[3][2][3][2];
        for (int d = 0; d < 3; ++d)
          for (int a3 = 0; a3 < 3; ++a3)
            for (int j = 0; j < 2; ++j) {
              w[d][0][a3][j] = c->coupling.C[a3][j];
              w[d][1][a3][j] = c->coupling.h[d] * c->coupling.N[a3][j];
            }
        rc = stfem_internal_set_gradient(c->scalar, set.ps[0], w, -set.wKu[0][rows[0]]);
      }
      if (rc == STFEM_OK) rc = stfem_st_vmult(c->scalar, nbo, nbi, a.data(), b.data(), 0, pass, vd, vs, st);
      if (grad_in_sweep) {
        grad_done = rc == STFEM_OK && c->scalar->grad_applied;
        (void)stfem_internal_set_gradient(c->scalar, nullptr, nullptr, 0.0);
      }
      if (vd) stfem_vector_destroy(vd);
      if (vs) stfem_vector_destroy(vs);
      if (rc != STFEM_OK) return stfem_set_error(rc, "velocity sweep: status %d (%s)", rc, stfem_last_error());
    }
  }
  if (forked) {
    STFEM_TRY(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    stokes_div_launch(k, c->Np, c->side);
    STFEM_TRY(hipEventRecord(c->ev_join, c->side));
  }
  // ---- 3. out_u -= sum_q wKu B^T p_q
  c->last_grad_in_sweep = grad_done;
  if (k_u && !grad_done) stokes_grad_launch(k, st);
  if (forked) STFEM_TRY(hipStreamWaitEvent(st, c->ev_join, 0));
  else if (any_p) stokes_div_launch(k, c->Np, st);
  return stfem_launch_end("stokes coupling kernels");
}

// In this fixed order: the linear part (Kronecker path or cell kernel), its boundary launches, then - with a convection mode - the
// convection colours 0..7 and the inflow colours (stfem_stokes_convection.hip), which add to what the linear part has written, then -
// with delta0 != 0 - the CIP colours 0..7 (stfem_stokes_cip.hip).
int stokes_launch(stfem_stokes_ctx *c, const StokesSet &set, int mode, const double *const *lin, hipStream_t st)
{
  // axis-aligned uniform mesh at degree 2: the Kronecker path; otherwise the cell kernel.  (A context of degree 3 has no scalar
  // context - its entry point is kept to degree 2: the cell operator, its boundary launches when
  // stfem_stokes_set_weak_boundaries_space has set weak faces, then the convection colours - never both, stokes_refuse_inflow_q3 -,
  // then the CIP colours when stfem_stokes_set_cip_space has set delta0)
  assert(c->degree == 2 || (!c->scalar && (!c->weak_mask || mode == STFEM_CONVECTION_NONE)));
  const int rc = c->scalar ? stokes_cart_launch(c, set, st) : stokes_cell_launch(c, set, st);
  if (rc != STFEM_OK) return rc;
  // LoopType::Full: the boundary-face loop of the same vmult (the mass operator has none)
  bool k_part = false;
  for (int o = 0; o < set.nout; ++o)
    for (int q = 0; q < set.nsrc; ++q) k_part = k_part || set.wKu[q][o] != 0.0 || set.wKp[q][o] != 0.0;
  if (c->weak_mask && k_part) {
    const int rb = stokes_boundary_launch(c, set, nullptr, st);
    if (rb != STFEM_OK) return rb;
  }
  if (mode != STFEM_CONVECTION_NONE) {
    const int rv = stokes_convection_launch(c, set, lin, mode, st);
    if (rv != STFEM_OK) return rv;
  }
  if (c->cip_delta0 != 0.0) { // last: the CIP interior faces (stfem_stokes_set_cip); without it exactly the launches above
    const double *w[MAXSRC];
    const bool from_lin = c->cip_weight == STFEM_CIP_WEIGHT_LINEARISATION && mode != STFEM_CONVECTION_NONE;
    for (int s = 0; s < set.nsrc; ++s) w[s] = from_lin && lin[s] ? lin[s] : set.us[s];
    return stokes_cip_launch(c, set, w, c->cip_delta0, st);
  }
  return STFEM_OK;
}

// BlockSlice::index, fe_time.h:956-967
int block_index(int nt, int variable_major, int it, int v, int d) { return variable_major ? it * (2 * nt) + v * nt + d : it * (2 * nt) + d * 2 + v; }

// The three entries that take a convection mode, in the form behind both their names: require_q2 - the entry of stfem.h, which refuses
// a mode on a context of degree 3 (stokes_require_q2); otherwise the _space entry of stfem_stokes_convection_space.h, which runs it.
int stokes_vmult_convection(stfem_stokes_ctx *c, int mode, double *dst_u, double *dst_p, const double *src_u, const double *src_p,
                            const double *lin_u, void *stream, bool require_q2)
{
  if (!c || !dst_u || !dst_p || !src_u || !src_p) return STFEM_ERR_INVALID_ARGUMENT;
  if (mode < STFEM_CONVECTION_NONE || mode > STFEM_CONVECTION_JACOBIAN || (mode != STFEM_CONVECTION_NONE && !lin_u))
    return STFEM_ERR_INVALID_ARGUMENT;
  if (dst_u == src_u || dst_p == src_p) return STFEM_ERR_ALIAS;
  if (mode != STFEM_CONVECTION_NONE && (lin_u == dst_u || lin_u == dst_p)) return STFEM_ERR_ALIAS;
  if (mode != STFEM_CONVECTION_NONE && require_q2)
    if (const int rq = stokes_require_q2(c, "stfem_stokes_vmult_convection with a convection mode")) return rq;
  if (mode != STFEM_CONVECTION_NONE)
    if (const int rq = stokes_refuse_inflow_q3(c, "stfem_stokes_vmult_convection_space with a convection mode")) return rq;
  if (const int rg = stokes_cip_source_ready(c, src_u)) return rg;
  STFEM_TRY(hipSetDevice(c->device));
  auto launch = stokes_set_builder(c, static_cast<hipStream_t>(stream), mode);
  launch.add_source(src_u, src_p, lin_u);
  const double one = 1.0, zero = 0.0;
  char written[2] = {0, 0}; // dst is overwritten
  const int rc = launch.add_destination(dst_u, dst_p, &one, &one, &zero, &written[0], &written[1]);
  return rc != STFEM_OK ? rc : launch.flush();
}

int stokes_st_vmult_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                               const double *Alpha, const double *Beta, double *const *dst_blocks, const double *const *src_blocks,
                               const double *const *lin_blocks, void *stream, bool require_q2);
int stokes_st_vmult_slice_add_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                                         const double *Gamma, const double *Zeta, double *const *dst_blocks, const double *src_u,
                                         const double *src_p, const double *lin_u, void *stream, bool require_q2);

} // namespace

extern "C" {

int stfem_stokes_vmult(stfem_stokes_ctx *c, double *dst_u, double *dst_p, const double *src_u,
                       const double *src_p, void *stream)
{
  return stfem_stokes_vmult_convection(c, STFEM_CONVECTION_NONE, dst_u, dst_p, src_u, src_p, nullptr, stream);
}

int stfem_stokes_vmult_convection(stfem_stokes_ctx *c, int mode, double *dst_u, double *dst_p, const double *src_u,
                                  const double *src_p, const double *lin_u, void *stream)
{
  return stokes_vmult_convection(c, mode, dst_u, dst_p, src_u, src_p, lin_u, stream, true);
}

int stfem_stokes_vmult_convection_space(stfem_stokes_ctx *c, int mode, double *dst_u, double *dst_p, const double *src_u,
                                        const double *src_p, const double *lin_u, void *stream)
{
  return stokes_vmult_convection(c, mode, dst_u, dst_p, src_u, src_p, lin_u, stream, false);
}

int stfem_stokes_mass_vmult(stfem_stokes_ctx *c, double *dst_u, const double *src_u, void *stream)
{
  if (!c || !dst_u || !src_u) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst_u == src_u) return STFEM_ERR_ALIAS;
  STFEM_TRY(hipSetDevice(c->device));
  auto launch = stokes_set_builder(c, static_cast<hipStream_t>(stream));
  launch.add_source(src_u, nullptr);
  const double one = 1.0, zero = 0.0;
  char written = 0; // dst is overwritten
  const int rc = launch.add_destination(dst_u, nullptr, &zero, &zero, &one, &written, nullptr);
  return rc != STFEM_OK ? rc : launch.flush();
}

int stfem_stokes_st_vmult(stfem_stokes_ctx *c, int n_timesteps_at_once, int n_timedofs, int variable_major,
                          const double *Alpha, const double *Beta, double *const *dst_blocks,
                          const double *const *src_blocks, void *stream)
{
  return stfem_stokes_st_vmult_convection(c, STFEM_CONVECTION_NONE, n_timesteps_at_once, n_timedofs, variable_major, Alpha, Beta,
                                          dst_blocks, src_blocks, nullptr, stream);
}

int stfem_stokes_st_vmult_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                                     const double *Alpha, const double *Beta, double *const *dst_blocks,
                                     const double *const *src_blocks, const double *const *lin_blocks, void *stream)
{
  return stokes_st_vmult_convection(c, mode, n_timesteps_at_once, n_timedofs, variable_major, Alpha, Beta, dst_blocks, src_blocks, lin_blocks,
                                    stream, true);
}

int stfem_stokes_st_vmult_convection_space(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                                           const double *Alpha, const double *Beta, double *const *dst_blocks,
                                           const double *const *src_blocks, const double *const *lin_blocks, void *stream)
{
  return stokes_st_vmult_convection(c, mode, n_timesteps_at_once, n_timedofs, variable_major, Alpha, Beta, dst_blocks, src_blocks, lin_blocks,
                                    stream, false);
}

} // extern "C"

namespace {

int stokes_st_vmult_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                               const double *Alpha, const double *Beta, double *const *dst_blocks, const double *const *src_blocks,
                               const double *const *lin_blocks, void *stream, bool require_q2)
{
  if (!c || !Alpha || !Beta || !dst_blocks || !src_blocks || n_timesteps_at_once < 1 || n_timedofs < 1)
    return STFEM_ERR_INVALID_ARGUMENT;
  if (mode < STFEM_CONVECTION_NONE || mode > STFEM_CONVECTION_JACOBIAN || (mode != STFEM_CONVECTION_NONE && !lin_blocks))
    return STFEM_ERR_INVALID_ARGUMENT;
  const bool navier = mode != STFEM_CONVECTION_NONE;
  const int nt = n_timedofs, ns = n_timesteps_at_once, nb = 2 * nt * ns;
  auto index = [&](int it, int v, int d) { return block_index(nt, variable_major, it, v, d); };
  if (navier)
    for (int it = 0; it < ns; ++it)
      for (int d = 0; d < nt; ++d)
        if (!lin_blocks[index(it, 0, d)]) return STFEM_ERR_INVALID_ARGUMENT; // (only the velocity entries are read)
  for (int j = 0; j < nb; ++j) {
    if (!dst_blocks[j] || !src_blocks[j]) return STFEM_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < nb; ++i)
      if (dst_blocks[j] == src_blocks[i]) return STFEM_ERR_ALIAS;
  }
  if (navier)
    for (int j = 0; j < nb; ++j)
      for (int it = 0; it < ns; ++it)
        for (int d = 0; d < nt; ++d)
          if (dst_blocks[j] == lin_blocks[index(it, 0, d)]) return STFEM_ERR_ALIAS;
  if (navier && require_q2)
    if (const int rq = stokes_require_q2(c, "stfem_stokes_st_vmult_convection with a convection mode")) return rq;
  if (navier)
    if (const int rq = stokes_refuse_inflow_q3(c, "stfem_stokes_st_vmult_convection_space with a convection mode")) return rq;
  for (int it = 0; it < ns; ++it)
    for (int d = 0; d < nt; ++d)
      if (const int rg = stokes_cip_source_ready(c, src_blocks[index(it, 0, d)])) return rg;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // dst = 0.0 (operators.h:833): the first launch that reaches a block overwrites it; blocks no launch
  // reaches are zeroed at the end
  std::vector<char> written(nb, 0);
  // up to MAXSRC time dofs: ONE set of launches - every cell is evaluated for all sources, the destinations are written once;
  // more (or STFEM_STOKES_FUSED=0): one set per source time dof
  static const bool fused_ok = [] {
    const char *e = getenv("STFEM_STOKES_FUSED");
    return !e || atoi(e) != 0;
  }();
  const int group = (fused_ok && ns * nt <= MAXSRC) ? ns * nt : 1;
  for (int s0 = 0; s0 < ns * nt; s0 += group) {
    auto launch = stokes_set_builder(c, st, mode);
    for (int s = s0; s < s0 + group; ++s)
      launch.add_source(src_blocks[index(s / nt, 0, s % nt)], src_blocks[index(s / nt, 1, s % nt)],
                        navier ? lin_blocks[index(s / nt, 0, s % nt)] : nullptr);
    for (int jt = 0; jt < ns; ++jt)
      for (int jd = 0; jd < nt; ++jd) {
        const int ju = index(jt, 0, jd), jp = index(jt, 1, jd);
        double aU[MAXSRC], aP[MAXSRC], bU[MAXSRC];
        for (int s = 0; s < group; ++s) {
          const int i = index((s0 + s) / nt, 0, (s0 + s) % nt); // the velocity column drives all scatters (operators.h:851-862)
          aU[s] = Alpha[size_t(ju) * nb + i]; aP[s] = Alpha[size_t(jp) * nb + i]; bU[s] = Beta[size_t(ju) * nb + i];
        }
        const int rc = launch.add_destination(dst_blocks[ju], dst_blocks[jp], aU, aP, bU, &written[ju], &written[jp]);
        if (rc != STFEM_OK) return rc;
      }
    const int rc = launch.flush();
    if (rc != STFEM_OK) return rc;
  }
  for (int it = 0; it < ns; ++it)
    for (int d = 0; d < nt; ++d) {
      if (!written[index(it, 0, d)]) STFEM_TRY(hipMemsetAsync(dst_blocks[index(it, 0, d)], 0, sizeof(double) * 3 * c->Nu, st));
      if (!written[index(it, 1, d)]) STFEM_TRY(hipMemsetAsync(dst_blocks[index(it, 1, d)], 0, sizeof(double) * c->Np, st));
    }
  return STFEM_OK;
}

} // namespace

extern "C" {

// SystemMatrixStokes::vmult_slice_add (operators.h:748-781): the n x 1 case used for the right-hand
// side: src = one (velocity, pressure) pair, dst[index(it,v,id)] += Gamma(index(it,v,id), 0) * (K_S src)_v
// and dst[index(it,0,id)] += Zeta(index(it,0,id), 0) * M u.  dst is NOT zeroed.
int stfem_stokes_st_vmult_slice_add(stfem_stokes_ctx *c, int n_timesteps_at_once, int n_timedofs, int variable_major,
                                    const double *Gamma, const double *Zeta, double *const *dst_blocks,
                                    const double *src_u, const double *src_p, void *stream)
{
  return stfem_stokes_st_vmult_slice_add_convection(c, STFEM_CONVECTION_NONE, n_timesteps_at_once, n_timedofs, variable_major, Gamma,
                                                    Zeta, dst_blocks, src_u, src_p, nullptr, stream);
}

int stfem_stokes_st_vmult_slice_add_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs,
                                               int variable_major, const double *Gamma, const double *Zeta,
                                               double *const *dst_blocks, const double *src_u, const double *src_p,
                                               const double *lin_u, void *stream)
{
  return stokes_st_vmult_slice_add_convection(c, mode, n_timesteps_at_once, n_timedofs, variable_major, Gamma, Zeta, dst_blocks, src_u, src_p,
                                              lin_u, stream, true);
}

int stfem_stokes_st_vmult_slice_add_convection_space(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs,
                                                     int variable_major, const double *Gamma, const double *Zeta,
                                                     double *const *dst_blocks, const double *src_u, const double *src_p,
                                                     const double *lin_u, void *stream)
{
  return stokes_st_vmult_slice_add_convection(c, mode, n_timesteps_at_once, n_timedofs, variable_major, Gamma, Zeta, dst_blocks, src_u, src_p,
                                              lin_u, stream, false);
}

} // extern "C"

namespace {

int stokes_st_vmult_slice_add_convection(stfem_stokes_ctx *c, int mode, int n_timesteps_at_once, int n_timedofs, int variable_major,
                                         const double *Gamma, const double *Zeta, double *const *dst_blocks, const double *src_u,
                                         const double *src_p, const double *lin_u, void *stream, bool require_q2)
{
  if (!c || !Gamma || !Zeta || !dst_blocks || !src_u || !src_p || n_timesteps_at_once < 1 || n_timedofs < 1)
    return STFEM_ERR_INVALID_ARGUMENT;
  if (mode < STFEM_CONVECTION_NONE || mode > STFEM_CONVECTION_JACOBIAN || (mode != STFEM_CONVECTION_NONE && !lin_u))
    return STFEM_ERR_INVALID_ARGUMENT;
  const int nt = n_timedofs, ns = n_timesteps_at_once, nb = 2 * nt * ns;
  for (int j = 0; j < nb; ++j) {
    if (!dst_blocks[j]) return STFEM_ERR_INVALID_ARGUMENT;
    if (dst_blocks[j] == src_u || dst_blocks[j] == src_p) return STFEM_ERR_ALIAS;
    if (mode != STFEM_CONVECTION_NONE && dst_blocks[j] == lin_u) return STFEM_ERR_ALIAS;
  }
  if (mode != STFEM_CONVECTION_NONE && require_q2)
    if (const int rq = stokes_require_q2(c, "stfem_stokes_st_vmult_slice_add_convection with a convection mode")) return rq;
  if (mode != STFEM_CONVECTION_NONE)
    if (const int rq = stokes_refuse_inflow_q3(c, "stfem_stokes_st_vmult_slice_add_convection_space with a convection mode")) return rq;
  if (const int rg = stokes_cip_source_ready(c, src_u)) return rg;
  STFEM_TRY(hipSetDevice(c->device));
  auto launch = stokes_set_builder(c, static_cast<hipStream_t>(stream), mode);
  launch.add_source(src_u, src_p, lin_u);
  for (int it = 0; it < ns; ++it)
    for (int id = 0; id < nt; ++id) {
      const int ju = block_index(nt, variable_major, it, 0, id), jp = block_index(nt, variable_major, it, 1, id);
      const int rc = launch.add_destination(dst_blocks[ju], dst_blocks[jp], &Gamma[ju], &Gamma[jp], &Zeta[ju], nullptr, nullptr);
      if (rc != STFEM_OK) return rc;
    }
  return launch.flush();
}

} // namespace
