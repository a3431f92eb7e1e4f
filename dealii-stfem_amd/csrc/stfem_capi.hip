// C-ABI of the MI355X space-time operator apply (see include/stfem.h): the context, the sweep planner and launcher,
// the metric of the general path and the diagonals.  Vectors: stfem_vector.hip; entry points without a device: stfem_host_helpers.cpp.
// (The entry points have C linkage through their declarations in the header.)
#include "stfem_internal.h"
#include "stfem_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#define STFEM_NS f64
#include "stfem_prec_decl.h"
#undef STFEM_NS
#define STFEM_NS f32
#include "stfem_prec_decl.h"
#undef STFEM_NS

using namespace stfem;

// the precision traits of the context's Number type T (stfem_by_prec)
template <class T> using PrecOf = std::conditional_t<std::is_same<T, float>::value, f32::Prec, f64::Prec>;

// The geometry of a new context: a box given by its extents, or a vertex grid, in which an axis-aligned uniform box is
// recognised (deal.II compresses such cells as "Cartesian").
static int set_geometry(stfem_ctx *c, const stfem_mesh_desc *mesh)
{
  if (!mesh->vertices) {
    c->cartesian = true;
    for (int d = 0; d < 3; ++d) {
      c->lower[d] = mesh->lower[d];
      c->h[d] = (mesh->upper[d] - mesh->lower[d]) / c->nc[d];
      if (!(c->h[d] > 0)) return STFEM_ERR_INVALID_ARGUMENT;
    }
    return STFEM_OK;
  }
  const int64_t nvx = c->nc[0] + 1, nvy = c->nc[1] + 1, nvz = c->nc[2] + 1;
  const int64_t nv = nvx * nvy * nvz;
  const double *v = mesh->vertices;
  double lo[3], up[3];
  for (int d = 0; d < 3; ++d) {
    lo[d] = v[d];
    up[d] = v[3 * (nv - 1) + d];
    c->lower[d] = lo[d];
    c->h[d] = (up[d] - lo[d]) / c->nc[d];
  }
  bool cart = c->h[0] > 0 && c->h[1] > 0 && c->h[2] > 0;
  const double tol = 1e-13 * std::max({std::abs(up[0] - lo[0]), std::abs(up[1] - lo[1]),
                                       std::abs(up[2] - lo[2]), 1e-300});
  for (int64_t k = 0, o = 0; k < nvz && cart; ++k)
    for (int64_t j = 0; j < nvy && cart; ++j)
      for (int64_t i = 0; i < nvx; ++i, ++o) {
        if (std::abs(v[3 * o] - (lo[0] + c->h[0] * i)) > tol ||
            std::abs(v[3 * o + 1] - (lo[1] + c->h[1] * j)) > tol ||
            std::abs(v[3 * o + 2] - (lo[2] + c->h[2] * k)) > tol) {
          cart = false;
          break;
        }
      }
  c->cartesian = cart;
  c->vertices.assign(v, v + 3 * nv);
  return STFEM_OK;
}

// tuning / experiment switches (STFEM_* environment variables), read once per context
static void read_switches(stfem_ctx *c)
{
  if (const char *v = getenv("STFEM_VARIANT")) c->variant = std::string(v) == "atomic" ? 1 : (std::string(v) == "tile" ? 2 : 0);
  auto env_int = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
  c->env_tile_lz = env_int("STFEM_TILE_LZ", 0);
  c->env_exp = env_int("STFEM_EXP", 0);
  c->env_stagger = env_int("STFEM_STAGGER", 0);
  c->env_stagger_div = std::max(1, env_int("STFEM_STAGGER_DIV", 256));
  c->env_pencil_ty = env_int("STFEM_PENCIL_TY", 0);
  c->env_pencil_lz = env_int("STFEM_PENCIL_LZ", 0);
  c->env_timeline = getenv("STFEM_TIMELINE");
}

const char *stfem_strerror(int s)
{
  switch (s) {
    case STFEM_OK: return "ok";
    case STFEM_ERR_INVALID_ARGUMENT: return "invalid argument";
    case STFEM_ERR_UNSUPPORTED: return "unsupported degree / block count / mesh mode";
    case STFEM_ERR_HIP: return "HIP runtime error";
    case STFEM_ERR_NO_DEVICE: return "no HIP device";
    case STFEM_ERR_SHAPE_MISMATCH: return "block count or size mismatch";
    case STFEM_ERR_ALIAS: return "dst aliases src";
    case STFEM_ERR_OUT_OF_MEMORY: return "out of memory";
    case STFEM_ERR_COMM: return "RCCL error";
    default: return "unknown status";
  }
}

int stfem_ctx_create(const stfem_mesh_desc *mesh, const stfem_space_desc *space, stfem_ctx **out)
{
  if (!mesh || !space || !out) return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (space->degree < 1 || space->degree > 5) return STFEM_ERR_UNSUPPORTED;
  if (space->n_q_points_1d != space->degree + 1 || space->n_components != 1) return STFEM_ERR_UNSUPPORTED;
  if (space->precision != 0 && space->precision != 1) return STFEM_ERR_UNSUPPORTED;
  for (int d = 0; d < 3; ++d)
    if (mesh->ncell[d] < 1) return STFEM_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return STFEM_ERR_NO_DEVICE;
  if (mesh->device < 0 || mesh->device >= ndev) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(mesh->device));
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, mesh->device) != hipSuccess) n_cu = 0;

  stfem_ctx *c = new (std::nothrow) stfem_ctx;
  if (!c) return STFEM_ERR_OUT_OF_MEMORY;
  c->p = space->degree;
  c->prec = space->precision;
  c->es = c->prec ? sizeof(float) : sizeof(double);
  c->device = mesh->device;
  c->n_cu = n_cu;
  c->ndofs = c->ncells = 1;
  for (int d = 0; d < 3; ++d) {
    c->nc[d] = mesh->ncell[d];
    c->nd[d] = c->p * c->nc[d] + 1;
    c->ndofs *= c->nd[d];
    c->ncells *= c->nc[d];
  }
  c->dmask = mesh->dirichlet_mask & 63;
  int rc = STFEM_OK;
  try {
    c->tab = make_shape_tables(c->p);
  } catch (...) {
    rc = STFEM_ERR_INVALID_ARGUMENT;
  }
  if (rc == STFEM_OK) rc = set_geometry(c, mesh);
  read_switches(c);
  if (rc == STFEM_OK && hipMalloc(&c->d_scratch, sizeof(double) * SCRATCH_DOUBLES) != hipSuccess) rc = STFEM_ERR_OUT_OF_MEMORY;
  if (rc != STFEM_OK) {
    delete c;
    return rc;
  }
  *out = c;
  return STFEM_OK;
}

void stfem_ctx_destroy(stfem_ctx *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (void *&p : c->d_coef)
    if (p) (void)hipFree(p);
  if (c->d_scratch) (void)hipFree(c->d_scratch);
  if (c->d_halo) (void)hipFree(c->d_halo);
  if (c->d_vertices) (void)hipFree(c->d_vertices);
  if (c->d_rule) (void)hipFree(c->d_rule);
  if (c->d_metric) (void)hipFree(c->d_metric);
  if (c->d_timeline) (void)hipFree(c->d_timeline);
  if (c->d_work) (void)hipFree(c->d_work);
  delete c;
}

int64_t stfem_n_dofs(const stfem_ctx *c) { return c ? c->ndofs : 0; }
int64_t stfem_n_cells(const stfem_ctx *c) { return c ? c->ncells : 0; }
int stfem_n_dofs_1d(const stfem_ctx *c, int32_t nd[3])
{
  if (!c || !nd) return STFEM_ERR_INVALID_ARGUMENT;
  for (int d = 0; d < 3; ++d) nd[d] = c->nd[d];
  return STFEM_OK;
}
int stfem_is_cartesian(const stfem_ctx *c) { return c && c->cartesian ? 1 : 0; }
int stfem_ctx_precision(const stfem_ctx *c) { return c ? c->prec : -1; }
const char *stfem_last_kernel_name(const stfem_ctx *c) { return c ? c->last_kernel : ""; }
int stfem_last_sweep_plan(const stfem_ctx *c, int32_t out[2])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  out[0] = c->last_sweep[0];
  out[1] = c->last_sweep[1];
  return STFEM_OK;
}
int stfem_last_tile_plan(const stfem_ctx *c, int32_t out[4])
{
  if (!c || !out) return STFEM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 4; ++i) out[i] = c->last_tile[i];
  return STFEM_OK;
}

int stfem_set_coefficient(stfem_ctx *c, int which, int layout, const double *host)
{
  if (!c || which < 0 || which > 1 || layout < 0 || layout > 2) return STFEM_ERR_INVALID_ARGUMENT;
  STFEM_TRY(hipSetDevice(c->device));
  if (c->d_coef[which]) {
    STFEM_TRY(hipFree(c->d_coef[which]));
    c->d_coef[which] = nullptr;
  }
  c->coef_layout[which] = 0;
  c->metric_valid = false;
  if (layout == 0) return STFEM_OK;
  if (!host) return STFEM_ERR_INVALID_ARGUMENT;
  const int nq = c->p + 1;
  const size_t n = size_t(c->ncells) * (layout == 2 ? size_t(nq) * nq * nq : 1);
  if (hipMalloc(&c->d_coef[which], n * c->es) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
  if (c->prec) {
    std::vector<float> tmp(host, host + n);
    STFEM_TRY(hipMemcpy(c->d_coef[which], tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
  } else {
    STFEM_TRY(hipMemcpy(c->d_coef[which], host, n * sizeof(double), hipMemcpyHostToDevice));
  }
  c->coef_layout[which] = layout;
  return STFEM_OK;
}

// ------------------------------------------------------------------------------------ operator

// general path: non-Cartesian cells or per-quadrature-point coefficients -> metric terms
static bool is_general(const stfem_ctx *c) { return !c->cartesian || c->coef_layout[0] == 2 || c->coef_layout[1] == 2; }

// operators.h:1152-1162: a term (which = 0 mass, 1 laplace) is present iff its scaling != 0; a coefficient table, if any,
// replaces the scaling
struct Scaling { double value; bool coef; };
static Scaling effective_scaling(const stfem_ctx *c, int which, double s)
{
  const bool coef = s != 0.0 && c->coef_layout[which] != 0;
  return {s != 0.0 ? (coef ? 1.0 : s) : 0.0, coef};
}

// cell volume and inverse squared mesh widths of the Cartesian path (SweepParams, DiagParams)
template <class P> static void fill_cell_scales(const stfem_ctx *c, P &prm)
{
  using real = decltype(prm.vol);
  prm.vol = real(c->h[0] * c->h[1] * c->h[2]);
  prm.ihx2 = real(1.0 / (c->h[0] * c->h[0]));
  prm.ihy2 = real(1.0 / (c->h[1] * c->h[1]));
  prm.ihz2 = real(1.0 / (c->h[2] * c->h[2]));
}

template <class PR> static void fill_common(const stfem_ctx *c, typename PR::Sweep &prm)
{
  using real = typename PR::real;
  std::memset(&prm, 0, sizeof(prm));
  prm.ncx = c->nc[0]; prm.ncy = c->nc[1]; prm.ncz = c->nc[2];
  prm.nx = c->nd[0]; prm.ny = c->nd[1]; prm.nz = c->nd[2];
  prm.ncells = c->ncells;
  prm.dmask = c->dmask;
  fill_cell_scales(c, prm);
  const int ne = eo_size(c->p + 1);
  for (int i = 0; i < ne; ++i) {
    prm.eo_Si[i] = real(c->tab.eo_Si[i]);
    prm.eo_L[i] = real(c->tab.eo_L[i]);
    prm.eo_S[i] = real(c->tab.eo_S[i]);
    prm.eo_Dq[i] = real(c->tab.eo_Dq[i]);
    prm.eo_DqT[i] = real(c->tab.eo_DqT[i]);
  }
  for (int i = 0; i < EO_N; ++i) {
    prm.fd_W[i] = real(c->tab.fd_W[i]);
    prm.fd_Mx[i] = real(c->tab.fd_M1[i]);
    prm.fd_Kx[i] = real(c->tab.fd_K1[i] / (c->h[0] * c->h[0]));
  }
  for (int i = 0; i < 8; ++i) {
    prm.fd_lx[i] = real(c->tab.fd_lam[i] / (c->h[0] * c->h[0]));
    prm.fd_ly[i] = real(c->tab.fd_lam[i] / (c->h[1] * c->h[1]));
    prm.fd_lz[i] = real(c->tab.fd_lam[i] / (c->h[2] * c->h[2]));
  }
}

// Chooses the z-chunking of the tile variant.  One colour launch has columns x ntc workgroups of
// ceil(ncz / ntc) layers (+ about one layer of start-up) that run in rounds of `slots` resident
// workgroups (`resident` per CU: what the runtime reports for the kernel, 2 if unknown); what
// matters is that the last round is full.  Fewer chunks win ties (smaller z-halo).
template <class PL> static void plan_chunks(const stfem_ctx *c, PL &tp, int nbm, int resident)
{
  tp.ntx = (c->nc[0] + tp.cw - 1) / tp.cw;
  tp.nty = (c->nc[1] + tp.rows - 1) / tp.rows;
  const int ncz = c->nc[2];
  int ntc = 1;
  if (c->env_tile_lz > 0) {
    const int lz = std::max(1, std::min(ncz, c->env_tile_lz));
    ntc = (ncz + lz - 1) / lz;
  } else {
    (void)nbm;
    const int wpc = std::max(2, resident); // (planning one-per-CU kernels in rounds of 256 measured 5 % slower)
    const int64_t slots = int64_t(c->n_cu > 0 ? c->n_cu : 256) * wpc;
    const int64_t columns = int64_t((tp.ntx + 1) / 2) * tp.nty; // of the larger colour
    double best = 1e300;
    for (int n = 1; n <= ncz; ++n) {
      const int64_t rounds = (columns * n + slots - 1) / slots;
      const double cost = double(rounds) * ((ncz + n - 1) / n + 1.0) * (1.0 + 1e-3 * n);
      if (cost < best) { best = cost; ntc = n; }
    }
  }
  tp.ntc = ntc;
  tp.lz = (ncz + ntc - 1) / ntc; // longest chunk
  tp.zp = c->p * tp.lz + 1;
}

// Chooses the decomposition of the pencil variant: pencils of cpw x ty cells, four of them stacked
// in y per workgroup, z-chunks such that the last round of resident workgroups (two per CU) is full.
template <class PL> static void plan_pencil(const stfem_ctx *c, PL &pp)
{
  pp.ntx = (c->nc[0] + pp.cpw - 2) / (pp.cpw - 1); // cpw - 1 owned cells per pencil
  const int cyw = pp.ty * 4;
  pp.ntyw = (c->nc[1] + cyw - 1) / cyw;
  const int ncz = c->nc[2];
  // z-chunks: B layers each (z-halo = 1 / (4 B) of the planes), tapering off towards the end of
  // the tile list: tiles are pulled at run time in the order of their numbers, and all tiles of one
  // size take the same time, so equal chunks would leave the last round of the resident workgroups
  // mostly empty (measured: 400 of 512 slots busy on average with 12 equal chunks on cfg 1)
  int B = c->env_pencil_lz > 0 ? c->env_pencil_lz : 8;
  B = std::max(B, (ncz + 47) / 48); // at most 64 chunks
  int n = 0, r = ncz;
  pp.zb[0] = 0;
  while (r > 0) {
    const int sz = c->env_pencil_lz < 0 ? std::min(std::max(-c->env_pencil_lz, (ncz + 47) / 48), r) // (negative: equal chunks, experiments)
                                        : std::min(B, std::max(1, (r + 2) / 3));
    r -= sz;
    pp.zb[n + 1] = pp.zb[n] + sz;
    if (n == 62 && r > 0) { // (cannot happen for B >= ncz / 48; guards the table)
      pp.zb[n + 2] = ncz;
      n += 2;
      r = 0;
      break;
    }
    ++n;
  }
  pp.ntc = n;
  pp.lz = 0;
  for (int q = 0; q < n; ++q) pp.lz = std::max(pp.lz, pp.zb[q + 1] - pp.zb[q]);
  pp.zp = c->p * pp.lz + 1;
}

// (Re)builds the per-quadrature-point metric of the general path.  The coefficients in force
// (effective_scaling) are baked in; the flags record
// which of them were used so that a K-only / M-only apply with a different set rebuilds.
template <class PR> static int ensure_metric(stfem_ctx *c, bool use_lap, bool use_mass, hipStream_t st)
{
  using real = typename PR::real;
  const int n = c->p + 1;
  const size_t nm = size_t(c->ncells) * 8 * n * n * n;
  const int flags = (use_lap ? 1 : 0) | (use_mass ? 2 : 0);
  if (c->metric_valid && c->metric_flags == flags) return STFEM_OK;
  if (!c->d_vertices) {
    std::vector<double> v = c->vertices;
    if (v.empty()) { // Cartesian box given by extents
      v.resize(size_t(c->nc[0] + 1) * (c->nc[1] + 1) * (c->nc[2] + 1) * 3);
      size_t o = 0;
      for (int k = 0; k <= c->nc[2]; ++k)
        for (int j = 0; j <= c->nc[1]; ++j)
          for (int i = 0; i <= c->nc[0]; ++i, ++o) {
            v[3 * o] = c->lower[0] + c->h[0] * i;
            v[3 * o + 1] = c->lower[1] + c->h[1] * j;
            v[3 * o + 2] = c->lower[2] + c->h[2] * k;
          }
    }
    // (both uploads complete before the context sees either pointer: a failure half way must not
    // leave d_vertices set and d_rule missing, the next call would launch with a null rule)
    std::vector<double> rule(c->tab.xq);
    rule.insert(rule.end(), c->tab.wq.begin(), c->tab.wq.end());
    double *dv = nullptr, *dr = nullptr;
    if (hipMalloc(&dv, v.size() * sizeof(double)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    if (hipMalloc(&dr, rule.size() * sizeof(double)) != hipSuccess) {
      (void)hipFree(dv);
      return STFEM_ERR_OUT_OF_MEMORY;
    }
    hipError_t e = hipMemcpy(dv, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dr, rule.data(), rule.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dv);
      (void)hipFree(dr);
      return stfem_set_error(STFEM_ERR_HIP, "metric table upload: %s", hipGetErrorString(e));
    }
    c->d_vertices = dv;
    c->d_rule = dr;
  }
  if (!c->d_metric && hipMalloc(&c->d_metric, nm * sizeof(real)) != hipSuccess)
    return STFEM_ERR_OUT_OF_MEMORY;
  const int rc = PR::metric(c->p, c->nc, c->d_vertices, c->d_rule, c->d_rule + n,
                            use_lap ? static_cast<const real *>(c->d_coef[1]) : nullptr, use_lap ? c->coef_layout[1] : 0,
                            use_mass ? static_cast<const real *>(c->d_coef[0]) : nullptr, use_mass ? c->coef_layout[0] : 0,
                            static_cast<real *>(c->d_metric), st);
  if (rc != 0) return rc; // (launch_build_metric has recorded the reason)
  c->metric_valid = true;
  c->metric_flags = flags;
  return STFEM_OK;
}

// for the other translation units of the library (stfem_internal.h): the stored metric in the record layout,
// built with the coefficient tables in force (what K and M of a SystemMatrix see)
int stfem_internal_metric(stfem_ctx *c, const void **metric, void *stream)
{
  const bool lap = c->coef_layout[1] != 0, mass = c->coef_layout[0] != 0;
  const int rc = stfem_by_prec(c, [&](auto t) { return ensure_metric<PrecOf<decltype(t)>>(c, lap, mass, static_cast<hipStream_t>(stream)); });
  if (rc == STFEM_OK) *metric = c->d_metric;
  return rc;
}

int stfem_internal_set_gradient(stfem_ctx *c, const double *p, const double (*w)[2][3][2], double scale)
{
  if (!c) return STFEM_ERR_INVALID_ARGUMENT;
  c->grad_p = p;
  c->grad_scale = scale;
  c->grad_applied = false;
  if (p && w) std::memcpy(c->grad_w, w, sizeof(c->grad_w));
  return STFEM_OK;
}

// halo slabs are laid out for the block counts the sweeps are instantiated for (the kernels' round_nbm, stfem_core.h)
static int block_slots(int nbm) { return nbm <= 4 ? nbm : (nbm <= 6 ? 6 : 8); }

// The only place that (re)allocates the halo slabs: at least `elements` of the context's Number type.  The stream is
// drained first, a sweep still in flight may use the old array.
static int grow_halo(stfem_ctx *c, size_t elements, hipStream_t st)
{
  if (elements <= c->halo_doubles) return STFEM_OK;
  STFEM_TRY(hipStreamSynchronize(st));
  if (c->d_halo) STFEM_TRY(hipFree(c->d_halo));
  c->d_halo = nullptr;
  c->halo_doubles = 0;
  if (hipMalloc(&c->d_halo, elements * c->es) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
  c->halo_doubles = elements;
  return STFEM_OK;
}

// Diagnostic builds only (tools/build_pencil_exp.sh -DSTFEM_PENCIL_TIMELINE, tools/build_abl.sh -DSTFEM_TIMELINE): phase
// timestamps of the even-colour launch, dumped to the file named by STFEM_TIMELINE after every apply.  timeline_arm before
// the launch zeroes n slots and hands the array to the plan; timeline_dump after it writes the four extents and the slots.
static int timeline_arm(stfem_ctx *c, size_t n, long long **plan_timeline, hipStream_t st)
{
  if (!c->env_timeline) return STFEM_OK;
  if (c->tl_n < n) {
    if (c->d_timeline) STFEM_TRY(hipFree(c->d_timeline));
    c->d_timeline = nullptr;
    if (hipMalloc(&c->d_timeline, n * sizeof(long long)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    c->tl_n = n;
  }
  STFEM_TRY(hipMemsetAsync(c->d_timeline, 0, n * sizeof(long long), st));
  *plan_timeline = c->d_timeline;
  return STFEM_OK;
}
static int timeline_dump(stfem_ctx *c, size_t n, long long h0, long long h1, long long h2, long long h3, hipStream_t st)
{
  if (!c->env_timeline) return STFEM_OK;
  STFEM_TRY(hipStreamSynchronize(st));
  std::vector<long long> h(n);
  STFEM_TRY(hipMemcpy(h.data(), c->d_timeline, n * sizeof(long long), hipMemcpyDeviceToHost));
  if (FILE *f = fopen(c->env_timeline, "wb")) {
    const long long hdr[4] = {h0, h1, h2, h3};
    fwrite(hdr, sizeof(long long), 4, f);
    fwrite(h.data(), sizeof(long long), n, f);
    fclose(f);
  }
  return STFEM_OK;
}

// what a launch_*_panel returns for the status of its kernel launcher (stfem_kernels_decl.h), which has recorded the reason
// of a failed launch itself
static int launch_status(int rc) { return rc == STFEM_OK || rc == STFEM_ERR_HIP ? rc : STFEM_ERR_UNSUPPORTED; }

// Systems with more blocks than one launch takes are cut into panels (dst += for the later column panels).  On the
// pencil path a launch needs two cells per wave - Q4 with seven or eight blocks has one - so those systems
// are cut into equal panels of a size the pencil sweep has (Q4 x 8 blocks: 2 x 2 panels of four).
template <class PR> static int panel_size(const stfem_ctx *c, bool general, int nbo, int nbi)
{
  int panel = MAX_BLOCKS;
  if (c->variant == 0 && !general && c->p <= 4) { // (FE_Q(5) has no pencil sweep: the tile sweep takes up to MAX_BLOCKS blocks)
    const int need = std::min(MAX_BLOCKS, std::max(nbo, nbi));
    typename PR::PPlan probe;
    std::memset(&probe, 0, sizeof(probe));
    if (PR::pencil_geometry(c->p, need, 0, probe) != 0) {
      int maxp = need;
      while (maxp > 1 && PR::pencil_geometry(c->p, maxp, 0, probe) != 0) --maxp;
      const int parts = (need + maxp - 1) / maxp;
      panel = (need + parts - 1) / parts;
    }
  }
  return panel;
}

// one launch: tj destination x ti source blocks
struct Panel {
  int tj, ti;
  bool add;  // dst += (asked for, or not the first launch into this row panel)
  bool last; // the last column panel
};

template <class PR> static int launch_atomic_panel(stfem_ctx *c, const typename PR::Sweep &prm, hipStream_t st)
{
  const int rc = PR::atomic(c->p, prm, st);
  c->last_kernel = PR::atomic_name();
  c->last_sweep[0] = c->last_sweep[1] = 0;
  std::fill(c->last_tile, c->last_tile + 4, 0);
  return launch_status(rc);
}

// pp: what pencil_geometry filled for this panel
template <class PR>
static int launch_pencil_panel(stfem_ctx *c, typename PR::Sweep &prm, typename PR::PPlan &pp, const Panel &pn, hipStream_t st)
{
  using real = typename PR::real;
  plan_pencil(c, pp);
  const int nbm_r = block_slots(std::max(pn.tj, pn.ti));
  const size_t ntiles = size_t(pp.ntx) * pp.ntyw * pp.ntc;
  const size_t nyh = ntiles * nbm_r * pp.zp * pp.tX, nzh = ntiles * nbm_r * pp.tYW * pp.tX;
  int rc = grow_halo(c, nyh + nzh, st);
  if (rc != STFEM_OK) return rc;
  pp.yh = static_cast<real *>(c->d_halo);
  pp.zh = pp.yh + nyh;
  pp.add = pn.add ? 1 : 0;
  prm.gp = nullptr;
  if constexpr (sizeof(real) == 8) { // the Stokes gradient term rides in this launch (three FE_Q(2) blocks, dst = ..., no coefficient tables)
    if (c->grad_p && c->p == 2 && pn.tj == 3 && pn.ti == 3 && !pp.add && pn.last && !prm.coef_lap && !prm.coef_mass) {
      prm.gp = c->grad_p;
      prm.gscale = c->grad_scale;
      std::memcpy(prm.gw, c->grad_w, sizeof(prm.gw));
      c->grad_applied = true;
    }
  }
  if (!c->d_work) {
    if (hipMalloc(&c->d_work, 8 * 32 * sizeof(int)) != hipSuccess) return STFEM_ERR_OUT_OF_MEMORY;
    STFEM_TRY(hipMemsetAsync(c->d_work, 0, 8 * 32 * sizeof(int), st));
  }
  pp.work = c->d_work;
  pp.grid = 2 * (c->n_cu > 0 ? c->n_cu : 256); // two 4-wave workgroups per CU (registers, LDS)
  const size_t tl_n = ntiles * 4 * pp.lz * pp.ty * 8;
  rc = timeline_arm(c, tl_n, &pp.timeline, st);
  if (rc != STFEM_OK) return rc;
  const int launched = PR::pencil(c->p, prm, pp, st);
  c->last_kernel = PR::pencil_name();
  c->last_sweep[0] = int(ntiles);
  c->last_sweep[1] = int(std::min<size_t>(ntiles, size_t(pp.grid))); // (launch_pencil_ty)
  std::fill(c->last_tile, c->last_tile + 4, 0);
  if (launched == 0) rc = timeline_dump(c, tl_n, (long long)ntiles, 4, (long long)pp.lz * pp.ty, 8, st);
  return rc != STFEM_OK ? rc : launch_status(launched);
}

template <class PR>
static int launch_tile_panel(stfem_ctx *c, const typename PR::Sweep &prm, bool general, const Panel &pn, hipStream_t st)
{
  using real = typename PR::real;
  typename PR::Plan tp;
  std::memset(&tp, 0, sizeof(tp));
  const int nbm = std::max(pn.tj, pn.ti);
  if (PR::geometry(c->p, nbm, general ? 1 : 0, tp) != 0) return STFEM_ERR_UNSUPPORTED;
  plan_chunks(c, tp, nbm, PR::occupancy(c->p, nbm, general ? 1 : 0));
  const int nbm_r = block_slots(nbm);
  const size_t ntiles = size_t(tp.ntx) * tp.nty * tp.ntc;
  const size_t nyh = ntiles * nbm_r * tp.zp * tp.tX, nzh = ntiles * nbm_r * tp.tY * tp.tX, nxs = ntiles * nbm_r * tp.zp * tp.tY;
  int rc = grow_halo(c, nyh + nzh + 2 * nxs, st);
  if (rc != STFEM_OK) return rc;
  tp.yh = static_cast<real *>(c->d_halo);
  tp.zh = tp.yh + nyh;
  tp.xl = tp.zh + nzh;
  tp.xr = tp.xl + nxs;
  tp.add = pn.add ? 1 : 0;
  tp.experiment = c->env_exp;
  tp.stagger = c->env_stagger;
  tp.stagger_div = c->env_stagger_div;
  const size_t tl_n = ntiles * 4 * tp.wx * tp.lz * 16;
  rc = timeline_arm(c, tl_n, &tp.timeline, st);
  if (rc != STFEM_OK) return rc;
  const int launched = PR::tile(c->p, prm, tp, st);
  c->last_kernel = PR::tile_name(prm.metric != nullptr);
  c->last_sweep[0] = c->last_sweep[1] = 0;
  c->last_tile[0] = tp.ntx;
  c->last_tile[1] = tp.nty;
  c->last_tile[2] = tp.ntc;
  c->last_tile[3] = tp.lz;
  if (launched == 0) rc = timeline_dump(c, tl_n, (long long)ntiles, 4 * tp.wx, tp.lz, 16, st);
  return rc != STFEM_OK ? rc : launch_status(launched);
}

// the weights, sizes and blocks of panel (j0, i0) of the nbo x nbi system; false if all its weights are zero
template <class PR>
static bool set_panel(typename PR::Sweep &prm, const Panel &pn, int j0, int i0, int nbi, const std::vector<double> &a,
                      const std::vector<double> &b, stfem_vec *dst, const stfem_vec *src)
{
  using real = typename PR::real;
  bool nonzero = false;
  for (int j = 0; j < pn.tj; ++j)
    for (int i = 0; i < pn.ti; ++i) {
      prm.alpha[j * pn.ti + i] = real(a[size_t(j0 + j) * nbi + i0 + i]);
      prm.beta[j * pn.ti + i] = real(b[size_t(j0 + j) * nbi + i0 + i]);
      nonzero = nonzero || prm.alpha[j * pn.ti + i] != real(0) || prm.beta[j * pn.ti + i] != real(0);
    }
  prm.nbo = pn.tj;
  prm.nbi = pn.ti;
  for (int j = 0; j < pn.tj; ++j) prm.dst[j] = static_cast<real *>(dst->blk[j0 + j]);
  for (int i = 0; i < pn.ti; ++i) prm.src[i] = static_cast<const real *>(src->blk[i0 + i]);
  return nonzero;
}

// a(j,i), b(j,i): effective nbo x nbi matrices (row-major)
template <class PR>
static int apply_tiled_t(stfem_ctx *c, int nbo, int nbi, const std::vector<double> &a, const std::vector<double> &b, stfem_vec *dst,
                         const stfem_vec *src, int add, bool use_lap_coef, bool use_mass_coef, hipStream_t st)
{
  using real = typename PR::real;
  STFEM_TRY(hipSetDevice(c->device));
  for (int j = 0; j < nbo; ++j)
    for (int i = 0; i < nbi; ++i)
      if (dst->blk[j] == src->blk[i]) return STFEM_ERR_ALIAS;
  const bool general = is_general(c);
  if (general) {
    const int rc = ensure_metric<PR>(c, use_lap_coef, use_mass_coef, st);
    if (rc != STFEM_OK) return rc;
  }
  const bool atomic = c->variant == 1 && !general;
  if (!add && atomic)
    for (int j = 0; j < nbo; ++j)
      STFEM_TRY(hipMemsetAsync(dst->blk[j], 0, size_t(c->ndofs) * sizeof(real), st));
  typename PR::Sweep prm;
  fill_common<PR>(c, prm);
  prm.coef_lap = (use_lap_coef && !general) ? static_cast<const real *>(c->d_coef[1]) : nullptr;
  prm.coef_mass = (use_mass_coef && !general) ? static_cast<const real *>(c->d_coef[0]) : nullptr;
  if (general) {
    prm.metric = static_cast<const real *>(c->d_metric);
    prm.vol = real(1); // detJ and the weights live in the metric
  }
  prm.experiment = c->env_exp;
  prm.gp = nullptr;
  const int panel = panel_size<PR>(c, general, nbo, nbi);
  for (int j0 = 0; j0 < nbo; j0 += panel) {
    bool first = true; // first launch into this row panel overwrites dst unless add
    for (int i0 = 0; i0 < nbi; i0 += panel) {
      const Panel pn{std::min(panel, nbo - j0), std::min(panel, nbi - i0), add || !first, i0 + panel >= nbi};
      const bool nonzero = set_panel<PR>(prm, pn, j0, i0, nbi, a, b, dst, src);
      // the reference skips exact zeros too (operators.h:551,556); a panel may only be skipped
      // if something else still defines dst
      if (!nonzero && (atomic || add || !first || !pn.last)) continue;
      typename PR::PPlan pp;
      std::memset(&pp, 0, sizeof(pp));
      int rc;
      if (atomic)
        rc = launch_atomic_panel<PR>(c, prm, st);
      else if (c->variant == 0 && !general && PR::pencil_geometry(c->p, std::max(pn.tj, pn.ti), c->env_pencil_ty, pp) == 0) // (0: the kernel's default ty for (p, n_blocks))
        rc = launch_pencil_panel<PR>(c, prm, pp, pn, st);
      else
        rc = launch_tile_panel<PR>(c, prm, general, pn, st);
      if (rc != STFEM_OK) return rc;
      first = false;
    }
  }
  return STFEM_OK;
}

static int apply_tiled(stfem_ctx *c, int nbo, int nbi, const std::vector<double> &a, const std::vector<double> &b,
                       stfem_vec *dst, const stfem_vec *src, int add, bool use_lap_coef, bool use_mass_coef, void *stream)
{
  return stfem_by_prec(c, [&](auto t) {
    return apply_tiled_t<PrecOf<decltype(t)>>(c, nbo, nbi, a, b, dst, src, add, use_lap_coef, use_mass_coef, static_cast<hipStream_t>(stream));
  });
}

// d <- |d| > tol ? 1 / d : 1   (operators.h:1107-1109)
template <typename T> __global__ __launch_bounds__(256) void invert_diagonal_kernel(int64_t n, T *d, T tol)
{
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const T v = d[i];
    d[i] = fabs(v) > tol ? T(1) / v : T(1);
  }
}
// out = a * x + b * y
template <typename T>
__global__ __launch_bounds__(256) void lincomb_kernel(int64_t n, T a, const T *x, T b, const T *y, T *out)
{
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = a * x[i] + b * y[i];
}
template <typename T> static int invert_diagonal(stfem_ctx *c, void *d, hipStream_t st)
{
  const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 4096);
  hipLaunchKernelGGL(invert_diagonal_kernel<T>, dim3(grid), dim3(256), 0, st, c->ndofs, static_cast<T *>(d),
                     std::sqrt(std::numeric_limits<T>::epsilon()));
  return stfem_launch_end("invert_diagonal_kernel");
}

template <class PR> static int diagonal_t(stfem_ctx *c, double ms, double ls, stfem_vec *diag, hipStream_t st)
{
  using real = typename PR::real;
  if (!c || !diag || diag->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (diag->nb != 1) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(c->device));
  const Scaling lap = effective_scaling(c, 1, ls), mass = effective_scaling(c, 0, ms);
  const bool general = is_general(c);
  if (general) {
    const int rc = ensure_metric<PR>(c, lap.coef, mass.coef, st);
    if (rc != STFEM_OK) return rc;
  }
  typename PR::Diag prm; // (the kernel stores every entry of the block: nothing to clear)
  std::memset(&prm, 0, sizeof(prm));
  prm.diag = static_cast<real *>(diag->blk[0]);
  prm.ncx = c->nc[0]; prm.ncy = c->nc[1]; prm.ncz = c->nc[2];
  prm.nx = c->nd[0]; prm.ny = c->nd[1];
  prm.p = c->p;
  prm.dmask = c->dmask;
  prm.ms = real(mass.value);
  prm.ls = real(lap.value);
  fill_cell_scales(c, prm);
  const int n = c->p + 1;
  if (general) {
    prm.metric = static_cast<const real *>(c->d_metric);
  } else {
    prm.coef_lap = lap.coef ? static_cast<const real *>(c->d_coef[1]) : nullptr;
    prm.coef_mass = mass.coef ? static_cast<const real *>(c->d_coef[0]) : nullptr;
  }
  for (int a = 0; a < n; ++a) {
    double m = 0, l = 0;
    for (int q = 0; q < n; ++q) {
      m += c->tab.wq[q] * c->tab.S[q * n + a] * c->tab.S[q * n + a];
      l += c->tab.wq[q] * c->tab.D[q * n + a] * c->tab.D[q * n + a];
    }
    prm.m1[a] = real(m);
    prm.l1[a] = real(l);
  }
  for (int i = 0; i < n * n; ++i) {
    prm.S[i] = real(c->tab.S[i]);
    prm.D[i] = real(c->tab.D[i]);
  }
  return PR::diagonal(prm, st);
}

int stfem_st_vmult(stfem_ctx *c, int nrows, int ncols, const double *alpha, const double *beta,
                   int transpose, int add, stfem_vec *dst, const stfem_vec *src, void *stream)
{
  if (!c || !alpha || !beta || !dst || !src || nrows < 1 || ncols < 1) return STFEM_ERR_INVALID_ARGUMENT;
  TraceScope scope(transpose ? "Tvmult" : "vmult");
  if (dst->ctx != c || src->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  const int nbi = transpose ? nrows : ncols, nbo = transpose ? ncols : nrows;
  if (src->nb != nbi || dst->nb != nbo) return STFEM_ERR_SHAPE_MISMATCH;
  std::vector<double> a(size_t(nbo) * nbi), b(size_t(nbo) * nbi);
  for (int j = 0; j < nbo; ++j)
    for (int i = 0; i < nbi; ++i) {
      const size_t s = transpose ? size_t(i) * ncols + j : size_t(j) * ncols + i;
      a[size_t(j) * nbi + i] = alpha[s];
      b[size_t(j) * nbi + i] = beta[s];
    }
  // K = MatrixFreeOperator(0,1), M = MatrixFreeOperator(1,0)
  return apply_tiled(c, nbo, nbi, a, b, dst, src, add, effective_scaling(c, 1, 1.0).coef, effective_scaling(c, 0, 1.0).coef, stream);
}

int stfem_space_vmult(stfem_ctx *c, double ms, double ls, stfem_vec *dst, const stfem_vec *src, void *stream)
{
  if (!c || !dst || !src) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst->ctx != c || src->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (dst->nb != 1 || src->nb != 1) return STFEM_ERR_SHAPE_MISMATCH;
  const Scaling lap = effective_scaling(c, 1, ls), mass = effective_scaling(c, 0, ms);
  std::vector<double> a{lap.value}, b{mass.value};
  return apply_tiled(c, 1, 1, a, b, dst, src, 0, lap.coef, mass.coef, stream);
}

int stfem_diagonal(stfem_ctx *c, double ms, double ls, stfem_vec *diag, void *stream)
{
  if (!c) return STFEM_ERR_INVALID_ARGUMENT;
  return stfem_by_prec(c, [&](auto t) { return diagonal_t<PrecOf<decltype(t)>>(c, ms, ls, diag, static_cast<hipStream_t>(stream)); });
}

int stfem_diagonal_inverse(stfem_ctx *c, double ms, double ls, stfem_vec *diag, void *stream)
{
  const int rc = stfem_diagonal(c, ms, ls, diag, stream);
  if (rc != STFEM_OK) return rc;
  return stfem_by_prec(c, [&](auto t) { return invert_diagonal<decltype(t)>(c, diag->blk[0], static_cast<hipStream_t>(stream)); });
}

int stfem_st_diagonal(stfem_ctx *c, int n, const double *alpha, const double *beta, int inverse, stfem_vec *diag, void *stream)
{
  if (!c || !alpha || !beta || !diag || n < 1 || diag->ctx != c) return STFEM_ERR_INVALID_ARGUMENT;
  if (diag->nb != n) return STFEM_ERR_SHAPE_MISMATCH;
  STFEM_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // diag K and diag M (or their guarded inverses) once, then one linear combination per block
  stfem_vec *dk = nullptr, *dm = nullptr;
  int rc = stfem_vector_create(c, 1, &dk);
  if (rc == STFEM_OK) rc = stfem_vector_create(c, 1, &dm);
  if (rc == STFEM_OK) rc = inverse ? stfem_diagonal_inverse(c, 0.0, 1.0, dk, stream) : stfem_diagonal(c, 0.0, 1.0, dk, stream);
  if (rc == STFEM_OK) rc = inverse ? stfem_diagonal_inverse(c, 1.0, 0.0, dm, stream) : stfem_diagonal(c, 1.0, 0.0, dm, stream);
  const unsigned grid = (unsigned)std::min<int64_t>((c->ndofs + 255) / 256, 4096);
  for (int i = 0; i < n && rc == STFEM_OK; ++i) {
    const double a = inverse ? 1.0 / alpha[size_t(i) * n + i] : alpha[size_t(i) * n + i];
    const double b = inverse ? 1.0 / beta[size_t(i) * n + i] : beta[size_t(i) * n + i];
    stfem_by_prec(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(lincomb_kernel<T>, dim3(grid), dim3(256), 0, st, c->ndofs, T(a), static_cast<const T *>(dk->blk[0]), T(b),
                         static_cast<const T *>(dm->blk[0]), static_cast<T *>(diag->blk[i]));
    });
    rc = stfem_launch_end("lincomb_kernel");
  }
  const hipError_t sync = hipStreamSynchronize(st); // the temporaries go away below
  if (sync != hipSuccess && rc == STFEM_OK) rc = stfem_set_error(STFEM_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(sync));
  stfem_vector_destroy(dk);
  stfem_vector_destroy(dm);
  return rc;
}
