// Internal layout of the opaque handles of include/stfem.h and the few helpers shared by the host-side translation
// units of the library (context and operator: stfem_capi.hip, vectors: stfem_vector.hip, space transfers: stfem_transfer.hip,
// streams and captured graphs: stfem_stream.hip, smoothers, driver, communicator; the Stokes operator's own:
// stfem_stokes_internal.h).  Not part of the boundary.
#pragma once
#include "../../include/stfem.h"

#include "host_tables.h"
#include "stfem_hip_check.h" // STFEM_TRY, stfem_launch_begin / _end, stfem_set_error

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <vector>

namespace stfem {
// stfem_ctx::d_scratch (always double): the results of the reductions, then the stage-1 partial sums of up to DOT_VECS inner
// products from at most DOT_GRID workgroups each (stfem_vector.hip)
constexpr int DOT_VECS = 8, DOT_GRID = 512, DOT_RESULTS = 256;
constexpr size_t SCRATCH_DOUBLES = DOT_RESULTS + size_t(DOT_VECS) * DOT_GRID;
} // namespace stfem

struct stfem_ctx {
  int p = 0, device = 0, n_cu = 0;
  int nc[3] = {0, 0, 0}, nd[3] = {0, 0, 0};
  int64_t ndofs = 0, ncells = 0;
  int dmask = 0;
  bool cartesian = false;
  double lower[3] = {0, 0, 0}, h[3] = {1, 1, 1};
  stfem::ShapeTables tab;
  std::vector<double> vertices; // host copy (general meshes)
  int prec = 0;                // 0 = fp64, 1 = fp32 (element type of vectors, coefficients, metric)
  size_t es = sizeof(double);  // element size
  void *d_coef[2] = {nullptr, nullptr}; // [0] mass, [1] laplace
  int coef_layout[2] = {0, 0};
  double *d_scratch = nullptr; // reductions: [DOT_RESULTS] results, [DOT_VECS][DOT_GRID] partial sums
  const char *last_kernel = "";
  int last_sweep[2] = {0, 0}; // {tiles, workgroups} of the last pencil launch (stfem_last_sweep_plan)
  int last_tile[4] = {0, 0, 0, 0}; // {ntx, nty, ntc, lz} of the last tile launch (stfem_last_tile_plan)
  // tile variant: halo slabs (grown on demand)
  void *d_halo = nullptr;
  size_t halo_doubles = 0; // elements
  int variant = 0; // 0 = pencil (default; tile where the pencil kernel has no instantiation), 1 = atomic, 2 = tile
  // tuning / experiment switches, read once at context creation (STFEM_* environment variables)
  int env_tile_lz = 0, env_exp = 0, env_stagger = 0, env_stagger_div = 256, env_pencil_ty = 0, env_pencil_lz = 0;
  const char *env_timeline = nullptr;
  int *d_work = nullptr;           // pencil variant: tile counters
  long long *d_timeline = nullptr; // diagnostic builds: phase timestamps of the last apply
  size_t tl_n = 0;
  // general-geometry path: device copies of vertices and the 1D rule, metric terms per (cell, q)
  double *d_vertices = nullptr, *d_rule = nullptr;
  void *d_metric = nullptr;
  bool metric_valid = false;
  int metric_flags = -1; // which coefficients are baked into d_metric (bit0 laplace, bit1 mass)
  // csrc/stfem_stokes.hip: the next store-mode sweep of three FE_Q(2) blocks adds - grad_scale B^T p (SweepParams::gp); set and
  // cleared around one stfem_st_vmult by stfem_internal_set_gradient, grad_applied tells whether a launch took it
  const double *grad_p = nullptr;
  double grad_w[3][2][3][2];
  double grad_scale = 0.0;
  bool grad_applied = false;
};
int stfem_internal_set_gradient(stfem_ctx *c, const double *p, const double (*w)[2][3][2], double scale);

struct stfem_vec {
  stfem_ctx *ctx = nullptr;
  int device = 0; // of ctx, kept here: a garbage-collected caller may destroy the context before its vectors
  int nb = 0;
  bool owns = false;
  std::vector<void *> blk; // device arrays of the context's element type
};

// calls f with a value of the context's Number type: stfem_by_prec(c, [&](auto t) { using T = decltype(t); ... })
template <class F> auto stfem_by_prec(const stfem_ctx *c, F &&f) { return c->prec ? f(float()) : f(double()); }

// a named trace range around a scope (stfem_host_helpers.cpp: roctx, bound at run time)
struct TraceScope {
  explicit TraceScope(const char *name) { stfem_trace_push(name); }
  ~TraceScope() { stfem_trace_pop(); }
};

// stfem_capi.hip: (re)builds the per-quadrature-point metric records [cell][qz][qy][qx][8] =
// (Gxx,Gxy,Gxz,Gyy,Gyz,Gzz,Mq,pad) with the coefficient tables in force; element type = the context's Number
int stfem_internal_metric(stfem_ctx *c, const void **metric, void *stream);

// stfem_stokes.hip: what stfem_stokes_vanka.hip needs to know about a Stokes context
struct stfem_stokes_desc {
  int device, cart, pspace, dmask, weak_mask, outflow_mask;
  int nc[3], ndu[3], ndp[3];
  long long Nu, Np;
  double lower[3], upper[3], nu, penalty1, penalty2;
};
int stfem_stokes_internal_desc(const stfem_stokes_ctx *c, stfem_stokes_desc *out);

#pragma GCC visibility push(hidden)
// stfem_stokes.hip: every entry point whose kernels hard-code the 27 nodes of FE_Q(2) asks this first.  On a context of another
// velocity degree (stfem_stokes_create_space): STFEM_ERR_UNSUPPORTED, "<entry> is built for velocity degree 2 only" in the record.
int stokes_require_q2(const stfem_stokes_ctx *c, const char *entry);
// stfem_stokes.hip: stfem_stokes_internal_desc without that question (stfem_stokes_vanka_create_space serves degree 3 too)
int stokes_desc_any_degree(const stfem_stokes_ctx *c, stfem_stokes_desc *out);
int stokes_velocity_degree(const stfem_stokes_ctx *c);
// stfem_stokes.hip: what takes a linearisation velocity asks this too.  On a context of velocity degree 3 with weak faces
// (stfem_stokes_set_weak_boundaries_space): STFEM_ERR_UNSUPPORTED - the inflow term - min(b.n, 0) u of the faces is not built there.
int stokes_refuse_inflow_q3(const stfem_stokes_ctx *c, const char *entry);
// stfem_vanka.hip: vanka_invert_kernel<double> on `count` m x m matrices at B (row-major, destroyed), the inverses in the apply's
// layout [kpad][mpad] from block cell0 of out; *singular (device) is set to 1 by a matrix without a pivot.  `stream`: a hipStream_t.
int stfem_vanka_invert_launch(double *B, double *out, int m, int mpad, int kpad, long long cell0, unsigned count, int *singular, void *stream);

// stfem_stokes_vanka_cell.hip: one block per cell of the two-variable Stokes system (stfem_stokes_vanka_create_linearised)
struct stokes_cell_vanka_desc {
  int nblk, m, mpad, kpad, mode;
  int var[8];                 // 0 velocity / 1 pressure, in BlockSlice order
  double Alpha[64], Beta[64]; // nblk x nblk, row-major
  double delta0;              // CIP term C(b_j; .) in the velocity-velocity entries (0: none; otherwise `lin` is read in every mode)
  // a z-slab (stfem_stokes_vanka_create_linearised_partitioned): the context the blocks are SET UP on - the slab plus one ghost cell
  // layer per z neighbour, `lin` lives there -, the first of its cell layers that is the slab's own, and whether there are cells beyond
  // a ghost layer (bit 4 / 5: its outer z face is interior for the CIP term).  nullptr: the context of the apply, all layers own.
  stfem_stokes_ctx *setup;
  int own0, beyond;
  // velocity degree of the context, set by every caller: 2, or 3 (stfem_stokes_vanka_create_space: mode 0, no CIP term, no slab);
  // anything else is refused
  int degree;
};
struct stokes_cell_vanka;
// row table: nblk-block rows -> (vector | variable << 8, element offset from the cell's first DoF of the variable), m entries of two ints
int stokes_cell_vanka_create(stfem_stokes_ctx *c, const stokes_cell_vanka_desc &d, const int *rowtab_xy, const double *const *lin,
                             stokes_cell_vanka **out);
int stokes_cell_vanka_update(stokes_cell_vanka *v, const double *const *lin);
int stokes_cell_vanka_setup_batches(const stokes_cell_vanka *v);
// rows of y = B_c^-1 gather(src) of every cell to the scratch array [cell][mpad], returned in *rows
int stokes_cell_vanka_apply(stokes_cell_vanka *v, const double *const *src_blocks, const double **rows, void *stream);
void stokes_cell_vanka_destroy(stokes_cell_vanka *v);
#pragma GCC visibility pop
