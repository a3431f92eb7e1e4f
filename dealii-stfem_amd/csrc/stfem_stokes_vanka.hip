// Cell-patch Vanka smoother of the two-variable Stokes space-time system (SURVEY 8 f-1 for BASELINE configs[4]).
//
// Replaces PreconditionVanka in its block form (reference include/stmg.h:626-738: the constructor over BlockSparseMatrixType with
// a BlockSlice, K_mask / M_mask; vmult 832-872) as tests/tp_03stokes.cc:537-540, 714-726 sets it up: per cell the block
//     B_c((i, k), (j, l)) = valence_iv(k) * (Alpha(i, j) K_{iv,jv}(k, l) + [iv = jv = 0] Beta(i, j) M(k, l)),
// i, j = blocks of the BlockSlice (time step, variable, time dof), k, l = the cell's DoFs of the block's variable (81 velocity
// DoFs, 8 FE_Q(1) or 4 FE_DGP(1) pressure DoFs), K = the ASSEMBLED Stokes matrix [[nu K, -B^T], [B, 0]] (+ the Nitsche terms of
// weak boundary faces) and M = the assembled vector mass, both restricted to the cell (compute_block_matrix.h:50-139) with the
// strong velocity constraints (row and column dropped, diagonal kept), inverted by Gauss-Jordan;
//     vmult: dst = sum over cells of scatter(B_c^-1 gather(src)).
// Axis-aligned uniform meshes (the Kronecker path of csrc/stfem_stokes.hip): there the block of a cell depends only on which
// neighbours it has - at most 27 blocks per mesh; general meshes and the linearised operator (stfem_stokes_vanka_create_linearised)
// hold one block per cell: set-up and streaming apply in stfem_stokes_vanka_cell.hip, the collecting launch is the one below.  Set-up
// of the class blocks: every class block is read off the device operator itself, applied to
// unit vectors on a mesh of 1 - 3 cells per direction with the cell in the position of its class (the reference's own method of
// getting matrix entries, tests/tp_05dgp_support.cc:140-149) - no second implementation of the cell matrices.  Apply: the
// MFMA class kernel of the scalar smoother (stfem_vanka_kernel.h) with a row table in place of its (block, node) arithmetic, rows
// to a scratch array, then one collecting launch that sums every DoF's cells in a fixed order: two launches, no colours, no
// atomics, bitwise reproducible.  Block classes, the flat cell list, the tile plan and the way from the probed matrices to the stored
// inverse are the shared host steps of stfem_vanka_setup.h.
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

struct StokesCollectParams {
  double *dst[VK_MAX_BLOCKS];
  const double *y;   // [slot][mpad]
  const int *slot;   // cell -> slot (nullptr: slot = cell, the one-block-per-cell layout)
  int nblk, mpad, pdg;
  int pu, npc; // velocity degree (2, or 3 with one block per cell), FE_DGP functions per cell (4 / 10)
  int var[VK_MAX_BLOCKS], rowbase[VK_MAX_BLOCKS];
  int nc[3], ndu[3], ndp[3];
  long long Nu, Np;
  double omega;
  int accumulate;
};

// blockIdx.y = block of the BlockSlice; a thread takes one DoF of it: (component, node) of a velocity block, a node or a cell
// function of a pressure block, and sums the rows its cells left in the scratch array (cells in z, y, x order)
__global__ __launch_bounds__(256) void stokes_vanka_collect_kernel(const StokesCollectParams P)
{
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int var = P.var[b];
  const long long n_dofs = var == 0 ? 3 * P.Nu : P.Np;
  if (i >= n_dofs) return;
  double s = 0.0;
  if (var == 1 && P.pdg) {
    const long long cell = i / P.npc;
    s = P.y[size_t(P.slot ? P.slot[cell] : cell) * P.mpad + P.rowbase[b] + int(i - cell * P.npc)];
  } else {
    const int p = var == 0 ? P.pu : P.pu - 1, np = p + 1;
    const int *nd = var == 0 ? P.ndu : P.ndp;
    const long long N = var == 0 ? P.Nu : P.Np;
    const int comp = int(i / N);
    const long long node = i - (long long)comp * N;
    const int idx[3] = {int(node % nd[0]), int((node / nd[0]) % nd[1]), int(node / ((long long)nd[0] * nd[1]))};
    int cc[3][2], ll[3][2], cnt[3];
    node_cells(idx, p, P.nc, cc, ll, cnt);
    const int rb = P.rowbase[b] + comp * (P.pu + 1) * (P.pu + 1) * (P.pu + 1);
    for (int kz = 0; kz < cnt[2]; ++kz)
      for (int ky = 0; ky < cnt[1]; ++ky)
        for (int kx = 0; kx < cnt[0]; ++kx) {
          const int cell = cc[0][kx] + P.nc[0] * (cc[1][ky] + P.nc[1] * cc[2][kz]);
          const int n = ll[0][kx] + np * (ll[1][ky] + np * ll[2][kz]);
          s += P.y[size_t(P.slot ? P.slot[cell] : cell) * P.mpad + rb + n];
        }
  }
  double *d = P.dst[b] + i;
  *d = P.accumulate ? *d + P.omega * s : P.omega * s;
}

template <int MT> const void *sv_kernel() { return reinterpret_cast<const void *>(&vanka_apply_kernel<double, 27, MT>); }
const void *sv_kernel(int mtw)
{
  switch (mtw) {
    case 1: return sv_kernel<1>();
    case 2: return sv_kernel<2>();
    case 3: return sv_kernel<3>();
    case 4: return sv_kernel<4>();
    case 6: return sv_kernel<6>();
    default: return nullptr;
  }
}

} // namespace

struct stfem_stokes_vanka {
  stfem_stokes_ctx *ctx = nullptr;
  stfem_stokes_desc d;
  int nblk = 0, var[VK_MAX_BLOCKS] = {0}, rowbase[VK_MAX_BLOCKS] = {0};
  int m = 0, mt = 0, mtw = 0, parts = 0, mpad = 0, kpad = 0, nclasses = 0, nquad = 0;
  double *d_blocks = nullptr, *d_flat = nullptr;
  int2 *d_rowtab = nullptr;
  int *d_cellu = nullptr, *d_cellp = nullptr, *d_cls = nullptr, *d_slot = nullptr;
  int degree = 2;                    // velocity degree (3: stfem_stokes_vanka_create_space, one block per cell)
  int mode = 0;                      // convection mode of the per-cell blocks
  double delta0 = 0.0;               // their CIP term (stfem_stokes_vanka_create_linearised_cip)
  stokes_cell_vanka *cell = nullptr; // one block per cell (stfem_stokes_vanka_cell.hip): none of the class arrays above
};

namespace {

// The restricted assembled matrices of one block class, read off the operator on a mesh of 1 - 3 cells per direction:
// A = [[nu K, -B^T], [B, 0]] (+ weak faces), Mu = vector mass, both (81 + npl)^2 / 81^2 over the cell's DoFs, unconstrained.
int probe_class(const stfem_stokes_desc &d, int key, int npl, std::vector<double> &A, std::vector<double> &Mu)
{
  const int nl = 81 + npl;
  A.assign(size_t(nl) * nl, 0.0);
  Mu.assign(size_t(81) * 81, 0.0);
  stfem_mesh_desc md;
  std::memset(&md, 0, sizeof(md));
  int cc[3], weak = 0;
  for (int k = 0; k < 3; ++k) {
    const int lo = (key >> (2 * k)) & 1, hi = (key >> (2 * k + 1)) & 1;
    md.ncell[k] = 1 + lo + hi;
    const double h = (d.upper[k] - d.lower[k]) / d.nc[k];
    md.lower[k] = 0.0;
    md.upper[k] = h * md.ncell[k];
    cc[k] = lo;
    if (!lo && (d.weak_mask & (1 << (2 * k)))) weak |= 1 << (2 * k);
    if (!hi && (d.weak_mask & (2 << (2 * k)))) weak |= 2 << (2 * k);
  }
  md.vertices = nullptr;
  md.dirichlet_mask = 0; // (the strong constraints are applied to the block afterwards: the diagonal of the unconstrained assembly stays)
  md.device = d.device;
  stfem_stokes_ctx *t = nullptr;
  int rc = stfem_stokes_create_ex(&md, 2, d.pspace, d.nu, &t);
  if (rc != STFEM_OK) return rc;
  if (weak) rc = stfem_stokes_set_weak_boundaries(t, weak, 0, d.penalty1, d.penalty2);
  const long long Nu = stfem_stokes_n_velocity_dofs(t), Np = stfem_stokes_n_pressure_dofs(t);
  const int ndu[3] = {2 * md.ncell[0] + 1, 2 * md.ncell[1] + 1, 2 * md.ncell[2] + 1};
  const int ndp[3] = {md.ncell[0] + 1, md.ncell[1] + 1, md.ncell[2] + 1};
  // global indices (within the u / p vector of the small mesh) of the cell's local DoFs
  std::vector<long long> gi(nl);
  for (int c = 0; c < 3; ++c)
    for (int n = 0; n < 27; ++n) {
      const int a = n % 3, b = (n / 3) % 3, e = n / 9;
      gi[c * 27 + n] = c * Nu + (2 * cc[0] + a) + (long long)ndu[0] * ((2 * cc[1] + b) + (long long)ndu[1] * (2 * cc[2] + e));
    }
  for (int n = 0; n < npl; ++n) {
    if (d.pspace) gi[81 + n] = 4ll * (cc[0] + md.ncell[0] * (cc[1] + md.ncell[1] * cc[2])) + n;
    else {
      const int a = n % 2, b = (n / 2) % 2, e = n / 4;
      gi[81 + n] = (cc[0] + a) + (long long)ndp[0] * ((cc[1] + b) + (long long)ndp[1] * (cc[2] + e));
    }
  }
  double *su = nullptr, *sp = nullptr, *du = nullptr, *dp = nullptr;
  if (rc == STFEM_OK) rc = stfem_stokes_vector_create(t, 0, &su);
  if (rc == STFEM_OK) rc = stfem_stokes_vector_create(t, 1, &sp);
  if (rc == STFEM_OK) rc = stfem_stokes_vector_create(t, 0, &du);
  if (rc == STFEM_OK) rc = stfem_stokes_vector_create(t, 1, &dp);
  const size_t lu = size_t(3 * Nu), lp = size_t(Np);
  std::vector<double> hu(lu, 0.0), hp(lp, 0.0), zu(lu, 0.0), zp(lp, 0.0);
  for (int col = 0; col < nl && rc == STFEM_OK; ++col) {
    std::vector<double> &z = col < 81 ? zu : zp;
    z[size_t(gi[col])] = 1.0;
    rc = stfem_stokes_vector_upload(t, col < 81 ? 0 : 1, col < 81 ? su : sp, z.data());
    if (rc == STFEM_OK) rc = stfem_stokes_vmult(t, du, dp, su, sp, nullptr);
    if (rc == STFEM_OK) rc = stfem_stokes_vector_download(t, 0, du, hu.data());
    if (rc == STFEM_OK) rc = stfem_stokes_vector_download(t, 1, dp, hp.data());
    for (int row = 0; row < nl; ++row) A[size_t(row) * nl + col] = row < 81 ? hu[size_t(gi[row])] : hp[size_t(gi[row])];
    if (rc == STFEM_OK && col < 81) {
      rc = stfem_stokes_mass_vmult(t, du, su, nullptr);
      if (rc == STFEM_OK) rc = stfem_stokes_vector_download(t, 0, du, hu.data());
      for (int row = 0; row < 81; ++row) Mu[size_t(row) * 81 + col] = hu[size_t(gi[row])];
    }
    z[size_t(gi[col])] = 0.0;
    if (rc == STFEM_OK) rc = stfem_stokes_vector_upload(t, col < 81 ? 0 : 1, col < 81 ? su : sp, z.data());
  }
  if (su) stfem_stokes_vector_destroy(t, su);
  if (sp) stfem_stokes_vector_destroy(t, sp);
  if (du) stfem_stokes_vector_destroy(t, du);
  if (dp) stfem_stokes_vector_destroy(t, dp);
  stfem_stokes_destroy(t);
  return rc;
}

// The inverted block of every class: probed matrices, strong velocity constraints, valence, Alpha / Beta, Gauss-Jordan
int build_class_blocks(stfem_stokes_vanka *v, const vanka::ClassTable &t, int npl, const double *Alpha, const double *Beta)
{
  const stfem_stokes_desc &d = v->d;
  const int nl = 81 + npl, m = v->m;
  const size_t bsz = size_t(v->kpad) * v->mpad;
  std::vector<double> all(bsz * t.key.size()), A, Mu, B;
  std::vector<int> dof(m); // row -> DoF of the cell (81 velocity, then npl pressure)
  for (int i = 0; i < v->nblk; ++i)
    for (int k = 0; k < (v->var[i] ? npl : 81); ++k) dof[v->rowbase[i] + k] = (v->var[i] ? 81 : 0) + k;
  for (size_t ci = 0; ci < t.key.size(); ++ci) {
    const int key = t.key[ci];
    const int rc = probe_class(d, key, npl, A, Mu);
    if (rc != STFEM_OK) return stfem_set_error(rc, "probing the block of class %d: status %d (%s)", key, rc, stfem_last_error());
    // valence and strong constraints of the cell's DoFs
    std::vector<double> val(nl, 1.0);
    std::vector<char> con(nl, 0);
    for (int c = 0; c < 3; ++c)
      for (int n = 0; n < 27; ++n) {
        const int a[3] = {n % 3, (n / 3) % 3, n / 9};
        for (int k = 0; k < 3; ++k) {
          const int kk = (key >> (2 * k)) & 3;
          if ((a[k] == 0 && (kk & 1)) || (a[k] == 2 && (kk & 2))) val[c * 27 + n] *= 2.0;
          if ((a[k] == 0 && !(kk & 1) && (d.dmask & (1 << (2 * k)))) || (a[k] == 2 && !(kk & 2) && (d.dmask & (2 << (2 * k))))) con[c * 27 + n] = 1;
        }
      }
    if (!d.pspace)
      for (int n = 0; n < 8; ++n) {
        const int a[3] = {n % 2, (n / 2) % 2, n / 4};
        for (int k = 0; k < 3; ++k) {
          const int kk = (key >> (2 * k)) & 3;
          if ((a[k] == 0 && (kk & 1)) || (a[k] == 1 && (kk & 2))) val[81 + n] *= 2.0;
        }
      }
    vanka::combine_two_variable(v->nblk, v->var, v->rowbase, m, 81, nl, Alpha, Beta, A, Mu, B);
    if (!vanka::finish_block(m, B, dof, con, val, all.data() + bsz * ci, v->mpad, v->kpad)) {
      return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "singular cell block (class %d)", key);
    }
  }
  return vk_upload(&v->d_blocks, all);
}

// The row table: row -> (vector, variable, element offset from the cell's first DoF of the variable)
int row_table(const stfem_stokes_vanka *v, std::vector<int2> &rowtab)
{
  const stfem_stokes_desc &d = v->d;
  std::vector<int> xy;
  if (!vanka::stokes_row_table(v->degree, d.pspace != 0, v->nblk, v->var, v->rowbase, d.Nu, d.ndu, d.ndp, xy)) return STFEM_ERR_UNSUPPORTED;
  rowtab.resize(v->m);
  for (int r = 0; r < v->m; ++r) rowtab[r] = make_int2(xy[2 * r], xy[2 * r + 1]);
  return STFEM_OK;
}

// The row table, the flat cell list with the cells' first velocity and pressure DoFs, and the scratch array
int build_tables(stfem_stokes_vanka *v, const vanka::ClassTable &t, int npl)
{
  const stfem_stokes_desc &d = v->d;
  std::vector<int2> rowtab;
  int rc = row_table(v, rowtab);
  if (rc != STFEM_OK) return rc;
  // ---- cells grouped by class into batches of 16, four batches of one class per workgroup
  std::vector<int> firstu(t.cls.size()), firstp(t.cls.size());
  for (int cz = 0; cz < d.nc[2]; ++cz)
    for (int cy = 0; cy < d.nc[1]; ++cy)
      for (int cx = 0; cx < d.nc[0]; ++cx) {
        const int cell = cx + d.nc[0] * (cy + d.nc[1] * cz);
        firstu[cell] = 2 * cx + d.ndu[0] * (2 * cy + d.ndu[1] * 2 * cz);
        firstp[cell] = d.pspace ? 4 * cell : cx + d.ndp[0] * (cy + d.ndp[1] * cz);
      }
  const vanka::CellList list = vanka::cell_list(t, -1);
  v->nquad = int(list.cls.size());
  rc = vk_upload(&v->d_rowtab, rowtab);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_cellu, vanka::gather_cells(list.order, firstu, -1));
  if (rc == STFEM_OK) rc = vk_upload(&v->d_cellp, vanka::gather_cells(list.order, firstp, 0));
  if (rc == STFEM_OK) rc = vk_upload(&v->d_cls, list.cls);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_slot, list.slot);
  if (rc == STFEM_OK) rc = vk_alloc(reinterpret_cast<void **>(&v->d_flat), list.order.size() * v->mpad * sizeof(double));
  return rc;
}

} // namespace

extern "C" {

void stfem_stokes_vanka_destroy(stfem_stokes_vanka *v)
{
  if (!v) return;
  (void)hipSetDevice(v->d.device);
  (void)hipFree(v->d_blocks);
  (void)hipFree(v->d_flat);
  (void)hipFree(v->d_rowtab);
  (void)hipFree(v->d_cellu);
  (void)hipFree(v->d_cellp);
  (void)hipFree(v->d_cls);
  (void)hipFree(v->d_slot);
  stokes_cell_vanka_destroy(v->cell);
  delete v;
}

int stfem_stokes_vanka_n_classes(const stfem_stokes_vanka *v) { return v ? v->nclasses : 0; }
int stfem_stokes_vanka_setup_batches(const stfem_stokes_vanka *v) { return v ? stokes_cell_vanka_setup_batches(v->cell) : 0; }

// the rows of the cell block at velocity degree `degree`: block i holds the cell's velocity DoFs (81, at degree 3 192) or its pressure
// DoFs from row rowbase[i]
static int block_rows(stfem_stokes_vanka *v, int n_blocks, const int32_t *block_variable, int degree)
{
  const int nvel = vanka::stokes_cell_velocity_dofs(degree), npl = vanka::stokes_cell_pressure_dofs(degree, v->d.pspace != 0);
  v->nblk = n_blocks;
  for (int i = 0; i < n_blocks; ++i) {
    if (block_variable[i] < 0 || block_variable[i] > 1) return STFEM_ERR_INVALID_ARGUMENT;
    v->var[i] = block_variable[i];
    v->rowbase[i] = v->m;
    v->m += block_variable[i] == 0 ? nvel : npl;
  }
  if (v->m > VK_MAX_ROWS)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "a cell block of %d rows (%d blocks at velocity degree %d): the limit is %d rows", v->m, n_blocks, degree, VK_MAX_ROWS);
  return STFEM_OK;
}

int stfem_stokes_vanka_create(stfem_stokes_ctx *ctx, int n_blocks, const int32_t *block_variable, const double *Alpha, const double *Beta,
                              stfem_stokes_vanka **out)
{
  if (!ctx || !block_variable || !Alpha || !Beta || !out || n_blocks < 1) return STFEM_ERR_INVALID_ARGUMENT;
  if (const int rq = stokes_require_q2(ctx, "stfem_stokes_vanka_create")) return rq;
  *out = nullptr;
  if (n_blocks > VK_MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  stfem_stokes_desc d;
  int rc = stfem_stokes_internal_desc(ctx, &d);
  if (rc != STFEM_OK) return rc;
  // one block per neighbour pattern needs identical cells; a general mesh gets one block per cell
  if (!d.cart) return stfem_stokes_vanka_create_linearised(ctx, n_blocks, block_variable, Alpha, Beta, STFEM_CONVECTION_NONE, nullptr, out);
  std::unique_ptr<stfem_stokes_vanka, void (*)(stfem_stokes_vanka *)> v(new (std::nothrow) stfem_stokes_vanka, stfem_stokes_vanka_destroy);
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->ctx = ctx;
  v->d = d;
  const int npl = d.pspace ? 4 : 8;
  rc = block_rows(v.get(), n_blocks, block_variable, 2);
  if (rc != STFEM_OK) return rc;
  const vanka::TilePlan plan = vanka::stokes_tile_plan((v->m + 15) / 16);
  v->mtw = plan.mtw; v->parts = plan.parts; v->mt = plan.parts * plan.mtw;
  v->mpad = 16 * v->mt;
  v->kpad = ((v->m + KS - 1) / KS) * KS;
  STFEM_TRY(hipSetDevice(d.device));
  const vanka::ClassTable t = vanka::class_table(d.nc, 0);
  v->nclasses = int(t.key.size());
  rc = build_class_blocks(v.get(), t, npl, Alpha, Beta);
  if (rc == STFEM_OK) rc = build_tables(v.get(), t, npl);
  if (rc == STFEM_OK) *out = v.release();
  return rc;
}

// One block per cell, on every mesh, of the operator linearised about lin_blocks (reinit_asm, stmg.h:929-965: set_data, then the
// assembled matrix of compute_matrix_helper<OperatorMode::jacobian>, operators.h:1310-1318, and one inverted block per cell from it,
// stmg.h:704-742, compute_block_matrix.h:50-139).  Every refusal is decided before anything touches the device.
// delta0 != 0: with the CIP term C(b_j; .) in the velocity-velocity entries (stfem_stokes_vanka_create_linearised_cip)
// setup != nullptr: a z-slab - the blocks of ctx's cells are set up on `setup` (ctx plus one ghost cell layer per z neighbour, own
// layers from own0; lin_blocks live there), see stfem_stokes_vanka_create_linearised_partitioned
static int create_per_cell(stfem_stokes_ctx *ctx, int n_blocks, const int32_t *block_variable, const double *Alpha, const double *Beta, int mode,
                           const double *const *lin_blocks, double delta0, stfem_stokes_vanka **out, stfem_stokes_ctx *setup = nullptr,
                           int own0 = 0, int beyond = 0, bool any_degree = false)
{
  if (!out) return STFEM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!ctx || !block_variable || !Alpha || !Beta || n_blocks < 1) return STFEM_ERR_INVALID_ARGUMENT;
  if (mode < STFEM_CONVECTION_NONE || mode > STFEM_CONVECTION_JACOBIAN || (mode != STFEM_CONVECTION_NONE && !lin_blocks)) return STFEM_ERR_INVALID_ARGUMENT;
  if (n_blocks > VK_MAX_BLOCKS) return STFEM_ERR_UNSUPPORTED;
  // (the _cip and _partitioned entries have asked under their own names before they come here)
  // any_degree: stfem_stokes_vanka_create_space and _create_linearised_space, the entries that serve velocity degree 3 (every mode, no
  // CIP term, no slab)
  if (!any_degree)
    if (const int rq = stokes_require_q2(ctx, "stfem_stokes_vanka_create_linearised")) return rq;
  const int degree = stokes_velocity_degree(ctx);
  if (degree != 2 && delta0 != 0.0)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "per-cell Stokes blocks with delta0 = %g at velocity degree %d: the CIP term is not built into the blocks of that degree", delta0, degree);
  stfem_stokes_desc d;
  int rc = stokes_desc_any_degree(ctx, &d);
  if (rc != STFEM_OK) return rc;
  std::unique_ptr<stfem_stokes_vanka, void (*)(stfem_stokes_vanka *)> v(new (std::nothrow) stfem_stokes_vanka, stfem_stokes_vanka_destroy);
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->ctx = ctx;
  v->d = d;
  v->degree = degree;
  rc = block_rows(v.get(), n_blocks, block_variable, degree);
  if (rc != STFEM_OK) return rc;
  if (mode != STFEM_CONVECTION_NONE) // (only the velocity entries are read: operators.h:835-866)
    for (int i = 0; i < n_blocks; ++i)
      if (v->var[i] == 0 && !lin_blocks[i]) return STFEM_ERR_INVALID_ARGUMENT;
  v->mt = (v->m + 15) / 16;
  v->mpad = 16 * v->mt;
  v->kpad = ((v->m + 3) / 4) * 4;
  v->nclasses = int((long long)d.nc[0] * d.nc[1] * d.nc[2]);
  std::vector<int2> rowtab;
  rc = row_table(v.get(), rowtab);
  if (rc != STFEM_OK) return rc;
  stokes_cell_vanka_desc cd;
  std::memset(&cd, 0, sizeof(cd));
  v->mode = mode;
  v->delta0 = delta0;
  cd.delta0 = delta0;
  cd.setup = setup; cd.own0 = own0; cd.beyond = beyond;
  cd.degree = degree;
  cd.nblk = n_blocks; cd.m = v->m; cd.mpad = v->mpad; cd.kpad = v->kpad; cd.mode = mode;
  for (int i = 0; i < n_blocks; ++i) cd.var[i] = v->var[i];
  for (int i = 0; i < n_blocks * n_blocks; ++i) { cd.Alpha[i] = Alpha[i]; cd.Beta[i] = Beta[i]; }
  STFEM_TRY(hipSetDevice(d.device));
  rc = stokes_cell_vanka_create(ctx, cd, &rowtab[0].x, lin_blocks, &v->cell);
  if (rc == STFEM_OK) *out = v.release();
  return rc;
}

int stfem_stokes_vanka_create_linearised(stfem_stokes_ctx *ctx, int n_blocks, const int32_t *block_variable, const double *Alpha, const double *Beta,
                                         int mode, const double *const *lin_blocks, stfem_stokes_vanka **out)
{
  return create_per_cell(ctx, n_blocks, block_variable, Alpha, Beta, mode, lin_blocks, 0.0, out);
}

// The constructor by descriptor (include/stfem_stokes_vanka_space.h): velocity degree 2 is stfem_stokes_vanka_create_linearised with
// STFEM_CONVECTION_NONE on its own path; degree 3 builds the same blocks (stmg.h:704-742, compute_block_matrix.h:50-139) from the cell
// matrices of the same kernel's degree-3 instantiations (stfem_stokes_vanka_cell.hip).  Every refusal is decided on the arguments, before the context or the device is touched.
int stfem_stokes_vanka_create_space(stfem_stokes_ctx *ctx, const stfem_stokes_vanka_space_desc *desc, stfem_stokes_vanka **out)
{
  const char *me = "stfem_stokes_vanka_create_space";
  if (!out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: out is null", me);
  *out = nullptr;
  if (!ctx) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: ctx is null", me);
  if (!desc) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: desc is null", me);
  for (int i = 0; i < 4; ++i)
    if (desc->reserved[i] != 0) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: reserved[%d] = %d, must be 0", me, i, desc->reserved[i]);
  if (desc->n_blocks < 1 || desc->n_blocks > VK_MAX_BLOCKS)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: n_blocks = %d, must be 1..%d", me, desc->n_blocks, VK_MAX_BLOCKS);
  if (!desc->block_variable || !desc->Alpha || !desc->Beta)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: %s is null", me, !desc->block_variable ? "block_variable" : (!desc->Alpha ? "Alpha" : "Beta"));
  for (int i = 0; i < desc->n_blocks; ++i)
    if (desc->block_variable[i] < 0 || desc->block_variable[i] > 1)
      return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: block_variable[%d] = %d, must be 0 (velocity) or 1 (pressure)", me, i, desc->block_variable[i]);
  if (stokes_velocity_degree(ctx) == 2)
    return stfem_stokes_vanka_create_linearised(ctx, desc->n_blocks, desc->block_variable, desc->Alpha, desc->Beta, STFEM_CONVECTION_NONE, nullptr, out);
  return create_per_cell(ctx, desc->n_blocks, desc->block_variable, desc->Alpha, desc->Beta, STFEM_CONVECTION_NONE, nullptr, 0.0, out, nullptr, 0, 0, true);
}

// The same constructor for the operator linearised about lin_blocks (include/stfem_stokes_vanka_linearised_space.h): velocity degree 2
// is stfem_stokes_vanka_create_linearised on its own path; degree 3 builds the blocks of A(b_j) per column block from the cell matrices
// of the same kernel's degree-3 instantiations in the mode, a launch per distinct state.  The refusals of stfem_stokes_vanka_create_space, then
// those of the mode, all decided on the arguments before the context or the device is touched.
int stfem_stokes_vanka_create_linearised_space(stfem_stokes_ctx *ctx, const stfem_stokes_vanka_linearised_space_desc *desc, stfem_stokes_vanka **out)
{
  const char *me = "stfem_stokes_vanka_create_linearised_space";
  if (!out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: out is null", me);
  *out = nullptr;
  if (!ctx) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: ctx is null", me);
  if (!desc) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: desc is null", me);
  for (int i = 0; i < 4; ++i)
    if (desc->reserved[i] != 0) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: reserved[%d] = %d, must be 0", me, i, desc->reserved[i]);
  if (desc->n_blocks < 1 || desc->n_blocks > VK_MAX_BLOCKS)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: n_blocks = %d, must be 1..%d", me, desc->n_blocks, VK_MAX_BLOCKS);
  if (!desc->block_variable || !desc->Alpha || !desc->Beta)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: %s is null", me, !desc->block_variable ? "block_variable" : (!desc->Alpha ? "Alpha" : "Beta"));
  for (int i = 0; i < desc->n_blocks; ++i)
    if (desc->block_variable[i] < 0 || desc->block_variable[i] > 1)
      return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: block_variable[%d] = %d, must be 0 (velocity) or 1 (pressure)", me, i, desc->block_variable[i]);
  if (desc->mode < STFEM_CONVECTION_NONE || desc->mode > STFEM_CONVECTION_JACOBIAN)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: mode = %d, must be 0 (none), 1 (form) or 2 (jacobian)", me, desc->mode);
  if (desc->mode != STFEM_CONVECTION_NONE) {
    if (!desc->lin_blocks) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: mode = %d needs lin_blocks, the linearisation states", me, desc->mode);
    for (int i = 0; i < desc->n_blocks; ++i)
      if (desc->block_variable[i] == 0 && !desc->lin_blocks[i])
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: mode = %d and lin_blocks[%d] of a velocity block is null", me, desc->mode, i);
  }
  if (stokes_velocity_degree(ctx) == 2)
    return stfem_stokes_vanka_create_linearised(ctx, desc->n_blocks, desc->block_variable, desc->Alpha, desc->Beta, desc->mode, desc->lin_blocks, out);
  if (desc->mode != STFEM_CONVECTION_NONE) // (degree 3 with weak faces: the linear blocks hold the Nitsche terms, the inflow term of a mode is not built)
    if (const int rq = stokes_refuse_inflow_q3(ctx, "stfem_stokes_vanka_create_linearised_space with a convection mode")) return rq;
  return create_per_cell(ctx, desc->n_blocks, desc->block_variable, desc->Alpha, desc->Beta, desc->mode, desc->lin_blocks, 0.0, out, nullptr, 0, 0, true);
}

// The same blocks of the operator WITH the CIP term (stfem_stokes_set_cip, weight STFEM_CIP_WEIGHT_LINEARISATION): K = the assembled
// A(b_j) + C(b_j; .), the weight velocity of C the linearisation state of the column block - in every mode, so lin_blocks is needed even
// with mode 0.  delta0 == 0 is stfem_stokes_vanka_create_linearised.
int stfem_stokes_vanka_create_linearised_cip(stfem_stokes_ctx *ctx, int n_blocks, const int32_t *block_variable, const double *Alpha,
                                             const double *Beta, int mode, const double *const *lin_blocks, double delta0, stfem_stokes_vanka **out)
{
  if (!out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_vanka_create_linearised_cip: out is null");
  if (const int rq = stokes_require_q2(ctx, "stfem_stokes_vanka_create_linearised_cip")) return rq;
  *out = nullptr;
  if (!std::isfinite(delta0)) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_vanka_create_linearised_cip: delta0 is not finite");
  if (delta0 == 0.0) return stfem_stokes_vanka_create_linearised(ctx, n_blocks, block_variable, Alpha, Beta, mode, lin_blocks, out);
  if (!lin_blocks)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_vanka_create_linearised_cip: delta0 = %g needs lin_blocks, the weight velocity of the term", delta0);
  if (block_variable && n_blocks >= 1 && n_blocks <= VK_MAX_BLOCKS)
    for (int i = 0; i < n_blocks; ++i)
      if (block_variable[i] == 0 && !lin_blocks[i])
        return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stfem_stokes_vanka_create_linearised_cip: delta0 = %g and lin_blocks[%d] of a velocity block is null", delta0, i);
  return create_per_cell(ctx, n_blocks, block_variable, Alpha, Beta, mode, lin_blocks, delta0, out);
}

// The per-cell blocks of a z-slab: set up on `extended`, stored and applied on `slab`.  Every refusal before the device is touched.
int stfem_stokes_vanka_create_linearised_partitioned(stfem_stokes_ctx *slab, stfem_stokes_ctx *extended, int n_blocks, const int32_t *block_variable,
                                                     const double *Alpha, const double *Beta, int mode, const double *const *lin_blocks_extended,
                                                     double delta0, int neighbour_mask, int beyond_mask, stfem_stokes_vanka **out)
{
  const char *me = "stfem_stokes_vanka_create_linearised_partitioned";
  if (!out) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: out is null", me);
  *out = nullptr;
  if (!slab || !extended) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: a context is null", me);
  if (!std::isfinite(delta0)) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: delta0 is not finite", me);
  if (neighbour_mask & ~48) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: neighbour_mask %d, only bits 4 and 5 name a z neighbour", me, neighbour_mask);
  if (beyond_mask & ~neighbour_mask)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: beyond_mask %d names a side without a neighbour (neighbour_mask %d)", me, beyond_mask, neighbour_mask);
  if (const int rq = stokes_require_q2(slab, me)) return rq;
  if (const int rq = stokes_require_q2(extended, me)) return rq;
  stfem_stokes_desc ds, de;
  int rc = stfem_stokes_internal_desc(slab, &ds);
  if (rc == STFEM_OK) rc = stfem_stokes_internal_desc(extended, &de);
  if (rc != STFEM_OK) return rc;
  const int ghosts = (neighbour_mask >> 4 & 1) + (neighbour_mask >> 5 & 1);
  if (de.nc[0] != ds.nc[0] || de.nc[1] != ds.nc[1] || de.nc[2] != ds.nc[2] + ghosts || de.pspace != ds.pspace || de.device != ds.device ||
      de.cart != ds.cart)
    return stfem_set_error(STFEM_ERR_SHAPE_MISMATCH, "%s: the extended context (%d x %d x %d cells, pressure space %d) is not the slab (%d x %d x %d, %d) plus %d "
                           "ghost layer(s)", me, de.nc[0], de.nc[1], de.nc[2], de.pspace, ds.nc[0], ds.nc[1], ds.nc[2], ds.pspace, ghosts);
  if (delta0 != 0.0) { // (the refusals of create_linearised_cip)
    if (!lin_blocks_extended) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: delta0 = %g needs lin_blocks, the weight velocity of the term", me, delta0);
    if (block_variable && n_blocks >= 1 && n_blocks <= VK_MAX_BLOCKS)
      for (int i = 0; i < n_blocks; ++i)
        if (block_variable[i] == 0 && !lin_blocks_extended[i])
          return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "%s: delta0 = %g and lin_blocks[%d] of a velocity block is null", me, delta0, i);
  }
  // (without the CIP term nothing reaches beyond a ghost layer: beyond_mask is ignored)
  return create_per_cell(slab, n_blocks, block_variable, Alpha, Beta, mode, lin_blocks_extended, delta0, out, extended, neighbour_mask >> 4 & 1,
                         delta0 != 0.0 ? beyond_mask : 0);
}

// The blocks of a smoother of stfem_stokes_vanka_create_linearised again, for new linearisation states: same mode, same storage
int stfem_stokes_vanka_update(stfem_stokes_vanka *v, const double *const *lin_blocks)
{
  if (!v) return STFEM_ERR_INVALID_ARGUMENT;
  if (!v->cell) return STFEM_ERR_UNSUPPORTED; // (class blocks hold the linear operator only)
  if (v->mode != STFEM_CONVECTION_NONE || v->delta0 != 0.0) { // (the CIP term keeps the delta0 of creation and reads its weight from lin_blocks)
    if (!lin_blocks) return STFEM_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < v->nblk; ++i)
      if (v->var[i] == 0 && !lin_blocks[i]) return STFEM_ERR_INVALID_ARGUMENT;
  }
  STFEM_TRY(hipSetDevice(v->d.device));
  return stokes_cell_vanka_update(v->cell, lin_blocks);
}

// dst = (accumulate ? dst : 0) + omega * (sum over cells of scatter(B_c^-1 gather(src))); blocks in the order of the BlockSlice
// the smoother was created with (velocity blocks: 3 n_velocity_dofs doubles, component-major; pressure blocks: n_pressure_dofs)
int stfem_stokes_vanka_step(stfem_stokes_vanka *v, double *const *dst_blocks, double omega, int accumulate, const double *const *src_blocks,
                            void *stream)
{
  if (!v || !dst_blocks || !src_blocks) return STFEM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < v->nblk; ++i) {
    if (!dst_blocks[i] || !src_blocks[i]) return STFEM_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < v->nblk; ++j)
      if (dst_blocks[i] == src_blocks[j]) return STFEM_ERR_ALIAS;
  }
  TraceScope scope("vanka"); // the reference's TimerOutput scope "vanka" (stmg.h:835)
  STFEM_TRY(hipSetDevice(v->d.device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double *rows = v->d_flat;
  stfem_launch_begin();
  if (v->cell) { // one block per cell: every block streamed once, rows to the scratch array
    const int rc = stokes_cell_vanka_apply(v->cell, src_blocks, &rows, st);
    if (rc != STFEM_OK) return rc;
  } else {
    VankaParams prm;
    std::memset(&prm, 0, sizeof(prm));
    for (int i = 0; i < v->nblk; ++i) {
      prm.src[i] = src_blocks[i];
      prm.dst[i] = dst_blocks[i];
    }
    prm.blocks = v->d_blocks;
    prm.cell = v->d_cellu; prm.cell2 = v->d_cellp; prm.cls = v->d_cls; prm.rowtab = v->d_rowtab;
    prm.nquad = v->nquad; prm.m = v->m; prm.mpad = v->mpad; prm.kpad = v->kpad; prm.p = 2;
    prm.flat = v->d_flat; prm.omega = 1.0;
    const void *k = sv_kernel(v->mtw);
    if (!k) return STFEM_ERR_UNSUPPORTED;
    const int rc = vk_launch(k, dim3(v->nquad, v->parts), &prm, st, "vanka_apply_kernel");
    if (rc != STFEM_OK) return rc;
  }
  StokesCollectParams cp;
  std::memset(&cp, 0, sizeof(cp));
  for (int i = 0; i < v->nblk; ++i) { cp.dst[i] = dst_blocks[i]; cp.var[i] = v->var[i]; cp.rowbase[i] = v->rowbase[i]; }
  cp.y = rows; cp.slot = v->d_slot; cp.nblk = v->nblk; cp.mpad = v->mpad; cp.pdg = v->d.pspace;
  cp.pu = v->degree; cp.npc = vanka::stokes_cell_pressure_dofs(v->degree, true);
  for (int k3 = 0; k3 < 3; ++k3) { cp.nc[k3] = v->d.nc[k3]; cp.ndu[k3] = v->d.ndu[k3]; cp.ndp[k3] = v->d.ndp[k3]; }
  cp.Nu = v->d.Nu; cp.Np = v->d.Np; cp.omega = omega; cp.accumulate = accumulate;
  const long long big = std::max(3 * v->d.Nu, v->d.Np);
  return vk_launch(reinterpret_cast<const void *>(&stokes_vanka_collect_kernel), dim3((unsigned)((big + 255) / 256), v->nblk), &cp, st,
                   "stokes_vanka_collect_kernel");
}

int stfem_stokes_vanka_vmult(stfem_stokes_vanka *v, double *const *dst_blocks, const double *const *src_blocks, void *stream)
{
  return stfem_stokes_vanka_step(v, dst_blocks, 1.0, 0, src_blocks, stream);
}

} // extern "C"
