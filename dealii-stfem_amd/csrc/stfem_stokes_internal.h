// What the translation units of the Stokes two-field operator share (stfem_stokes.hip and stfem_stokes_{cell,coupling,boundary,
// pressure,convection,cip,divergence,traction}.hip): the description of a launch, the context and the launchers.  Not part of the boundary.
#pragma once
#include "stfem_internal.h"
#include "stfem_mapping_q1.h"
#include "stfem_stokes_set.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

// The kernel argument of the linear operator at velocity degree DEG: the geometry and 1D tables of a context (constant, filled once
// by stokes_describe) around the set of one launch (stfem_stokes_set.h; stokes_params<DEG> below writes a StokesSet into it):
//   out_u[o] (=, +=) sum_s wKu[s][o] (nu K u_s - B^T p_s) + wM[s][o] M u_s,  out_p[o] (=, +=) sum_s wKp[s][o] B u_s
// DEG: the velocity degree, FE_Q(DEG)^3 x FE_Q(DEG - 1) / FE_DGP(DEG - 1) with QGauss(DEG + 1).  StokesParams, the description of
// degree 2, is what every kernel of the operator outside the cell kernel takes.
template <int DEG> struct StokesParamsT {
  const double *vertices; // device, (nc+1)^3 * 3
  int ncx, ncy, ncz;
  int ndu[3], ndp[3];     // DEG nc + 1, (DEG - 1) nc + 1
  long long Nu, Np;
  int dmask;
  double nu;
  // the set of this launch, member for member a StokesSet
  int nsrc;
  const double *us[MAXSRC], *ps[MAXSRC];
  int nout;
  double *out_u[MAXOUT], *out_p[MAXOUT]; // (nullptr: this part of the pair is not written)
  // [source][destination pair]: the kernels with one source walk row 0 with the destination index, as they walk out_u / out_p
  // (with the destination index first that walk needed a second scaled index: more scalar registers spilled in the cell kernel)
  double wKu[MAXSRC][MAXOUT], wKp[MAXSRC][MAXOUT], wM[MAXSRC][MAXOUT];
  int store_u[MAXOUT], store_p[MAXOUT]; // 1: the first cell to touch a DoF (lowest colour) stores, the others add; 0: all add
  // FE_Q(DEG) and FE_Q(DEG - 1) on Gauss-Lobatto nodes at the Gauss points: [q*(DEG+1)+a], [q*(DEG+1)+a], [q*DEG+a]
  double Su[(DEG + 1) * (DEG + 1)], Du[(DEG + 1) * (DEG + 1)], Sp[(DEG + 1) * DEG];
  double xq[DEG + 1], wq[DEG + 1];
  int interleave;             // cell -> half-wave assignment at degree 2 (see the cell kernel)
  int colour;                 // this launch handles the cells with (cx & 1) + 2 (cy & 1) + 4 (cz & 1) == colour
  int cart;                   // axis-aligned uniform cells: constant diagonal Jacobian
  double hinv[3], detJ;       // 1 / h_d, hx hy hz
  // pressure space: 0 = FE_Q(DEG - 1) on its node lattice, 1 = FE_DGP(DEG - 1), the reference's dGPressure (tests/tp_03stokes.cc:83-86):
  // per cell the products l_i(xi) l_j(eta) l_k(zeta), i + j + k <= DEG - 1, i fastest, of the orthonormal Legendre functions
  // l_1(x) = sqrt 3 (2 x - 1), l_2(x) = sqrt 5 (6 x^2 - 6 x + 1); degree 2: deal.II's basis 1, l(xi), l(eta), l(zeta), p[cell * 4 + j]
  int pdg;
  double lq[DEG - 1][DEG + 1]; // l_1 (and l_2) at the Gauss points
};
using StokesParams = StokesParamsT<2>;
static_assert(sizeof(StokesParams) == 1440, "the degree-2 description is the argument of every Stokes kernel: its layout stays");
static_assert(sizeof(StokesParamsT<3>) == 1656, "the degree-3 description is the argument of the degree-3 cell kernel: its layout stays");
static_assert(offsetof(StokesParams, nsrc) == 80 && offsetof(StokesParamsT<3>, nsrc) == 80, "the set follows the mesh part");
static_assert(offsetof(StokesParams, Su) == 1120 && offsetof(StokesParamsT<3>, Su) == 1120, "the 1D tables follow the set");

// The coupling kernels of the Kronecker path (stfem_stokes_coupling.hip)
struct CouplingParams {
  int ncx, ncy, ncz;
  int ndu[3], ndp[3];
  long long Nu;
  int dmask, pdg;
  double h[3];
  // 1D reference integrals, Q2 node a: FE_Q(1): N[a][j], C[a][j], j = 0, 1; FE_DGP(1): N[a][0] = int phi_a, N[a][1] = int l phi_a (same for C)
  double N[3][2], C[3][2];
  int nsrc, nout;
  const double *u[MAXSRC], *p[MAXSRC];
  double *out_u[MAXOUT], *out_p[MAXOUT];
  double wKu[MAXOUT][MAXSRC], wKp[MAXOUT][MAXSRC]; // [output][source]
  int store_p[MAXOUT];
};

// The weak (Nitsche) boundary faces (stfem_stokes_boundary.hip)
struct BoundaryParams {
  int weak_mask;
  double gamma1, gamma2;
  int foff[7];             // first work item (cell of a face, t1 fastest) of every face, [6] = total
  const double *g;         // rhs mode: Dirichlet data at the face quadrature points [point][3]; nullptr: operator mode
  // end-point tables [s * n + a] of the context's degree: FE_Q(DEG) values / derivatives (n = DEG + 1), FE_Q(DEG - 1) values (n = DEG)
  // at 0 and 1; sized for degree 3
  double Eu[8], EDu[8], Ep[6];
};

// The convection launches of the Navier-Stokes modes (stfem_stokes_convection.hip): a description of their own, so that StokesParams,
// the by-value argument of every kernel of the linear operator, stays what it is.
//   out_u[o] += sum_s wKu[s][o] C(b_s, u_s),   C = C_form(b, u) (form) or C_form(b, u) + C_form(u, b) (jacobian),
//   C_form(b, u)(v) = - int (u (x) b) : grad v  - int_{weak faces} min(b.n, 0) u.v
// Geometry and tables are copied from the context's description of its degree, sources and weights from the StokesSet of the same
// launches; only destinations with a non-zero wKu are listed (stokes_k_destinations).  DEG: the velocity degree, as in StokesParamsT.
template <int DEG> struct ConvectionParamsT {
  const double *vertices;
  int ncx, ncy, ncz;
  int ndu[3];
  long long Nu;
  int dmask;
  int nsrc;
  const double *us[MAXSRC], *bs[MAXSRC]; // source and linearisation velocity of every source
  int nout;
  double *out_u[MAXOUT];
  double wKu[MAXSRC][MAXOUT];
  double Su[(DEG + 1) * (DEG + 1)], Du[(DEG + 1) * (DEG + 1)]; // [q*(DEG+1)+a]
  double xq[DEG + 1], wq[DEG + 1];
  int interleave, colour, cart;
  double hinv[3], detJ;
};
// Degree 2 with the inflow term on the weak faces (a degree-3 context has none): what the launcher fills and the inflow kernel takes.
// Not members of the common part: behind the degree-3 description they move the hidden kernel arguments (the grid size, read in
// the prologue) into a 64-byte line of their own, 2 us per vmult on 32^3 cells of a box (profiles/stokes_convection_merge.txt)
struct ConvectionParams : ConvectionParamsT<2> {
  int weak_mask;
  int foff[7];
  double Eu[6];
};

// The CIP interior-face launches (stfem_stokes_cip.hip), again a description of their own:
//   out_u[o] += sum_s wKu[s][o] C(w_s; u_s),   C(w; u)(v) = sum_F int_F delta0 h_F^2 / pa (w.n)^2 [d_n u] . [d_n v] dA
// Geometry and tables are copied from the context's description, the weights from the StokesSet of the same launches; only destinations
// with a non-zero wKu are listed (stokes_k_destinations).
struct CipParams {
  const double *vertices;
  int ncx, ncy, ncz;
  int ndu[3];
  long long Nu;
  int dmask;
  int nsrc;
  const double *us[MAXSRC], *ws[MAXSRC]; // source and weight velocity of every source
  int nout;
  double *out_u[MAXOUT];
  double wKu[MAXSRC][MAXOUT];
  double Su[9], Du[9], Eu[6], EDu[6]; // [q*3+a] at the Gauss points, [s*3+a] at the end points 0 and 1
  double xq[3], wq[3];
  int colour, cart;
  double hinv[3], detJ;
  double scale; // delta0 / pa
};
// The same at velocity degree 3 (stokes_cip_q3_kernel): FE_Q(3) tables, QGauss(4).  A description of its own: CipParams is the
// by-value argument of the degree-2 kernel, and its layout stays.
struct CipQ3Params {
  const double *vertices;
  int ncx, ncy, ncz;
  int ndu[3];
  long long Nu;
  int dmask;
  int nsrc;
  const double *us[MAXSRC], *ws[MAXSRC];
  int nout;
  double *out_u[MAXOUT];
  double wKu[MAXSRC][MAXOUT];
  double Su[16], Du[16], Eu[8], EDu[8]; // [q*4+a] at the Gauss points, [s*4+a] at the end points 0 and 1
  double xq[4], wq[4];
  int colour, cart;
  double hinv[3], detJ;
  double scale; // delta0 / pa, pa = 3^3.5
};
// The same on a z-slab with neighbours (stfem_stokes_set_cip_neighbours): the kernel's SLAB instantiations take this description, the
// others CipParams as before.
struct CipSlabParams : CipParams {
  int neighbours; // bit 4: a slab below (face 4 of the bottom cell layer is interior), bit 5: a slab above
  // general meshes: two vertex planes per side, [ghost plane | the slab's plane 0] below and [the slab's top plane | ghost plane]
  // above, (ncx + 1)(ncy + 1) * 3 doubles each - the neighbour cell of an interface face as cell layer 0 of a mesh of its own
  const double *ghost_vertices[2];
  // per source the two velocity DoF planes beyond each interface, [comp][plane, ascending z][ndy][ndx] (stfem_stokes_cip_pack)
  const double *ghost_lo[MAXSRC], *ghost_hi[MAXSRC];
};

struct stfem_stokes_ctx {
  int device = 0;
  int nc[3] = {0, 0, 0};
  int ndu[3] = {0, 0, 0}, ndp[3] = {0, 0, 0};
  long long Nu = 0, Np = 0;
  int dmask = 0;
  double nu = 1.0;
  double *d_vertices = nullptr;
  int n_cu = 256;
  int pspace = 0; // 0 = FE_Q(degree - 1), 1 = FE_DGP(degree - 1)
  // velocity degree: 2, or 3 (stfem_stokes_create_space): the linear cell operator, the convection term of the Navier-Stokes modes,
  // the divergence functional and the pressure space helpers.
  int degree = 2;
  // what does not depend on the degree (stokes_describe): axis-aligned uniform cells, and on those 1 / h_d and hx hy hz
  bool cart = false;
  double hinv[3] = {0, 0, 0}, detJ = 0;
  // Geometry and 1D tables as the kernels of degree DEG take them: the description of the context's own degree, the only one
  // stokes_create_degree fills.  Everything outside it reaches the two through desc<DEG>(), under stokes_with_degree or on a path that
  // stokes_require_q2 has kept to degree 2.
  StokesParams base{};
  StokesParamsT<3> base3{};
  template <int DEG> const StokesParamsT<DEG> &desc() const
  {
    assert(degree == DEG);
    if constexpr (DEG == 3) return base3;
    else return base;
  }
  bool cell_launched = false;
  int cell_plan[2] = {0, 0}; // workgroups and longest run of cells per cell slot of the last colour launch (stfem_stokes_last_cell_plan)
  bool convection_launched = false;
  int convection_plan[2] = {0, 0}; // the same of the last convection colour launch (stfem_stokes_last_convection_plan)
  bool divergence_launched = false;
  int divergence_plan[2] = {0, 0}; // workgroups and longest run of cells per cell slot of the last divergence launch (stfem_stokes_last_divergence_plan)
  // axis-aligned uniform meshes: the scalar FE_Q(2) context whose pencil sweep applies nu K + wM M to the velocity components,
  // and the 1D tables of the coupling kernels
  stfem_ctx *scalar = nullptr;
  bool last_grad_in_sweep = false; // the last vmult's velocity sweep added - B^T p itself (stfem_stokes_last_sweep_plan)
  CouplingParams coupling;
  // the divergence kernel reads the sources and writes the pressure destinations only: it runs beside the velocity sweep on the
  // side stream - ONE per device, shared by all Stokes contexts (stokes_side_stream), not owned - forked from and joined to the
  // caller's stream with the two events of this context
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  stfem_ctx *pressure_space = nullptr; // scalar context behind the pressure vectors (stfem_stokes_pressure_ctx), made on demand
  double *d_pq = nullptr;              // exact values at the pressure quadrature points (stfem_stokes_pressure_difference)
  size_t pq_points = 0;
  double *d_pred = nullptr;            // its reduction results
  double *d_div = nullptr;             // cell values and their sum of stfem_stokes_divergence (n_cells + 1), made on demand
  double *d_trac = nullptr;            // item values and their sums of stfem_stokes_drag_lift (trac_cap doubles), made on demand
  size_t trac_cap = 0;
  // weak (Nitsche) / outflow boundary faces (operators.h:1206-1211): bit f = 2 d + s
  int weak_mask = 0, outflow_mask = 0;
  double penalty1 = 20.0, penalty2 = 10.0;
  BoundaryParams bnd;
  double *d_g = nullptr; // Dirichlet data at the face quadrature points (stfem_stokes_nitsche_rhs)
  size_t g_points = 0;
  bool face_launched = false;
  int face_plan[2] = {0, 0}; // workgroups and longest run of items per wave / half-wave of the last boundary colour launch (stfem_stokes_last_face_plan)
  std::vector<double> h_vertices;
  // CIP interior-face stabilisation (stfem_stokes_set_cip): 0.0 = no launches; whose velocity weighs it (STFEM_CIP_WEIGHT_*)
  double cip_delta0 = 0.0;
  int cip_weight = 0;
  bool cip_launched = false;
  int cip_plan[2] = {0, 0}; // workgroups and passes of the grid-stride loop of the last CIP colour launch (stfem_stokes_last_cip_plan)
  // the slab's z neighbours for that term (stfem_stokes_set_cip_neighbours): mask, the two-plane vertex arrays of
  // CipSlabParams::ghost_vertices (general meshes), and the ghost planes bound to velocity sources (stfem_stokes_cip_bind_ghosts)
  int cip_neighbours = 0;
  double *d_cip_vertices[2] = {nullptr, nullptr};
  struct CipBinding { const double *src, *lower, *upper; };
  std::vector<CipBinding> cip_bindings;
};

// The one place where the context's degree becomes a template parameter: f(std::integral_constant<int, DEG>) at the context's DEG
template <class F> inline auto stokes_with_degree(const stfem_stokes_ctx *c, F &&f)
{
  return c->degree == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 2>{});
}

// The kernel argument of a launch: the context's description of degree DEG with `set` written into it, unused slots null
template <int DEG> inline StokesParamsT<DEG> stokes_params(const stfem_stokes_ctx *c, const StokesSet &set)
{
  StokesParamsT<DEG> prm = c->desc<DEG>();
  prm.nsrc = set.nsrc; prm.nout = set.nout;
  for (int s = 0; s < MAXSRC; ++s) {
    prm.us[s] = s < set.nsrc ? set.us[s] : nullptr;
    prm.ps[s] = s < set.nsrc ? set.ps[s] : nullptr;
    for (int o = 0; o < MAXOUT; ++o) { prm.wKu[s][o] = set.wKu[s][o]; prm.wKp[s][o] = set.wKp[s][o]; prm.wM[s][o] = set.wM[s][o]; }
  }
  for (int o = 0; o < MAXOUT; ++o) {
    prm.out_u[o] = o < set.nout ? set.out_u[o] : nullptr;
    prm.out_p[o] = o < set.nout ? set.out_p[o] : nullptr;
    prm.store_u[o] = set.store_u[o]; prm.store_p[o] = set.store_p[o];
  }
  return prm;
}

template <typename Params> // (StokesParamsT or ConvectionParamsT)
__device__ __forceinline__ bool constrained_u(const Params &prm, int ix, int iy, int iz)
{
  return ((prm.dmask & 1) && ix == 0) || ((prm.dmask & 2) && ix == prm.ndu[0] - 1) ||
         ((prm.dmask & 4) && iy == 0) || ((prm.dmask & 8) && iy == prm.ndu[1] - 1) ||
         ((prm.dmask & 16) && iz == 0) || ((prm.dmask & 32) && iz == prm.ndu[2] - 1);
}

// Orders the LDS traffic of one wave (a cell lives in one half of a wave: no workgroup barrier needed)
__device__ __forceinline__ void wave_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// FE_DGP(DEG - 1): function f is l_i(xi) l_j(eta) l_k(zeta) with i + j + k <= DEG - 1, i fastest (l_n: the orthonormal Legendre
// functions on [0, 1]); d[f] = (i, j, k).  Degree 2: 1, l(xi), l(eta), l(zeta), deal.II's basis.  (The cell kernel and the boundary kernel)
template <int DEG> struct DgpDegrees {
  int d[DEG * (DEG + 1) * (DEG + 2) / 6][3];
};
template <int DEG> constexpr DgpDegrees<DEG> dgp_degrees()
{
  DgpDegrees<DEG> r{};
  int f = 0;
  for (int k = 0; k < DEG; ++k)
    for (int j = 0; j + k < DEG; ++j)
      for (int i = 0; i + j + k < DEG; ++i, ++f) { r.d[f][0] = i; r.d[f][1] = j; r.d[f][2] = k; }
  return r;
}

// What the sum-factorised cell kernels (stokes_cell_kernel in stfem_stokes_cell.hip, stokes_convection_kernel in
// stfem_stokes_convection.hip) share.
// Which 1D tables a lane holds in registers (Coef, with dot below).  The rows of its quadrature index (evaluation) always.  The columns
// of its node index (integration) and the pressure tables at degree 2 only: at degree 3 they are 44 doubles more, and with all of them
// in registers five of the eight instantiations of the cell kernel need 256 VGPRs and spills to AGPRs, one wave per SIMD
// (profiles/stokes_q3.txt).
template <int DEG> constexpr bool COLUMNS_HELD = DEG == 2;
// The lane's N coefficients p[0], p[STRIDE], ... of a 1D table in LDS: HELD - copied into registers once, for the whole kernel;
// otherwise read where they are used.
template <int N, int STRIDE, bool HELD> struct Coef {
  const double *p;
  double r[HELD ? N : 1];
  __device__ __forceinline__ explicit Coef(const double *q) : p(q)
  {
    if constexpr (HELD) {
#pragma unroll
      for (int n = 0; n < N; ++n) r[n] = q[n * STRIDE];
    }
  }
  __device__ __forceinline__ double operator[](int n) const
  {
    if constexpr (HELD) return r[n];
    else return p[n * STRIDE];
  }
};
// sum_n w[n] v[n * stride], ascending, one fma chain.  The values are read last first: the compiler's order of the LDS reads in the
// integration stages follows the order here, and this one is the faster (profiles/stokes_cell_merge.txt)
template <int N, class W> __device__ __forceinline__ double dot(const W &w, const double *v, int stride = 1)
{
  double x[N];
#pragma unroll
  for (int n = N - 1; n >= 0; --n) x[n] = v[n * stride];
  double s = w[0] * x[0];
#pragma unroll
  for (int n = 1; n < N; ++n) s = fma(w[n], x[n], s);
  return s;
}
// Their launchers: persistent workgroups, exactly as many as stay resident - asked once per instantiation (`cached`), not on the
// launch path
inline int stokes_resident(int &cached, const void *kern)
{
  if (cached < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&cached, kern, 256, 0) != hipSuccess || cached < 1)) cached = 2;
  return cached;
}
// and the eight colour launches, ascending, like every colour sequence of the operator: launch(colour, grid) for every colour that has
// cells, with min(ceil(n / cells), n_cu * per_cu) workgroups of `cells` cells at a time; plan = (workgroups, longest run of cells per
// cell slot) of the last one.  STFEM_STOKES_Q3_WORKGROUPS=<n>, read at every call: at most n workgroups per colour launch (tests:
// several cells per wave or half-wave on a small mesh)
template <class Launch> inline void stokes_colour_launches(const stfem_stokes_ctx *c, int cells, int per_cu, int plan[2], Launch launch)
{
  long long cap = 0;
  if (const char *e = getenv("STFEM_STOKES_Q3_WORKGROUPS")) cap = std::max(1ll, atoll(e));
  for (int colour = 0; colour < 8; ++colour) {
    const long long n = (long long)((c->nc[0] - (colour & 1) + 1) / 2) * ((c->nc[1] - ((colour >> 1) & 1) + 1) / 2) *
                        ((c->nc[2] - (colour >> 2) + 1) / 2);
    if (n == 0) continue;
    long long grid = std::min<long long>((n + cells - 1) / cells, (long long)c->n_cu * per_cu);
    if (cap) grid = std::min(grid, cap);
    launch(colour, (unsigned)grid);
    plan[0] = (int)grid;
    plan[1] = (int)((n + grid * cells - 1) / (grid * cells));
  }
}

// What the CIP kernel of the operator (stfem_stokes_cip.hip) and the CIP cell matrices of the per-cell Vanka blocks
// (stfem_stokes_vanka_cell.hip) share.
// The face tables: (g0, g1, g2) = d phi_n / d xi_e of FE_Q(2) node n at point q = q1 + 3 q2 (lower tangential axis fastest) of face
// f = 2 d + s, from the 1D tables tS / tD [q * 3 + a] at the Gauss points and tE / tED [s * 3 + a] at the end points 0 and 1
__device__ __forceinline__ void cip_face_gradient(const double *tS, const double *tD, const double *tE, const double *tED, int f, int q, int n,
                                                  double &g0, double &g1, double &g2)
{
  const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0;
  const int ka = n % 3, kb = (n / 3) % 3, kc = n / 9, qa = q % 3, qb = q / 3;
  // (selects, no arrays indexed at run time: those would live in scratch)
  const int t2 = d == 2 ? 1 : 2;
  const int kd = d == 0 ? ka : (d == 1 ? kb : kc), k1 = t1 == 0 ? ka : kb, k2 = t2 == 1 ? kb : kc;
  const double vd = tE[s * 3 + kd], v1 = tS[qa * 3 + k1], v2 = tS[qb * 3 + k2];
  const double gd = tED[s * 3 + kd] * v1 * v2, gt1 = vd * tD[qa * 3 + k1] * v2, gt2 = vd * v1 * tD[qb * 3 + k2];
  g0 = d == 0 ? gd : gt1;
  g1 = d == 1 ? gd : (d == 0 ? gt1 : gt2);
  g2 = d == 2 ? gd : gt2;
}

#pragma GCC visibility push(hidden) // (the library exports what include/stfem.h declares)

// FE_Q(2) values / derivatives at the end points 0 and 1, [s * 3 + a] (stfem_stokes_cip.hip)
void stokes_cip_end_tables(double Eu[6], double EDu[6]);
// Every launcher takes the set of its launches and builds its kernel argument from the context's description of its degree.
// The eight colour launches of the cell kernel (stfem_stokes_cell.hip), at the context's degree: general meshes at degree 2, boxes
// included at degree 3
int stokes_cell_launch(stfem_stokes_ctx *c, const StokesSet &set, hipStream_t st);
// The cell matrices of A(b) for the per-cell Vanka blocks (stfem_stokes_vanka_cell.hip), at the context's degree: `count` cells from cell0,
// Ac[cell][nl][nl] with nl = 81 + 8 / 4 or 192 + 27 / 10 (FE_Q / FE_DGP pressure), Mc[cell][27 or 64][.] (nullptr: not wanted)
int stokes_cell_matrices_launch(const stfem_stokes_ctx *c, double *Ac, double *Mc, long long cell0, unsigned count, int mode, const double *b);
// The coupling kernels (stfem_stokes_coupling.hip): out_u -= sum_s wKu B^T p_s; out_p (=, +=) sum_s wKp B u_s.  A failed launch is
// left to the caller's stfem_launch_end (stokes_cart_launch).
void stokes_grad_launch(const CouplingParams &k, hipStream_t st);
void stokes_div_launch(const CouplingParams &k, long long Np, hipStream_t st);
// The eight colour launches of the boundary kernel (stfem_stokes_boundary.hip), at the context's degree; d_g: the Dirichlet data of
// the rhs mode, or nullptr.  STFEM_STOKES_FACE_WORKGROUPS=<n>, read at every launch: at most n workgroups per colour launch.
int stokes_boundary_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *d_g, hipStream_t st);
// The convection launches after those of the linear operator (stfem_stokes_convection.hip), at the context's degree: eight colour
// launches of the cell kernel, then, with weak faces (degree 2), eight of the inflow-face kernel.  mode: STFEM_CONVECTION_FORM /
// _JACOBIAN; lin[s]: the linearisation velocity of source s.  Nothing is launched when all wKu of the set are zero.
// STFEM_STOKES_Q3_WORKGROUPS=<n>, read at every launch, caps the workgroups of the colour launches at either degree, as it caps
// those of stokes_cell_launch.
int stokes_convection_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *lin, int mode, hipStream_t st);
// The CIP launches after those (stfem_stokes_cip.hip): eight colour launches; weight[s]: the weight velocity of source s.  Nothing is
// launched with delta0 == 0, on a mesh without interior faces, for a colour without cells or when all wKu of the set are zero.
int stokes_cip_launch(stfem_stokes_ctx *c, const StokesSet &set, const double *const *weight, double delta0, hipStream_t st);
// On a slab with neighbours (stfem_stokes_set_cip_neighbours) and delta0 != 0 that launch looks up the ghost planes bound to each
// source; the entry points ask this before anything touches the device: STFEM_ERR_INVALID_ARGUMENT, with its reason, for a velocity
// source without a binding or with a binding that lacks a side
int stokes_cip_source_ready(const stfem_stokes_ctx *c, const double *src_u);
#pragma GCC visibility pop

