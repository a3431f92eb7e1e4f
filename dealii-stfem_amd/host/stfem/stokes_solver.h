// The solver side of the Stokes slab problem (tests/tp_03stokes.cc:536-560, 840-1090) over the C-ABI: the two-variable block vector
// with the vector arithmetic of the Krylov solver, the relaxation smoother around the two-variable Vanka smoother, and the first-order
// time integrator of include/time_integrators.h:30-336 with a velocity force, for FE_Q(2)^3 x FE_Q(1) (BASELINE configs[4]).
// Over an operator of velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)): StokesSpaces, StokesBlockVector, StokesSystem,
// RelaxedVankaStokes, PressureErrorCalculator and the zero-mean shift of StokesSlab, through the _space entries of
// include/stfem_stokes_pressure_space.h; GMGStokes, the time integrators and partitions refuse it.
// Control flow only: every vector operation, integral and operator application is a call into libstfem_hip.so.
#pragma once
#include "stmg.h"
#include "stokes.h"
#include "time_integrators.h"

#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace stfem {

// The scalar spaces behind the two variables, for the velocity degree k = 2 or 3 the Stokes context was made with
// (stfem_stokes_get_space): a velocity component is a FE_Q(k) function (with the velocity's strong constraints), the pressure a
// FE_Q(k - 1) function without constraints.  Their contexts serve the vector arithmetic, the load vectors, the interpolation and
// the error norms of the Stokes vectors (VectorTools::* per variable in the reference).
struct StokesSpaces {
  // q2: the scalar FE_Q(k) space of a velocity component; q1: the pressure space's context (FE_Q(k - 1): a real one; FE_DGP(k - 1): a
  // carrier for the vector arithmetic).  (The names are those of k = 2.)
  std::shared_ptr<Context> q2, q1;
  stfem_stokes_ctx *stokes;
  StokesSpaces(const Mesh &mesh, stfem_stokes_ctx *stokes_) : stokes(stokes_)
  {
    stfem_stokes_space_desc sd{};
    check(stfem_stokes_get_space(stokes, &sd), "stfem_stokes_get_space");
    velocity_degree = unsigned(sd.velocity_degree);
    MatrixFreeOperator<3, 1, double> a(mesh, velocity_degree, 0.0, 1.0);
    q2 = a.context();
    stfem_ctx *pc = nullptr;
    check(stfem_stokes_pressure_ctx_space(stokes, &pc), "stfem_stokes_pressure_ctx_space");
    q1 = std::make_shared<Context>(pc, false);
    const int pressure_degree = sd.velocity_degree - 1;
    int32_t nd[3];
    check(stfem_n_dofs_1d(pc, nd), "stfem_n_dofs_1d");
    // (FE_DGP(1): 2 x 2 x n_cells, FE_DGP(2): 2 x 5 x n_cells; FE_Q(k - 1): (k - 1) ncell + 1 nodes per direction)
    carrier = nd[0] != pressure_degree * mesh.ncell[0] + 1 || nd[1] != pressure_degree * mesh.ncell[1] + 1 || nd[2] != pressure_degree * mesh.ncell[2] + 1;
    q1->degree = carrier ? 1 : unsigned(pressure_degree);
    box = mesh.vertices.empty();
  }
  // z-slab partition (the mesh is this rank's slab, interface faces taken out of its Dirichlet mask): the operator leaves partial
  // sums in the interface planes of every velocity component and of the pressure (tests/test_gpu_stokes.py::
  // test_stokes_on_z_slabs_equals_whole_mesh); StokesSystem::vmult completes them with the scalar spaces' add-exchange
  // (stfem_halo_begin / end), inner products count owned planes only (stfem_dot_global) - as for the scalar operators.  FE_DGP(1)
  // pressure DoFs are cell-local: nothing to exchange and every entry owned, and the "planes" of the carrier context are the DoFs of
  // the slab's first and last cell - it gets the communicator (its inner products are summed over the ranks) and no neighbours
  // The CIP term (delta0 != 0) crosses the interfaces once the operator knows its neighbours (stfem_stokes_set_cip_neighbours): on a
  // box from this call alone; on a general mesh when the vertex plane one cell layer beyond each interface is handed in
  // ((ncx + 1)(ncy + 1) * 3 doubles) - without them the operator is not told, and StokesSystem::vmult / form refuse delta0 != 0 on
  // such a slab (the term would lack the interface faces).  Told, they pack, exchange and bind the ghost planes of their velocity
  // sources.  The slabs are cuts of one mesh: on a box all of them have this slab's cell size.
  void set_partition(const std::shared_ptr<Communicator> &comm, int lower_rank, int upper_rank, const double *lower_vertices = nullptr,
                     const double *upper_vertices = nullptr)
  {
    if (velocity_degree != 2) throw Error(STFEM_ERR_UNSUPPORTED, "StokesSpaces::set_partition: slabs are not built at velocity degree 3");
    for (auto &c : {q2, q1}) {
      const bool exchanges = c == q2 || !carrier;
      c->comm = comm;
      c->lower_rank = exchanges ? lower_rank : -1;
      c->upper_rank = exchanges ? upper_rank : -1;
    }
    const bool planes = box || ((lower_rank < 0 || lower_vertices) && (upper_rank < 0 || upper_vertices));
    cip_neighbours = comm && planes ? (lower_rank >= 0 ? 16 : 0) | (upper_rank >= 0 ? 32 : 0) : 0;
    check(stfem_stokes_set_cip_neighbours(stokes, cip_neighbours, lower_vertices, upper_vertices), "stfem_stokes_set_cip_neighbours");
  }
  unsigned velocity_degree = 2;
  bool carrier = false; // q1 is the FE_DGP carrier context
  bool box = true;      // axis-aligned uniform mesh (no vertex array)
  int cip_neighbours = 0;
};

// BlockVectorT over a two-variable BlockSlice (LinearAlgebra::distributed::BlockVector with velocity and pressure blocks)
class StokesBlockVector {
public:
  StokesBlockVector() = default;
  void reinit(const std::shared_ptr<StokesSpaces> &spaces, stfem_stokes_ctx *stokes, const BlockSlice &slice)
  {
    spaces_ = spaces; stokes_ = stokes; slice_ = std::make_shared<BlockSlice>(slice);
    blocks_.clear();
    views_.clear();
    const size_t nu = size_t(stfem_stokes_n_velocity_dofs(stokes));
    for (unsigned i = 0; i < slice.n_blocks(); ++i) {
      const int var = int(slice.decompose(i)[1]);
      blocks_.emplace_back(stokes, var);
      BlockVectorT<double> v;
      if (var == 0) {
        void *ptrs[3] = {blocks_.back().data(), blocks_.back().data() + nu, blocks_.back().data() + 2 * nu};
        v.wrap(spaces->q2, ptrs, 3);
      } else {
        void *ptrs[1] = {blocks_.back().data()};
        v.wrap(spaces->q1, ptrs, 1);
      }
      views_.push_back(std::move(v));
    }
  }
  bool empty() const { return blocks_.empty(); }
  unsigned n_blocks() const { return unsigned(blocks_.size()); }
  std::vector<StokesVector> &blocks() { return blocks_; }
  const std::vector<StokesVector> &blocks() const { return blocks_; }
  // block i as a block vector of its scalar space (velocity: the three components)
  BlockVectorT<double> &view(unsigned i) { return views_.at(i); }
  const BlockVectorT<double> &view(unsigned i) const { return views_.at(i); }
  const std::shared_ptr<StokesSpaces> &spaces() const { return spaces_; }
  stfem_stokes_ctx *stokes() const { return stokes_; }
  const BlockSlice &slice() const { return *slice_; }

private:
  std::shared_ptr<StokesSpaces> spaces_;
  stfem_stokes_ctx *stokes_ = nullptr;
  std::shared_ptr<BlockSlice> slice_;
  std::vector<StokesVector> blocks_;
  std::vector<BlockVectorT<double>> views_;
};

inline void reinit_like(StokesBlockVector &v, const StokesBlockVector &x)
{
  if (v.empty()) v.reinit(x.spaces(), x.stokes(), x.slice());
}
// all blocks in one launch (stfem_axpby_many: the blocks of the two variables differ in length)
inline void axpby(double a, const StokesBlockVector &x, double b, StokesBlockVector &y, void *stream = nullptr)
{
  const unsigned nb = y.n_blocks();
  std::vector<int64_t> len(nb);
  std::vector<const void *> px(nb);
  std::vector<void *> py(nb);
  for (unsigned i = 0; i < nb; ++i) {
    if (x.blocks()[i].size() != y.blocks()[i].size()) throw Error(STFEM_ERR_SHAPE_MISMATCH, "axpby: block sizes");
    len[i] = int64_t(y.blocks()[i].size());
    px[i] = x.blocks()[i].data();
    py[i] = y.blocks()[i].data();
  }
  check(stfem_axpby_many(y.spaces()->q2->h, int(nb), len.data(), a, px.data(), b, py.data(), stream), "stfem_axpby_many");
}
inline void set_zero(StokesBlockVector &v, void *stream = nullptr) { axpby(0.0, v, 0.0, v, stream); }
inline double dot(const StokesBlockVector &a, const StokesBlockVector &b)
{
  double s = 0.0;
  for (unsigned i = 0; i < a.n_blocks(); ++i) s += dot(a.view(i), b.view(i));
  return s;
}
inline double norm(const StokesBlockVector &x) { return std::sqrt(dot(x, x)); }
// the Gram-Schmidt step of the Krylov solver: classical scheme, the k inner products of a pass in one launch per block
// (stfem_multi_dot on the block's scalar view, summed over the blocks on the host), the k updates in one launch per block
// (stfem_multi_axpy); a second pass when the first cancelled most of w, as for the scalar systems (time_integrators.h)
inline double orthogonalize(const std::vector<StokesBlockVector> &vs, unsigned k, StokesBlockVector &w, double *h)
{
  const unsigned nb = w.n_blocks();
  std::vector<const stfem_vec *> handles(k);
  std::vector<double> part(k), minus(k);
  auto pass = [&](double *hh) {
    for (unsigned i = 0; i < k; ++i) hh[i] = 0.0;
    for (unsigned b = 0; b < nb; ++b) {
      for (unsigned i = 0; i < k; ++i) handles[i] = vs[i].view(b).handle();
      check(stfem_multi_dot(w.view(b).context()->h, int(k), handles.data(), w.view(b).handle(), 0, part.data(), nullptr), "stfem_multi_dot");
      for (unsigned i = 0; i < k; ++i) hh[i] += part[i];
    }
    for (unsigned i = 0; i < k; ++i) minus[i] = -hh[i];
    for (unsigned b = 0; b < nb; ++b) {
      for (unsigned i = 0; i < k; ++i) handles[i] = vs[i].view(b).handle();
      check(stfem_multi_axpy(w.view(b).context()->h, int(k), minus.data(), handles.data(), w.view(b).handle(), nullptr), "stfem_multi_axpy");
    }
  };
  if (k == 0 || k > 240 || w.spaces()->q2->comm) { // (partitioned vectors: the modified scheme with reducing inner products)
    for (unsigned i = 0; i < k; ++i) {
      h[i] = dot(w, vs[i]);
      axpby(-h[i], vs[i], 1.0, w);
    }
    return norm(w);
  }
  const double before = dot(w, w);
  pass(h);
  double after = dot(w, w);
  if (!(after > 0.01 * before)) {
    std::vector<double> h2(k);
    pass(h2.data());
    for (unsigned i = 0; i < k; ++i) h[i] += h2[i];
    after = dot(w, w);
  }
  return std::sqrt(std::max(after, 0.0));
}

// SystemMatrixStokes on StokesBlockVector (the operator interface the solver consumes)
template <int dim, typename Number> class StokesSystem {
public:
  StokesSystem(const SystemMatrixStokes<dim, Number> &A, const std::shared_ptr<StokesSpaces> &spaces, stfem_stokes_ctx *stokes, const BlockSlice &slice)
    : A(A), spaces(spaces), stokes(stokes), slice(slice)
  {}
  void initialize_dof_vector(StokesBlockVector &v) const { v.reinit(spaces, stokes, slice); }
  void vmult(StokesBlockVector &dst, const StokesBlockVector &src, void *stream = nullptr) const
  {
    bind_cip_ghosts(src, stream);
    A.vmult(dst.blocks(), src.blocks(), stream);
    if (spaces->q2->comm) // partitioned: dst.compress(add) on every block through its scalar view
      for (unsigned b = 0; b < dst.n_blocks(); ++b) compress_add(*dst.view(b).context(), dst.view(b).handle(), stream);
  }
  // the nonlinear weak form (SystemMatrixStokes::form) and the linearisation vector of both (referred to, not copied)
  void form(StokesBlockVector &dst, const StokesBlockVector &src, void *stream = nullptr) const
  {
    bind_cip_ghosts(src, stream);
    A.form(dst.blocks(), src.blocks(), stream);
    if (spaces->q2->comm)
      for (unsigned b = 0; b < dst.n_blocks(); ++b) compress_add(*dst.view(b).context(), dst.view(b).handle(), stream);
  }
  void set_data(const StokesBlockVector &lin) const { A.set_data(lin.blocks()); }
  void set_cip_weight(int weight) const { A.set_cip_weight(weight); }

private:
  // Partitioned with the CIP term: every velocity source's two DoF planes next to each interface go to that neighbour
  // (stfem_stokes_cip_pack, stfem_neighbour_exchange: one more message per neighbour and source, before the operator call) and what
  // arrives is bound to the source (stfem_stokes_cip_bind_ghosts).  A pool of one receive pair per velocity block of the slice, of
  // ghost size (CipGhost): slot k serves the k-th velocity block of every apply, and the source it served before is unbound, so the
  // context holds at most that many bindings and none of a vector that has since been freed.  The two send buffers are shared:
  // `stream` has waited for the arrival before the next pack.  All applies of one system are taken to run on one stream.  A weight
  // velocity needs no ghosts (a face reads it on its own plane).
  // A partitioned slab with delta0 != 0 whose operator was NOT told of its neighbours (set_partition on a general mesh without the
  // vertex planes) would silently lack the interface faces: refused here.  Only vmult and form bind; the slice-add entry points of
  // SystemMatrixStokes on such a slab return STFEM_ERR_INVALID_ARGUMENT from the boundary (no binding), they are not served yet.
  void bind_cip_ghosts(const StokesBlockVector &src, void *stream) const
  {
    const Context &c = *spaces->q2;
    if (!c.comm || A.delta0() == 0) return;
    const int expected = (c.lower_rank >= 0 ? 16 : 0) | (c.upper_rank >= 0 ? 32 : 0);
    if (spaces->cip_neighbours != expected)
      throw Error(STFEM_ERR_INVALID_ARGUMENT, "StokesSystem: delta0 != 0 on a partitioned general mesh needs the neighbours' vertex planes "
                                              "(StokesSpaces::set_partition): the CIP term would lack the interface faces");
    if (!expected) return;
    const int64_t n = stfem_stokes_cip_ghost_size(stokes);
    if (!send[0].data())
      for (CipGhost &g : send) g = CipGhost(stokes);
    for (Slot &s : pool) { // (all first: an address may have moved to another slot since the last apply)
      if (s.bound) check(stfem_stokes_cip_bind_ghosts(stokes, s.bound, nullptr, nullptr), "stfem_stokes_cip_bind_ghosts");
      s.bound = nullptr;
    }
    unsigned k = 0;
    for (unsigned b = 0; b < src.n_blocks(); ++b) {
      if (slice.decompose(b)[1] != 0) continue;
      const double *u = src.blocks()[b].data();
      if (k == pool.size()) pool.push_back({nullptr, {CipGhost(stokes), CipGhost(stokes)}});
      Slot &s = pool[k++];
      if (c.lower_rank >= 0) check(stfem_stokes_cip_pack(stokes, u, 0, send[0].data(), stream), "stfem_stokes_cip_pack");
      if (c.upper_rank >= 0) check(stfem_stokes_cip_pack(stokes, u, 1, send[1].data(), stream), "stfem_stokes_cip_pack");
      check(stfem_neighbour_exchange(c.comm->handle(), c.lower_rank, c.upper_rank, n, send[0].data(), send[1].data(), s.recv[0].data(),
                                     s.recv[1].data(), stream),
            "stfem_neighbour_exchange");
      check(stfem_stokes_cip_bind_ghosts(stokes, u, c.lower_rank >= 0 ? s.recv[0].data() : nullptr,
                                         c.upper_rank >= 0 ? s.recv[1].data() : nullptr),
            "stfem_stokes_cip_bind_ghosts");
      s.bound = u;
    }
  }
  struct Slot {
    const double *bound; // the source this slot's planes are bound to
    std::array<CipGhost, 2> recv;
  };
  const SystemMatrixStokes<dim, Number> &A;
  std::shared_ptr<StokesSpaces> spaces;
  stfem_stokes_ctx *stokes;
  BlockSlice slice;
  mutable std::array<CipGhost, 2> send;
  mutable std::vector<Slot> pool;
};

// the start vector of the power iteration (estimate_max_eigenvalue in stmg.h): (i mod 11) - mean on every block, each of its own size
inline void power_iteration_start(StokesBlockVector &v)
{
  for (StokesVector &b : v.blocks()) b.copy_from_host(power_iteration_start(b.size()));
}

// Wall time of a scope added to `acc`, the device synchronised at both edges; nothing at all when off
struct SynchronisedTimer {
  SynchronisedTimer(double &acc, bool on = true) : acc(acc), on(on)
  {
    if (on) {
      (void)stfem_stream_synchronize(nullptr);
      t0 = std::chrono::steady_clock::now();
    }
  }
  ~SynchronisedTimer()
  {
    if (on) {
      (void)stfem_stream_synchronize(nullptr);
      acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  double &acc;
  bool on;
  std::chrono::steady_clock::time_point t0;
};

// The smoother of one Stokes level, or of a single-level preconditioner: the two-variable Vanka smoother, its damping omega and
// PreconditionRelaxation (stmg.h:1199-1238) around both.  Without a nonlinear treatment all three are made by the constructor.
// With one they belong to a linearisation: the first set_data makes the per-cell smoother of the operator linearised about `lin`,
// every later one updates its blocks (PreconditionVankaStokes::update), and the damping follows the operator.  relaxation == 0:
// omega is estimated as the reference's default does (20 power iterations on P^-1 A), at the first set_data and - unless
// reestimate_relaxation is false - at every later one.  The preconditioner interface of TimeIntegratorNavierStokes beside GMGStokes.
// delta0 != 0 (a nonlinear treatment only): the blocks hold the CIP term weighted by the linearisation
// (PreconditionVankaStokes, stfem_stokes_vanka_create_linearised_cip); the estimate sees whatever `system` applies.
// Either velocity degree: over a degree-3 operator the smoother is the per-cell one of stfem_stokes_vanka_create_space /
// _create_linearised_space (delta0 == 0 only: such an operator has no CIP term).
template <int dim> class RelaxedVankaStokes {
public:
  RelaxedVankaStokes(const StokesMatrixFreeOperator<dim, double> &K, const StokesSystem<dim, double> &system, const FullMatrix<double> &Alpha,
                     const FullMatrix<double> &Beta, const BlockSlice &slice, NonlinearTreatment treatment, unsigned n_iterations, double relaxation = 0.0,
                     bool reestimate_relaxation = true, double delta0 = 0.0)
    : K(K), system(system), Alpha(Alpha), Beta(Beta), slice(slice), treatment(treatment), n_iterations(n_iterations), relaxation_(relaxation),
      reestimate(reestimate_relaxation), delta0(delta0)
  {
    if (delta0 != 0.0 && treatment == NonlinearTreatment::None)
      throw std::invalid_argument("RelaxedVankaStokes: the CIP term in the blocks (delta0 != 0) needs a nonlinear treatment");
    if (treatment != NonlinearTreatment::None) return;
    vanka = std::make_unique<PreconditionVankaStokes<double>>(K, Alpha, Beta, slice);
    relax_with_new_omega();
  }
  void set_data(const StokesBlockVector &lin)
  {
    if (treatment == NonlinearTreatment::None) throw std::invalid_argument("RelaxedVankaStokes::set_data: a smoother without a nonlinear treatment");
    if (vanka) vanka->update(lin.blocks());
    else vanka = std::make_unique<PreconditionVankaStokes<double>>(K, Alpha, Beta, slice, treatment, lin.blocks(), delta0);
    relax_with_new_omega();
  }
  void vmult(StokesBlockVector &dst, const StokesBlockVector &src, void *stream = nullptr) const
  {
    if (!relax) throw std::invalid_argument("RelaxedVankaStokes::vmult: set_data first");
    relax->vmult(dst, src, stream);
  }
  bool ready() const { return bool(relax); }
  double relaxation() const { return omega; }

private:
  using Relaxation = PreconditionRelaxation<double, StokesSystem<dim, double>, PreconditionVankaStokes<double>, StokesBlockVector>;
  void relax_with_new_omega() // omega: given, the first estimate or a fresh one
  {
    if (relaxation_ != 0.0) omega = relaxation_;
    else if (!relax || reestimate) omega = estimate_relaxation<StokesBlockVector>(system, *vanka, 20, 1.0);
    if (relax) relax->set_relaxation(omega);
    else relax = std::make_unique<Relaxation>(system, *vanka, omega, n_iterations);
  }
  const StokesMatrixFreeOperator<dim, double> &K;
  const StokesSystem<dim, double> &system;
  const FullMatrix<double> &Alpha, &Beta;
  BlockSlice slice;
  NonlinearTreatment treatment;
  unsigned n_iterations;
  double relaxation_, omega = 1.0;
  bool reestimate;
  double delta0;
  std::unique_ptr<PreconditionVankaStokes<double>> vanka;
  std::unique_ptr<Relaxation> relax;
};

// The geometric multigrid of the reference's Stokes runs (tests/tp_03stokes.cc:283-290, 484-770: coarsening sequence in space from
// MGTransferGlobalCoarseningTools::create_geometric_coarsening_sequence, one StokesMatrixFreeOperator / SystemMatrixStokes /
// PreconditionVanka per level, MGTwoLevelBlockTransfer with one space transfer per variable; include/stmg.h:1160-1419: GMG with
// Multigrid, MGSmootherPrecondition around PreconditionRelaxation(Vanka), MGCoarseGridApplySmoother, PreconditionMG) over the
// C-ABI: the velocity components are transferred as FE_Q(2) functions with the constraints of both levels, the pressure as a
// FE_Q(1) function (stfem_transfer_*), every level smooths with relaxation sweeps of the two-variable Vanka smoother.  The first
// constructor coarsens in space only (the temporal blocks are the same on every level); the second takes the reference's level
// sequence (tests/tp_03stokes.cc:294-326: MGType h, k, tau from get_mg_sequence) - a k level lowers the temporal degree, a tau
// level halves the time steps per slab, both with the time transfers of MGTwoLevelTransferTime applied per variable
// (include/stmg.h:557-600: MGTwoLevelBlockTransfer with the time matrices), and every level has its own temporal matrices
// (get_fe_time_weights_stokes of its degree, step count and step size) and block structure.
template <int dim> class GMGStokes {
public:
  struct AdditionalData {
    unsigned smoothing_steps = 1;      // PreconditionerGMGAdditionalData::smoothing_steps
    bool variable = true;              // MGSmootherPrecondition variable: 2^(max_level - level) steps on level `level`
    unsigned smoothing_degree = 1;     // sweeps of PreconditionRelaxation per step
    double relaxation = 0.0;           // its omega; 0: estimated per level (20 power iterations on P^-1 A), as the reference's default
    bool reestimate_relaxation = true; // linearised levels, relaxation == 0: a fresh estimate at every set_data (false: the first one is kept)
    // the CIP term on every level (tests/tp_03stokes.cc:610-623: stokes_parameters.delta0 to the operator of every level, h_F of the
    // level's own mesh does the scaling): level operators with set_cip(delta0, STFEM_CIP_WEIGHT_LINEARISATION), level smoothers with
    // the term in their blocks; needs a nonlinear treatment.  0: levels and smoothers of the operator without it
    double delta0 = 0.0;
  };
  // the finest mesh has mesh.ncell cells; level l < n_levels - 1 has them halved n_levels - 1 - l times
  GMGStokes(const Mesh &mesh, unsigned n_levels, double viscosity, const FullMatrix<double> &Alpha, const FullMatrix<double> &Beta,
            const BlockSlice &slice, const AdditionalData &data = AdditionalData(), const std::set<boundary_id> &weak_boundary_ids = {},
            bool dg_pressure = false, NonlinearTreatment treatment = NonlinearTreatment::None)
    : data_(data)
  {
    if (n_levels < 1) throw std::invalid_argument("GMGStokes: at least one level");
    if (data.delta0 != 0.0 && treatment == NonlinearTreatment::None)
      throw std::invalid_argument("GMGStokes: the CIP term on the levels (delta0 != 0) needs a nonlinear treatment");
    dg_ = dg_pressure;
    treatment_ = treatment;
    levels_.resize(n_levels);
    for (unsigned l = 0; l < n_levels; ++l) {
      levels_[l].halvings = n_levels - 1 - l;
      levels_[l].Alpha = Alpha;
      levels_[l].Beta = Beta;
      levels_[l].slice = slice;
      levels_[l].from_below = MGType::h;
    }
    build(mesh, viscosity, weak_boundary_ids, TimeStepType::CGP);
  }
  // mg_type_level[l]: how level l + 1 (finer) arises from level l, finest last, as get_mg_sequence returns it (h, k and tau; the
  // Stokes element has no p levels); poly_time_sequence: the temporal degrees, ascending (get_poly_mg_sequence); the finest level has
  // degree poly_time_sequence.back(), n_timesteps_at_once steps of size time_step_size per slab
  GMGStokes(const Mesh &mesh, const std::vector<MGType> &mg_type_level, const std::vector<unsigned> &poly_time_sequence, TimeStepType type,
            double time_step_size, unsigned n_timesteps_at_once, double viscosity, const AdditionalData &data = AdditionalData(),
            const std::set<boundary_id> &weak_boundary_ids = {}, bool dg_pressure = false, NonlinearTreatment treatment = NonlinearTreatment::None)
    : data_(data)
  {
    if (treatment != NonlinearTreatment::None) throw std::invalid_argument("GMGStokes: the linearisation on k / tau levels is not built");
    if (data.delta0 != 0.0) throw std::invalid_argument("GMGStokes: the CIP term on the levels (delta0 != 0) needs a nonlinear treatment");
    dg_ = dg_pressure;
    const unsigned n_levels = unsigned(mg_type_level.size()) + 1;
    levels_.resize(n_levels);
    const auto blk = get_blk_indices(type, n_timesteps_at_once, 2, n_levels, mg_type_level, poly_time_sequence);
    auto p_mg = poly_time_sequence.rbegin();
    unsigned halvings = 0;
    for (unsigned l = n_levels; l-- > 0;) {
      Level &L = levels_[l];
      L.halvings = halvings;
      L.slice = blk[l];
      const auto w = get_fe_time_weights_stokes<double>(type, *p_mg, time_step_size, n_timesteps_at_once);
      L.Alpha = w[0];
      L.Beta = w[1];
      if (l == 0) break;
      L.from_below = mg_type_level[l - 1];
      switch (mg_type_level[l - 1]) {
        case MGType::h: ++halvings; break;
        case MGType::k: ++p_mg; break;
        case MGType::tau: n_timesteps_at_once /= 2; time_step_size *= 2; break;
        default: throw std::invalid_argument("GMGStokes: h, k and tau levels");
      }
    }
    build(mesh, viscosity, weak_boundary_ids, type);
  }
  const StokesSystem<dim, double> &finest_system() const { return *levels_.back().system; }
  const StokesMatrixFreeOperator<dim, double> &finest_operator() const { return *levels_.back().K; }
  const std::shared_ptr<StokesSpaces> &finest_spaces() const { return levels_.back().spaces; }
  double relaxation(unsigned level) const { return levels_.at(level).smoother->relaxation(); }
  unsigned n_levels() const { return unsigned(levels_.size()); }
  NonlinearTreatment nonlinear_treatment() const { return treatment_; }
  // The hierarchy of the operator linearised about `lin` (the reference's set_data + reinit_asm(..., mg_data), include/stmg.h:929-965):
  // the finest level refers to lin itself (only its velocity blocks are read; it has to outlive the cycles), every coarser level
  // holds the nodal interpolation of the level above (MGTwoLevelTransfer::interpolate on the three components of every time dof:
  // the reference's mg_data[l]), in storage made at the first call.  Then, level by level: the operator's set_data, the per-cell
  // smoother of the linearised operator and the damping of its relaxation (RelaxedVankaStokes::set_data).
  void set_data(const StokesBlockVector &lin)
  {
    if (treatment_ == NonlinearTreatment::None) throw std::invalid_argument("GMGStokes::set_data: a hierarchy without a nonlinear treatment");
    const unsigned top = unsigned(levels_.size()) - 1;
    if (lin.n_blocks() != levels_[top].slice.n_blocks()) throw Error(STFEM_ERR_SHAPE_MISMATCH, "GMGStokes::set_data: blocks");
    for (unsigned l = levels_.size(); l-- > 0;) {
      Level &L = levels_[l];
      if (l < top) {
        const Level &F = levels_[l + 1];
        if (L.lin.empty()) L.system->initialize_dof_vector(L.lin);
        for (unsigned b = 0; b < L.slice.n_blocks(); ++b) {
          if (L.slice.decompose(b)[1] != 0) continue;
          // (the caller's vector may live on contexts of its own for the same mesh: viewed through this hierarchy's spaces)
          const BlockVectorT<double> caller = l + 1 == top ? foreign_view(lin, b) : BlockVectorT<double>();
          const stfem_vec *fine = l + 1 == top ? caller.handle() : F.lin.view(b).handle();
          check(stfem_transfer_interpolate(F.tr_u->handle(), L.lin.view(b).handle(), fine, nullptr), "GMGStokes::set_data: interpolate");
        }
      }
      const StokesBlockVector &about = l == top ? lin : L.lin;
      L.A->set_data(about.blocks());
      L.smoother->set_data(about);
    }
  }
  // the linearisation a level below the finest holds (set_data)
  const StokesBlockVector &level_linearization(unsigned level) const
  {
    if (level + 1 >= levels_.size() || levels_[level].lin.empty()) throw std::invalid_argument("GMGStokes::level_linearization");
    return levels_[level].lin;
  }
  // STFEM_MG_TIMING=1: wall time per level (smoothing, residual + transfers), with a device synchronisation around every section -
  // the sections of the reference's TimerOutput ("gmg" and below); the synchronisations cost the overlap of launches and kernels
  void print_timing(FILE *f) const
  {
    if (!timing_) return;
    for (unsigned l = 0; l < levels_.size(); ++l)
      std::fprintf(f, "level %u: smoothing %.3f s, residual and transfers %.3f s (%u cycles)\n", l, levels_[l].t_smooth, levels_[l].t_transfer, cycles_);
  }

  // PreconditionMG::vmult: copy_to_mg, one V-cycle from zero, copy_from_mg
  void vmult(StokesBlockVector &dst, const StokesBlockVector &src, void * = nullptr) const
  {
    TraceRange scope("gmg");
    const unsigned top = unsigned(levels_.size()) - 1;
    if (!levels_[top].smoother->ready()) throw std::invalid_argument("GMGStokes::vmult: set_data first");
    // (the caller's vectors may live on contexts of their own for the same mesh: view their blocks through this level's spaces)
    const unsigned nb = levels_[top].slice.n_blocks();
    for (unsigned b = 0; b < nb; ++b) axpby(1.0, foreign_view(src, b), 0.0, levels_[top].defect.view(b));
    level_v_step(top);
    ++cycles_;
    for (unsigned b = 0; b < nb; ++b) {
      BlockVectorT<double> d = foreign_view(dst, b);
      axpby(1.0, levels_[top].solution.view(b), 0.0, d);
    }
  }

private:
  struct Level {
    Mesh mesh;
    unsigned halvings = 0;            // of the finest mesh's cell counts
    FullMatrix<double> Alpha, Beta;   // the level's temporal matrices and block structure
    BlockSlice slice;
    MGType from_below = MGType::h;    // the transfer between this level and the one below
    FullMatrix<double> time_prolongation, time_restriction; // k / tau: one variable's blocks (BlockSlice(steps, 1, dofs) order)
    std::unique_ptr<StokesMatrixFreeOperator<dim, double>> K;
    std::shared_ptr<StokesSpaces> spaces;
    std::unique_ptr<SystemMatrixStokes<dim, double>> A;
    std::unique_ptr<StokesSystem<dim, double>> system;
    std::unique_ptr<RelaxedVankaStokes<dim>> smoother; // (linearised levels: smoother and damping belong to a linearisation - set_data)
    std::unique_ptr<MGTwoLevelTransfer<double>> tr_u, tr_p; // to the level below
    mutable StokesBlockVector defect, solution, t, tmp;
    StokesBlockVector lin; // linearised levels below the finest: the interpolated linearisation (mg_data[l])
    mutable double t_smooth = 0.0, t_transfer = 0.0;
  };
  void build(const Mesh &mesh, double viscosity, const std::set<boundary_id> &weak_boundary_ids, TimeStepType type)
  {
    const unsigned n_levels = unsigned(levels_.size());
    for (unsigned l = 0; l < n_levels; ++l) {
      Level &L = levels_[l];
      L.mesh = mesh;
      for (int d = 0; d < 3; ++d) {
        const int f = 1 << L.halvings;
        if (mesh.ncell[d] % f) throw std::invalid_argument("GMGStokes: the cell counts must be divisible by 2^(space levels - 1)");
        L.mesh.ncell[d] = mesh.ncell[d] / f;
      }
      L.K = std::make_unique<StokesMatrixFreeOperator<dim, double>>(L.mesh, 2, viscosity, weak_boundary_ids, std::set<boundary_id>(), 20.0, 10.0, 0.0, data_.delta0, 0.0,
                                                                   dg_, treatment_);
      if (data_.delta0 != 0.0) L.K->set_cip_weight(STFEM_CIP_WEIGHT_LINEARISATION);
      L.spaces = std::make_shared<StokesSpaces>(L.mesh, L.K->handle());
      L.A = std::make_unique<SystemMatrixStokes<dim, double>>(*L.K, L.Alpha, L.Beta, L.slice, treatment_);
      L.system = std::make_unique<StokesSystem<dim, double>>(*L.A, L.spaces, L.K->handle(), L.slice);
      L.smoother = std::make_unique<RelaxedVankaStokes<dim>>(*L.K, *L.system, L.Alpha, L.Beta, L.slice, treatment_, data_.smoothing_degree, data_.relaxation,
                                                           data_.reestimate_relaxation, data_.delta0);
      L.system->initialize_dof_vector(L.defect);
      L.system->initialize_dof_vector(L.solution);
      L.system->initialize_dof_vector(L.t);
      if (l == 0) continue;
      const Level &C = levels_[l - 1];
      if (L.from_below == MGType::h) {
        L.tr_u = std::make_unique<MGTwoLevelTransfer<double>>(L.spaces->q2, C.spaces->q2);
        if (!dg_) L.tr_p = std::make_unique<MGTwoLevelTransfer<double>>(L.spaces->q1, C.spaces->q1);
      } else { // (restrict = transposed prolongation: the reference's default, parameters.h:29)
        const MGTwoLevelTransferTime<double> tt(BlockSlice(L.slice.n_timesteps_at_once(), 1, L.slice.n_timedofs()),
                                                BlockSlice(C.slice.n_timesteps_at_once(), 1, C.slice.n_timedofs()), type, true, L.from_below);
        L.time_prolongation = tt.prolongation();
        L.time_restriction = tt.restriction();
      }
    }
  }
  // dst (+)= (matrix x identity) src on the blocks of every variable: matrix acts between the (step, time dof) blocks of one variable
  void time_transfer(const Level &D, StokesBlockVector &dst, const FullMatrix<double> &matrix, const Level &S, const StokesBlockVector &src) const
  {
    for (unsigned v = 0; v < 2; ++v) {
      const unsigned ncomp = v == 0 ? 3 : 1;
      const size_t len = v == 0 ? size_t(stfem_stokes_n_velocity_dofs(D.K->handle())) : 0;
      auto gather = [&](const Level &L, const StokesBlockVector &x) {
        std::vector<void *> ptrs;
        for (unsigned it = 0; it < L.slice.n_timesteps_at_once(); ++it)
          for (unsigned id = 0; id < L.slice.n_timedofs(); ++id)
            for (unsigned c = 0; c < ncomp; ++c) ptrs.push_back(x.blocks()[L.slice.index(it, v, id)].data() + c * len);
        return ptrs;
      };
      std::vector<void *> pd = gather(D, dst), ps = gather(S, src);
      BlockVectorT<double> vd, vs;
      const auto &ctx = v == 0 ? D.spaces->q2 : D.spaces->q1; // (the same mesh on both levels: one context serves both)
      vd.wrap(ctx, pd.data(), unsigned(pd.size()));
      vs.wrap(ctx, ps.data(), unsigned(ps.size()));
      std::vector<double> a(pd.size() * ps.size(), 0.0);
      for (unsigned i = 0; i < matrix.m(); ++i)
        for (unsigned j = 0; j < matrix.n(); ++j)
          for (unsigned c = 0; c < ncomp; ++c) a[size_t(i * ncomp + c) * ps.size() + j * ncomp + c] = matrix(i, j);
      check(stfem_tensorproduct_add(ctx->h, int(pd.size()), int(ps.size()), a.data(), vd.handle(), vs.handle(), nullptr), "GMGStokes: time transfer");
    }
  }
  BlockVectorT<double> foreign_view(const StokesBlockVector &x, unsigned b) const
  {
    const StokesSpaces &sp = *levels_.back().spaces;
    // (the levels are degree-2 operators made from the mesh: a vector over a degree-3 operator is not theirs)
    if (!x.spaces() || x.spaces()->velocity_degree != sp.velocity_degree)
      throw Error(STFEM_ERR_UNSUPPORTED, "GMGStokes is built for velocity degree 2 only: its level operators are FE_Q(2)^3 x FE_Q(1) / FE_DGP(1) on the "
                                         "mesh, and vmult / set_data were given a vector that is not over such an operator (velocity degree 3 has "
                                         "RelaxedVankaStokes as its preconditioner)");
    BlockVectorT<double> v;
    double *base = x.blocks()[b].data();
    if (levels_.back().slice.decompose(b)[1] == 0) {
      const size_t nu = size_t(stfem_stokes_n_velocity_dofs(levels_.back().K->handle()));
      void *ptrs[3] = {base, base + nu, base + 2 * nu};
      v.wrap(sp.q2, ptrs, 3);
    } else {
      void *ptrs[1] = {base};
      v.wrap(sp.q1, ptrs, 1);
    }
    return v;
  }
  // MGSmootherPrecondition::smooth / apply: u (= | +=) P (rhs - A u), `steps` times
  void smooth(unsigned level, bool from_zero) const
  {
    const Level &L = levels_[level];
    const unsigned steps = data_.smoothing_steps * (data_.variable ? 1u << (unsigned(levels_.size()) - 1 - level) : 1u);
    unsigned i = 0;
    if (from_zero) {
      L.smoother->vmult(L.solution, L.defect);
      i = 1;
    }
    for (; i < steps; ++i) {
      reinit_like(L.tmp, L.defect);
      L.system->vmult(L.t, L.solution);
      axpby(1.0, L.defect, -1.0, L.t);
      L.smoother->vmult(L.tmp, L.t);
      axpby(1.0, L.tmp, 1.0, L.solution);
    }
  }
  // Multigrid::level_v_step
  void level_v_step(unsigned level) const
  {
    const Level &L = levels_[level];
    if (level == 0) { // MGCoarseGridApplySmoother
      SynchronisedTimer sec(L.t_smooth, timing_);
      smooth(0, true);
      return;
    }
    const Level &C = levels_[level - 1];
    {
      SynchronisedTimer sec(L.t_smooth, timing_);
      smooth(level, true);
    }
    auto down = std::make_unique<SynchronisedTimer>(L.t_transfer, timing_);
    L.system->vmult(L.t, L.solution);
    axpby(1.0, L.defect, -1.0, L.t);
    set_zero(C.defect);
    const BlockSlice &slice = L.slice;
    const bool in_time = L.from_below != MGType::h; // MGTwoLevelBlockTransfer with the time matrices, or one space transfer per variable
    if (in_time) time_transfer(C, C.defect, L.time_restriction, L, L.t);
    for (unsigned b = 0; b < slice.n_blocks() && !in_time; ++b) { // restrict_and_add: block by block with its variable's transfer
      if (slice.decompose(b)[1] == 1 && dg_) {
        check(stfem_stokes_dgp_restrict(L.K->handle(), C.K->handle(), C.defect.blocks()[b].data(), L.t.blocks()[b].data(), 1, nullptr), "GMGStokes: restrict_and_add");
        continue;
      }
      const MGTwoLevelTransfer<double> &tr = slice.decompose(b)[1] == 0 ? *L.tr_u : *L.tr_p;
      check(stfem_transfer_restrict(tr.handle(), C.defect.view(b).handle(), L.t.view(b).handle(), 1, nullptr), "GMGStokes: restrict_and_add");
    }
    down.reset();
    level_v_step(level - 1);
    auto up = std::make_unique<SynchronisedTimer>(L.t_transfer, timing_);
    if (in_time) time_transfer(L, L.solution, L.time_prolongation, C, C.solution);
    for (unsigned b = 0; b < slice.n_blocks() && !in_time; ++b) {
      if (slice.decompose(b)[1] == 1 && dg_) {
        check(stfem_stokes_dgp_prolongate(L.K->handle(), C.K->handle(), L.solution.blocks()[b].data(), C.solution.blocks()[b].data(), 1, nullptr),
              "GMGStokes: prolongate_and_add");
        continue;
      }
      const MGTwoLevelTransfer<double> &tr = slice.decompose(b)[1] == 0 ? *L.tr_u : *L.tr_p;
      check(stfem_transfer_prolongate(tr.handle(), L.solution.view(b).handle(), C.solution.view(b).handle(), 1, nullptr), "GMGStokes: prolongate_and_add");
    }
    up.reset();
    SynchronisedTimer sec(L.t_smooth, timing_);
    smooth(level, false);
  }
  bool timing_ = [] {
    const char *e = std::getenv("STFEM_MG_TIMING");
    return e && std::atoi(e) != 0;
  }();
  mutable unsigned cycles_ = 0;
  AdditionalData data_;
  bool dg_ = false;
  NonlinearTreatment treatment_ = NonlinearTreatment::None;
  std::vector<Level> levels_;
};

// ErrorCalculator (include/exact_solution.h:503-649) for the pressure variable in either pressure space: the temporal Lagrange
// combination of the pressure blocks (evaluate_numerical_solution), then stfem_stokes_pressure_difference with QGauss(nq)^3
class PressureErrorCalculator {
public:
  PressureErrorCalculator(TimeStepType type, unsigned time_degree, int nq_space, const std::shared_ptr<StokesSpaces> &spaces, const PointFunction &exact)
    : type(type), time_degree(time_degree), nq(nq_space), spaces(spaces), exact(exact), nodes(time_points(type, time_degree)), tq(time_degree + 1),
      tw(time_degree + 1)
  {
    check(stfem_gauss_rule(int(time_degree + 1), tq.data(), tw.data()), "stfem_gauss_rule");
    numeric.reinit(spaces->q1, 1);
    const size_t ncells = size_t(stfem_n_cells(spaces->q2->h));
    qpoints.resize(ncells * nq * nq * nq * 3);
    check(stfem_stokes_pressure_quadrature_points_space(spaces->stokes, nq, qpoints.data()), "stfem_stokes_pressure_quadrature_points_space");
  }
  // {L2^2 contribution, Linfty} of the slab; x: the pressure blocks of the time dofs (views on the pressure space), prev: the previous one
  std::array<double, 2> evaluate_error(double time, double time_step, const BlockVectorT<double> &x, const BlockVectorT<double> &prev)
  {
    std::array<double, 2> err{0.0, -1.0};
    const unsigned nt_dofs = type == TimeStepType::DG ? time_degree + 1 : time_degree;
    std::vector<double> pe;
    for (unsigned q = 0; q < tq.size(); ++q) {
      const std::vector<double> L = lagrange_values(nodes, tq[q]);
      set_zero(numeric);
      if (type == TimeStepType::DG) {
        for (unsigned i = 0; i < nt_dofs; ++i) axpby(L[i], block_view(x, i), 1.0, numeric);
      } else {
        axpby(L[0], prev, 1.0, numeric);
        for (unsigned i = 1; i <= time_degree; ++i) axpby(L[i], block_view(x, i - 1), 1.0, numeric);
      }
      exact(time + tq[q] * time_step, qpoints, pe);
      double out[2];
      check(stfem_stokes_pressure_difference_space(spaces->stokes, nq, static_cast<const double *>(stfem_vector_block(numeric.handle(), 0)), pe.data(), out,
                                                   nullptr),
            "stfem_stokes_pressure_difference_space");
      err[0] += time_step * tw[q] * out[0];
      err[1] = std::max(err[1], out[1]);
    }
    return err;
  }

private:
  TimeStepType type;
  unsigned time_degree;
  int nq;
  std::shared_ptr<StokesSpaces> spaces;
  PointFunction exact;
  std::vector<double> nodes, tq, tw, qpoints;
  BlockVectorT<double> numeric;
};

// A vector function of (x, t) at a list of points: out[c][i] = f_c(points[3 i .. 3 i + 2], t)
using VectorPointFunction = std::function<void(double time, const std::vector<double> &points, std::array<std::vector<double>, 3> &out)>;

// What the slab solves of the two-variable system share (include/time_integrators.h:30-336): the time quadrature of the velocity
// force (assemble_force per variable, 73-111: the pressure load is zero), the start value, and the shift of every time dof's pressure
// to zero mean afterwards (tests/tp_03stokes.cc:1047-1062).  Alpha_1 / Gamma_1: the ONE-step scalar temporal matrices.  The device
// vectors are made at the first use.
class StokesSlab {
public:
  StokesSlab(TimeStepType type, unsigned time_degree, const FullMatrix<double> &Alpha_1, const FullMatrix<double> &Gamma_1, const VectorPointFunction &force,
             bool zero_mean_pressure)
    : type(type), quad_time(time_points(type, time_degree)), Alpha(Alpha_1), Gamma(Gamma_1), force(force),
      nt_dofs(type == TimeStepType::DG ? time_degree + 1 : time_degree), zero_mean(zero_mean_pressure)
  {}
  // rhs += the force's load vectors: Alpha is diagonal (time quadrature = support points)
  void assemble_force(StokesBlockVector &rhs, double time, double time_step)
  {
    const StokesSpaces &sp = *rhs.spaces();
    if (sp.velocity_degree != 2) // (the load vectors below are those of FE_Q(2) with QGauss(3))
      throw Error(STFEM_ERR_UNSUPPORTED, "StokesSlab::assemble_force: the time integrators are built for velocity degree 2 only");
    if (qpoints.empty()) {
      qpoints.resize(size_t(stfem_n_cells(sp.q2->h)) * 27 * 3);
      check(stfem_quadrature_points(sp.q2->h, 3, qpoints.data()), "stfem_quadrature_points");
      load.reinit(sp.q2, 3);
    }
    std::array<std::vector<double>, 3> fq;
    for (unsigned j = 0; j < quad_time.size(); ++j) {
      force(time + time_step * quad_time[j], qpoints, fq);
      for (int c = 0; c < 3; ++c) check(stfem_integrate_rhs(sp.q2->h, 3, fq[c].data(), load.handle(), c, nullptr), "stfem_integrate_rhs");
      auto add = [&](unsigned timedof, double w) { axpby(w, load, 1.0, rhs.view(rhs.slice().index(0, 0, timedof))); };
      if (type == TimeStepType::DG) add(j, Alpha(j, j));
      else if (j == 0)
        for (unsigned i = 0; i < nt_dofs; ++i) add(i, -Gamma(i, 0));
      else add(j - 1, Alpha(j - 1, j - 1));
    }
  }
  // extrapolate (time_integrators.h:184-194): every time dof starts from the previous solution; prev: one (velocity, pressure) pair
  void extrapolate(StokesBlockVector &x, const StokesBlockVector &prev) const
  {
    for (unsigned i = 0; i < x.n_blocks(); ++i) axpby(1.0, prev.view(x.slice().decompose(i)[1]), 0.0, x.view(i));
  }
  // mean(p) = weights . p / |Omega|, p -= mean * ones (VectorTools::compute_mean_value / add_constant); nothing unless asked for
  void shift_pressure_to_zero_mean(StokesBlockVector &x)
  {
    if (!zero_mean) return;
    const StokesSpaces &sp = *x.spaces();
    if (!weights.handle()) {
      weights.reinit(sp.q1, 1);
      ones.reinit(sp.q1, 1);
      std::vector<std::vector<double>> h1(1, std::vector<double>(ones.block_size())), hw(1, std::vector<double>(ones.block_size()));
      check(stfem_stokes_pressure_mean_vectors_space(sp.stokes, h1[0].data(), hw[0].data(), &volume), "stfem_stokes_pressure_mean_vectors_space");
      ones.copy_from_host(h1);
      weights.copy_from_host(hw);
    }
    for (unsigned a = 0; a < nt_dofs; ++a) {
      BlockVectorT<double> &p = x.view(x.slice().index(0, 1, a));
      axpby(-dot(weights, p) / volume, ones, 1.0, p);
    }
  }

private:
  TimeStepType type;
  std::vector<double> quad_time;
  const FullMatrix<double> &Alpha, &Gamma;
  VectorPointFunction force;
  unsigned nt_dofs;
  bool zero_mean;
  std::vector<double> qpoints;
  BlockVectorT<double> load, weights, ones;
  double volume = 1.0;
};

// The slab problem of the Stokes equations: rhs = rhs_matrix (prev_u, prev_p) + force, FGMRES on the slab system from the
// extrapolated start value, zero-mean pressure.
template <int dim, typename System, typename Preconditioner> class TimeIntegratorStokes {
public:
  TimeIntegratorStokes(TimeStepType type, unsigned time_degree, const FullMatrix<double> &Alpha_1, const FullMatrix<double> &Gamma_1,
                       double gmres_tolerance, const System &matrix, const Preconditioner &preconditioner,
                       const SystemMatrixStokes<dim, double> &rhs_matrix, const VectorPointFunction &force, bool zero_mean_pressure,
                       double abstol = 1e-12, unsigned max_steps = 400)
    : slab(type, time_degree, Alpha_1, Gamma_1, force, zero_mean_pressure), solver(max_steps, abstol, gmres_tolerance, 200),
      preconditioner(preconditioner), matrix(matrix), rhs_matrix(rhs_matrix)
  {
    if (const char *e = std::getenv("STFEM_FGMRES_VERBOSE")) solver.verbose = unsigned(std::atoi(e));
  }

  // x, rhs: the slab's blocks; prev: one (velocity, pressure) pair (BlockSlice(1, 2, 1))
  void solve(StokesBlockVector &x, const StokesBlockVector &prev, StokesBlockVector &rhs, double time, double time_step)
  {
    TraceRange scope("step");
    set_zero(rhs);
    rhs_matrix.vmult_slice_add(rhs.blocks(), prev.blocks());
    slab.assemble_force(rhs, time, time_step);
    slab.extrapolate(x, prev);
    (void)dot(rhs.view(0), rhs.view(0)); // (synchronises: the clock below sees the Krylov solve alone)
    const auto t0 = std::chrono::steady_clock::now();
    solver.solve(matrix, x, rhs, preconditioner);
    (void)dot(x.view(0), x.view(0));
    solver_seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    slab.shift_pressure_to_zero_mean(x);
  }
  unsigned last_step() const { return solver.last_step(); }
  double solver_seconds() const { return solver_seconds_; } // wall time of the FGMRES solves so far (without the right-hand sides)

private:
  double solver_seconds_ = 0.0;
  StokesSlab slab;
  SolverFGMRES<double, StokesBlockVector> solver;
  const Preconditioner &preconditioner;
  const System &matrix;
  const SystemMatrixStokes<dim, double> &rhs_matrix;
};

// The slab problem of the Navier-Stokes equations: TimeIntegratorStokes with a Newton / Picard iteration in place of the one linear
// solve.  The reference prepares the interfaces (PDE<>::residual / form / vmult, set_data, reinit_asm(..., mg_data)) and has no
// nonlinear loop (include/time_integrators.h:20-22); this is the loop they are prepared for.  Per time dof the nonlinear term is the
// weak form linearised about that time dof's own velocity (include/operators.h:835-866), so the discrete problem is
//     sum_j Alpha(i, j) F(x_j) + Beta(i, j) M u_j = rhs_i,   F(u, p) = (nu K u - B^T p + C(u, u), B u),
// and the previous-slab term (j = 0 of the same sum, moved to the right) is rhs_matrix.form_slice_add about the previous end value.
//   matrix (System): set_data(x), form(dst, x), vmult(dst, src) - a StokesSystem whose operator carries the treatment: Implicit
//       applies the jacobian about x (Newton), Explicit the form about x (Picard), as in StokesMatrixFreeOperator::vmult;
//   preconditioner: set_data(x), vmult - GMGStokes with the same treatment or RelaxedVankaStokes.
// Per slab: x = previous solution; r = rhs - form(x); until |r| <= max(abstol, reltol |r_0|) or max_nonlinear steps (reported by
// converged(), not thrown): set_data(x) on both, FGMRES on J delta = r from zero, x += delta.
// With the CIP term (delta0 != 0) the system matrix is switched to the linearisation weight: the residual rhs - form(x) is taken about
// x itself, where both weights coincide, and the Krylov operator becomes linear in the increment (with the source weight of the
// reference it is cubic).  The preconditioners hold the term when they are given its delta0 themselves (GMGStokes::AdditionalData::delta0,
// the last argument of RelaxedVankaStokes); without it they are those of the operator without the stabilisation.
template <int dim, typename System, typename Preconditioner> class TimeIntegratorNavierStokes {
public:
  TimeIntegratorNavierStokes(TimeStepType type, unsigned time_degree, const FullMatrix<double> &Alpha_1, const FullMatrix<double> &Gamma_1,
                             double linear_tolerance, const System &matrix, Preconditioner &preconditioner,
                             const SystemMatrixStokes<dim, double> &rhs_matrix, const VectorPointFunction &force, bool zero_mean_pressure,
                             double nonlinear_reltol = 1e-12, double nonlinear_abstol = 1e-14, unsigned max_nonlinear = 30, double linear_abstol = 1e-16,
                             unsigned max_steps = 400)
    : slab(type, time_degree, Alpha_1, Gamma_1, force, zero_mean_pressure), solver(max_steps, linear_abstol, linear_tolerance, 200),
      preconditioner(preconditioner), matrix(matrix), rhs_matrix(rhs_matrix), reltol(nonlinear_reltol), abstol(nonlinear_abstol),
      max_nonlinear(max_nonlinear)
  {
    if (const char *e = std::getenv("STFEM_FGMRES_VERBOSE")) solver.verbose = unsigned(std::atoi(e));
    matrix.set_cip_weight(STFEM_CIP_WEIGHT_LINEARISATION);
  }

  // x, rhs: the slab's blocks; prev: one (velocity, pressure) pair (BlockSlice(1, 2, 1))
  void solve(StokesBlockVector &x, const StokesBlockVector &prev, StokesBlockVector &rhs, double time, double time_step)
  {
    TraceRange scope("step");
    set_zero(rhs);
    rhs_matrix.set_data(prev.blocks());
    rhs_matrix.form_slice_add(rhs.blocks(), prev.blocks());
    slab.assemble_force(rhs, time, time_step);
    slab.extrapolate(x, prev);
    reinit_like(residual, x);
    reinit_like(delta, x);
    nonlinear_steps_ = 0;
    linear_steps_ = 0;
    converged_ = false;
    residuals_.clear();
    double r0 = 0.0;
    for (;;) {
      double rn;
      {
        SynchronisedTimer c(residual_seconds_);
        matrix.set_data(x);
        matrix.form(residual, x);
        axpby(1.0, rhs, -1.0, residual);
        rn = norm(residual);
      }
      residuals_.push_back(rn);
      if (nonlinear_steps_ == 0) r0 = rn;
      if (rn <= std::max(abstol, reltol * r0)) {
        converged_ = true;
        break;
      }
      if (nonlinear_steps_ == max_nonlinear) break;
      {
        SynchronisedTimer c(set_data_seconds_);
        preconditioner.set_data(x);
      }
      {
        SynchronisedTimer c(solver_seconds_);
        set_zero(delta);
        solver.solve(matrix, delta, residual, preconditioner);
        linear_steps_ += solver.last_step();
      }
      axpby(1.0, delta, 1.0, x);
      ++nonlinear_steps_;
    }
    slab.shift_pressure_to_zero_mean(x);
  }
  // the last slab: Newton / Picard steps, FGMRES iterations over all of them, whether the tolerance was met, the residual norms
  unsigned nonlinear_steps() const { return nonlinear_steps_; }
  unsigned last_step() const { return linear_steps_; }
  bool converged() const { return converged_; }
  const std::vector<double> &residuals() const { return residuals_; }
  // wall time so far, the device synchronised at the section edges: residual evaluations, set_data of the preconditioner (smoother
  // update + relaxation estimate), Krylov solves
  double residual_seconds() const { return residual_seconds_; }
  double set_data_seconds() const { return set_data_seconds_; }
  double solver_seconds() const { return solver_seconds_; }

private:
  double residual_seconds_ = 0.0, set_data_seconds_ = 0.0, solver_seconds_ = 0.0;
  StokesSlab slab;
  SolverFGMRES<double, StokesBlockVector> solver;
  Preconditioner &preconditioner;
  const System &matrix;
  const SystemMatrixStokes<dim, double> &rhs_matrix;
  double reltol, abstol;
  unsigned max_nonlinear;
  unsigned nonlinear_steps_ = 0, linear_steps_ = 0;
  bool converged_ = false;
  std::vector<double> residuals_;
  StokesBlockVector residual, delta;
};

} // namespace stfem
