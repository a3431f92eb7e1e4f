// Host-side mirror of the reference's Stokes operators (include/operators.h:666-868
// SystemMatrixStokes, 1193-1766 StokesMatrixFreeOperator, 1768-1951 StokesNitscheMatrixFreeOperator;
// include/fe_time.h:901-1221 BlockSlice, 1242-1285 get_fe_time_weights_stokes) on the C-ABI (stfem_stokes_*):
// cell loop and, for weak boundary ids, the boundary-face loop; with a NonlinearTreatment the convection modes of the Navier-Stokes
// operator (OperatorMode::form / jacobian) and the NavierStokesOperator alias over PDE<> (operators.h:2052-2063).  Velocity degree 3
// with a NonlinearTreatment: the constructor by descriptor (StokesSpace).
#pragma once
#include "fe_time.h"
#include "operators.h"

#include <array>
#include <cmath>
#include <functional>
#include <limits>
#include <map>
#include <set>

namespace stfem {

// fe_time.h:901-1010 block_indexing / BlockSlice: block <-> (timestep, variable, timedof)
class BlockSlice {
public:
  BlockSlice(unsigned n_timesteps_at_once = 1, unsigned n_variables = 1, unsigned n_timedofs = 1, bool variable_major = true)
    : nts_(n_timesteps_at_once), nv_(n_variables), ntd_(n_timedofs), variable_major_(variable_major)
  {}
  unsigned index(unsigned timestep, unsigned variable, unsigned timedof) const
  {
    return variable_major_ ? timestep * (nv_ * ntd_) + variable * ntd_ + timedof
                           : timestep * (nv_ * ntd_) + timedof * nv_ + variable;
  }
  std::array<unsigned, 3> decompose(unsigned i) const
  {
    const unsigned ts = i / (nv_ * ntd_), r = i % (nv_ * ntd_);
    return variable_major_ ? std::array<unsigned, 3>{{ts, r / ntd_, r % ntd_}}
                           : std::array<unsigned, 3>{{ts, r % nv_, r / nv_}};
  }
  unsigned n_timesteps_at_once() const { return nts_; }
  unsigned n_variables() const { return nv_; }
  unsigned n_timedofs() const { return ntd_; }
  unsigned n_blocks() const { return nts_ * nv_ * ntd_; }
  bool variable_major() const { return variable_major_; }

private:
  unsigned nts_, nv_, ntd_;
  bool variable_major_;
};

// fe_time.h:1242-1285: {Alpha, Beta, Gamma, Zeta} in the (variable, time dof) block structure: the
// scalar matrices of get_fe_time_weights scattered over the two variables; no pressure-pressure
// block in Alpha, only velocity-velocity in Beta; Gamma / Zeta (right-hand side) on the velocity
// rows, Gamma for cG on the pressure rows too (1275-1282)
template <typename Number>
std::array<FullMatrix<Number>, 4> get_fe_time_weights_stokes(TimeStepType type, unsigned r, double time_step_size,
                                                             unsigned n_timesteps_at_once = 1)
{
  const auto tw = get_fe_time_weights<Number>(type, r, time_step_size, n_timesteps_at_once);
  const unsigned n = tw[0].m(), nt = n / n_timesteps_at_once;
  BlockSlice s(n_timesteps_at_once, 2, nt);
  std::array<FullMatrix<Number>, 4> ret{{FullMatrix<Number>(2 * n, 2 * n), FullMatrix<Number>(2 * n, 2 * n),
                                         FullMatrix<Number>(2 * n, tw[2].n()), FullMatrix<Number>(2 * n, tw[3].n())}};
  auto idx = [&](unsigned v, unsigned k) { return s.index(k / nt, v, k % nt); };
  for (unsigned a = 0; a < n; ++a) {
    for (unsigned b = 0; b < n; ++b) {
      for (unsigned iv = 0; iv < 2; ++iv)
        for (unsigned jv = 0; jv < 2; ++jv)
          if (!(iv == 1 && jv == 1)) ret[0](idx(iv, a), idx(jv, b)) = tw[0](a, b);
      ret[1](idx(0, a), idx(0, b)) = tw[1](a, b);
    }
    for (unsigned q = 0; q < tw[2].n(); ++q) {
      ret[2](idx(0, a), q) = tw[2](a, q);
      if (type == TimeStepType::CGP) ret[2](idx(1, a), q) = tw[2](a, q);
    }
    for (unsigned q = 0; q < tw[3].n(); ++q) ret[3](idx(0, a), q) = tw[3](a, q);
  }
  return ret;
}

// one device vector of a Stokes operator (velocity: 3 * n_velocity doubles, pressure: n_pressure)
class StokesVector {
public:
  StokesVector() = default;
  StokesVector(stfem_stokes_ctx *c, int variable) : c_(c), variable_(variable)
  {
    check(stfem_stokes_vector_create(c, variable, &d_), "stfem_stokes_vector_create");
    n_ = variable == 0 ? 3 * size_t(stfem_stokes_n_velocity_dofs(c)) : size_t(stfem_stokes_n_pressure_dofs(c));
  }
  StokesVector(StokesVector &&o) noexcept : c_(o.c_), variable_(o.variable_), d_(o.d_), n_(o.n_) { o.d_ = nullptr; }
  StokesVector &operator=(StokesVector &&o) noexcept
  {
    std::swap(c_, o.c_); std::swap(variable_, o.variable_); std::swap(d_, o.d_); std::swap(n_, o.n_);
    return *this;
  }
  StokesVector(const StokesVector &) = delete;
  ~StokesVector() { if (d_) stfem_stokes_vector_destroy(c_, d_); }
  double *data() const { return d_; }
  size_t size() const { return n_; }
  stfem_stokes_ctx *context() const { return c_; }
  void copy_from_host(const std::vector<double> &h)
  {
    if (h.size() != n_) throw std::invalid_argument("StokesVector size mismatch");
    check(stfem_stokes_vector_upload(c_, variable_, d_, h.data()), "stfem_stokes_vector_upload");
  }
  std::vector<double> copy_to_host() const
  {
    std::vector<double> h(n_);
    check(stfem_stokes_vector_download(c_, variable_, d_, h.data()), "stfem_stokes_vector_download");
    return h;
  }

private:
  stfem_stokes_ctx *c_ = nullptr;
  int variable_ = 0;
  double *d_ = nullptr;
  size_t n_ = 0;
};

// boundary ids of the structured block: 2 d + s (direction d, side s), as deal.II colorizes a hyper_rectangle
using boundary_id = unsigned;

// dst = rhs - dst, block by block in one launch (PDE::residual on the Stokes block vectors)
inline void rhs_minus(std::vector<StokesVector> &dst, const std::vector<StokesVector> &rhs)
{
  const size_t nb = dst.size();
  if (rhs.size() != nb) throw Error(STFEM_ERR_SHAPE_MISMATCH, "PDE::residual: blocks");
  if (nb == 0) return;
  std::vector<int64_t> len(nb);
  std::vector<const void *> px(nb);
  std::vector<void *> py(nb);
  for (size_t i = 0; i < nb; ++i) {
    if (rhs[i].size() != dst[i].size()) throw Error(STFEM_ERR_SHAPE_MISMATCH, "PDE::residual: block sizes");
    len[i] = int64_t(dst[i].size());
    px[i] = rhs[i].data();
    py[i] = dst[i].data();
  }
  stfem_ctx *pc = nullptr; // (any scalar context of the device serves the vector arithmetic: the pressure space's is at hand)
  check(stfem_stokes_pressure_ctx_space(dst[0].context(), &pc), "stfem_stokes_pressure_ctx_space"); // (either velocity degree)
  check(stfem_axpby_many(pc, int(nb), len.data(), 1.0, px.data(), -1.0, py.data(), nullptr), "PDE::residual");
}

// The operator by descriptor: what the second constructor of StokesMatrixFreeOperator takes.  velocity_degree 2 or 3; at degree 3 the
// cell operator with the convection term of the nonlinear treatment, or - linear operator only - with weak (Nitsche) faces; with
// delta0 != 0 the CIP interior-face term on top of either.
// The trailing members are those of the first constructor's arguments of the same names, applied through
// stfem_stokes_set_weak_boundaries_space (stfem_stokes_boundary_space.h) and stfem_stokes_set_cip_space (stfem_stokes_cip_space.h),
// which serve either degree; cip_weight is what set_cip_weight would set afterwards.
template <typename Number> struct StokesSpace {
  unsigned velocity_degree = 2;
  bool dg_pressure = false;
  Number viscosity = 1;
  NonlinearTreatment nonlinear_treatment = NonlinearTreatment::None;
  std::set<boundary_id> weak_boundary_ids = {};
  std::set<boundary_id> outflow_boundary_ids = {};
  Number penalty1 = 20;
  Number penalty2 = 10;
  Number delta0 = 0;
  int cip_weight = STFEM_CIP_WEIGHT_SOURCE;
};

// operators.h:1193-1766: cell loop + boundary-face loop for the weak (Nitsche) ids.  Same constructor arguments after the mesh as
// the reference (1199-1213), with dg_pressure before the nonlinear treatment.  delta0 != 0 switches the CIP interior-face term on
// (1605-1633, stfem_stokes_set_cip), weighted with the source of every vmult as in the reference; set_cip_weight chooses the
// linearisation velocity instead.  delta1 is accepted and unused, as in the reference.  A nonlinear treatment together with
// outflow_penalty != 0 throws (the outflow faces' value term, 1705-1709, is not built).
template <int dim, typename Number> class StokesMatrixFreeOperator {
  static_assert(dim == 3 && std::is_same<Number, double>::value, "3D, fp64");

public:
  using BlockVectorType = std::vector<StokesVector>; // {velocity, pressure}

  StokesMatrixFreeOperator(const Mesh &mesh, unsigned velocity_degree, Number viscosity, const std::set<boundary_id> &weak_boundary_ids = {},
                           const std::set<boundary_id> &outflow_boundary_ids = {}, Number penalty1 = 20, Number penalty2 = 10,
                           Number outflow_penalty = 0.0, Number delta0 = 0.0, Number /*delta1*/ = 0.0, bool dg_pressure = false,
                           NonlinearTreatment nonlinear_treatment_ = NonlinearTreatment::None)
    : nonlinear_treatment(nonlinear_treatment_), nonlinear(nonlinear_treatment_ != NonlinearTreatment::None)
  {
    // dg_pressure: FE_DGP(degree - 1) instead of FE_Q(degree - 1) for the pressure (the reference chooses the element of its
    // second DoFHandler, tests/tp_03stokes.cc:83-86: dGPressure)
    if (!std::isfinite(delta0)) throw Error(STFEM_ERR_INVALID_ARGUMENT, "StokesMatrixFreeOperator: delta0 is not finite");
    if (nonlinear && outflow_penalty != 0.0)
      throw Error(STFEM_ERR_UNSUPPORTED, "StokesMatrixFreeOperator: outflow_penalty != 0 with a nonlinear treatment is not built");
    // velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), QGauss(4)) has the linear cell operator alone: weak / outflow ids and
    // delta0 != 0 are refused by the C-ABI below, a nonlinear treatment here (its launches would only be refused at the first vmult)
    if (velocity_degree != 2 && nonlinear)
      throw Error(STFEM_ERR_UNSUPPORTED, "StokesMatrixFreeOperator: a nonlinear treatment is built for velocity degree 2 only");
    create(mesh, velocity_degree, viscosity, dg_pressure);
    try {
      int weak = 0, outflow = 0;
      for (boundary_id f : weak_boundary_ids) weak |= 1 << f;
      for (boundary_id f : outflow_boundary_ids) outflow |= 1 << f;
      if (weak || outflow) check(stfem_stokes_set_weak_boundaries(h_, weak, outflow, penalty1, penalty2), "stfem_stokes_set_weak_boundaries");
      delta0_ = delta0;
      if (delta0 != 0.0) check(stfem_stokes_set_cip(h_, delta0, STFEM_CIP_WEIGHT_SOURCE), "stfem_stokes_set_cip");
    } catch (...) { // (no destructor runs for a constructor that throws)
      stfem_stokes_destroy(h_);
      h_ = nullptr;
      throw;
    }
  }
  // By descriptor: a nonlinear treatment is accepted at velocity degree 3 too.  vmult, form and the SystemMatrixStokes calls over this
  // operator go through the _space entries of stfem_stokes_convection_space.h, which run a convection mode at either degree (degree 2:
  // the entries of the first constructor's operator, bit for bit).  Weak / outflow ids go through the _space setter of
  // stfem_stokes_boundary_space.h: at degree 3 the linear operator and the per-cell Vanka blocks over it hold the Nitsche terms; a
  // nonlinear treatment with weak ids is refused there (the inflow term of the faces is not built at degree 3).  delta0 / cip_weight go
  // through stfem_stokes_set_cip_space of stfem_stokes_cip_space.h: the CIP term at either degree, added last by every vmult.
  StokesMatrixFreeOperator(const Mesh &mesh, const StokesSpace<Number> &space)
    : nonlinear_treatment(space.nonlinear_treatment), nonlinear(space.nonlinear_treatment != NonlinearTreatment::None), space_entries_(true)
  {
    if (!std::isfinite(space.delta0)) throw Error(STFEM_ERR_INVALID_ARGUMENT, "StokesMatrixFreeOperator: delta0 is not finite");
    int weak = 0, outflow = 0;
    for (boundary_id f : space.weak_boundary_ids) weak |= 1 << f;
    for (boundary_id f : space.outflow_boundary_ids) outflow |= 1 << f;
    if (space.velocity_degree == 3 && nonlinear && (weak & ~outflow))
      throw Error(STFEM_ERR_UNSUPPORTED, "StokesMatrixFreeOperator: a nonlinear treatment with weak boundary ids is built for velocity degree 2 only");
    create(mesh, space.velocity_degree, space.viscosity, space.dg_pressure);
    if (weak || outflow) {
      const int rc = stfem_stokes_set_weak_boundaries_space(h_, weak, outflow, space.penalty1, space.penalty2);
      if (rc != STFEM_OK) { // (no destructor runs for a constructor that throws)
        stfem_stokes_destroy(h_);
        h_ = nullptr;
        check(rc, "stfem_stokes_set_weak_boundaries_space");
      }
    }
    delta0_ = space.delta0;
    cip_weight_ = space.cip_weight;
    if (space.delta0 != 0.0 || space.cip_weight != STFEM_CIP_WEIGHT_SOURCE) {
      const int rc = stfem_stokes_set_cip_space(h_, space.delta0, space.cip_weight);
      if (rc != STFEM_OK) {
        stfem_stokes_destroy(h_);
        h_ = nullptr;
        check(rc, "stfem_stokes_set_cip_space");
      }
    }
  }
  // whether the convection entries of this operator are the _space forms (the constructor by descriptor)
  bool space_entries() const { return space_entries_; }
  // Whose velocity weighs the CIP term: STFEM_CIP_WEIGHT_SOURCE (the reference: the source of the vmult, cubic in it) or
  // STFEM_CIP_WEIGHT_LINEARISATION (with a nonlinear treatment the linearisation velocity of set_data: linear in the source, what a
  // Krylov method needs).  form(x) about x itself is the same with both.  The state of the device context, like set_data.
  void set_cip_weight(int weight) const
  {
    if (space_entries_) check(stfem_stokes_set_cip_space(h_, delta0_, weight), "stfem_stokes_set_cip_space"); // (either degree)
    else check(stfem_stokes_set_cip(h_, delta0_, weight), "stfem_stokes_set_cip");
    cip_weight_ = weight;
  }
  // dst_u += C(weight_u; src_u) with the given delta0: the CIP term by itself, independent of the operator's own delta0
  // (stfem_stokes_cip_add; over an operator made by descriptor its _space form, which serves either degree)
  void cip_add(double *dst_u, const double *src_u, const double *weight_u, Number delta0, void *stream = nullptr) const
  {
    if (space_entries_) check(stfem_stokes_cip_add_space(h_, dst_u, src_u, weight_u, delta0, stream), "stfem_stokes_cip_add_space");
    else check(stfem_stokes_cip_add(h_, dst_u, src_u, weight_u, delta0, stream), "stfem_stokes_cip_add");
  }
  Number delta0() const { return delta0_; }
  unsigned velocity_degree() const { return velocity_degree_; }
  int cip_weight() const { return cip_weight_; }
  // The CIP term on a z-slab (stfem_stokes_set_cip_neighbours and its companions): neighbour_mask bit 4 / 5 a slab below / above,
  // the vertex plane one cell layer beyond each interface on a general mesh; the ghost planes of a velocity source are what the
  // neighbour's cip_pack made (StokesSystem packs, exchanges and binds them on a partitioned StokesSpaces).
  void set_cip_neighbours(int neighbour_mask, const double *lower_vertices = nullptr, const double *upper_vertices = nullptr) const
  {
    check(stfem_stokes_set_cip_neighbours(h_, neighbour_mask, lower_vertices, upper_vertices), "stfem_stokes_set_cip_neighbours");
  }
  size_t cip_ghost_size() const { return size_t(stfem_stokes_cip_ghost_size(h_)); }
  void cip_pack(const double *src_u, int side, double *out, void *stream = nullptr) const
  {
    check(stfem_stokes_cip_pack(h_, src_u, side, out, stream), "stfem_stokes_cip_pack");
  }
  void cip_add_slab(double *dst_u, const double *src_u, const double *weight_u, Number delta0, const double *lower_ghost,
                    const double *upper_ghost, void *stream = nullptr) const
  {
    check(stfem_stokes_cip_add_slab(h_, dst_u, src_u, weight_u, delta0, lower_ghost, upper_ghost, stream), "stfem_stokes_cip_add_slab");
  }
  void cip_bind_ghosts(const double *src_u, const double *lower_ghost, const double *upper_ghost) const
  {
    check(stfem_stokes_cip_bind_ghosts(h_, src_u, lower_ghost, upper_ghost), "stfem_stokes_cip_bind_ghosts");
  }

private:
  void create(const Mesh &mesh, unsigned velocity_degree, Number viscosity, bool dg_pressure)
  {
    stfem_mesh_desc md{};
    for (int d = 0; d < 3; ++d) {
      md.ncell[d] = mesh.ncell[d];
      md.lower[d] = mesh.lower[d];
      md.upper[d] = mesh.upper[d];
    }
    md.vertices = mesh.vertices.empty() ? nullptr : mesh.vertices.data();
    md.dirichlet_mask = mesh.dirichlet_mask;
    md.device = mesh.device;
    stfem_stokes_space_desc sd{};
    sd.velocity_degree = int32_t(velocity_degree);
    sd.pressure_space = dg_pressure ? 1 : 0;
    sd.viscosity = viscosity;
    check(stfem_stokes_create_space(&md, &sd, &h_), "stfem_stokes_create_space");
    velocity_degree_ = velocity_degree;
    n_cells_ = size_t(mesh.ncell[0]) * size_t(mesh.ncell[1]) * size_t(mesh.ncell[2]);
  }

public:
  ~StokesMatrixFreeOperator()
  {
    cells_ = StokesVector(); // (freed through the context, so before it)
    stfem_stokes_destroy(h_);
  }
  StokesMatrixFreeOperator(const StokesMatrixFreeOperator &) = delete;

  void initialize_dof_vector(BlockVectorType &vec) const // operators.h:1254-1262
  {
    vec.clear();
    vec.emplace_back(h_, 0);
    vec.emplace_back(h_, 1);
  }
  void initialize_dof_vector(StokesVector &vec, unsigned variable) const { vec = StokesVector(h_, int(variable)); }

  // operators.h:1288-1297: none / form (Explicit) / jacobian (Implicit)
  void vmult(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const { apply(vmult_mode(), dst, src, stream); }
  // operators.h:1279-1286: the nonlinear weak form; the linear operator without a nonlinear treatment
  void form(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const { apply(form_mode(), dst, src, stream); }
  // operators.h:1333-1342: the linearisation state, {velocity, pressure} (only the velocity is read) or the velocity alone; it is
  // referred to, not copied
  void set_data(const BlockVectorType &data) const { set_data(data.at(0)); }
  void set_data(const StokesVector &velocity) const
  {
    if (!nonlinear) throw Error(STFEM_ERR_INVALID_ARGUMENT, "StokesMatrixFreeOperator::set_data: not allowed without a nonlinear treatment");
    lin_ = velocity.data();
  }
  // the STFEM_CONVECTION_* mode behind vmult / form
  int vmult_mode() const
  {
    return nonlinear_treatment == NonlinearTreatment::None ? STFEM_CONVECTION_NONE
           : nonlinear_treatment == NonlinearTreatment::Explicit ? STFEM_CONVECTION_FORM : STFEM_CONVECTION_JACOBIAN;
  }
  int form_mode() const { return nonlinear ? STFEM_CONVECTION_FORM : STFEM_CONVECTION_NONE; }
  // the MassMatrixType of SystemMatrixStokes (vector mass)
  void mass_vmult(StokesVector &dst, const StokesVector &src, void *stream = nullptr) const
  {
    check(stfem_stokes_mass_vmult(h_, dst.data(), src.data(), stream), "vector mass vmult");
  }
  // operators.h:1391-1415: sqrt(sum_cells int (div u_h)^2) of the velocity of src, read plain; cell_vector (the reference's
  // ReadWriteVector) receives the cell values, cells lexicographic
  Number compute_divergence(const BlockVectorType &src, std::vector<Number> &cell_vector, void *stream = nullptr) const
  {
    return compute_divergence(src.at(0), cell_vector, stream);
  }
  Number compute_divergence(const StokesVector &velocity, std::vector<Number> &cell_vector, void *stream = nullptr) const
  {
    // (the cell values land in a pressure vector: either pressure space has at least one DoF per cell)
    if (!cells_.data()) cells_ = StokesVector(h_, 1);
    Number total = 0;
    check(divergence_entry()(h_, velocity.data(), cells_.data(), &total, stream), divergence_entry_name());
    const std::vector<double> h = cells_.copy_to_host();
    cell_vector.assign(h.begin(), h.begin() + (long long)n_cells_);
    return total;
  }
  Number compute_divergence(const StokesVector &velocity, void *stream = nullptr) const // (the total alone)
  {
    Number total = 0;
    check(divergence_entry()(h_, velocity.data(), nullptr, &total, stream), divergence_entry_name());
    return total;
  }
  // (an operator by descriptor or of velocity degree 3: the _space form of stfem_stokes_pressure_space.h, which runs at either degree)
  decltype(&stfem_stokes_divergence) divergence_entry() const
  {
    return space_entries_ || velocity_degree_ != 2 ? stfem_stokes_divergence_space : stfem_stokes_divergence;
  }
  const char *divergence_entry_name() const
  {
    return space_entries_ || velocity_degree_ != 2 ? "stfem_stokes_divergence_space" : "stfem_stokes_divergence";
  }
  // operators.h:1344-1389: scale * sum over the boundary faces of obstacle_id of int (p n - nu (grad u + grad u^T) n) dA for the pair
  // src = {velocity, pressure}, the reference's argument order.  Velocity entries on strongly constrained DoFs read as 0 as in the
  // reference (read_dof_values, 1366); plain = true reads them as stored (inhomogeneous strong data).  Slabs: every rank leaves its
  // interface faces out of obstacle_id and the ranks' results add (the reference's MPI sum, 1387).
  std::array<Number, 3> compute_drag_lift(const BlockVectorType &src, const std::set<boundary_id> &obstacle_id, Number scale,
                                          bool plain = false, void *stream = nullptr) const
  {
    return compute_drag_lift(std::vector<const StokesVector *>{&src.at(0)}, std::vector<const StokesVector *>{&src.at(1)}, obstacle_id, scale,
                             plain, stream)[0];
  }
  // several (velocity, pressure) pairs in one call - the time DoFs of a slab, tests/tp_03stokes.cc:936-966: bit for bit what the calls
  // with one pair give, the face geometry evaluated once for (up to four of) them
  std::vector<std::array<Number, 3>> compute_drag_lift(const std::vector<const StokesVector *> &velocities,
                                                       const std::vector<const StokesVector *> &pressures,
                                                       const std::set<boundary_id> &obstacle_id, Number scale, bool plain = false,
                                                       void *stream = nullptr) const
  {
    if (velocities.size() != pressures.size()) throw Error(STFEM_ERR_SHAPE_MISMATCH, "compute_drag_lift: velocities and pressures");
    int faces = 0;
    for (boundary_id f : obstacle_id) {
      if (f > 5) throw Error(STFEM_ERR_INVALID_ARGUMENT, "compute_drag_lift: boundary id above 5");
      faces |= 1 << f;
    }
    const size_t n = velocities.size();
    std::vector<const double *> u(n), p(n);
    for (size_t i = 0; i < n; ++i) {
      u[i] = velocities[i] ? velocities[i]->data() : nullptr;
      p[i] = pressures[i] ? pressures[i]->data() : nullptr;
    }
    std::vector<std::array<Number, 3>> f(n);
    static_assert(sizeof(std::array<Number, 3>) == 3 * sizeof(double), "out is [n][3]");
    check(stfem_stokes_drag_lift(h_, faces, scale, plain ? 1 : 0, int(n), u.data(), p.data(), nullptr, n ? f[0].data() : nullptr, stream),
          "stfem_stokes_drag_lift");
    return f;
  }
  unsigned long long m() const { return 3ull * stfem_stokes_n_velocity_dofs(h_) + stfem_stokes_n_pressure_dofs(h_); }
  stfem_stokes_ctx *handle() const { return h_; }

private:
  void apply(int mode, BlockVectorType &dst, const BlockVectorType &src, void *stream) const
  {
    if (mode != STFEM_CONVECTION_NONE && !lin_) throw Error(STFEM_ERR_INVALID_ARGUMENT, "StokesMatrixFreeOperator: no linearization set");
    check((space_entries_ ? stfem_stokes_vmult_convection_space : stfem_stokes_vmult_convection)(
            h_, mode, dst.at(0).data(), dst.at(1).data(), src.at(0).data(), src.at(1).data(), lin_, stream),
          "StokesMatrixFreeOperator::vmult");
  }
  stfem_stokes_ctx *h_ = nullptr;
  NonlinearTreatment nonlinear_treatment;
  bool nonlinear;
  bool space_entries_ = false;
  mutable const double *lin_ = nullptr; // data_lin[0]
  Number delta0_ = 0.0;
  unsigned velocity_degree_ = 2;
  mutable int cip_weight_ = STFEM_CIP_WEIGHT_SOURCE;
  size_t n_cells_ = 0;
  mutable StokesVector cells_; // device cell values of compute_divergence, made on demand
};

// operators.h:1768-1951: the right-hand-side functional of the weakly imposed Dirichlet data.  It shares the geometry
// of the StokesMatrixFreeOperator it is built from (the reference builds a second MatrixFree from the same arguments).
template <int dim, typename Number> class StokesNitscheMatrixFreeOperator {
public:
  using BlockVectorType = std::vector<StokesVector>;
  using Function = std::function<std::array<Number, 3>(const std::array<Number, 3> &)>; // Function<dim, Number>::vector_value

  explicit StokesNitscheMatrixFreeOperator(const StokesMatrixFreeOperator<dim, Number> &op) : op_(op)
  {
    // (an operator made by descriptor: the _space entries of stfem_stokes_boundary_space.h, which serve velocity degree 3 too)
    if (op.space_entries()) {
      points_.resize(3 * size_t(stfem_stokes_n_face_points_space(op.handle())));
      if (!points_.empty()) check(stfem_stokes_face_points_space(op.handle(), points_.data()), "stfem_stokes_face_points_space");
    } else {
      points_.resize(3 * size_t(stfem_stokes_n_face_points(op.handle())));
      if (!points_.empty()) check(stfem_stokes_face_points(op.handle(), points_.data()), "stfem_stokes_face_points");
    }
  }
  // operators.h:1801-1807.  One function for all weak faces here (the reference maps boundary ids to functions; the
  // points of the faces come in ascending face order, so a caller with several functions can switch on the point)
  void set_dirichlet_functions(const Function &g) const { g_ = g; }
  void initialize_dof_vector(BlockVectorType &vec) const { op_.initialize_dof_vector(vec); }
  // operators.h:1833-1849: dst += the boundary integrals of g; nothing without Dirichlet functions
  void vmult(BlockVectorType &dst, void *stream = nullptr) const
  {
    if (!g_ || points_.empty()) return;
    std::vector<Number> gq(points_.size());
    for (size_t q = 0; q < points_.size() / 3; ++q) {
      const auto v = g_({{points_[3 * q], points_[3 * q + 1], points_[3 * q + 2]}});
      for (int e = 0; e < 3; ++e) gq[3 * q + e] = v[e];
    }
    check((op_.space_entries() ? stfem_stokes_nitsche_rhs_space : stfem_stokes_nitsche_rhs)(op_.handle(), gq.data(), dst.at(0).data(), dst.at(1).data(), stream),
          "StokesNitscheMatrixFreeOperator::vmult");
  }
  unsigned long long m() const { return op_.m(); }

private:
  const StokesMatrixFreeOperator<dim, Number> &op_;
  std::vector<double> points_;
  mutable Function g_;
};

// The ghost planes of one side of a slab for the CIP term (stfem_stokes_cip_ghost_create): 3 * 2 * ndx * ndy doubles on the device
class CipGhost {
public:
  CipGhost() = default;
  explicit CipGhost(stfem_stokes_ctx *c) : c_(c) { check(stfem_stokes_cip_ghost_create(c, &d_), "stfem_stokes_cip_ghost_create"); }
  CipGhost(CipGhost &&o) noexcept : c_(o.c_), d_(o.d_) { o.d_ = nullptr; }
  CipGhost &operator=(CipGhost &&o) noexcept
  {
    std::swap(c_, o.c_); std::swap(d_, o.d_);
    return *this;
  }
  CipGhost(const CipGhost &) = delete;
  ~CipGhost() { if (d_) stfem_stokes_cip_ghost_destroy(c_, d_); } // (drops the bindings that name it)
  double *data() const { return d_; }

private:
  stfem_stokes_ctx *c_ = nullptr;
  double *d_ = nullptr;
};

// operators.h:666-868; blocks in BlockSlice order
template <int dim, typename Number> class SystemMatrixStokes {
public:
  using BlockVectorType = std::vector<StokesVector>;

  SystemMatrixStokes(const StokesMatrixFreeOperator<dim, Number> &K, const FullMatrix<Number> &Alpha_,
                     const FullMatrix<Number> &Beta_, const BlockSlice &blk_slice_,
                     NonlinearTreatment nonlinear_treatment_ = NonlinearTreatment::None)
    : K(K), Alpha(Alpha_), Beta(Beta_), blk_slice(blk_slice_), nonlinear(nonlinear_treatment_ != NonlinearTreatment::None)
  {
    if (Alpha.m() != blk_slice.n_blocks() || (Alpha.n() != Alpha.m() && Alpha.n() != 1) || Beta.m() != Alpha.m() ||
        Beta.n() != Alpha.n())
      throw std::invalid_argument("Alpha/Beta do not match the block slice");
  }
  void initialize_dof_vector(BlockVectorType &vec) const // operators.h:802-812
  {
    vec.clear();
    for (unsigned i = 0; i < blk_slice.n_blocks(); ++i) vec.emplace_back(K.handle(), int(blk_slice.decompose(i)[1]));
  }
  // operators.h:385-388: the linearisation vector, in BlockSlice order (n x 1 systems: one {velocity, pressure} pair); referred to,
  // not copied.  Source time dof (it, id) is linearised about its block index(it, 0, id) (473-484, 843-846).
  void set_data(const BlockVectorType &solution_linearization_) const { solution_linearization = &solution_linearization_; }
  // the weight velocity of the operator's CIP term (StokesMatrixFreeOperator::set_cip_weight)
  void set_cip_weight(int weight) const { K.set_cip_weight(weight); }
  Number delta0() const { return K.delta0(); }
  void vmult(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const // 696-700
  {
    tensorproduct_eval(dst, src, K.vmult_mode(), stream);
  }
  void form(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const // 702-706
  {
    tensorproduct_eval(dst, src, K.form_mode(), stream);
  }

private:
  // the velocity blocks of the linearisation vector for the operator's mode (pressure entries stay null)
  std::vector<const double *> linearization(int mode, unsigned n_expected, const char *what) const
  {
    std::vector<const double *> l;
    if (mode == STFEM_CONVECTION_NONE) return l;
    if (!nonlinear || !solution_linearization) throw Error(STFEM_ERR_INVALID_ARGUMENT, std::string(what) + ": no linearization set");
    if (solution_linearization->size() != n_expected) throw Error(STFEM_ERR_SHAPE_MISMATCH, std::string(what) + ": linearization blocks");
    l.assign(n_expected, nullptr);
    return l;
  }
  void tensorproduct_eval(BlockVectorType &dst, const BlockVectorType &src, int mode, void *stream) const // 819-867
  {
    const unsigned nb = blk_slice.n_blocks();
    if (dst.size() != nb || src.size() != nb) throw Error(STFEM_ERR_SHAPE_MISMATCH, "SystemMatrixStokes::vmult");
    std::vector<double *> d(nb);
    std::vector<const double *> s(nb);
    for (unsigned i = 0; i < nb; ++i) { d[i] = dst[i].data(); s[i] = src[i].data(); }
    std::vector<const double *> l = linearization(mode, nb, "SystemMatrixStokes::vmult");
    if (!l.empty())
      for (unsigned it = 0; it < blk_slice.n_timesteps_at_once(); ++it)
        for (unsigned id = 0; id < blk_slice.n_timedofs(); ++id) {
          const unsigned i = blk_slice.index(it, 0, id);
          l[i] = (*solution_linearization)[i].data();
        }
    check((K.space_entries() ? stfem_stokes_st_vmult_convection_space : stfem_stokes_st_vmult_convection)(
            K.handle(), mode, int(blk_slice.n_timesteps_at_once()), int(blk_slice.n_timedofs()), blk_slice.variable_major() ? 1 : 0,
            Alpha.data(), Beta.data(), d.data(), s.data(), l.empty() ? nullptr : l.data(), stream),
          "SystemMatrixStokes::vmult");
  }

public:
  // operators.h:708-745, as the reference has it: its scatter overload (operators.h:111-123) reads j = index(it, v, id),
  // i = index(jt, v, jd) - the result of source time dof (it, id) only reaches the destination blocks of the SAME time dof,
  // weighted with the entries of row j summed over (jt, jd).  Not a transpose; reproduced as one vmult with those matrices.
  void Tvmult(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const
  {
    const unsigned nb = blk_slice.n_blocks(), ns = blk_slice.n_timesteps_at_once(), nt = blk_slice.n_timedofs();
    if (dst.size() != nb || src.size() != nb || Alpha.n() != nb) throw Error(STFEM_ERR_SHAPE_MISMATCH, "SystemMatrixStokes::Tvmult");
    const double eps10 = 10 * std::numeric_limits<Number>::epsilon();
    FullMatrix<Number> Ae(nb, nb), Be(nb, nb);
    for (unsigned it = 0; it < ns; ++it)
      for (unsigned id = 0; id < nt; ++id) {
        const unsigned col = blk_slice.index(it, 0, id);
        for (unsigned v = 0; v < 2; ++v) {
          const unsigned j = blk_slice.index(it, v, id);
          for (unsigned jt = 0; jt < ns; ++jt)
            for (unsigned jd = 0; jd < nt; ++jd) {
              const unsigned i = blk_slice.index(jt, v, jd);
              if (std::abs(Alpha(j, i)) > eps10) Ae(j, col) += Alpha(j, i);
              if (v == 0 && std::abs(Beta(j, i)) > eps10) Be(j, col) += Beta(j, i);
            }
        }
      }
    std::vector<double *> d(nb);
    std::vector<const double *> s(nb);
    for (unsigned i = 0; i < nb; ++i) { d[i] = dst[i].data(); s[i] = src[i].data(); }
    check(stfem_stokes_st_vmult(K.handle(), int(ns), int(nt), blk_slice.variable_major() ? 1 : 0, Ae.data(), Be.data(), d.data(), s.data(), stream),
          "SystemMatrixStokes::Tvmult");
  }
  // n x 1 case for the right-hand side (operators.h:748-781): Alpha, Beta are n x 1 here and src is one
  // (velocity, pressure) pair; dst is accumulated into
  void vmult_slice_add(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const
  {
    slice_add(dst, src, K.vmult_mode(), stream);
  }
  // the same with the nonlinear weak form (form in place of vmult): the previous-slab term of a Navier-Stokes slab, whose j = 0
  // time dof is linearised about itself whatever the treatment of the system (set_data(src) first)
  void form_slice_add(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const
  {
    slice_add(dst, src, K.form_mode(), stream);
  }

private:
  void slice_add(BlockVectorType &dst, const BlockVectorType &src, int mode, void *stream) const
  {
    const unsigned nb = blk_slice.n_blocks();
    if (dst.size() != nb || src.size() != 2 || Alpha.n() != 1) throw Error(STFEM_ERR_SHAPE_MISMATCH, "vmult_slice_add");
    std::vector<double *> d(nb);
    for (unsigned i = 0; i < nb; ++i) d[i] = dst[i].data();
    // (759-761: set_linearization_data_slice - one linearisation pair for the one source pair)
    const std::vector<const double *> l = linearization(mode, 2, "SystemMatrixStokes::vmult_slice_add");
    check((K.space_entries() ? stfem_stokes_st_vmult_slice_add_convection_space : stfem_stokes_st_vmult_slice_add_convection)(
            K.handle(), mode, int(blk_slice.n_timesteps_at_once()), int(blk_slice.n_timedofs()), blk_slice.variable_major() ? 1 : 0,
            Alpha.data(), Beta.data(), d.data(), src[0].data(), src[1].data(),
            l.empty() ? nullptr : (*solution_linearization)[0].data(), stream),
          "SystemMatrixStokes::vmult_slice_add");
  }

public:
  unsigned long long m() const { return (unsigned long long)(blk_slice.n_blocks() / 2) * K.m(); }

private:
  const StokesMatrixFreeOperator<dim, Number> &K;
  const FullMatrix<Number> &Alpha;
  const FullMatrix<Number> &Beta;
  BlockSlice blk_slice;
  bool nonlinear;
  mutable const BlockVectorType *solution_linearization = nullptr;
};

// operators.h:2052-2063: the nonlinear-solver face of the space-time Navier-Stokes system: residual = rhs - form(src), vmult = the
// Jacobian (or, with the Explicit treatment, the form), set_data = the linearisation vector
template <int dim, typename Number>
using NavierStokesOperator =
  PDE<dim, Number, SystemMatrixStokes<dim, Number>, SystemMatrixStokes<dim, Number>, std::vector<StokesVector>>;

// PreconditionVanka in its block form (include/stmg.h:626-738, 832-872) as tests/tp_03stokes.cc:537-540, 714-726 creates it for the
// Stokes levels: the assembled Stokes and mass matrices restricted to every cell's velocity and pressure DoFs, combined with
// Alpha / Beta over the blocks of the BlockSlice (K_mask empty, M_mask(0, 0) only), inverted.  The assembled matrices and DoF
// handlers of the reference's constructor are not needed: the blocks follow from the operator (stfem_stokes_vanka_create; one block
// per neighbour pattern on a box, one per cell on a general mesh and, second constructor, for the linearised operator).  An operator
// of velocity degree 3 goes through stfem_stokes_vanka_create_space (first constructor) or stfem_stokes_vanka_create_linearised_space
// (second constructor, delta0 == 0 only): one block per cell on every mesh.
template <typename Number> class PreconditionVankaStokes {
  static_assert(std::is_same<Number, double>::value, "fp64");

public:
  using BlockVectorType = std::vector<StokesVector>;
  template <int dim>
  PreconditionVankaStokes(const StokesMatrixFreeOperator<dim, Number> &K, const FullMatrix<Number> &Alpha, const FullMatrix<Number> &Beta,
                          const BlockSlice &blk_slice)
    : nb_(blk_slice.n_blocks()), slice_(blk_slice)
  {
    if (Alpha.m() != nb_ || Alpha.n() != nb_ || Beta.m() != nb_ || Beta.n() != nb_) throw std::invalid_argument("Alpha/Beta do not match the block slice");
    std::vector<int32_t> var(nb_);
    for (unsigned i = 0; i < nb_; ++i) var[i] = int32_t(blk_slice.decompose(i)[1]);
    stfem_stokes_vanka *v = nullptr;
    if (K.velocity_degree() != 2) { // FE_Q(3)^3 x FE_Q(2) / FE_DGP(2): the constructor by descriptor, one block per cell of the linear operator
      stfem_stokes_vanka_space_desc d{}; // (reserved: 0)
      d.n_blocks = int32_t(nb_);
      d.block_variable = var.data();
      d.Alpha = Alpha.data();
      d.Beta = Beta.data();
      const int rc = stfem_stokes_vanka_create_space(K.handle(), &d, &v);
      if (rc != STFEM_OK) throw Error(rc, "stfem_stokes_vanka_create_space");
    } else {
      const int rc = stfem_stokes_vanka_create(K.handle(), int(nb_), var.data(), Alpha.data(), Beta.data(), &v);
      if (rc != STFEM_OK) throw Error(rc, "stfem_stokes_vanka_create");
    }
    v_.reset(v, stfem_stokes_vanka_destroy);
  }
  // The smoother of the LINEARISED operator, one block per cell (reinit_asm, stmg.h:929-965: set_data(mg_data[l]), the assembled
  // matrix of compute_matrix_helper<OperatorMode::jacobian>, operators.h:1310-1318, and the blocks from it, stmg.h:704-742): the
  // column blocks of time dof (it, id) are linearised about block index(it, 0, id) of solution_linearization (operators.h:835-866).
  // NonlinearTreatment::None gives the plain Stokes blocks, Explicit the form, Implicit the jacobian (as the operator's vmult).
  // delta0 != 0: the blocks hold the CIP term C(b_j; .) weighted by the linearisation state too (the reference's blocks are cut out of
  // the matrix of an operator that holds delta0, tests/tp_03stokes.cc:610-623, 655-726); update keeps it.
  template <int dim>
  PreconditionVankaStokes(const StokesMatrixFreeOperator<dim, Number> &K, const FullMatrix<Number> &Alpha, const FullMatrix<Number> &Beta,
                          const BlockSlice &blk_slice, NonlinearTreatment nonlinear_treatment, const BlockVectorType &solution_linearization,
                          Number delta0 = 0)
    : nb_(blk_slice.n_blocks()), slice_(blk_slice)
  {
    if (Alpha.m() != nb_ || Alpha.n() != nb_ || Beta.m() != nb_ || Beta.n() != nb_) throw std::invalid_argument("Alpha/Beta do not match the block slice");
    std::vector<int32_t> var(nb_);
    for (unsigned i = 0; i < nb_; ++i) var[i] = int32_t(blk_slice.decompose(i)[1]);
    const int mode = nonlinear_treatment == NonlinearTreatment::None ? STFEM_CONVECTION_NONE
                     : nonlinear_treatment == NonlinearTreatment::Explicit ? STFEM_CONVECTION_FORM : STFEM_CONVECTION_JACOBIAN;
    const std::vector<const double *> l = linearization(solution_linearization);
    stfem_stokes_vanka *v = nullptr;
    if (K.velocity_degree() != 2) { // FE_Q(3)^3 x FE_Q(2) / FE_DGP(2): the constructor by descriptor of the linearised blocks
      if (delta0 != 0) throw Error(STFEM_ERR_UNSUPPORTED, "PreconditionVankaStokes: delta0 != 0 at velocity degree 3 (the CIP term is not built into the blocks of that degree)");
      stfem_stokes_vanka_linearised_space_desc d{}; // (reserved: 0)
      d.n_blocks = int32_t(nb_);
      d.block_variable = var.data();
      d.Alpha = Alpha.data();
      d.Beta = Beta.data();
      d.mode = mode;
      d.lin_blocks = l.data();
      const int rc = stfem_stokes_vanka_create_linearised_space(K.handle(), &d, &v);
      if (rc != STFEM_OK) throw Error(rc, "stfem_stokes_vanka_create_linearised_space");
      v_.reset(v, stfem_stokes_vanka_destroy);
      return;
    }
    const int rc = delta0 != 0 ? stfem_stokes_vanka_create_linearised_cip(K.handle(), int(nb_), var.data(), Alpha.data(), Beta.data(), mode, l.data(), delta0, &v)
                               : stfem_stokes_vanka_create_linearised(K.handle(), int(nb_), var.data(), Alpha.data(), Beta.data(), mode, l.data(), &v);
    if (rc != STFEM_OK) throw Error(rc, delta0 != 0 ? "stfem_stokes_vanka_create_linearised_cip" : "stfem_stokes_vanka_create_linearised");
    v_.reset(v, stfem_stokes_vanka_destroy);
  }
  // The same on a z-slab of a partitioned mesh (stfem_stokes_vanka_create_linearised_partitioned).  K_extended: the operator of the slab
  // plus ONE ghost cell layer on every z side of neighbour_mask (bit 4 below, bit 5 above; a z face of a ghost layer constrained / weak
  // exactly where it is the global boundary); solution_linearization, also that of update, lives on K_extended; beyond_mask: there are
  // cells beyond that ghost layer (read with delta0 != 0).  Blocks for the slab's own cells, applied on K_slab: vmult / step leave
  // partial sums in the interface planes, completed by the add-exchange of the scalar views.  K_extended must outlive the smoother.
  template <int dim>
  PreconditionVankaStokes(const StokesMatrixFreeOperator<dim, Number> &K_slab, const StokesMatrixFreeOperator<dim, Number> &K_extended,
                          const FullMatrix<Number> &Alpha, const FullMatrix<Number> &Beta, const BlockSlice &blk_slice,
                          NonlinearTreatment nonlinear_treatment, const BlockVectorType &solution_linearization, Number delta0,
                          int neighbour_mask, int beyond_mask)
    : nb_(blk_slice.n_blocks()), slice_(blk_slice)
  {
    if (Alpha.m() != nb_ || Alpha.n() != nb_ || Beta.m() != nb_ || Beta.n() != nb_) throw std::invalid_argument("Alpha/Beta do not match the block slice");
    std::vector<int32_t> var(nb_);
    for (unsigned i = 0; i < nb_; ++i) var[i] = int32_t(blk_slice.decompose(i)[1]);
    const int mode = nonlinear_treatment == NonlinearTreatment::None ? STFEM_CONVECTION_NONE
                     : nonlinear_treatment == NonlinearTreatment::Explicit ? STFEM_CONVECTION_FORM : STFEM_CONVECTION_JACOBIAN;
    const std::vector<const double *> l = linearization(solution_linearization);
    stfem_stokes_vanka *v = nullptr;
    const int rc = stfem_stokes_vanka_create_linearised_partitioned(K_slab.handle(), K_extended.handle(), int(nb_), var.data(), Alpha.data(),
                                                                    Beta.data(), mode, l.data(), delta0, neighbour_mask, beyond_mask, &v);
    if (rc != STFEM_OK) throw Error(rc, "stfem_stokes_vanka_create_linearised_partitioned");
    v_.reset(v, stfem_stokes_vanka_destroy);
  }
  // the blocks again for a new linearisation vector (same treatment, same storage): the next Newton / Picard step
  void update(const BlockVectorType &solution_linearization)
  {
    const std::vector<const double *> l = linearization(solution_linearization);
    const int rc = stfem_stokes_vanka_update(v_.get(), l.data());
    if (rc != STFEM_OK) throw Error(rc, "stfem_stokes_vanka_update");
  }
  void vmult(BlockVectorType &dst, const BlockVectorType &src, void *stream = nullptr) const { step(dst, 1.0, false, src, stream); }
  void smooth(BlockVectorType &u, const BlockVectorType &rhs) const { vmult(u, rhs); }
  // dst = (accumulate ? dst : 0) + omega * vmult(src): the step of the PreconditionRelaxation around the smoother (stmg.h:1199-1238)
  void step(BlockVectorType &dst, double omega, bool accumulate, const BlockVectorType &src, void *stream = nullptr) const
  {
    if (dst.size() != nb_ || src.size() != nb_) throw Error(STFEM_ERR_SHAPE_MISMATCH, "PreconditionVankaStokes::vmult");
    std::vector<double *> d(nb_);
    std::vector<const double *> s(nb_);
    for (unsigned i = 0; i < nb_; ++i) { d[i] = dst[i].data(); s[i] = src[i].data(); }
    const int rc = stfem_stokes_vanka_step(v_.get(), d.data(), omega, accumulate ? 1 : 0, s.data(), stream);
    if (rc != STFEM_OK) throw Error(rc, "PreconditionVankaStokes::vmult");
  }
  // the same on a vector that holds its blocks (StokesBlockVector): the smoother interface PreconditionRelaxation and the power iteration consume
  template <typename V> void vmult(V &dst, const V &src, void *stream = nullptr) const { step(dst.blocks(), 1.0, false, src.blocks(), stream); }
  template <typename V> void step(V &dst, double omega, bool accumulate, const V &src, void *stream = nullptr) const { step(dst.blocks(), omega, accumulate, src.blocks(), stream); }
  int n_classes() const { return stfem_stokes_vanka_n_classes(v_.get()); }

private:
  // the velocity blocks of the linearisation vector (pressure entries stay null)
  std::vector<const double *> linearization(const BlockVectorType &lin) const
  {
    if (lin.size() != nb_) throw Error(STFEM_ERR_SHAPE_MISMATCH, "PreconditionVankaStokes: linearization blocks");
    std::vector<const double *> l(nb_, nullptr);
    for (unsigned i = 0; i < nb_; ++i)
      if (slice_.decompose(i)[1] == 0) l[i] = lin[i].data();
    return l;
  }
  unsigned nb_;
  BlockSlice slice_;
  std::shared_ptr<stfem_stokes_vanka> v_;
};

} // namespace stfem
