// C++ caller of the smoother of the linearised operator WITH the CIP term in its blocks (the delta0 argument of the linearised
// constructor of PreconditionVankaStokes, its update and one relaxation step; RelaxedVankaStokes with its trailing delta0) on a
// perturbed mesh, against the values the same calls give through the C-ABI (stfem_stokes_vanka_create_linearised_cip / _step).
//   test_host_navier_cip_vanka ncx ncy ncz type r nsteps viscosity delta0
// Prints one line: blocks=<n> cells=<n> mirror_vs_capi=<max |difference|> update_changed=<0|1> term_changed=<0|1>
// zero_vs_plain=<max |difference|> relaxed_vs_step=<max |difference|> exceptions=<count of the refusals that threw as they should>
#include "stfem/stokes_solver.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace stfem;

static std::vector<double> seeded(size_t n, unsigned seed)
{
  std::vector<double> h(n);
  std::mt19937_64 rng(seed);
  for (double &v : h) v = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  return h;
}
static std::vector<double> host(const std::vector<StokesVector> &v)
{
  std::vector<double> all;
  for (const auto &b : v) {
    const auto h = b.copy_to_host();
    all.insert(all.end(), h.begin(), h.end());
  }
  return all;
}
static double max_difference(const std::vector<double> &a, const std::vector<double> &b)
{
  if (a.size() != b.size()) return 1e300;
  double worst = 0.0;
  for (size_t i = 0; i < a.size(); ++i) worst = std::max(worst, std::abs(a[i] - b[i]));
  return worst;
}

int main(int argc, char **argv)
{
  if (argc != 9) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    mesh.dirichlet_mask = 63;
    const TimeStepType type = std::atoi(argv[4]) == 0 ? TimeStepType::CGP : TimeStepType::DG;
    const unsigned r = unsigned(std::atoi(argv[5])), ns = unsigned(std::atoi(argv[6]));
    const double nu = std::atof(argv[7]), delta0 = std::atof(argv[8]);
    const auto w = get_fe_time_weights_stokes<double>(type, r, 1.0 / 32, ns);
    const unsigned nt = type == TimeStepType::CGP ? r : r + 1;
    BlockSlice slice(ns, 2, nt);
    const NonlinearTreatment treatment = NonlinearTreatment::Implicit;
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, delta0, 0.0, false, treatment);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
    std::vector<StokesVector> src, lin1, lin2, y1, y2, y3, yz, yp;
    for (auto *v : {&src, &lin1, &lin2, &y1, &y2, &y3, &yz, &yp}) A.initialize_dof_vector(*v);
    const unsigned nb = unsigned(src.size());
    for (unsigned b = 0; b < nb; ++b) {
      src[b].copy_from_host(seeded(src[b].size(), 4321 + b));
      lin1[b].copy_from_host(seeded(src[b].size(), 8765 + b));
      lin2[b].copy_from_host(seeded(src[b].size(), 1357 + b));
    }
    const double omega = 0.7;
    int thrown = 0;
    // the mirror: created about lin1 with the term, updated to lin2 (the delta0 of creation is kept), one step
    PreconditionVankaStokes<double> V(K, w[0], w[1], slice, treatment, lin1, delta0);
    V.step(y1, omega, false, src);
    V.update(lin2);
    V.step(y2, omega, false, src);
    // the same through the C-ABI, created about lin2 at once
    std::vector<int32_t> var(nb);
    std::vector<const double *> l(nb, nullptr), s(nb);
    std::vector<double *> d(nb);
    for (unsigned i = 0; i < nb; ++i) {
      var[i] = int32_t(slice.decompose(i)[1]);
      if (var[i] == 0) l[i] = lin2[i].data();
      s[i] = src[i].data();
      d[i] = y3[i].data();
    }
    stfem_stokes_vanka *h = nullptr;
    check(stfem_stokes_vanka_create_linearised_cip(K.handle(), int(nb), var.data(), w[0].data(), w[1].data(), STFEM_CONVECTION_JACOBIAN, l.data(), delta0, &h),
          "stfem_stokes_vanka_create_linearised_cip");
    const int cells = stfem_stokes_vanka_n_classes(h);
    const int rc = stfem_stokes_vanka_step(h, d.data(), omega, 0, s.data(), nullptr);
    stfem_stokes_vanka_destroy(h);
    check(rc, "stfem_stokes_vanka_step");
    // delta0 = 0 in the mirror: the constructor without the argument
    PreconditionVankaStokes<double> Vz(K, w[0], w[1], slice, treatment, lin2, 0.0), Vp(K, w[0], w[1], slice, treatment, lin2);
    Vz.step(yz, omega, false, src);
    Vp.step(yp, omega, false, src);
    // RelaxedVankaStokes with the trailing delta0 and a given damping, one sweep from zero: the step above
    const StokesMatrixFreeOperator<3, double> &Kc = K;
    auto spaces = std::make_shared<StokesSpaces>(mesh, K.handle());
    StokesSystem<3, double> system(A, spaces, K.handle(), slice);
    RelaxedVankaStokes<3> relaxed(Kc, system, w[0], w[1], slice, treatment, 1, omega, true, delta0);
    StokesBlockVector bl, bs, bd;
    for (StokesBlockVector *v : {&bl, &bs, &bd}) system.initialize_dof_vector(*v);
    for (unsigned b = 0; b < nb; ++b) {
      bl.blocks()[b].copy_from_host(lin2[b].copy_to_host());
      bs.blocks()[b].copy_from_host(src[b].copy_to_host());
    }
    relaxed.set_data(bl);
    relaxed.vmult(bd, bs);
    // refusals: the term without a nonlinear treatment, and a non-finite delta0 through the mirror
    try { RelaxedVankaStokes<3> bad(Kc, system, w[0], w[1], slice, NonlinearTreatment::None, 1, omega, true, delta0); } catch (const std::invalid_argument &) { ++thrown; }
    try { PreconditionVankaStokes<double> bad(K, w[0], w[1], slice, treatment, lin1, std::nan("")); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; }
    std::printf("blocks=%u cells=%d mirror_vs_capi=%.3e update_changed=%d term_changed=%d zero_vs_plain=%.3e relaxed_vs_step=%.3e exceptions=%d\n", nb, cells,
                max_difference(host(y2), host(y3)), max_difference(host(y1), host(y2)) > 1e-9 ? 1 : 0, max_difference(host(y2), host(yp)) > 1e-9 ? 1 : 0,
                max_difference(host(yz), host(yp)), max_difference(host(bd.blocks()), host(y2)), thrown);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "test_host_navier_cip_vanka: %s\n", e.what());
    return 1;
  }
}
