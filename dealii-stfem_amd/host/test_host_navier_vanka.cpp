// C++ caller of the smoother of the linearised operator (PreconditionVankaStokes with a NonlinearTreatment and a linearisation
// vector, its update and one relaxation step) on a perturbed mesh, against the values the same calls give through the C-ABI
// (stfem_stokes_vanka_create_linearised / _step).
//   test_host_navier_vanka ncx ncy ncz type r nsteps viscosity
// Prints one line: blocks=<n> cells=<n> mirror_vs_capi=<max |difference|> update_changed=<0|1> none_vs_create=<max |difference|>
// exceptions=<count of the refusals that threw as they should>
#include "stfem/stokes.h"

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
  if (argc != 8) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    mesh.dirichlet_mask = 63;
    const TimeStepType type = std::atoi(argv[4]) == 0 ? TimeStepType::CGP : TimeStepType::DG;
    const unsigned r = unsigned(std::atoi(argv[5])), ns = unsigned(std::atoi(argv[6]));
    const double nu = std::atof(argv[7]);
    const auto w = get_fe_time_weights_stokes<double>(type, r, 1.0 / 32, ns);
    const unsigned nt = type == TimeStepType::CGP ? r : r + 1;
    BlockSlice slice(ns, 2, nt);
    const NonlinearTreatment treatment = NonlinearTreatment::Implicit;
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, false, treatment);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
    std::vector<StokesVector> src, lin1, lin2, y1, y2, y3, yn, yc;
    for (auto *v : {&src, &lin1, &lin2, &y1, &y2, &y3, &yn, &yc}) A.initialize_dof_vector(*v);
    const unsigned nb = unsigned(src.size());
    for (unsigned b = 0; b < nb; ++b) {
      src[b].copy_from_host(seeded(src[b].size(), 4321 + b));
      lin1[b].copy_from_host(seeded(src[b].size(), 8765 + b));
      lin2[b].copy_from_host(seeded(src[b].size(), 1357 + b));
    }
    const double omega = 0.7;
    int thrown = 0;
    // the mirror: created about lin1, updated to lin2, one step
    PreconditionVankaStokes<double> V(K, w[0], w[1], slice, treatment, lin1);
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
    check(stfem_stokes_vanka_create_linearised(K.handle(), int(nb), var.data(), w[0].data(), w[1].data(), STFEM_CONVECTION_JACOBIAN, l.data(), &h),
          "stfem_stokes_vanka_create_linearised");
    const int cells = stfem_stokes_vanka_n_classes(h);
    const int rc = stfem_stokes_vanka_step(h, d.data(), omega, 0, s.data(), nullptr);
    stfem_stokes_vanka_destroy(h);
    check(rc, "stfem_stokes_vanka_step");
    // NonlinearTreatment::None: the plain Stokes blocks, what the first constructor builds on this general mesh
    PreconditionVankaStokes<double> Vn(K, w[0], w[1], slice, NonlinearTreatment::None, lin1), Vc(K, w[0], w[1], slice);
    Vn.vmult(yn, src);
    Vc.vmult(yc, src);
    // refusals
    std::vector<StokesVector> too_few;
    too_few.emplace_back(K.handle(), 0);
    try { V.update(too_few); } catch (const Error &e) { thrown += e.status == STFEM_ERR_SHAPE_MISMATCH; }
    try { PreconditionVankaStokes<double> bad(K, w[0], w[1], slice, treatment, too_few); } catch (const Error &e) { thrown += e.status == STFEM_ERR_SHAPE_MISMATCH; }
    try { V.vmult(src, src); } catch (const Error &e) { thrown += e.status == STFEM_ERR_ALIAS; }
    stfem_stokes_vanka *none = reinterpret_cast<stfem_stokes_vanka *>(1);
    thrown += stfem_stokes_vanka_create_linearised(K.handle(), int(nb), var.data(), w[0].data(), w[1].data(), 3, l.data(), &none) == STFEM_ERR_INVALID_ARGUMENT &&
              none == nullptr;
    std::printf("blocks=%u cells=%d mirror_vs_capi=%.3e update_changed=%d none_vs_create=%.3e exceptions=%d\n", nb, cells,
                max_difference(host(y2), host(y3)), max_difference(host(y1), host(y2)) > 1e-9 ? 1 : 0, max_difference(host(yn), host(yc)), thrown);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "test_host_navier_vanka: %s\n", e.what());
    return 1;
  }
}
