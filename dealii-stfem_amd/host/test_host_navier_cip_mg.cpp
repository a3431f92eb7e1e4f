// C++ caller of the multigrid of the linearised Stokes operator WITH the CIP term on every level (GMGStokes::AdditionalData::delta0,
// host/stfem/stokes_solver.h: level operators with set_cip(delta0, STFEM_CIP_WEIGHT_LINEARISATION), level smoothers with the term in
// their blocks): one V-cycle about a seeded linearisation applied to a seeded vector, the same cycle with delta0 = 0, a second set_data
// against a freshly built hierarchy, and the refusal without a treatment - written out for tests/test_gpu_navier_cip_mg.py, which
// compares with the numpy V-cycle of oracle/stmg_oracle.py on the dense levels of tests/navier_cip_mg_reference.py.
//   test_host_navier_cip_mg nx ny nz levels type r viscosity smoothing_degree omega variable treatment dg_pressure weak_mask delta0 out.bin
// The arguments of test_host_navier_mg (same seeds) and delta0; omega != 0: given, no estimate enters.  The file is a sequence of
// arrays, each a 64-bit length followed by the doubles:
//   lin1[nb], x[nb], y1[nb] = cycle about lin1 with delta0, y0[nb] = the cycle with AdditionalData::delta0 = 0;
//   y2[nb] = cycle after a second set_data(lin2), y2f[nb] = cycle of a fresh hierarchy about lin2, both with delta0.
#include "stfem/stokes_solver.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

using namespace stfem;

namespace {
void write_array(FILE *f, const std::vector<double> &h)
{
  const unsigned long long n = h.size();
  std::fwrite(&n, sizeof n, 1, f);
  std::fwrite(h.data(), sizeof(double), n, f);
}
void write_blocks(FILE *f, const StokesBlockVector &v)
{
  for (unsigned b = 0; b < v.n_blocks(); ++b) write_array(f, v.blocks()[b].copy_to_host());
}
void fill(StokesBlockVector &v, unsigned seed, double amplitude)
{
  for (unsigned b = 0; b < v.n_blocks(); ++b) {
    std::vector<double> h(v.blocks()[b].size());
    std::mt19937_64 rng(seed + b);
    for (double &e : h) e = amplitude * (double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0);
    v.blocks()[b].copy_from_host(h);
  }
}
} // namespace

int main(int argc, char **argv)
{
  if (argc != 16) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    const unsigned levels = unsigned(std::atoi(argv[4]));
    const TimeStepType type = std::atoi(argv[5]) == 0 ? TimeStepType::CGP : TimeStepType::DG;
    const unsigned r = unsigned(std::atoi(argv[6]));
    const double nu = std::atof(argv[7]);
    GMGStokes<3>::AdditionalData ad;
    ad.smoothing_degree = unsigned(std::atoi(argv[8]));
    ad.relaxation = std::atof(argv[9]);
    ad.variable = std::atoi(argv[10]) != 0;
    const NonlinearTreatment treatment = std::atoi(argv[11]) == 1 ? NonlinearTreatment::Implicit : NonlinearTreatment::Explicit;
    const bool dg = std::atoi(argv[12]) != 0;
    const int weak_mask = std::atoi(argv[13]);
    ad.delta0 = std::atof(argv[14]);
    std::set<boundary_id> weak;
    for (unsigned f = 0; f < 6; ++f)
      if (weak_mask >> f & 1) weak.insert(f);
    mesh.dirichlet_mask = 63 & ~weak_mask;
    const unsigned nt = type == TimeStepType::CGP ? r : r + 1;
    const BlockSlice slice(1, 2, nt);
    const auto w = get_fe_time_weights_stokes<double>(type, r, 1.0 / 16, 1);
    auto make = [&](const GMGStokes<3>::AdditionalData &data, NonlinearTreatment t) {
      return std::make_unique<GMGStokes<3>>(mesh, levels, nu, w[0], w[1], slice, data, weak, dg, t);
    };

    // the refusals: the term on the levels without a nonlinear treatment, in both constructors
    unsigned refusals = 0;
    try {
      make(ad, NonlinearTreatment::None);
    } catch (const std::invalid_argument &) {
      ++refusals;
    }
    try {
      GMGStokes<3> g(mesh, std::vector<MGType>{MGType::h}, std::vector<unsigned>{r}, type, 1.0 / 16, 1, nu, ad, weak, dg);
    } catch (const std::invalid_argument &) {
      ++refusals;
    }

    auto gmg = make(ad, treatment);
    StokesBlockVector lin1, lin2, x, y;
    for (StokesBlockVector *v : {&lin1, &lin2, &x, &y}) gmg->finest_system().initialize_dof_vector(*v);
    fill(lin1, 4201, 1.0);
    fill(lin2, 5303, 2.0);
    fill(x, 977, 1.0);
    FILE *f = std::fopen(argv[15], "wb");
    if (!f) return 3;
    write_blocks(f, lin1);
    write_blocks(f, x);
    gmg->set_data(lin1);
    gmg->vmult(y, x);
    write_blocks(f, y);
    {
      GMGStokes<3>::AdditionalData without = ad;
      without.delta0 = 0.0;
      auto plain = make(without, treatment);
      plain->set_data(lin1);
      plain->vmult(y, x);
      write_blocks(f, y);
    }
    auto again = make(ad, treatment), fresh = make(ad, treatment);
    again->set_data(lin1);
    again->vmult(y, x);
    again->set_data(lin2);
    again->vmult(y, x);
    write_blocks(f, y);
    fresh->set_data(lin2);
    fresh->vmult(y, x);
    write_blocks(f, y);
    std::fclose(f);
    std::printf("blocks=%u refusals=%u\n", x.n_blocks(), refusals);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
