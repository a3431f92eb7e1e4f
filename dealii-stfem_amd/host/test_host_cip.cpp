// C++ caller of the CIP interior-face term through the Stokes mirror (in the style of tests/tp_03stokes.cc, which hands delta0 to every
// operator it creates): builds the operator with the mirror constructor and delta0, the space-time system and the NavierStokesOperator
// over it, and writes inputs and results for the Python test.
//   test_host_cip ncx ncy ncz type r nsteps viscosity delta0 out.bin
// File: n_blocks; per block its length and the source x; the linearisation vector; the right-hand side; then for Explicit and for
// Implicit, with the source weight (the constructor's) and then with the linearisation weight: NavierStokesOperator::residual(x) and
// ::vmult(x); then, of the Implicit spatial operator with the linearisation of time dof (0, 0) and the linearisation weight: form and
// vmult of the first (velocity, pressure) pair.
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
static void dump(FILE *f, const std::vector<StokesVector> &v)
{
  for (const auto &b : v) {
    const auto h = b.copy_to_host();
    std::fwrite(h.data(), sizeof(double), h.size(), f);
  }
}

int main(int argc, char **argv)
{
  if (argc != 10) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    const TimeStepType type = std::atoi(argv[4]) == 0 ? TimeStepType::CGP : TimeStepType::DG;
    const unsigned r = unsigned(std::atoi(argv[5])), ns = unsigned(std::atoi(argv[6]));
    const double nu = std::atof(argv[7]), delta0 = std::atof(argv[8]);
    mesh.dirichlet_mask = 63;
    const auto w = get_fe_time_weights_stokes<double>(type, r, 1.0 / 32, ns);
    const unsigned nt = type == TimeStepType::CGP ? r : r + 1;
    BlockSlice slice(ns, 2, nt);
    FILE *f = std::fopen(argv[9], "wb");
    if (!f) return 3;
    int thrown = 0;
    for (const NonlinearTreatment treatment : {NonlinearTreatment::Explicit, NonlinearTreatment::Implicit}) {
      StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, delta0, /*delta1, stored and never read:*/ 7.0, false, treatment);
      if (K.delta0() != delta0 || K.cip_weight() != STFEM_CIP_WEIGHT_SOURCE) return 5;
      SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
      NavierStokesOperator<3, double> navier;
      std::vector<StokesVector> x, lin, rhs, res, y;
      navier.init(A, rhs);
      for (auto *v : {&x, &lin, &rhs, &res, &y}) navier.initialize_dof_vector(*v);
      const unsigned long long nb = x.size();
      if (treatment == NonlinearTreatment::Explicit) std::fwrite(&nb, sizeof nb, 1, f);
      for (unsigned b = 0; b < nb; ++b) {
        const auto h = seeded(x[b].size(), 4321 + b);
        x[b].copy_from_host(h);
        lin[b].copy_from_host(seeded(x[b].size(), 8765 + b));
        rhs[b].copy_from_host(seeded(x[b].size(), 1357 + b));
        if (treatment == NonlinearTreatment::Explicit) {
          const unsigned long long n = h.size();
          std::fwrite(&n, sizeof n, 1, f);
          std::fwrite(h.data(), sizeof(double), n, f);
        }
      }
      if (treatment == NonlinearTreatment::Explicit) { dump(f, lin); dump(f, rhs); }
      navier.set_data(lin);
      for (const int weight : {STFEM_CIP_WEIGHT_SOURCE, STFEM_CIP_WEIGHT_LINEARISATION}) {
        navier.set_cip_weight(weight);
        if (K.cip_weight() != weight) return 5;
        navier.residual(res, x);
        dump(f, res);
        navier.vmult(y, x);
        dump(f, y);
      }
      try { K.set_cip_weight(2); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; } // no such weight
      if (treatment == NonlinearTreatment::Implicit) { // the spatial operator by itself, linearised about time dof (0, 0)
        std::vector<StokesVector> xs, ys;
        K.initialize_dof_vector(xs);
        K.initialize_dof_vector(ys);
        xs[0].copy_from_host(x[slice.index(0, 0, 0)].copy_to_host());
        xs[1].copy_from_host(x[slice.index(0, 1, 0)].copy_to_host());
        K.set_data(lin[slice.index(0, 0, 0)]);
        K.form(ys, xs);
        dump(f, ys);
        K.vmult(ys, xs);
        dump(f, ys);
      }
    }
    std::fclose(f);
    // the outflow penalty is still refused with a nonlinear treatment, with and without the CIP term
    try {
      StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.5, delta0, 0.0, false, NonlinearTreatment::Implicit);
    } catch (const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED; }
    try {
      StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.5, 0.0, 0.0, false, NonlinearTreatment::Explicit);
    } catch (const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED; }
    { // a non-finite delta0 is refused by the library
      try {
        StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, std::nan(""));
      } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; }
    }
    std::printf("exceptions=%d\n", thrown);
    return thrown == 5 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
