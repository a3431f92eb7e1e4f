// C++ caller of the Stokes mirror at velocity degree 3 WITH weak (Nitsche) faces: the operator by descriptor
// (StokesSpace with weak_boundary_ids, through stfem_stokes_set_weak_boundaries_space), its vmult on a seeded pair and
// StokesNitscheMatrixFreeOperator::vmult for the Dirichlet data g(x) = (y z, x + z^2, x y - 1); writes inputs and results for the
// Python test and counts the refusals itself: the first constructor with weak ids at degree 3, a nonlinear treatment with weak ids.
//   test_host_stokes_q3_faces ncx ncy ncz dg_pressure viscosity out.bin
#include "stfem/stokes.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 7) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    mesh.dirichlet_mask = 0b001010; // x+ and y+ strong; x-, y-, z+ weak, z- natural
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]);
    const StokesSpace<double> space{3, dg, nu, NonlinearTreatment::None, {0, 2, 5}, {}, 15.0, 7.0};
    StokesMatrixFreeOperator<3, double> K(mesh, space);
    std::vector<StokesVector> x, y;
    K.initialize_dof_vector(x);
    K.initialize_dof_vector(y);
    FILE *f = std::fopen(argv[6], "wb");
    if (!f) return 3;
    for (unsigned b = 0; b < 2; ++b) {
      std::vector<double> h(x[b].size());
      std::mt19937_64 rng(4321 + b);
      for (double &v : h) v = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
      x[b].copy_from_host(h);
      const unsigned long long n = h.size();
      std::fwrite(&n, sizeof n, 1, f);
      std::fwrite(h.data(), sizeof(double), n, f);
    }
    auto write = [&](const std::vector<StokesVector> &v) {
      for (unsigned b = 0; b < 2; ++b) {
        const auto h = v[b].copy_to_host();
        std::fwrite(h.data(), sizeof(double), h.size(), f);
      }
    };
    K.vmult(y, x);
    write(y);
    StokesNitscheMatrixFreeOperator<3, double> N(K);
    N.set_dirichlet_functions([](const std::array<double, 3> &p) { return std::array<double, 3>{{p[1] * p[2], p[0] + p[2] * p[2], p[0] * p[1] - 1.0}}; });
    std::vector<StokesVector> rhs;
    N.initialize_dof_vector(rhs); // zeroed; vmult adds
    N.vmult(rhs);
    write(rhs);
    std::fclose(f);
    int thrown = 0;
    auto refused = [&](const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED && std::strstr(e.what(), "velocity degree 2 only") != nullptr; };
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {0, 2, 5}); } catch (const Error &e) { refused(e); }
    try {
      StokesSpace<double> s = space;
      s.nonlinear_treatment = NonlinearTreatment::Implicit;
      StokesMatrixFreeOperator<3, double> W(mesh, s);
    } catch (const Error &e) { refused(e); }
    std::printf("m=%llu exceptions=%d\n", K.m(), thrown);
    return thrown == 2 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
