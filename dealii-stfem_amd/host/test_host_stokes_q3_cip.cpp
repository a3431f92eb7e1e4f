// C++ caller of the Stokes mirror at velocity degree 3 WITH the CIP interior-face term: the operator by descriptor (StokesSpace with
// delta0, through stfem_stokes_set_cip_space), its vmult on a seeded pair, the same after set_cip_weight (no nonlinear treatment: the
// weight stays the source, the bits stay), the operator without the term, and cip_add with a weight velocity of its own; writes inputs
// and results for the Python test and counts the refusals itself: the first constructor with delta0 != 0 at degree 3 and
// PreconditionVankaStokes with delta0 != 0 over a degree-3 operator.
//   test_host_stokes_q3_cip ncx ncy ncz dg_pressure viscosity delta0 out.bin
#include "stfem/stokes.h"
#include "stfem/stokes_solver.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 8) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    mesh.dirichlet_mask = 0b001010; // x+ and y+ strong
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]), delta0 = std::atof(argv[6]);
    StokesSpace<double> space{3, dg, nu};
    StokesMatrixFreeOperator<3, double> K0(mesh, space); // without the term
    space.delta0 = delta0;
    StokesMatrixFreeOperator<3, double> K(mesh, space);
    std::vector<StokesVector> x, y, w;
    K.initialize_dof_vector(x);
    K.initialize_dof_vector(y);
    K.initialize_dof_vector(w);
    FILE *f = std::fopen(argv[7], "wb");
    if (!f) return 3;
    auto seeded = [&](std::vector<StokesVector> &v, unsigned seed) {
      for (unsigned b = 0; b < 2; ++b) {
        std::vector<double> h(v[b].size());
        std::mt19937_64 rng(seed + b);
        for (double &e : h) e = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
        v[b].copy_from_host(h);
        const unsigned long long n = h.size();
        std::fwrite(&n, sizeof n, 1, f);
        std::fwrite(h.data(), sizeof(double), n, f);
      }
    };
    auto write = [&](const std::vector<StokesVector> &v, unsigned blocks) {
      for (unsigned b = 0; b < blocks; ++b) {
        const auto h = v[b].copy_to_host();
        std::fwrite(h.data(), sizeof(double), h.size(), f);
      }
    };
    seeded(x, 4321);
    seeded(w, 8765);
    K.vmult(y, x);
    write(y, 2);
    K.set_cip_weight(STFEM_CIP_WEIGHT_LINEARISATION);
    K.vmult(y, x);
    write(y, 2);
    K0.vmult(y, x);
    write(y, 2);
    K0.cip_add(y[0].data(), x[0].data(), w[0].data(), delta0); // onto the result without the term, the weight velocity w
    write(y, 1);
    std::fclose(f);
    int thrown = 0;
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, delta0); } catch (const Error &e) {
      thrown += e.status == STFEM_ERR_UNSUPPORTED && std::strstr(e.what(), "velocity degree 2 only") != nullptr;
    }
    try {
      FullMatrix<double> A(2, 2), B(2, 2);
      A(0, 0) = A(1, 1) = 1.0;
      std::vector<StokesVector> lin;
      K.initialize_dof_vector(lin);
      BlockSlice slice(1, 2, 1);
      PreconditionVankaStokes<double> V(K, A, B, slice, NonlinearTreatment::None, lin, delta0);
    } catch (const Error &e) {
      thrown += e.status == STFEM_ERR_UNSUPPORTED && std::strstr(e.what(), "velocity degree 3") != nullptr;
    }
    std::printf("m=%llu delta0=%g weight=%d exceptions=%d\n", K.m(), K.delta0(), K.cip_weight(), thrown);
    return thrown == 2 && K.cip_weight() == STFEM_CIP_WEIGHT_LINEARISATION ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
