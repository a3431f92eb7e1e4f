// C++ caller of the Stokes mirror at velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), QGauss(4)): builds the operator and the
// cG(2) space-time system, applies vmult, Tvmult and vmult_slice_add to seeded vectors and writes inputs and results for the Python
// test; counts the refusals of the constructor (weak ids, delta0, a nonlinear treatment) itself.
//   test_host_stokes_q3 ncx ncy ncz dg_pressure viscosity out.bin
#include "stfem/stokes.h"

#include <cmath>
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
    mesh.dirichlet_mask = 0b111011;
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]);
    StokesMatrixFreeOperator<3, double> K(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg);
    const unsigned ns = 1, r = 2, nt = r;
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, r, 1.0 / 32, ns);
    BlockSlice slice(ns, 2, nt);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice);
    std::vector<StokesVector> x, y;
    A.initialize_dof_vector(x);
    A.initialize_dof_vector(y);
    FILE *f = std::fopen(argv[6], "wb");
    if (!f) return 3;
    const unsigned long long nb = x.size();
    std::fwrite(&nb, sizeof nb, 1, f);
    std::vector<std::vector<double>> hx(nb);
    for (unsigned b = 0; b < nb; ++b) {
      std::vector<double> &h = hx[b];
      h.resize(x[b].size());
      std::mt19937_64 rng(4321 + b);
      for (double &v : h) v = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
      x[b].copy_from_host(h);
      const unsigned long long n = h.size();
      std::fwrite(&n, sizeof n, 1, f);
      std::fwrite(h.data(), sizeof(double), n, f);
    }
    auto write = [&](const std::vector<StokesVector> &v) {
      for (unsigned b = 0; b < nb; ++b) {
        const auto h = v[b].copy_to_host();
        std::fwrite(h.data(), sizeof(double), h.size(), f);
      }
    };
    A.vmult(y, x);
    write(y);
    A.Tvmult(y, x);
    write(y);
    // the right-hand-side case: Gamma, Zeta are n x 1; onto destinations that hold the sources' values
    if (w[2].n() != 1 || w[3].n() != 1) return 5;
    SystemMatrixStokes<3, double> R(K, w[2], w[3], slice);
    for (unsigned b = 0; b < nb; ++b) y[b].copy_from_host(hx[b]);
    std::vector<StokesVector> pair;
    K.initialize_dof_vector(pair);
    pair[0].copy_from_host(hx[slice.index(0, 0, 1)]);
    pair[1].copy_from_host(hx[slice.index(0, 1, 1)]);
    R.vmult_slice_add(y, pair);
    write(y);
    std::fclose(f);
    // refusals: the C-ABI's STFEM_ERR_UNSUPPORTED with its reason
    int thrown = 0;
    auto refused = [&](const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED && std::strstr(e.what(), "velocity degree 2 only") != nullptr; };
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {0}); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {2}); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.5); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg, NonlinearTreatment::Explicit); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg, NonlinearTreatment::Implicit); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 4, nu); } catch (const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED; }
    try { A.vmult(x, x); } catch (const Error &e) { thrown += e.status == STFEM_ERR_ALIAS; }
    std::printf("m=%llu blocks=%llu exceptions=%d\n", A.m(), nb, thrown);
    return thrown == 7 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
