// C++ caller of the Stokes mirror at velocity degree 3 with a nonlinear treatment (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), QGauss(4)): the
// constructor by descriptor (StokesSpace), set_data, vmult and form of the operator and the cG(2) SystemMatrixStokes::vmult over it, on
// seeded vectors; writes inputs and results for the Python test.  Counts itself: the first constructor still throws for a treatment at
// degree 3, vmult without set_data throws, and the alias refusal.
//   test_host_navier_q3 ncx ncy ncz dg_pressure viscosity treatment(1 Implicit, 2 Explicit) lin_scale out.bin
#include "stfem/stokes.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 9) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.distort_random(0.1, 99);
    mesh.dirichlet_mask = 0b111011;
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]);
    const NonlinearTreatment treatment = std::atoi(argv[6]) == 1 ? NonlinearTreatment::Implicit : NonlinearTreatment::Explicit;
    const double lin_scale = std::atof(argv[7]);
    StokesSpace<double> space;
    space.velocity_degree = 3;
    space.dg_pressure = dg;
    space.viscosity = nu;
    space.nonlinear_treatment = treatment;
    StokesMatrixFreeOperator<3, double> K(mesh, space);
    if (!K.space_entries() || K.velocity_degree() != 3) return 6;
    const unsigned ns = 1, r = 2, nt = r;
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, r, 1.0 / 32, ns);
    BlockSlice slice(ns, 2, nt);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
    std::vector<StokesVector> x, y, lin;
    A.initialize_dof_vector(x);
    A.initialize_dof_vector(y);
    A.initialize_dof_vector(lin);
    FILE *f = std::fopen(argv[8], "wb");
    if (!f) return 3;
    const unsigned long long nb = x.size();
    std::fwrite(&nb, sizeof nb, 1, f);
    // the sources, then the linearisation blocks (scaled)
    for (unsigned set = 0; set < 2; ++set)
      for (unsigned b = 0; b < nb; ++b) {
        StokesVector &v = set == 0 ? x[b] : lin[b];
        std::vector<double> h(v.size());
        std::mt19937_64 rng(4321 + 100 * set + b);
        for (double &e : h) e = (set == 0 ? 1.0 : lin_scale) * (double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0);
        v.copy_from_host(h);
        const unsigned long long n = h.size();
        std::fwrite(&n, sizeof n, 1, f);
        std::fwrite(h.data(), sizeof(double), n, f);
      }
    auto write = [&](const StokesVector &v) {
      const auto h = v.copy_to_host();
      std::fwrite(h.data(), sizeof(double), h.size(), f);
    };
    // the operator itself on the pair of time dof 0, linearised about the velocity block of time dof 1
    const unsigned u0 = slice.index(0, 0, 0), p0 = slice.index(0, 1, 0), u1 = slice.index(0, 0, 1);
    std::vector<StokesVector> src, dst;
    K.initialize_dof_vector(src);
    K.initialize_dof_vector(dst);
    src[0].copy_from_host(x[u0].copy_to_host());
    src[1].copy_from_host(x[p0].copy_to_host());
    int thrown = 0;
    try { K.vmult(dst, src); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; } // no linearisation set
    K.set_data(lin[u1]);
    K.vmult(dst, src);
    write(dst[0]); write(dst[1]);
    K.form(dst, src);
    write(dst[0]); write(dst[1]);
    // the space-time system: time dof d linearised about its own block of lin
    A.set_data(lin);
    A.vmult(y, x);
    for (unsigned b = 0; b < nb; ++b) write(y[b]);
    std::fclose(f);
    // the first constructor still refuses a treatment at degree 3
    auto refused = [&](const Error &e) { thrown += e.status == STFEM_ERR_UNSUPPORTED && std::strstr(e.what(), "velocity degree 2 only") != nullptr; };
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg, NonlinearTreatment::Explicit); } catch (const Error &e) { refused(e); }
    try { StokesMatrixFreeOperator<3, double> W(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg, NonlinearTreatment::Implicit); } catch (const Error &e) { refused(e); }
    try { A.vmult(x, x); } catch (const Error &e) { thrown += e.status == STFEM_ERR_ALIAS; }
    std::printf("m=%llu blocks=%llu exceptions=%d\n", A.m(), nb, thrown);
    return thrown == 4 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
