// C++ caller of the Stokes Vanka mirror at velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)): builds the operator on a box, the cG(2)
// weights and PreconditionVankaStokes over it - which goes through stfem_stokes_vanka_create_space -, applies the smoother to the blocks
// read from a file and writes the result for the Python test; then the relaxation step, the repeat and the alias refusal, counted here.
//   test_host_stokes_q3_vanka ncx ncy ncz dg_pressure viscosity tau in.bin out.bin
// in.bin: uint64 number of blocks, then per block uint64 length and the doubles; out.bin: the result blocks, doubles only.
#include "stfem/stokes.h"

#include <cstdio>
#include <cstdlib>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 9) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.dirichlet_mask = 63;
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]), tau = std::atof(argv[6]);
    StokesMatrixFreeOperator<3, double> K(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg);
    const unsigned ns = 1, r = 2, nt = r;
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, r, tau, ns);
    BlockSlice slice(ns, 2, nt);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice);
    PreconditionVankaStokes<double> V(K, w[0], w[1], slice);
    std::vector<StokesVector> x, y;
    A.initialize_dof_vector(x);
    A.initialize_dof_vector(y);
    FILE *f = std::fopen(argv[7], "rb");
    if (!f) return 3;
    unsigned long long nb = 0;
    if (std::fread(&nb, sizeof nb, 1, f) != 1 || nb != x.size()) return 5;
    for (unsigned b = 0; b < nb; ++b) {
      unsigned long long n = 0;
      if (std::fread(&n, sizeof n, 1, f) != 1 || n != x[b].size()) return 5;
      std::vector<double> h(n);
      if (std::fread(h.data(), sizeof(double), n, f) != n) return 5;
      x[b].copy_from_host(h);
    }
    std::fclose(f);
    V.vmult(y, x);
    std::vector<std::vector<double>> first(nb);
    f = std::fopen(argv[8], "wb");
    if (!f) return 3;
    for (unsigned b = 0; b < nb; ++b) {
      first[b] = y[b].copy_to_host();
      std::fwrite(first[b].data(), sizeof(double), first[b].size(), f);
    }
    std::fclose(f);
    // a second apply gives the same bits; step with accumulate adds omega times them
    int ok = 0;
    V.vmult(y, x);
    bool same = true;
    for (unsigned b = 0; b < nb; ++b) same = same && y[b].copy_to_host() == first[b];
    ok += same;
    V.step(y, 0.5, true, x);
    bool stepped = true;
    for (unsigned b = 0; b < nb; ++b) {
      const auto h = y[b].copy_to_host();
      for (size_t i = 0; i < h.size(); ++i) stepped = stepped && h[i] == first[b][i] + 0.5 * first[b][i];
    }
    ok += stepped;
    try { V.vmult(x, x); } catch (const Error &e) { ok += e.status == STFEM_ERR_ALIAS; }
    std::printf("blocks=%llu cells=%d checks=%d\n", nb, V.n_classes(), ok);
    return ok == 3 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
