// C++ caller of the Stokes Vanka mirror of the LINEARISED operator at velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)): builds the
// operator on a box, the cG(2) weights and PreconditionVankaStokes over it with a NonlinearTreatment and a linearisation vector - which
// goes through stfem_stokes_vanka_create_linearised_space -, applies the smoother to the blocks read from a file and writes the result
// for the Python test; then update against a fresh construction, the way back, and the refusal of delta0 != 0, counted here.
//   test_host_navier_q3_vanka ncx ncy ncz dg_pressure viscosity tau treatment in.bin lin.bin out.bin
// treatment: 1 Explicit (form), 2 Implicit (jacobian).  in.bin / lin.bin: uint64 number of blocks, then per block uint64 length and the
// doubles (the pressure blocks of lin.bin are not read by the smoother); out.bin: the result blocks, doubles only.
#include "stfem/stokes.h"

#include <cstdio>
#include <cstdlib>

using namespace stfem;

static bool read_blocks(const char *path, std::vector<StokesVector> &x, std::vector<std::vector<double>> *host = nullptr)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  unsigned long long nb = 0;
  bool ok = std::fread(&nb, sizeof nb, 1, f) == 1 && nb == x.size();
  for (unsigned b = 0; ok && b < nb; ++b) {
    unsigned long long n = 0;
    ok = std::fread(&n, sizeof n, 1, f) == 1 && n == x[b].size();
    if (!ok) break;
    std::vector<double> h(n);
    ok = std::fread(h.data(), sizeof(double), n, f) == n;
    if (ok) x[b].copy_from_host(h);
    if (ok && host) host->push_back(h);
  }
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv)
{
  if (argc != 11) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.dirichlet_mask = 63;
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]), tau = std::atof(argv[6]);
    const NonlinearTreatment treatment = std::atoi(argv[7]) == 1 ? NonlinearTreatment::Explicit : NonlinearTreatment::Implicit;
    StokesMatrixFreeOperator<3, double> K(mesh, 3, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg);
    const unsigned ns = 1, r = 2, nt = r;
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, r, tau, ns);
    BlockSlice slice(ns, 2, nt);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice);
    std::vector<StokesVector> x, y, lin, other;
    A.initialize_dof_vector(x);
    A.initialize_dof_vector(y);
    A.initialize_dof_vector(lin);
    A.initialize_dof_vector(other);
    std::vector<std::vector<double>> lin_host;
    if (!read_blocks(argv[8], x) || !read_blocks(argv[9], lin, &lin_host)) return 5;
    const unsigned nb = unsigned(x.size());
    for (unsigned b = 0; b < nb; ++b) { // other states: the given ones reversed and halved
      std::vector<double> h(lin_host[b].rbegin(), lin_host[b].rend());
      for (double &v : h) v *= 0.5;
      other[b].copy_from_host(h);
    }
    PreconditionVankaStokes<double> V(K, w[0], w[1], slice, treatment, lin);
    V.vmult(y, x);
    std::vector<std::vector<double>> first(nb);
    FILE *f = std::fopen(argv[10], "wb");
    if (!f) return 3;
    for (unsigned b = 0; b < nb; ++b) {
      first[b] = y[b].copy_to_host();
      std::fwrite(first[b].data(), sizeof(double), first[b].size(), f);
    }
    std::fclose(f);
    auto apply = [&](const PreconditionVankaStokes<double> &P) {
      P.vmult(y, x);
      std::vector<std::vector<double>> out(nb);
      for (unsigned b = 0; b < nb; ++b) out[b] = y[b].copy_to_host();
      return out;
    };
    int ok = 0;
    // update reproduces a fresh construction about the other states, which differ; and the way back gives the first bits again
    PreconditionVankaStokes<double> W(K, w[0], w[1], slice, treatment, other);
    const auto fresh = apply(W);
    ok += fresh != first;
    V.update(other);
    ok += apply(V) == fresh;
    V.update(lin);
    ok += apply(V) == first;
    try {
      PreconditionVankaStokes<double> C(K, w[0], w[1], slice, treatment, lin, 0.1);
    } catch (const Error &e) {
      ok += e.status == STFEM_ERR_UNSUPPORTED;
    }
    std::printf("blocks=%u cells=%d checks=%d\n", nb, V.n_classes(), ok);
    return ok == 4 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
