// C++ caller of the partitioned Stokes / Navier-Stokes system (host/stfem/stokes_solver.h: StokesSpaces::set_partition, the comm
// branches of StokesSystem::vmult / form, the reducing inner product and Gram-Schmidt step), in the manner of test_host_sharded.cpp:
// one GPU holds one rank of a communicator, so this is the one-rank communicator with the rank itself as lower and upper neighbour.
// The add-exchange then returns every interface partial to its sender (both interface planes of every velocity component and of the
// FE_Q(1) pressure double; FE_DGP(1) pressure DoFs are cell-local and take no part), inner products count the top plane out.  The
// pytest driver rebuilds exactly that from the CPU oracle.
//   test_host_stokes_sharded ncx ncy ncz dg_pressure out.bin
// A box with both z faces out of the mask, cG(2), one step, two variables, Newton treatment (vmult: jacobian, form: the weak form,
// both about a second vector).  File: n_blocks, block sizes, then x, lin, vmult(x), form(x), the Gram-Schmidt result of vmult(x)
// against {x, lin}; then (x, vmult(x)), the two Gram-Schmidt coefficients and the norm it returns.
#include "stfem/stokes_solver.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace stfem;

static void dump(FILE *f, const StokesBlockVector &v)
{
  for (const auto &b : v.blocks()) {
    const auto h = b.copy_to_host();
    std::fwrite(h.data(), sizeof(double), h.size(), f);
  }
}

int main(int argc, char **argv)
{
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s ncx ncy ncz dg_pressure out.bin\n", argv[0]);
    return 2;
  }
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.upper[1] = 0.75;
    mesh.upper[2] = 1.25;
    mesh.dirichlet_mask = 63 & ~(16 | 32); // both z faces are partition interfaces
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = 0.3;
    const NonlinearTreatment treatment = NonlinearTreatment::Implicit;
    auto comm = std::make_shared<Communicator>(Communicator::unique_id(), 0, 1, mesh.device);
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg, treatment);
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, 2, 1.0 / 32, 1);
    BlockSlice slice(1, 2, 2);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
    auto spaces = std::make_shared<StokesSpaces>(mesh, K.handle());
    spaces->set_partition(comm, 0, 0);
    StokesSystem<3, double> system(A, spaces, K.handle(), slice);
    StokesBlockVector x, lin, y, form, gs;
    for (auto *v : {&x, &lin, &y, &form, &gs}) system.initialize_dof_vector(*v);
    FILE *f = std::fopen(argv[5], "wb");
    if (!f) return 3;
    const unsigned long long nb = x.n_blocks();
    std::fwrite(&nb, sizeof nb, 1, f);
    for (unsigned b = 0; b < nb; ++b) {
      const unsigned long long n = x.blocks()[b].size();
      std::fwrite(&n, sizeof n, 1, f);
    }
    for (StokesBlockVector *v : {&x, &lin})
      for (unsigned b = 0; b < nb; ++b) {
        std::vector<double> h(v->blocks()[b].size());
        std::mt19937_64 rng((v == &x ? 4321 : 8765) + b);
        for (double &e : h) e = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
        v->blocks()[b].copy_from_host(h);
      }
    system.set_data(lin);
    system.vmult(y, x);
    system.form(form, x);
    const double xy = dot(x, y);
    axpby(1.0, y, 0.0, gs);
    const std::vector<StokesBlockVector *> basis_ptr = {&x, &lin};
    std::vector<StokesBlockVector> basis(2);
    for (unsigned i = 0; i < 2; ++i) {
      system.initialize_dof_vector(basis[i]);
      axpby(1.0, *basis_ptr[i], 0.0, basis[i]);
    }
    double h[2] = {0.0, 0.0};
    const double norm_after = orthogonalize(basis, 2, gs, h);
    for (const StokesBlockVector *v : {&x, &lin, &y, &form, &gs}) dump(f, *v);
    const double scalars[4] = {xy, h[0], h[1], norm_after};
    std::fwrite(scalars, sizeof(double), 4, f);
    std::fclose(f);
    std::printf("ranks=%d blocks=%llu carrier=%d\n", comm->size(), nb, int(spaces->carrier));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
