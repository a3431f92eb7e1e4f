// C++ caller of the partitioned Stokes system WITH the CIP term (host/stfem/stokes_solver.h: StokesSpaces::set_partition tells the
// operator of its z neighbours, StokesSystem::vmult packs, exchanges and binds the ghost planes of its velocity sources), in the
// manner of test_host_stokes_sharded.cpp: the one-rank communicator with the rank itself as lower and upper neighbour.  The slab then
// is the middle one of a stack of copies of itself: what it sends up arrives as its own lower ghost planes, and the add-exchange
// returns every interface partial to its sender.  For the stack to be a mesh with one field on it the top DoF plane of every
// velocity source repeats the bottom one.  The pytest driver rebuilds the result from the numpy term.
//   test_host_stokes_cip_sharded ncx ncy ncz dg_pressure delta0 out.bin
// A box with both z faces out of the mask, cG(2), one step, two variables, no nonlinear treatment (the weight velocity is the source).
// File: n_blocks, block sizes, then x and vmult(x).
#include "stfem/stokes_solver.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s ncx ncy ncz dg_pressure delta0 out.bin\n", argv[0]);
    return 2;
  }
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.upper[1] = 0.75;
    mesh.upper[2] = 1.25;
    mesh.dirichlet_mask = 63 & ~(16 | 32); // both z faces are partition interfaces
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = 0.3, delta0 = std::atof(argv[5]);
    auto comm = std::make_shared<Communicator>(Communicator::unique_id(), 0, 1, mesh.device);
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, delta0, 0.0, dg);
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, 2, 1.0 / 32, 1);
    BlockSlice slice(1, 2, 2);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice);
    auto spaces = std::make_shared<StokesSpaces>(mesh, K.handle());
    spaces->set_partition(comm, 0, 0);
    StokesSystem<3, double> system(A, spaces, K.handle(), slice);
    StokesBlockVector x, y;
    system.initialize_dof_vector(x);
    system.initialize_dof_vector(y);
    FILE *f = std::fopen(argv[6], "wb");
    if (!f) return 3;
    const unsigned long long nb = x.n_blocks();
    std::fwrite(&nb, sizeof nb, 1, f);
    for (unsigned b = 0; b < nb; ++b) {
      const unsigned long long n = x.blocks()[b].size();
      std::fwrite(&n, sizeof n, 1, f);
    }
    const size_t plane = size_t(2 * mesh.ncell[0] + 1) * (2 * mesh.ncell[1] + 1), ndz = 2 * mesh.ncell[2] + 1;
    for (unsigned b = 0; b < nb; ++b) {
      std::vector<double> h(x.blocks()[b].size());
      std::mt19937_64 rng(4321 + b);
      for (double &e : h) e = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
      if (slice.decompose(b)[1] == 0) // velocity: [component][z plane][plane], the top plane repeats the bottom one
        for (size_t comp = 0; comp < 3; ++comp)
          for (size_t i = 0; i < plane; ++i) h[(comp * ndz + ndz - 1) * plane + i] = h[comp * ndz * plane + i];
      x.blocks()[b].copy_from_host(h);
    }
    system.vmult(y, x);
    system.vmult(y, x); // (a second apply: the buffers and bindings of the first are reused)
    for (const StokesBlockVector *v : {&x, &y})
      for (const auto &blk : v->blocks()) {
        const auto h = blk.copy_to_host();
        std::fwrite(h.data(), sizeof(double), h.size(), f);
      }
    std::fclose(f);
    // the smoother of such a slab: per-cell blocks set up on the slab plus one ghost cell layer on either side (the middle of the stack
    // again), applied on the slab.  Its numbers are held by tests/test_gpu_stokes_vanka_slabs.py through the same entry point; here the
    // mirror's constructor, update and apply run once.
    Mesh ext = mesh;
    ext.ncell[2] = mesh.ncell[2] + 2;
    const double hz = (mesh.upper[2] - mesh.lower[2]) / mesh.ncell[2];
    ext.lower[2] = mesh.lower[2] - hz;
    ext.upper[2] = mesh.upper[2] + hz;
    StokesMatrixFreeOperator<3, double> K_ext(ext, 2, nu, {}, {}, 20, 10, 0.0, delta0, 0.0, dg);
    SystemMatrixStokes<3, double> A_ext(K_ext, w[0], w[1], slice);
    std::vector<StokesVector> lin_ext;
    A_ext.initialize_dof_vector(lin_ext);
    for (auto &blk : lin_ext) {
      std::vector<double> h(blk.size());
      std::mt19937_64 rng(99);
      for (double &e : h) e = double(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
      blk.copy_from_host(h);
    }
    PreconditionVankaStokes<double> vanka(K, K_ext, w[0], w[1], slice, NonlinearTreatment::None, lin_ext, delta0, 48, 48);
    vanka.update(lin_ext);
    vanka.vmult(y, x);
    double sum = 0.0;
    for (const auto &blk : y.blocks())
      for (double e : blk.copy_to_host()) sum += e * e;
    std::printf("ranks=%d blocks=%llu carrier=%d cip_neighbours=%d vanka_blocks=%d vanka_finite=%d\n", comm->size(), nb, int(spaces->carrier),
                spaces->cip_neighbours, vanka.n_classes(), int(std::isfinite(sum) && sum > 0.0));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
