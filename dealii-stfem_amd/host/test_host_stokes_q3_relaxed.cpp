// C++ caller of the solver-side classes over an operator of velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)): StokesSpaces,
// StokesBlockVector, StokesSystem and RelaxedVankaStokes with a given relaxation and one iteration, linear or - with a treatment - after
// set_data; the estimated relaxation of two constructions; the zero-mean shift of StokesSlab on a box; compute_divergence; and the
// refusals of set_partition, of GMGStokes::vmult and of the slab's force quadrature.  cG(1), one step: one velocity and one pressure block.
//   test_host_stokes_q3_relaxed ncx ncy ncz dg_pressure viscosity tau treatment omega sweeps vertices.bin f.bin lin.bin cells.bin
// treatment: 0 None, 1 Explicit (form), 2 Implicit (jacobian).  vertices.bin: the (ncx + 1)(ncy + 1)(ncz + 1) x 3 doubles of the mesh;
// f.bin / lin.bin: uint64 number of blocks, then per block uint64 length and the doubles (lin.bin is not read with treatment 0; its
// velocity block is also the vector whose divergence is taken); cells.bin: the cell values of compute_divergence, doubles only.
// stdout, one line each: "history r_0 r_1 ..." (the residual norms of x <- x + omega V (f - A x) from x = 0), "omega w_1 w_2" (the
// estimates of two constructions with relaxation 0), "mean m max p" (weights . p / volume after the shift and max |p|, on the box
// with the same cells), "divergence total", "checks n".
#include "stfem/stokes_solver.h"

#include <cstdio>
#include <cstdlib>

using namespace stfem;

static bool read_blocks(const char *path, std::vector<StokesVector> &x)
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
  }
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv)
{
  if (argc != 14) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    mesh.dirichlet_mask = 63;
    const bool dg = std::atoi(argv[4]) != 0;
    const double nu = std::atof(argv[5]), tau = std::atof(argv[6]);
    const int tr = std::atoi(argv[7]);
    const NonlinearTreatment treatment = tr == 0 ? NonlinearTreatment::None : tr == 1 ? NonlinearTreatment::Explicit : NonlinearTreatment::Implicit;
    const double omega = std::atof(argv[8]);
    const unsigned sweeps = unsigned(std::atoi(argv[9]));
    {
      const size_t nv = size_t(mesh.ncell[0] + 1) * (mesh.ncell[1] + 1) * (mesh.ncell[2] + 1) * 3;
      mesh.vertices.resize(nv);
      FILE *f = std::fopen(argv[10], "rb");
      if (!f) return 5;
      const bool ok = std::fread(mesh.vertices.data(), sizeof(double), nv, f) == nv;
      std::fclose(f);
      if (!ok) return 5;
    }
    StokesSpace<double> space;
    space.velocity_degree = 3;
    space.dg_pressure = dg;
    space.viscosity = nu;
    space.nonlinear_treatment = treatment;
    StokesMatrixFreeOperator<3, double> K(mesh, space);
    const unsigned ns = 1, r = 1, nt = r;
    const auto w = get_fe_time_weights_stokes<double>(TimeStepType::CGP, r, tau, ns);
    BlockSlice slice(ns, 2, nt);
    SystemMatrixStokes<3, double> A(K, w[0], w[1], slice, treatment);
    auto spaces = std::make_shared<StokesSpaces>(mesh, K.handle());
    StokesSystem<3, double> system(A, spaces, K.handle(), slice);
    int ok = 0;
    ok += spaces->velocity_degree == 3 && spaces->carrier == dg && spaces->q2->degree == 3 && spaces->q1->degree == (dg ? 1u : 2u);

    StokesBlockVector f, lin, x, t, y;
    for (StokesBlockVector *v : {&f, &lin, &x, &t, &y}) system.initialize_dof_vector(*v);
    if (!read_blocks(argv[11], f.blocks())) return 5;
    if (treatment != NonlinearTreatment::None) {
      if (!read_blocks(argv[12], lin.blocks())) return 5;
      system.set_data(lin);
    }
    RelaxedVankaStokes<3> S(K, system, w[0], w[1], slice, treatment, 1, omega);
    if (treatment != NonlinearTreatment::None) S.set_data(lin);
    ok += S.relaxation() == omega;
    set_zero(x);
    std::printf("history");
    for (unsigned s = 0; s < sweeps; ++s) {
      system.vmult(t, x);
      axpby(1.0, f, -1.0, t); // t = f - A x
      std::printf(" %.17g", norm(t));
      S.vmult(y, t);
      axpby(1.0, y, 1.0, x);
    }
    std::printf("\n");

    // relaxation == 0: the estimate (20 power iterations on P^-1 A), of two constructions
    double est[2];
    for (double &e : est) {
      RelaxedVankaStokes<3> E(K, system, w[0], w[1], slice, treatment, 1, 0.0);
      if (treatment != NonlinearTreatment::None) E.set_data(lin);
      e = E.relaxation();
    }
    std::printf("omega %.17g %.17g\n", est[0], est[1]);

    // compute_divergence of the velocity block of lin.bin (of f.bin without a treatment)
    {
      const StokesBlockVector &src = treatment != NonlinearTreatment::None ? lin : f;
      std::vector<double> cells;
      const double total = K.compute_divergence(src.blocks()[slice.index(0, 0, 0)], cells);
      ok += K.compute_divergence(src.blocks()[slice.index(0, 0, 0)]) == total;
      std::printf("divergence %.17g\n", total);
      FILE *o = std::fopen(argv[13], "wb");
      if (!o) return 3;
      std::fwrite(cells.data(), sizeof(double), cells.size(), o);
      std::fclose(o);
    }

    // the zero-mean shift: the pressure helpers are those of boxes, so on the box with the same cells and unequal edges
    {
      Mesh box;
      for (int d = 0; d < 3; ++d) box.ncell[d] = mesh.ncell[d];
      box.upper[1] = 0.7;
      box.upper[2] = 1.3;
      StokesMatrixFreeOperator<3, double> Kb(box, space);
      SystemMatrixStokes<3, double> Ab(Kb, w[0], w[1], slice, treatment);
      auto sb = std::make_shared<StokesSpaces>(box, Kb.handle());
      StokesSystem<3, double> sysb(Ab, sb, Kb.handle(), slice);
      StokesBlockVector p;
      sysb.initialize_dof_vector(p);
      power_iteration_start(p);
      StokesVector &pb = p.blocks()[slice.index(0, 1, 0)];
      std::vector<double> h = pb.copy_to_host();
      for (size_t i = 0; i < h.size(); ++i) h[i] = 0.25 * h[i] + 1.5 + double(i % 7); // (not of zero mean)
      pb.copy_from_host(h);
      const auto w1 = get_fe_time_weights<double>(TimeStepType::CGP, r, tau, 1);
      StokesSlab slab(TimeStepType::CGP, r, w1[0], w1[2], VectorPointFunction(), true);
      slab.shift_pressure_to_zero_mean(p);
      std::vector<double> ones(h.size()), weights(h.size());
      double volume = 0.0;
      check(stfem_stokes_pressure_mean_vectors_space(Kb.handle(), ones.data(), weights.data(), &volume), "stfem_stokes_pressure_mean_vectors_space");
      const std::vector<double> after = pb.copy_to_host();
      double mean = 0.0, pmax = 0.0, before = 0.0;
      for (size_t i = 0; i < h.size(); ++i) {
        mean += weights[i] * after[i];
        before += weights[i] * h[i];
        pmax = std::max(pmax, std::abs(after[i]));
      }
      ok += std::abs(before / volume) > 1.0; // (the shift had something to do)
      std::printf("mean %.17g max %.17g\n", mean / volume, pmax);
      // slabs are not built at degree 3
      try {
        sb->set_partition(nullptr, -1, -1);
      } catch (const Error &e) {
        ok += e.status == STFEM_ERR_UNSUPPORTED;
      }
      // nor GMGStokes: its levels are degree-2 operators on the mesh, and it refuses the vectors of this operator
      try {
        GMGStokes<3> gmg(box, 1, nu, w[0], w[1], slice, GMGStokes<3>::AdditionalData(), {}, dg);
        StokesBlockVector q;
        sysb.initialize_dof_vector(q);
        gmg.vmult(q, p);
      } catch (const Error &e) {
        ok += e.status == STFEM_ERR_UNSUPPORTED;
      }
      // nor the time integrators: the force quadrature of the slab refuses
      try {
        slab.assemble_force(p, 0.0, tau);
      } catch (const Error &e) {
        ok += e.status == STFEM_ERR_UNSUPPORTED;
      }
    }
    std::printf("checks %d\n", ok);
    return ok == 7 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
