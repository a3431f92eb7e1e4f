// Space-time convergence test of the instationary NAVIER-STOKES problem in 3D on the device: stokes_convergence.cpp with the convection
// term and a Newton / Picard iteration per slab (TimeIntegratorNavierStokes in host/stfem/stokes_solver.h).  Same exact solution and
// pressure (velocity = curl of psi e_z, psi = sin t (sin pi x sin pi y sin pi z)^2; pressure sin t cos pi x cos pi y cos pi z); the
// force is extended by (u . grad) u, which is the continuous counterpart of the operator's - int (u (x) u) : grad v because u is
// divergence-free and zero on the boundary.  FE_Q(2)^3 x FE_Q(1) / FE_DGP(1), dG(k) / cG(k), tau = 2^-(refinement + 1), 2^refinement
// cells per direction, homogeneous Dirichlet velocity, pressure with zero mean.
// treatment=newton: the system applies the jacobian about the last iterate (NonlinearTreatment::Implicit); treatment=picard: the form
// about it (Explicit).  Linear solves: FGMRES to lintol (relative), preconditioned by relaxation sweeps of the per-cell Vanka smoother
// of the linearised operator, or with mg=<levels> by one V-cycle of GMGStokes with linearised levels.
// delta0=<value>: the CIP interior-face stabilisation of the operator (default 0: none), weighted with the linearisation velocity in the
// system matrix (TimeIntegratorNavierStokes).  cipprec=1 (default 0) hands that delta0 to the preconditioner too: the term in the
// blocks of the per-cell Vanka smoother, or with mg= on every level (level operators and level smoothers); without it the
// preconditioners are those of the operator without the stabilisation.
// Usage: navier_convergence <type 0 = cG | 1 = dG> <k> <refinement> [treatment=newton|picard] [mg=<levels>] [dg=1] [nu=1] [nltol=1e-12]
//                           [delta0=0] [cipprec=0] [lintol=1e-3] [sweeps=3] [omega=0: estimated] [end_time=1] [warmup=<untimed slabs>]
// Prints: cells u-dofs p-dofs t-dofs  u:Linf-Linf  u:L2-L2  u:L2-H1semi  p:L2-L2  fgmres-iterations-per-solve
//         nonlinear-steps-per-slab  fgmres-iterations-per-slab  |div u_h|(end time)  share:residuals  share:set_data  share:krylov
//         most-nonlinear-steps-in-a-slab  all-slabs-converged
#include "stokes_problem.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace stfem;

int main(int argc_all, char **argv_all)
{
  unsigned mg_levels = 0, sweeps = 3, warmup = 0;
  bool dg_pressure = false, newton = true, cipprec = false;
  double nu = 1.0, nltol = 1e-12, lintol = 1e-3, omega_arg = 0.0, end_time = 1.0, delta0 = 0.0;
  std::vector<char *> pos;
  for (int i = 0; i < argc_all; ++i) {
    const char *a = argv_all[i];
    if (i == 0) pos.push_back(argv_all[i]);
    else if (std::strncmp(a, "mg=", 3) == 0) mg_levels = unsigned(std::atoi(a + 3));
    else if (std::strncmp(a, "dg=", 3) == 0) dg_pressure = std::atoi(a + 3) != 0;
    else if (std::strcmp(a, "treatment=newton") == 0) newton = true;
    else if (std::strcmp(a, "treatment=picard") == 0) newton = false;
    else if (std::strncmp(a, "nu=", 3) == 0) nu = std::atof(a + 3);
    else if (std::strncmp(a, "nltol=", 6) == 0) nltol = std::atof(a + 6);
    else if (std::strncmp(a, "delta0=", 7) == 0) delta0 = std::atof(a + 7);
    else if (std::strncmp(a, "cipprec=", 8) == 0) cipprec = std::atoi(a + 8) != 0;
    else if (std::strncmp(a, "lintol=", 7) == 0) lintol = std::atof(a + 7);
    else if (std::strncmp(a, "sweeps=", 7) == 0) sweeps = unsigned(std::atoi(a + 7));
    else if (std::strncmp(a, "omega=", 6) == 0) omega_arg = std::atof(a + 6);
    else if (std::strncmp(a, "end_time=", 9) == 0) end_time = std::atof(a + 9);
    else if (std::strncmp(a, "warmup=", 7) == 0) warmup = unsigned(std::atoi(a + 7));
    else if (std::strchr(a, '=')) {
      std::fprintf(stderr, "unknown argument %s\n", a);
      return 2;
    } else pos.push_back(argv_all[i]);
  }
  const int argc = int(pos.size());
  char **argv = pos.data();
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s type k refinement [treatment=newton|picard] [mg=<levels>] [dg=1] [nu=] [nltol=] [lintol=]\n", argv[0]);
    return 2;
  }
  const auto type = std::atoi(argv[1]) == 0 ? TimeStepType::CGP : TimeStepType::DG;
  const unsigned k = std::atoi(argv[2]), refinement = std::atoi(argv[3]);
  const int n = 1 << refinement;
  const double tau = std::ldexp(1.0, -int(refinement + 1));
  const NonlinearTreatment treatment = newton ? NonlinearTreatment::Implicit : NonlinearTreatment::Explicit;
  const unsigned max_nonlinear = 40;
  const double prec_delta0 = cipprec ? delta0 : 0.0;
  try {
    Mesh mesh;
    mesh.ncell[0] = mesh.ncell[1] = mesh.ncell[2] = n;
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, std::set<boundary_id>(), std::set<boundary_id>(), 20.0, 10.0, 0.0, delta0, 0.0, dg_pressure, treatment);
    auto spaces = std::make_shared<StokesSpaces>(mesh, K.handle());
    const unsigned nt = type == TimeStepType::CGP ? k : k + 1;
    const BlockSlice slice(1, 2, nt), slice1(1, 2, 1);
    const auto w = get_fe_time_weights_stokes<double>(type, k, tau, 1); // Alpha, Beta, Gamma, Zeta (fe_time.h:1242-1285)
    auto [Alpha_1, Beta_1, Gamma_1, Zeta_1] = get_fe_time_weights<double>(type, k, tau, 1);
    (void)Beta_1; (void)Zeta_1;
    SystemMatrixStokes<3, double> matrix(K, w[0], w[1], slice, treatment);
    // right-hand-side matrices (tests/tp_03stokes.cc:243-244): cG: Gamma on K_S, Zeta on M; dG: Gamma on M
    FullMatrix<double> zero(w[2].m(), w[2].n());
    const bool cgp = type == TimeStepType::CGP;
    SystemMatrixStokes<3, double> rhs_matrix(K, cgp ? w[2] : zero, cgp ? w[3] : w[2], slice, treatment);
    StokesSystem<3, double> system(matrix, spaces, K.handle(), slice);
    RelaxedVankaStokes<3> preconditioner(K, system, w[0], w[1], slice, treatment, sweeps, omega_arg, true, prec_delta0);

    const VectorPointFunction force = stokes_problem::force(nu, true);

    // the preconditioner behind one interface: relaxation sweeps on the finest level, or one V-cycle of the linearised levels
    std::unique_ptr<GMGStokes<3>> gmg;
    if (mg_levels > 0) {
      GMGStokes<3>::AdditionalData ad;
      ad.smoothing_degree = sweeps;
      ad.relaxation = omega_arg;
      ad.delta0 = prec_delta0;
      gmg = std::make_unique<GMGStokes<3>>(mesh, mg_levels, nu, w[0], w[1], slice, ad, std::set<boundary_id>(), dg_pressure, treatment);
    }
    struct Prec {
      RelaxedVankaStokes<3> *relax;
      GMGStokes<3> *gmg;
      void set_data(const StokesBlockVector &lin)
      {
        if (gmg) gmg->set_data(lin);
        else relax->set_data(lin);
      }
      void vmult(StokesBlockVector &dst, const StokesBlockVector &src) const
      {
        if (gmg) gmg->vmult(dst, src);
        else relax->vmult(dst, src);
      }
    } prec{&preconditioner, gmg.get()};
    std::unique_ptr<TimeIntegratorNavierStokes<3, StokesSystem<3, double>, Prec>> step;
    auto make_step = [&] {
      step = std::make_unique<TimeIntegratorNavierStokes<3, StokesSystem<3, double>, Prec>>(type, k, Alpha_1, Gamma_1, lintol, system, prec, rhs_matrix, force, true,
                                                                                          nltol, 1e-14, max_nonlinear);
    };
    make_step();
    stokes_problem::SlabErrors err(type, k, spaces);

    StokesBlockVector x, rhs, prev;
    x.reinit(spaces, K.handle(), slice);
    rhs.reinit(spaces, K.handle(), slice);
    prev.reinit(spaces, K.handle(), slice1); // u(0) = 0, p(0) = 0
    const size_t nu_dofs = size_t(stfem_stokes_n_velocity_dofs(K.handle()));
    double time = 0.0;
    unsigned slabs = 0, iterations = 0, nonlinear = 0, most_nonlinear = 0;
    bool all_converged = true;
    double solve_seconds = 0.0;
    // warmup=<slabs>: the first slabs are solved untimed (code objects, smoother set-up, first estimates), then the run starts over
    for (unsigned i = 0; i < warmup; ++i) step->solve(x, prev, rhs, tau * i, tau);
    if (warmup) {
      set_zero(x);
      make_step();
    }
    while (time < end_time - 1e-12) {
      const auto t0 = std::chrono::steady_clock::now();
      step->solve(x, prev, rhs, time, tau);
      (void)dot(x, x); // synchronises
      solve_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      iterations += step->last_step();
      nonlinear += step->nonlinear_steps();
      most_nonlinear = std::max(most_nonlinear, step->nonlinear_steps());
      all_converged = all_converged && step->converged();
      ++slabs;
      std::fprintf(stderr, "slab %u: %u %s steps, %u FGMRES iterations, residuals", slabs, step->nonlinear_steps(), newton ? "Newton" : "Picard", step->last_step());
      for (double r : step->residuals()) std::fprintf(stderr, " %.2e", r);
      std::fprintf(stderr, "%s\n", step->converged() ? "" : " NOT CONVERGED");
      err.add(time, tau, x, prev);
      err.advance(x, prev);
      time += tau;
    }
    const double divergence = K.compute_divergence(prev.blocks()[0]); // |div u_h| at the end time
    const double tr = step->residual_seconds(), ts = step->set_data_seconds(), tk = step->solver_seconds(), tsum = std::max(tr + ts + tk, 1e-300);
    std::fprintf(stderr,
                 "%u slabs: %.3f s (right-hand side on the host + nonlinear solve); residuals %.3f s, set_data %.3f s, FGMRES %.3f s for %u iterations = %.2f ms per "
                 "iteration, %u nonlinear steps\n",
                 slabs, solve_seconds, tr, ts, tk, iterations, 1e3 * tk / std::max(1u, iterations), nonlinear);
    if (gmg) {
      for (unsigned l = 0; l < gmg->n_levels(); ++l) std::fprintf(stderr, "level %u: relaxation %.4f\n", l, gmg->relaxation(l));
      gmg->print_timing(stderr);
    } else
      std::fprintf(stderr, "relaxation %.4f\n", preconditioner.relaxation());
    std::printf("%d %lld %lld %u %.12e %.12e %.12e %.12e %.2f %.2f %.2f %.12e %.4f %.4f %.4f %u %d\n", n * n * n, 3ll * (long long)nu_dofs,
                (long long)stfem_stokes_n_pressure_dofs(K.handle()), nt, err.l8, std::sqrt(err.l2), std::sqrt(err.h1), std::sqrt(err.l2p),
                double(iterations) / std::max(1u, nonlinear), double(nonlinear) / slabs, double(iterations) / slabs, divergence, tr / tsum, ts / tsum, tk / tsum,
                most_nonlinear, all_converged ? 1 : 0);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
