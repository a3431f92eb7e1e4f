// Space-time convergence test of the instationary NAVIER-STOKES problem in 3D on the device: stokes_convergence.cpp with the convection
// term and a Newton / Picard iteration per slab (TimeIntegratorNavierStokes in host/stfem/stokes_solver.h).  Same exact solution and
// pressure (velocity = curl of psi e_z, psi = sin t (sin pi x sin pi y sin pi z)^2; pressure sin t cos pi x cos pi y cos pi z); the
// force is extended by (u . grad) u, which is the continuous counterpart of the operator's - int (u (x) u) : grad v because u is
// divergence-free and zero on the boundary.  FE_Q(2)^3 x FE_Q(1) / FE_DGP(1), dG(k) / cG(k), tau = 2^-(refinement + 1), 2^refinement
// cells per direction, homogeneous Dirichlet velocity, pressure with zero mean.
// treatment=newton: the system applies the jacobian about the last iterate (NonlinearTreatment::Implicit); treatment=picard: the form
// about it (Explicit).  Linear solves: FGMRES to lintol (relative), preconditioned by relaxation sweeps of the per-cell Vanka smoother
// of the linearised operator, or with mg=<levels> by one V-cycle of GMGStokes with linearised levels.
// Usage: navier_convergence <type 0 = cG | 1 = dG> <k> <refinement> [treatment=newton|picard] [mg=<levels>] [dg=1] [nu=1] [nltol=1e-12]
//                           [lintol=1e-3] [sweeps=3] [omega=0: estimated] [end_time=1] [warmup=<untimed slabs>]
// Prints: cells u-dofs p-dofs t-dofs  u:Linf-Linf  u:L2-L2  u:L2-H1semi  p:L2-L2  fgmres-iterations-per-solve
//         nonlinear-steps-per-slab  fgmres-iterations-per-slab  |div u_h|(end time)  share:residuals  share:set_data  share:krylov
//         most-nonlinear-steps-in-a-slab  all-slabs-converged
#include "stfem/stokes_solver.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

using namespace stfem;

namespace {
const double PI = 3.14159265358979323846;
inline double A(double s) { const double q = std::sin(PI * s); return q * q; }
inline double dA(double s) { return PI * std::sin(2 * PI * s); }
inline double d2A(double s) { return 2 * PI * PI * std::cos(2 * PI * s); }
inline double B(double s) { return 0.5 * std::sin(2 * PI * s); }
inline double dB(double s) { return PI * std::cos(2 * PI * s); }
inline double d2B(double s) { return -4 * PI * PI * B(s); }
// the analytic functions are evaluated at up to 10^7 points per call (27 quadrature points per cell): the point loop in slices on
// the host's cores (the reference evaluates its Functions inside the threaded cell loops of deal.II)
template <typename Body> void for_points(size_t n, Body &&body)
{
  const unsigned nthreads = n < 65536 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (nthreads == 1) {
    body(size_t(0), n);
    return;
  }
  std::vector<std::thread> pool;
  const size_t chunk = (n + nthreads - 1) / nthreads;
  for (unsigned t = 0; t < nthreads; ++t) {
    const size_t lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
    if (lo < hi) pool.emplace_back([&body, lo, hi] { body(lo, hi); });
  }
  for (auto &th : pool) th.join();
}
} // namespace

int main(int argc_all, char **argv_all)
{
  unsigned mg_levels = 0, sweeps = 3, warmup = 0;
  bool dg_pressure = false, newton = true;
  double nu = 1.0, nltol = 1e-12, lintol = 1e-3, omega_arg = 0.0, end_time = 1.0;
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
  try {
    Mesh mesh;
    mesh.ncell[0] = mesh.ncell[1] = mesh.ncell[2] = n;
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, std::set<boundary_id>(), std::set<boundary_id>(), 20.0, 10.0, 0.0, 0.0, 0.0, dg_pressure, treatment);
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
    PreconditionRelaxationLinearisedStokes<3> preconditioner(K, system, w[0], w[1], slice, treatment, sweeps, omega_arg);

    const VectorPointFunction force = [&](double t, const std::vector<double> &p, std::array<std::vector<double>, 3> &out) {
      const size_t np = p.size() / 3;
      const double st = std::sin(t), ct = std::cos(t);
      for (auto &o : out) o.resize(np);
      for_points(np, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        const double lap1 = d2A(x) * B(y) * A(z) + A(x) * d2B(y) * A(z) + A(x) * B(y) * d2A(z);
        const double lap2 = d2B(x) * A(y) * A(z) + B(x) * d2A(y) * A(z) + B(x) * A(y) * d2A(z);
        const double sx = std::sin(PI * x), sy = std::sin(PI * y), sz = std::sin(PI * z), cx = std::cos(PI * x), cy = std::cos(PI * y), cz = std::cos(PI * z);
        // (u . grad) u of u = a (A(x) B(y) A(z), - B(x) A(y) A(z), 0), a = 2 pi sin t
        const double a = 2 * PI * st, u1 = a * A(x) * B(y) * A(z), u2 = -a * B(x) * A(y) * A(z);
        const double conv1 = u1 * a * dA(x) * B(y) * A(z) + u2 * a * A(x) * dB(y) * A(z);
        const double conv2 = -u1 * a * dB(x) * A(y) * A(z) - u2 * a * B(x) * dA(y) * A(z);
        out[0][i] = 2 * PI * (ct * A(x) * B(y) * A(z) - nu * st * lap1) - PI * st * sx * cy * cz + conv1;
        out[1][i] = -2 * PI * (ct * B(x) * A(y) * A(z) - nu * st * lap2) - PI * st * cx * sy * cz + conv2;
        out[2][i] = -PI * st * cx * cy * sz;
      }
      });
    };
    auto exact_u = [&](int c) {
      return PointFunction([c](double t, const std::vector<double> &p, std::vector<double> &out) {
        out.resize(p.size() / 3);
        const double a = 2 * PI * std::sin(t);
        for_points(out.size(), [&](size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; ++i) {
            const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            out[i] = c == 0 ? a * A(x) * B(y) * A(z) : (c == 1 ? -a * B(x) * A(y) * A(z) : 0.0);
          }
        });
      });
    };
    auto exact_grad_u = [&](int c) {
      return PointFunction([c](double t, const std::vector<double> &p, std::vector<double> &out) {
        out.assign(p.size(), 0.0);
        const double a = 2 * PI * std::sin(t);
        for_points(p.size() / 3, [&](size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; ++i) {
            const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            if (c == 0) { out[3 * i] = a * dA(x) * B(y) * A(z); out[3 * i + 1] = a * A(x) * dB(y) * A(z); out[3 * i + 2] = a * A(x) * B(y) * dA(z); }
            if (c == 1) { out[3 * i] = -a * dB(x) * A(y) * A(z); out[3 * i + 1] = -a * B(x) * dA(y) * A(z); out[3 * i + 2] = -a * B(x) * A(y) * dA(z); }
          }
        });
      });
    };
    const PointFunction exact_p = [](double t, const std::vector<double> &p, std::vector<double> &out) {
      out.resize(p.size() / 3);
      for_points(out.size(), [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) out[i] = std::sin(t) * std::cos(PI * p[3 * i]) * std::cos(PI * p[3 * i + 1]) * std::cos(PI * p[3 * i + 2]);
      });
    };

    // the preconditioner behind one interface: relaxation sweeps on the finest level, or one V-cycle of the linearised levels
    std::unique_ptr<GMGStokes<3>> gmg;
    if (mg_levels > 0) {
      GMGStokes<3>::AdditionalData ad;
      ad.smoothing_degree = sweeps;
      ad.relaxation = omega_arg;
      gmg = std::make_unique<GMGStokes<3>>(mesh, mg_levels, nu, w[0], w[1], slice, ad, std::set<boundary_id>(), dg_pressure, treatment);
    }
    struct Prec {
      PreconditionRelaxationLinearisedStokes<3> *relax;
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
    // ErrorCalculator (exact_solution.h:503-649): QGauss(k + 1) in time; QGauss(3) per direction for the velocity components, QGauss(2) for the pressure
    std::vector<ErrorCalculator<double>> err_u;
    for (int c = 0; c < 3; ++c) err_u.emplace_back(type, k, 3, spaces->q2, exact_u(c), exact_grad_u(c));
    PressureErrorCalculator err_p(type, k, 2, spaces, exact_p);

    StokesBlockVector x, rhs, prev;
    x.reinit(spaces, K.handle(), slice);
    rhs.reinit(spaces, K.handle(), slice);
    prev.reinit(spaces, K.handle(), slice1); // u(0) = 0, p(0) = 0
    const size_t nu_dofs = size_t(stfem_stokes_n_velocity_dofs(K.handle()));
    double time = 0.0, l2 = 0.0, l8 = -1.0, h1 = 0.0, l2p = 0.0;
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
      for (int c = 0; c < 3; ++c) {
        std::vector<void *> ptrs(nt);
        for (unsigned a = 0; a < nt; ++a) ptrs[a] = x.blocks()[slice.index(0, 0, a)].data() + c * nu_dofs;
        BlockVectorT<double> xc, pc;
        xc.wrap(spaces->q2, ptrs.data(), nt);
        void *pp[1] = {prev.blocks()[0].data() + c * nu_dofs};
        pc.wrap(spaces->q2, pp, 1);
        const auto e = err_u[c].evaluate_error(time, tau, xc, pc, 1);
        l2 += e[0];
        l8 = std::max(l8, e[1]);
        h1 += e[2];
      }
      {
        std::vector<void *> ptrs(nt);
        for (unsigned a = 0; a < nt; ++a) ptrs[a] = x.blocks()[slice.index(0, 1, a)].data();
        BlockVectorT<double> xp, pp;
        xp.wrap(spaces->q1, ptrs.data(), nt);
        void *q[1] = {prev.blocks()[1].data()};
        pp.wrap(spaces->q1, q, 1);
        l2p += err_p.evaluate_error(time, tau, xp, pp)[0];
      }
      axpby(1.0, x.view(slice.index(0, 0, nt - 1)), 0.0, prev.view(0));
      axpby(1.0, x.view(slice.index(0, 1, nt - 1)), 0.0, prev.view(1));
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
                (long long)stfem_stokes_n_pressure_dofs(K.handle()), nt, l8, std::sqrt(l2), std::sqrt(h1), std::sqrt(l2p),
                double(iterations) / std::max(1u, nonlinear), double(nonlinear) / slabs, double(iterations) / slabs, divergence, tr / tsum, ts / tsum, tk / tsum,
                most_nonlinear, all_converged ? 1 : 0);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
