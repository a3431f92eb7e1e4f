// The test problem of stokes_convergence.cpp and navier_convergence.cpp.  The reference's exact solution (include/exact_solution.h:199-325)
// is two-dimensional; this is its 3D analogue: the velocity is the curl of psi e_z, psi = sin t (sin pi x sin pi y sin pi z)^2, i.e.
// u = 2 pi sin t (A(x) B(y) A(z), - B(x) A(y) A(z), 0), the pressure sin t cos pi x cos pi y cos pi z.  Plus the error sums of a run.
#pragma once
#include "stfem/stokes_solver.h"

#include <thread>

namespace stokes_problem {
using namespace stfem;

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

// d_t u - nu Laplace u + grad p; with `convection` also (u . grad) u, the continuous counterpart of the operator's
// - int (u (x) u) : grad v because u is divergence-free and zero on the boundary
inline VectorPointFunction force(double nu, bool convection)
{
  return [nu, convection](double t, const std::vector<double> &p, std::array<std::vector<double>, 3> &out) {
    const size_t np = p.size() / 3;
    const double st = std::sin(t), ct = std::cos(t);
    for (auto &o : out) o.resize(np);
    for_points(np, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        const double lap1 = d2A(x) * B(y) * A(z) + A(x) * d2B(y) * A(z) + A(x) * B(y) * d2A(z);
        const double lap2 = d2B(x) * A(y) * A(z) + B(x) * d2A(y) * A(z) + B(x) * A(y) * d2A(z);
        const double sx = std::sin(PI * x), sy = std::sin(PI * y), sz = std::sin(PI * z), cx = std::cos(PI * x), cy = std::cos(PI * y), cz = std::cos(PI * z);
        out[0][i] = 2 * PI * (ct * A(x) * B(y) * A(z) - nu * st * lap1) - PI * st * sx * cy * cz;
        out[1][i] = -2 * PI * (ct * B(x) * A(y) * A(z) - nu * st * lap2) - PI * st * cx * sy * cz;
        out[2][i] = -PI * st * cx * cy * sz;
        if (!convection) continue;
        const double a = 2 * PI * st, u1 = a * A(x) * B(y) * A(z), u2 = -a * B(x) * A(y) * A(z);
        out[0][i] += u1 * a * dA(x) * B(y) * A(z) + u2 * a * A(x) * dB(y) * A(z);
        out[1][i] += -u1 * a * dB(x) * A(y) * A(z) - u2 * a * B(x) * dA(y) * A(z);
      }
    });
  };
}
inline PointFunction exact_u(int c)
{
  return [c](double t, const std::vector<double> &p, std::vector<double> &out) {
    out.resize(p.size() / 3);
    const double a = 2 * PI * std::sin(t);
    for_points(out.size(), [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        out[i] = c == 0 ? a * A(x) * B(y) * A(z) : (c == 1 ? -a * B(x) * A(y) * A(z) : 0.0);
      }
    });
  };
}
inline PointFunction exact_grad_u(int c)
{
  return [c](double t, const std::vector<double> &p, std::vector<double> &out) {
    out.assign(p.size(), 0.0);
    const double a = 2 * PI * std::sin(t);
    for_points(p.size() / 3, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (c == 0) { out[3 * i] = a * dA(x) * B(y) * A(z); out[3 * i + 1] = a * A(x) * dB(y) * A(z); out[3 * i + 2] = a * A(x) * B(y) * dA(z); }
        if (c == 1) { out[3 * i] = -a * dB(x) * A(y) * A(z); out[3 * i + 1] = -a * B(x) * dA(y) * A(z); out[3 * i + 2] = -a * B(x) * A(y) * dA(z); }
      }
    });
  };
}
inline void exact_p(double t, const std::vector<double> &p, std::vector<double> &out)
{
  out.resize(p.size() / 3);
  for_points(out.size(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) out[i] = std::sin(t) * std::cos(PI * p[3 * i]) * std::cos(PI * p[3 * i + 1]) * std::cos(PI * p[3 * i + 2]);
  });
}

// The error sums of a run, slab by slab.  ErrorCalculator (exact_solution.h:503-649): QGauss(k + 1) in time; QGauss(3) per direction for
// the velocity components, QGauss(2) for the pressure.  x: one time step's blocks, prev: one (velocity, pressure) pair.
class SlabErrors {
public:
  SlabErrors(TimeStepType type, unsigned k, const std::shared_ptr<StokesSpaces> &spaces) : spaces(spaces), err_p(type, k, 2, spaces, exact_p)
  {
    for (int c = 0; c < 3; ++c) err_u.emplace_back(type, k, 3, spaces->q2, exact_u(c), exact_grad_u(c));
  }
  void add(double time, double tau, const StokesBlockVector &x, const StokesBlockVector &prev)
  {
    const BlockSlice &slice = x.slice();
    const unsigned nt = slice.n_timedofs();
    const size_t nu_dofs = size_t(stfem_stokes_n_velocity_dofs(x.stokes()));
    // the time dofs of one variable from `offset` into its blocks on, and prev likewise, as block vectors of the scalar space ctx:
    // a velocity component on the FE_Q(2) space, the pressure on its own
    auto wrap = [&](unsigned var, size_t offset, const std::shared_ptr<Context> &ctx) {
      std::vector<void *> ptrs(nt);
      for (unsigned a = 0; a < nt; ++a) ptrs[a] = x.blocks()[slice.index(0, var, a)].data() + offset;
      void *pp[1] = {prev.blocks()[var].data() + offset};
      std::array<BlockVectorT<double>, 2> v;
      v[0].wrap(ctx, ptrs.data(), nt);
      v[1].wrap(ctx, pp, 1);
      return v;
    };
    for (int c = 0; c < 3; ++c) {
      const auto v = wrap(0, c * nu_dofs, spaces->q2);
      const auto e = err_u[c].evaluate_error(time, tau, v[0], v[1], 1);
      l2 += e[0];
      l8 = std::max(l8, e[1]);
      h1 += e[2];
    }
    const auto v = wrap(1, 0, spaces->q1);
    l2p += err_p.evaluate_error(time, tau, v[0], v[1])[0];
  }
  // the end value of the slab becomes the previous solution
  static void advance(const StokesBlockVector &x, StokesBlockVector &prev)
  {
    for (unsigned var = 0; var < 2; ++var) axpby(1.0, x.view(x.slice().index(0, var, x.slice().n_timedofs() - 1)), 0.0, prev.view(var));
  }
  double l2 = 0.0, l8 = -1.0, h1 = 0.0, l2p = 0.0; // squares of the L2-L2 and L2-H1semi velocity errors, Linf-Linf, square of the pressure's L2-L2

private:
  std::shared_ptr<StokesSpaces> spaces;
  std::vector<ErrorCalculator<double>> err_u;
  PressureErrorCalculator err_p;
};

} // namespace stokes_problem
