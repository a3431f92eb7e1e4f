// C++ caller of StokesMatrixFreeOperator::compute_drag_lift through the Stokes mirror (as tests/tp_03stokes.cc:958-964 calls it for
// every time DoF): Poiseuille flow u = (y (1 - y), 0, 0), p = -2 nu x + c on the box [0, Lx] x [0, 1] x [0, Lz] with the no-slip walls
// y = 0, 1 strongly constrained, whose force on every face has a closed form.
//   test_host_drag_lift ncx ncy ncz dg Lx Lz viscosity c
// Prints, 17 digits: "face f fx fy fz" for the six faces, "all fx fy fz" for the six together, "scaled fx fy fz" (face 3, scale -2.5),
// and "pair k fx fy fz" for the five pairs (k u, k p), k = 1..5, of ONE several-pairs call on faces {2, 3}; compares that call with
// the five single calls bit for bit itself ("pairs_equal=1") and counts the refusals ("exceptions=3").
#include "stfem/stokes.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace stfem;

int main(int argc, char **argv)
{
  if (argc != 9) return 2;
  try {
    Mesh mesh;
    for (int d = 0; d < 3; ++d) mesh.ncell[d] = std::atoi(argv[1 + d]);
    const bool dg = std::atoi(argv[4]) != 0;
    const double Lx = std::atof(argv[5]), Lz = std::atof(argv[6]), nu = std::atof(argv[7]), c = std::atof(argv[8]);
    mesh.upper[0] = Lx; mesh.upper[2] = Lz;
    mesh.dirichlet_mask = 4 | 8;
    StokesMatrixFreeOperator<3, double> K(mesh, 2, nu, {}, {}, 20, 10, 0.0, 0.0, 0.0, dg);
    const int ndu[3] = {2 * mesh.ncell[0] + 1, 2 * mesh.ncell[1] + 1, 2 * mesh.ncell[2] + 1};
    const size_t Nu = size_t(ndu[0]) * ndu[1] * ndu[2];
    std::vector<double> u(3 * Nu, 0.0), p;
    for (int k = 0; k < ndu[2]; ++k)
      for (int j = 0; j < ndu[1]; ++j)
        for (int i = 0; i < ndu[0]; ++i) {
          const double y = double(j) / (ndu[1] - 1);
          u[size_t(i) + ndu[0] * (size_t(j) + ndu[1] * size_t(k))] = y * (1 - y);
        }
    const double hx = Lx / mesh.ncell[0];
    if (dg) { // p[4 cell + j] of the basis 1, l(xi), l(eta), l(zeta), l(x) = sqrt 3 (2 x - 1): -2 nu (x0 + hx xi) + c
      const size_t ncells = size_t(mesh.ncell[0]) * mesh.ncell[1] * mesh.ncell[2];
      p.assign(4 * ncells, 0.0);
      for (size_t cell = 0; cell < ncells; ++cell) {
        const double xm = (double(cell % mesh.ncell[0]) + 0.5) * hx;
        p[4 * cell] = c - 2 * nu * xm;
        p[4 * cell + 1] = -nu * hx / std::sqrt(3.0);
      }
    } else {
      const int ndp[3] = {mesh.ncell[0] + 1, mesh.ncell[1] + 1, mesh.ncell[2] + 1};
      p.assign(size_t(ndp[0]) * ndp[1] * ndp[2], 0.0);
      for (size_t n = 0; n < p.size(); ++n) p[n] = -2 * nu * hx * double(n % ndp[0]) + c;
    }
    StokesMatrixFreeOperator<3, double>::BlockVectorType x;
    K.initialize_dof_vector(x);
    x[0].copy_from_host(u);
    x[1].copy_from_host(p);
    for (unsigned f = 0; f < 6; ++f) {
      const auto F = K.compute_drag_lift(x, {f}, 1.0);
      std::printf("face %u %.17g %.17g %.17g\n", f, F[0], F[1], F[2]);
    }
    {
      const auto F = K.compute_drag_lift(x, {0, 1, 2, 3, 4, 5}, 1.0);
      std::printf("all %.17g %.17g %.17g\n", F[0], F[1], F[2]);
      const auto S = K.compute_drag_lift(x, {3}, -2.5);
      std::printf("scaled %.17g %.17g %.17g\n", S[0], S[1], S[2]);
    }
    // five pairs in one call (a group of four and one more) against the five single calls
    std::vector<StokesMatrixFreeOperator<3, double>::BlockVectorType> xs(5);
    std::vector<const StokesVector *> us, ps;
    for (int k = 0; k < 5; ++k) {
      K.initialize_dof_vector(xs[k]);
      std::vector<double> uk(u), pk(p);
      for (double &v : uk) v *= k + 1;
      for (double &v : pk) v *= k + 1;
      xs[k][0].copy_from_host(uk);
      xs[k][1].copy_from_host(pk);
      us.push_back(&xs[k][0]);
      ps.push_back(&xs[k][1]);
    }
    const auto many = K.compute_drag_lift(us, ps, {2, 3}, 1.0);
    bool equal = many.size() == 5;
    for (int k = 0; k < 5 && equal; ++k) {
      const auto one = K.compute_drag_lift(xs[k], {2, 3}, 1.0);
      equal = one == many[k];
      std::printf("pair %d %.17g %.17g %.17g\n", k + 1, many[k][0], many[k][1], many[k][2]);
    }
    std::printf("pairs_equal=%d\n", int(equal));
    int thrown = 0;
    try { K.compute_drag_lift(x, {}, 1.0); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; } // no face
    try { K.compute_drag_lift(x, {6}, 1.0); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; }
    try { K.compute_drag_lift(x, {0}, std::nan("")); } catch (const Error &e) { thrown += e.status == STFEM_ERR_INVALID_ARGUMENT; }
    std::printf("exceptions=%d\n", thrown);
    return equal && thrown == 3 ? 0 : 4;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
