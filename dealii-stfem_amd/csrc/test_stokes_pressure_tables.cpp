// CPU self-test of the host-side 1D tables of the degree-2 pressure spaces (host_tables.cpp: legendre01, lagrange_q2_01,
// dgp_child_tables), against quadrature with the library's own Gauss rule: the Legendre functions are orthonormal on [0, 1], the
// Lagrange functions are the nodal basis of 0, 1/2, 1 and sum to 1, and T[s][i][j] is the L2 projection of the parent's l_i on child
// s onto the child's l_j - the closed formulas equal the integrals to rounding, and the parent's function equals its expansion at
// every point of the child.  Plain host code (tests/test_stokes_pressure_tables_cpu.py builds and runs it; HOSTFLAGS takes sanitizers).
#include "host_tables.h"

#include <cmath>
#include <cstdio>

int main()
{
  int bad = 0;
  auto expect = [&](bool ok, const char *what) {
    if (!ok) {
      std::printf("FAILED: %s\n", what);
      ++bad;
    }
  };
  std::vector<double> x, w;
  stfem::gauss_rule(4, x, w); // exact to degree 7
  // orthonormality
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (size_t q = 0; q < x.size(); ++q) {
        double l[3];
        stfem::legendre01(x[q], l);
        s += w[q] * l[i] * l[j];
      }
      expect(std::abs(s - (i == j ? 1.0 : 0.0)) < 1e-14, "the Legendre functions are orthonormal");
    }
  // the nodal basis of FE_Q(2)
  const double nodes[3] = {0.0, 0.5, 1.0};
  for (int n = 0; n < 3; ++n) {
    double l[3];
    stfem::lagrange_q2_01(nodes[n], l);
    for (int a = 0; a < 3; ++a) expect(l[a] == (a == n ? 1.0 : 0.0), "the Lagrange functions are nodal");
  }
  for (double p : x) {
    double l[3];
    stfem::lagrange_q2_01(p, l);
    expect(std::abs(l[0] + l[1] + l[2] - 1.0) < 1e-15, "the Lagrange functions sum to 1");
  }
  // the embedding into the two children
  double T[2][3][3];
  stfem::dgp_child_tables(T);
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        double proj = 0.0;
        for (size_t q = 0; q < x.size(); ++q) {
          double parent[3], child[3];
          stfem::legendre01(0.5 * (s + x[q]), parent);
          stfem::legendre01(x[q], child);
          proj += w[q] * parent[i] * child[j];
        }
        expect(std::abs(proj - T[s][i][j]) < 1e-14, "T is the projection of the parent's function onto the child's");
        if (j > i || (i == 2 && j == 0)) expect(T[s][i][j] == 0.0, "T is lower triangular with T[2][0] = 0");
      }
      for (int k = 0; k <= 10; ++k) {
        const double xi = 0.1 * k;
        double parent[3], child[3];
        stfem::legendre01(0.5 * (s + xi), parent);
        stfem::legendre01(xi, child);
        const double sum = T[s][i][0] * child[0] + T[s][i][1] * child[1] + T[s][i][2] * child[2];
        expect(std::abs(sum - parent[i]) < 1e-14, "the expansion equals the parent's function on the child");
      }
    }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
