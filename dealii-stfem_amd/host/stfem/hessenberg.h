// The dense part of the GMRES solvers (SolverFGMRES in time_integrators.h, GMG::coarse_gmres in stmg.h): the (m + 1) x m Hessenberg
// matrix of the Arnoldi process, brought to triangular form by Givens rotations column by column, with the right-hand side beta e_1
// rotated along.  Plain host code: no device call.
#pragma once
#include <cmath>
#include <vector>

namespace stfem {

struct HessenbergLeastSquares {
  unsigned m, j = 0; // columns at most / so far
  std::vector<double> H, cs, sn, g;
  HessenbergLeastSquares(unsigned m, double beta) : m(m), H(size_t(m + 1) * m, 0.0), cs(m), sn(m), g(m + 1, 0.0) { g[0] = beta; }
  // column j: hcol[0 .. j] from the Gram-Schmidt step and hn below the diagonal.  The earlier rotations are applied to it, the new one
  // annihilates hn; returns |g[j + 1]|, the residual norm of min |beta e_1 - H y| over the columns so far
  double append_column(const std::vector<double> &hcol, double hn)
  {
    for (unsigned i = 0; i <= j; ++i) H[i * m + j] = hcol[i];
    H[(j + 1) * m + j] = hn;
    for (unsigned i = 0; i < j; ++i) {
      const double t = cs[i] * H[i * m + j] + sn[i] * H[(i + 1) * m + j];
      H[(i + 1) * m + j] = -sn[i] * H[i * m + j] + cs[i] * H[(i + 1) * m + j];
      H[i * m + j] = t;
    }
    const double d = std::hypot(H[j * m + j], H[(j + 1) * m + j]);
    cs[j] = H[j * m + j] / d;
    sn[j] = H[(j + 1) * m + j] / d;
    H[j * m + j] = d;
    H[(j + 1) * m + j] = 0.0;
    g[j + 1] = -sn[j] * g[j];
    g[j] = cs[j] * g[j];
    return std::abs(g[++j]);
  }
  // the minimiser y (one entry per column so far): back-substitution in the triangular matrix
  std::vector<double> solve() const
  {
    std::vector<double> y(j);
    for (int i = int(j) - 1; i >= 0; --i) {
      double s = g[i];
      for (unsigned k = i + 1; k < j; ++k) s -= H[i * m + k] * y[k];
      y[i] = s / H[i * m + i];
    }
    return y;
  }
};

} // namespace stfem
