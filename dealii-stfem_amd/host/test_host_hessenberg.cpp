// C++ caller of HessenbergLeastSquares (host/stfem/hessenberg.h), the dense part of SolverFGMRES and GMG::coarse_gmres: a fixed 5 x 4 upper
// Hessenberg matrix is fed column by column with the right-hand side beta e_1.  Prints beta, the matrix, the residual norm reported
// after each column and the minimiser y; tests/test_host_hessenberg_cpu.py compares with numpy.linalg.lstsq.  No device, no library.
#include "stfem/hessenberg.h"

#include <cstdio>

int main()
{
  const unsigned m = 4;
  const double beta = 1.75;
  const double H[m + 1][m] = {{2.0, 0.5, -0.3, 0.1}, {1.0, 1.5, 0.4, -0.2}, {0.0, 0.8, 1.2, 0.3}, {0.0, 0.0, 0.6, 1.1}, {0.0, 0.0, 0.0, 0.4}};
  std::printf("beta %.17g\n", beta);
  for (unsigned i = 0; i <= m; ++i) std::printf("H %.17g %.17g %.17g %.17g\n", H[i][0], H[i][1], H[i][2], H[i][3]);
  stfem::HessenbergLeastSquares ls(m, beta);
  for (unsigned j = 0; j < m; ++j) {
    std::vector<double> hcol(j + 1);
    for (unsigned i = 0; i <= j; ++i) hcol[i] = H[i][j];
    std::printf("residual %.17g\n", ls.append_column(hcol, H[j + 1][j]));
  }
  std::printf("y");
  for (double v : ls.solve()) std::printf(" %.17g", v);
  std::printf("\n");
  return 0;
}
