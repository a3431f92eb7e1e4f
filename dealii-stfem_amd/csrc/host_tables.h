// Host-side numerics of the product library: 1D rules, shape tables in even-odd form,
// temporal matrices (fe_time.h of the reference), mesh and coefficient helpers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stfem {

// ---- 1D rules on [0,1] (deal.II QGauss, QGaussLobatto, QGaussRadau(right)) ----
void gauss_rule(int n, std::vector<double> &x, std::vector<double> &w);
std::vector<double> lobatto_points(int n);
std::vector<double> radau_right_points(int n);

using Mat = std::vector<double>; // row-major

// Lagrange basis on `nodes` evaluated at `x`: V[q*n+a] = l_a(x_q), G[q*n+a] = l_a'(x_q)
void lagrange_tables(const std::vector<double> &nodes, const std::vector<double> &x, Mat &V, Mat &G);

// Even-odd packing of an n x n matrix X with X[q][a] = sign * X[n-1-q][n-1-a].
// Layout (h = n/2): ee[q*h+i] | oo[q*h+i] | em[q] | mm[i] | mmm     (last three only for odd n)
constexpr int eo_size(int n) { return 2 * (n / 2) * (n / 2) + ((n & 1) ? 2 * (n / 2) + 1 : 0); }
constexpr int EO_MAX = 32; // >= eo_size(7)
void eo_pack(int n, const Mat &X, double *out);

// Per-degree kernel tables.  Quadrature weights are folded into the tables:
//   Si  = diag(sqrt w) S            (nodes -> Gauss points, "interpolate")
//   Dc  = diag(sqrt w) Dcol diag(1/sqrt w)   (collocation derivative at Gauss points)
// so that M_cell = vol * Si^T Si and K_cell,d = vol/h_d^2 * Si^T Dc^T Dc Si per direction.
struct ShapeTables {
  int n; // p+1 == n_q
  Mat S, D;      // plain S[q][a] = l_a(x_q), D[q][a] = l_a'(x_q)   (nodal -> Gauss)
  Mat Dcol;      // plain collocation derivative on the Gauss points
  std::vector<double> xq, wq, nodes;
  double eo_Si[EO_MAX], eo_SiT[EO_MAX], eo_Dc[EO_MAX], eo_DcT[EO_MAX];
  double eo_L[EO_MAX]; // L = Dc^T Dc: 1D weighted collocation Laplacian (symmetric type)
  double eo_S[EO_MAX], eo_ST[EO_MAX], eo_Dq[EO_MAX], eo_DqT[EO_MAX]; // unweighted S, Dcol
  // Simultaneous diagonalisation of the 1D nodal mass and stiffness matrices of the reference
  // cell, M1 = S^T diag(w) S and K1 = D^T diag(w) D:  W M1^-1 W^T = I,  K1 = W^T diag(lam) W
  // (W = V^-1 for the M1-orthonormal generalised eigenvectors V).  Both matrices are
  // persymmetric, so every mode is even or odd: rows 0..ne-1 of W are even (ne = ceil(n/2)),
  // rows ne..n-1 odd.  fd_W packs only the independent half:
  //   We[m*ne + i], i < ne   (coefficient of u_i + u_{n-1-i}, and of u_{n/2} for the middle)
  //   Wo[m*h + i],  i < h    (coefficient of u_i - u_{n-1-i}),   h = n/2, stored after We
  double fd_W[EO_MAX], fd_lam[8];
  // M1 and K1 themselves in parity form, for applying them to a line directly (W^T W = M1 and W^T diag(lam) W = K1, but
  // the tables are packed from the assembled matrices, not from products of the rounded W).  For X = M1 or K1, with
  //   ae_i = u_i + u_{n-1-i},  ao_i = u_i - u_{n-1-i}  (i < h),  ae_h = u_h for odd n,
  //   e = Xe ae,  o = Xo ao,   (X u)_i = e_i + o_i,  (X u)_{n-1-i} = e_i - o_i,  (X u)_h = e_h:
  //   Xe[i][j] = (X[i][j] + X[i][n-1-j]) / 2,  Xo[i][j] = (X[i][j] - X[i][n-1-j]) / 2   (i, j < h; the halves folded in),
  //   Xe[i][h] = Xe[h][i] = X[i][h],  Xe[h][h] = X[h][h].
  // Xe (ne x ne) and Xo (h x h) are symmetric; only their upper triangles are stored, row by row, Xe first:
  // entry (i, j), i <= j, of an m x m block at fd_sym_index(m, i, j); Xo starts at fd_sym_index(ne, ne, ne) = ne (ne + 1) / 2.
  double fd_M1[EO_MAX], fd_K1[EO_MAX];
};
constexpr int fd_sym_index(int m, int i, int j) { return i <= j ? i * m - i * (i - 1) / 2 + (j - i) : fd_sym_index(m, j, i); }
ShapeTables make_shape_tables(int p);

// ---- temporal matrices ----
int time_nb(int type, int r, int nsteps);
int fe_time_weights(int type, int r, double tau, int nsteps, Mat &Alpha, Mat &Beta, Mat &Gamma,
                    Mat &Zeta);
int fe_time_weights_wave(int type, int r, double tau, int nsteps, Mat &A_lhs, Mat &B_lhs,
                         Mat &rhs_uK, Mat &rhs_uM, Mat &rhs_vM);

// time-multigrid transfer matrices (fe_time.h:749-898), row-major m x n; return 0 or -1 (bad arguments)
int time_prolongation(int type, int r, int nsteps, Mat &out, int &m, int &n);
int time_restriction(int type, int r, int nsteps, Mat &out, int &m, int &n);
int time_projection(int type, int r_src, int r_dst, int nsteps, Mat &out, int &m, int &n);
// get_time_evaluation_matrix (fe_time.h:308-326) of the basis of get_time_basis(type, r): samples x (r + 1), the basis at s / (samples - 1)
int time_evaluation(int type, int r, int samples, Mat &out, int &m, int &n);

// ---- level schedule of the space-time multigrid (fe_time.cc:17-150); levels are 't' (tau), 'k', 'h', 'p' like MGType ----
// get_poly_mg_sequence: sequence_type 0 = bisect, 1 = decrease_by_one, 2 = go_to_one; coarsest first
std::vector<int> poly_mg_sequence(int k_max, int k_min, int sequence_type);
// get_mg_sequence: n_k / n_p = lengths of the temporal / spatial degree sequences; coarsest transfer first
std::string mg_sequence(int n_sp_lvl, int n_k, int n_p, int n_timesteps_at_once, int n_timesteps_at_once_min, char lower_lvl,
                        int coarsening_type, bool time_before_space, bool use_p_multigrid_space, bool zip_from_back);
// get_precondition_stmg_types: one smoother id per level (0 = identity)
std::vector<int> precondition_stmg_types(const std::string &mg_type_level, int coarsening_type, bool time_before_space, int smoother);

// ---- 1D factors of the space transfers ----
// line index -> (cell, local node) of a 1D FE_Q(p) line with n cells
void cell_of(int i, int p, int n, int &cell, int &j);
// 1D embedding P[n_f x n_c] (coarse nodal values -> fine nodal values of the same function) and the nodal
// interpolation I[n_c x n_f] (the fine function at the coarse nodes); nc_f / nc_c = fine cells per coarse cell
void line_matrices(int nc_f, int p_f, int nc_c, int p_c, std::vector<double> &P, std::vector<double> &I);

// ---- the 1D functions of the degree-2 pressure spaces on [0, 1] ----
// the orthonormal Legendre functions l_0 = 1, l_1 = sqrt 3 (2 x - 1), l_2 = sqrt 5 (6 x^2 - 6 x + 1) of FE_DGP at x
void legendre01(double x, double out[3]);
// the Lagrange functions of FE_Q(2) on the nodes 0, 1/2, 1 at x
void lagrange_q2_01(double x, double out[3]);
// The parent's Legendre functions on child s of [0, 1] halved, x = (s + xi) / 2:  l_i(x) = sum_j T[s][i][j] l_j(xi) - lower triangular:
//   l_0 = l_0,  l_1 = 1/2 l_1 + (2 s - 1) (sqrt 3 / 2) l_0,  l_2 = 1/4 l_2 + (2 s - 1) (sqrt 15 / 4) l_1
void dgp_child_tables(double T[2][3][3]);

// ---- mesh / coefficient ----
void mesh_vertices(const int32_t gn[3], const double lo[3], const double up[3], double distort,
                   uint64_t seed, int32_t z0, int32_t z1, double *out);
void coefficient_per_cell(const int32_t nc[3], const double *vertices, double c1, double c2,
                          double c3, double distort, const int32_t sub[3], const double lo[3],
                          const double up[3], double *out);

} // namespace stfem
