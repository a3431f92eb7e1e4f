// CPU self-test of stfem_mapping_q1.h (the MappingQ1 geometry every kernel that maps a cell calls): exit status 0 = all checks hold.
// Affine cells with dyadic data: every comparison exact.  A trilinear cell: comparisons against an independent route in long double,
// within bounds derived below from the operation counts - never from what the code gives; the largest observed ratio to each bound is
// printed.  Built by `make test_mapping_q1` (host compiler only; HOSTFLAGS takes -fsanitize=address,undefined), run by
// tests/test_mapping_q1_cpu.py.
#include "stfem_mapping_q1.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++failures;                                \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
    }                                            \
  } while (0)

typedef long double ld;
static const double u = DBL_EPSILON / 2; // unit roundoff 2^-53

// ---- affine cells: all exact -----------------------------------------------------------------------------------------------------

// Lattice o + i e0 + j e1 + k e2 of 2 x 3 x 2 cells (different counts per direction: the vertex strides matter).  The edge vectors
// are the columns of JA: powers of two, sheared, det JA = -2, so every product and sum below is exact in double and the inverse,
// written down by hand, is dyadic too.
static const double JA[3][3] = {{-0.5, -0.5, 4.0}, {4.0, -1.0, -1.0}, {1.0, -0.5, 0.5}};
static const double JAI[3][3] = {{0.5, 0.875, -2.25}, {1.5, 2.125, -7.75}, {0.5, 0.375, -1.25}};
static const double OA[3] = {0.5, -1.0, 2.0};

static void test_affine()
{
  const int ncx = 2, ncy = 3, ncz = 2;
  std::vector<double> v;
  for (int k = 0; k <= ncz; ++k)
    for (int j = 0; j <= ncy; ++j)
      for (int i = 0; i <= ncx; ++i)
        for (int d = 0; d < 3; ++d) v.push_back(OA[d] + i * JA[d][0] + j * JA[d][1] + k * JA[d][2]);
  const double pts[4] = {0.0, 0.25, 0.5, 1.0};
  for (int cz = 0; cz < ncz; ++cz)
    for (int cy = 0; cy < ncy; ++cy)
      for (int cx = 0; cx < ncx; ++cx)
        for (int c = 0; c < 4; ++c)
          for (int b = 0; b < 4; ++b)
            for (int a = 0; a < 4; ++a) {
              const double xi[3] = {pts[a], pts[b], pts[c]};
              double J[3][3], Ji[3][3], Ji2[3][3], x[3];
              mapping_q1_jacobian(v.data(), ncx, ncy, cx, cy, cz, xi, J);
              const double det = mapping_q1_inverse(J, Ji);
              const double det2 = mapping_q1_inverse(v.data(), ncx, ncy, cx, cy, cz, xi, Ji2);
              CHECK(mapping_q1_det(J) == -2.0 && det == -2.0 && det2 == -2.0, "affine det %g %g %g", mapping_q1_det(J), det, det2);
              for (int d = 0; d < 3; ++d)
                for (int e = 0; e < 3; ++e) {
                  CHECK(J[d][e] == JA[d][e], "affine J[%d][%d] = %g, cell (%d, %d, %d)", d, e, J[d][e], cx, cy, cz);
                  CHECK(Ji[d][e] == JAI[d][e] && Ji2[d][e] == JAI[d][e], "affine Ji[%d][%d] = %g / %g", d, e, Ji[d][e], Ji2[d][e]);
                }
              mapping_q1_point(v.data(), ncx, ncy, cx, cy, cz, xi, x);
              const double g[3] = {cx + xi[0], cy + xi[1], cz + xi[2]};
              for (int d = 0; d < 3; ++d) {
                const double want = OA[d] + g[0] * JA[d][0] + g[1] * JA[d][1] + g[2] * JA[d][2]; // (exact: dyadic)
                CHECK(x[d] == want, "affine point x[%d] = %g, want %g", d, x[d], want);
              }
            }
}

// Axis-aligned box with power-of-two spacings: Ji = diag(1 / h), the normals of the six faces are +- e_d, len = 1 / h_d, all exact
static void test_box()
{
  const double h[3] = {0.5, 2.0, 0.25}, lo[3] = {-1.0, 0.5, 3.0};
  std::vector<double> v;
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 2; ++j)
      for (int i = 0; i < 2; ++i) {
        v.push_back(lo[0] + i * h[0]); v.push_back(lo[1] + j * h[1]); v.push_back(lo[2] + k * h[2]);
      }
  for (int f = 0; f < 6; ++f) {
    const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    double xi[3], Ji[3][3], nrm[3], unsgn[3];
    xi[d] = s; xi[t1] = 0.25; xi[t2] = 0.5;
    const double det = mapping_q1_inverse(v.data(), 1, 1, 0, 0, 0, xi, Ji);
    CHECK(det == h[0] * h[1] * h[2], "box det %g", det);
    const double len = mapping_q1_face_normal(Ji, d, s ? 1 : -1, nrm), len0 = mapping_q1_face_normal(Ji, d, 0, unsgn);
    CHECK(len == 1.0 / h[d] && len0 == len, "box face %d: len %g / %g, want %g", f, len, len0, 1.0 / h[d]);
    for (int k = 0; k < 3; ++k) {
      CHECK(nrm[k] == (k == d ? (s ? 1.0 : -1.0) : 0.0), "box face %d: nrm[%d] = %g", f, k, nrm[k]);
      CHECK(unsgn[k] == (k == d ? 1.0 : 0.0), "box face %d: unsigned nrm[%d] = %g", f, k, unsgn[k]);
    }
  }
}

// ---- a trilinear cell -------------------------------------------------------------------------------------------------------------

// The unit cube with every vertex moved by dyadic offsets (multiples of 1 / 64) of magnitude <= 9 / 64 < 0.15, the perturbation of the
// GPU tests.  The x offsets of the four vertices with i = 0 are 0: face 0 lies in the plane x = 0 (the area check).  Vertex i + 2 j + 4 k.
static const int OFF[8][3] = {{0, 5, -7}, {9, -4, 3}, {0, -8, 6}, {-6, 7, 9}, {0, 3, 8}, {-9, -5, -2}, {0, 9, -4}, {7, -3, 5}};
static const double VMAX = 1.0 + 9.0 / 64; // largest |coordinate|

static std::vector<double> trilinear_vertices()
{
  std::vector<double> v;
  for (int n = 0; n < 8; ++n) {
    const int ijk[3] = {n & 1, (n >> 1) & 1, n >> 2};
    for (int d = 0; d < 3; ++d) v.push_back(ijk[d] + OFF[n][d] / 64.0);
  }
  return v;
}

// The independent route: column e of J is the bilinear blend of the four edge vectors along direction e, in long double
static void reference_jacobian(const std::vector<double> &v, const double xi[3], ld J[3][3])
{
  for (int e = 0; e < 3; ++e) {
    const int t1 = e == 0 ? 1 : 0, t2 = e == 2 ? 1 : 2, st[3] = {1, 2, 4};
    for (int d = 0; d < 3; ++d) J[d][e] = 0;
    for (int b = 0; b < 2; ++b)
      for (int a = 0; a < 2; ++a) {
        const int n0 = a * st[t1] + b * st[t2], n1 = n0 + st[e];
        const ld w = (a ? (ld)xi[t1] : 1 - (ld)xi[t1]) * (b ? (ld)xi[t2] : 1 - (ld)xi[t2]);
        for (int d = 0; d < 3; ++d) J[d][e] += w * ((ld)v[3 * n1 + d] - (ld)v[3 * n0 + d]);
      }
  }
}

static double worst_J = 0, worst_I = 0, worst_n = 0, worst_s = 0, worst_a = 0; // largest observed error / bound

// The bounds.  With gamma_n = n u (first order; the neglected u^2 terms are covered by the factor 1.01 on every bound):
//  J:   an entry is a sum of 8 terms V * dd * f * f: dd = +-1 is exact, each f = 1 - xi or xi carries at most one rounding, the two
//       products one each, the eight additions at most 8 more: |J_hat - J| <= gamma_12 sum |V| f f <= 12 u * 2 VMAX =: bJ
//       (sum_{ijk} f_j f_k = 2).  The long double reference is 2^11 times more accurate; its error is added as bJ / 2048.
//  Ji:  a cofactor a b - c d has two rounded products and a rounded difference: error <= gamma_2 C, C = |a b| + |c d|.  det = sum of
//       three J_0i * cofactor_i: error <= gamma_5 P, P = sum |J_0i| C_i.  Ji = cofactor * (1 / det): two more roundings.  To first order
//       |Ji_hat - inverse(J_hat)| <= E := u (2 C / |det| + |Ji| (5 P / |det| + 2)), entry by entry; |Ji| is large where the cell is
//       distorted, C / |det| where the cofactor cancels.  Hence |J_hat Ji_hat - I| <= |J_hat| E (matrix product of the moduli).
//  Against the exact geometry the error of J_hat enters too: inverse(J + dJ) - inverse(J) = - Ji dJ Ji, so
//       |Ji_hat - inverse(J)| <= Et := E + bJ (row sums of |Ji|)(column sums of |Ji|)   and   |det_hat - det| <= 5 u P + bJ |det| sum |Ji|.
//  normal: m / |m| moves by at most 2 |dm|_2 / |m|_2 when m moves by dm (dm = row d of Et); len has 3 products, 2 additions, a root:
//       relative error <= 3 u, the division one more: |nrm_hat - n| <= 2 |Et_d|_2 / len + 4 u.
//  len |det| against the length of the cross product of the tangents (= |det| |J^-T e_d| exactly):
//       relative error <= |Et_d|_2 / len + 3 u + 5 u P / |det| + bJ sum |Ji| + u (the product).
// The bounds are evaluated with the J, Ji and det that the code under test returned: to first order that is the same bound (they differ
// from the exact ones by O(u) relative, which moves a bound of size O(u) by O(u^2)), and the identity and cross-product checks would
// expose a J or Ji wrong by more than that.
struct PointBounds {
  double E[3][3], Et[3][3], det_rel;
};
static PointBounds bounds_at(const double J[3][3], const double Ji[3][3], double det, double bJ)
{
  PointBounds B;
  auto C = [&](int r, int c) { // of the cofactor that gives Ji[r][c]: the minor without row c, column r of J
    const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
    return std::fabs(J[r1][c1] * J[r2][c2]) + std::fabs(J[r1][c2] * J[r2][c1]);
  };
  const double P = std::fabs(J[0][0]) * C(0, 0) + std::fabs(J[0][1]) * C(1, 0) + std::fabs(J[0][2]) * C(2, 0), ad = std::fabs(det);
  double row[3] = {0, 0, 0}, col[3] = {0, 0, 0}, all = 0;
  for (int e = 0; e < 3; ++e)
    for (int d = 0; d < 3; ++d) { row[e] += std::fabs(Ji[e][d]); col[d] += std::fabs(Ji[e][d]); all += std::fabs(Ji[e][d]); }
  for (int e = 0; e < 3; ++e)
    for (int d = 0; d < 3; ++d) {
      B.E[e][d] = 1.01 * u * (2 * C(e, d) / ad + std::fabs(Ji[e][d]) * (5 * P / ad + 2));
      B.Et[e][d] = B.E[e][d] + 1.01 * bJ * row[e] * col[d];
    }
  B.det_rel = 1.01 * (5 * u * P / ad + bJ * all);
  return B;
}

static void note(double &worst, double err, double bound, const char *what, int f, int q)
{
  worst = std::max(worst, err / bound);
  CHECK(err <= bound, "%s, face %d point %d: error %.3e > bound %.3e", what, f, q, err, bound);
}

static void test_trilinear()
{
  const std::vector<double> v = trilinear_vertices();
  const double bJ = 12 * u * 2 * VMAX * (1 + 1.0 / 2048);
  const double gx[3] = {0.5 - 0.5 * std::sqrt(0.6), 0.5, 0.5 + 0.5 * std::sqrt(0.6)}, gw[3] = {5.0 / 18, 8.0 / 18, 5.0 / 18};
  // the corners map onto the vertices exactly (weights 0 and 1)
  for (int n = 0; n < 8; ++n) {
    const double xi[3] = {double(n & 1), double((n >> 1) & 1), double(n >> 2)};
    double x[3];
    mapping_q1_point(v.data(), 1, 1, 0, 0, 0, xi, x);
    for (int d = 0; d < 3; ++d) CHECK(x[d] == v[3 * n + d], "corner %d: x[%d] = %g", n, d, x[d]);
  }
  ld centre[3] = {0, 0, 0};
  for (int n = 0; n < 8; ++n)
    for (int d = 0; d < 3; ++d) centre[d] += (ld)v[3 * n + d] / 8;
  for (int f = 0; f < 6; ++f) {
    const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    double area = 0.0, area_rel = 0.0;
    for (int q = 0; q < 9; ++q) {
      const int q1 = q % 3, q2 = q / 3;
      double xi[3], J[3][3], Ji[3][3], nrm[3], x[3];
      xi[d] = s; xi[t1] = gx[q1]; xi[t2] = gx[q2];
      mapping_q1_jacobian(v.data(), 1, 1, 0, 0, 0, xi, J);
      const double det = mapping_q1_inverse(J, Ji);
      const double len = mapping_q1_face_normal(Ji, d, s ? 1 : -1, nrm);
      const PointBounds B = bounds_at(J, Ji, det, bJ);
      ld Jr[3][3];
      reference_jacobian(v, xi, Jr);
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          note(worst_J, (double)fabsl((ld)J[a][b] - Jr[a][b]), bJ, "J against the blend of the edge vectors", f, q);
          ld p = 0;
          double bound = 0.0;
          for (int e = 0; e < 3; ++e) { p += (ld)J[a][e] * (ld)Ji[e][b]; bound += std::fabs(J[a][e]) * B.E[e][b]; }
          note(worst_I, (double)fabsl(p - (a == b ? 1 : 0)), bound, "J Ji against the identity", f, q);
        }
      // the outward unit normal from the tangents: their cross product, turned away from the cell's centre
      ld cr[3] = {Jr[1][t1] * Jr[2][t2] - Jr[2][t1] * Jr[1][t2], Jr[2][t1] * Jr[0][t2] - Jr[0][t1] * Jr[2][t2],
                  Jr[0][t1] * Jr[1][t2] - Jr[1][t1] * Jr[0][t2]};
      const ld cl = sqrtl(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
      mapping_q1_point(v.data(), 1, 1, 0, 0, 0, xi, x);
      const ld out = cr[0] * (x[0] - centre[0]) + cr[1] * (x[1] - centre[1]) + cr[2] * (x[2] - centre[2]);
      const double e2 = std::sqrt(B.Et[d][0] * B.Et[d][0] + B.Et[d][1] * B.Et[d][1] + B.Et[d][2] * B.Et[d][2]);
      for (int k = 0; k < 3; ++k)
        note(worst_n, (double)fabsl((ld)nrm[k] - (out > 0 ? cr[k] : -cr[k]) / cl), 1.01 * (2 * e2 / len + 4 * u),
             "normal against the cross product", f, q);
      const double surf_rel = 1.01 * (e2 / len + 4 * u) + B.det_rel;
      note(worst_s, (double)fabsl((ld)len * fabsl((ld)det) - cl), surf_rel * (double)cl, "len |det| against the cross product's length", f, q);
      area += std::fabs(det) * len * gw[q1] * gw[q2];
      area_rel = std::max(area_rel, surf_rel);
    }
    if (f == 0) {
      // Face 0 is planar (x = 0), a convex quadrilateral: its surface element is bilinear in the face coordinates, which the 3 x 3 Gauss
      // rule integrates exactly.  Area from the corners: half the cross product of the diagonals (shoelace formula).  Each of the nine
      // terms carries its surface element's bound, the rounding of its two weights (2 u), of the two products with them (2 u) and of
      // at most 8 additions (8 u); the rounding of the Gauss points (2 u of xi) moves a bilinear integrand of slope <= 2 |value| by 4 u.
      const double *a = &v[0], *b = &v[3 * 2], *c = &v[3 * 6], *e = &v[3 * 4]; // (j, k) = (0, 0), (1, 0), (1, 1), (0, 1)
      const ld want = fabsl(((ld)c[1] - a[1]) * ((ld)e[2] - b[2]) - ((ld)e[1] - b[1]) * ((ld)c[2] - a[2])) / 2;
      const double bound = 1.01 * (area_rel + 16 * u) * (double)want;
      worst_a = std::max(worst_a, (double)fabsl((ld)area - want) / bound);
      CHECK(fabsl((ld)area - want) <= bound, "area of the planar face: %.17g, want %.17Lg, bound %.3e", area, want, bound);
    }
  }
}

int main()
{
  test_affine();
  test_box();
  test_trilinear();
  printf("largest error / bound: J %.3f, J Ji - I %.3f, normal %.3f, len |det| %.3f, planar face area %.3f\n", worst_J, worst_I, worst_n,
         worst_s, worst_a);
  if (failures == 0) printf("stfem_mapping_q1.h: all checks hold\n");
  return failures == 0 ? 0 : 1;
}
