// CPU self-test of stfem_vanka_setup.h, the host set-up steps of the cell-patch smoothers: exit status 0 = all checks hold.
// Built by `make test_vanka_setup` (host compiler only), run by tests/test_vanka_setup_cpu.py.
#include "stfem_vanka_setup.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>

namespace vanka = stfem::vanka;

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

// uniform numbers in [-1, 1] from a fixed seed (splitmix64)
struct Rng {
  uint64_t s;
  double next()
  {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return double(z >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  }
};

static double inverse_defect(int n, const std::vector<double> &A, const std::vector<double> &Ai) // max |A Ai - I|
{
  double worst = 0.0;
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += A[size_t(r) * n + k] * Ai[size_t(k) * n + c];
      worst = std::max(worst, std::abs(s - (r == c ? 1.0 : 0.0)));
    }
  return worst;
}

static void test_inverse()
{
  Rng rng{2024};
  for (int n : {1, 2, 17, 89}) {
    std::vector<double> A(size_t(n) * n);
    for (double &a : A) a = rng.next();
    for (int i = 0; i < n; ++i) A[size_t(i) * n + i] += n;
    std::vector<double> Ai = A;
    CHECK(vanka::invert(n, Ai), "n = %d reported singular", n);
    const double defect = inverse_defect(n, A, Ai);
    CHECK(defect <= 1e-10, "n = %d: max |A A^-1 - I| = %.3e", n, defect);
  }
  { // a zero in the leading diagonal entry: rows must be exchanged
    const std::vector<double> A = {0.0, 2.0, 1.0, 1.0, 1.0, 0.0, 3.0, 0.0, 1.0};
    std::vector<double> Ai = A;
    CHECK(vanka::invert(3, Ai), "row exchange: reported singular");
    const double defect = inverse_defect(3, A, Ai);
    CHECK(defect <= 1e-13, "row exchange: max |A A^-1 - I| = %.3e", defect);
  }
  {
    std::vector<double> A = {1.0, 0.0, 2.0, 3.0, 0.0, 4.0, 5.0, 0.0, 7.0};
    CHECK(!vanka::invert(3, A), "an all-zero column was inverted");
    std::vector<double> N = {1.0, 2.0, 3.0, std::numeric_limits<double>::quiet_NaN()};
    CHECK(!vanka::invert(2, N), "a NaN entry was inverted");
    std::vector<double> N1 = {std::numeric_limits<double>::quiet_NaN()};
    CHECK(!vanka::invert(1, N1), "a NaN pivot was inverted");
  }
}

static void test_class_table()
{
  const int meshes[4][3] = {{1, 1, 1}, {2, 1, 4}, {3, 3, 3}, {5, 4, 3}};
  for (const auto &nc : meshes) {
    const vanka::ClassTable t = vanka::class_table(nc, 0);
    const size_t want = size_t(std::min(nc[0], 3)) * std::min(nc[1], 3) * std::min(nc[2], 3);
    CHECK(t.key.size() == want, "(%d, %d, %d): %zu classes, expected %zu", nc[0], nc[1], nc[2], t.key.size(), want);
    CHECK(t.cls.size() == size_t(nc[0]) * nc[1] * nc[2] && t.local.size() == t.cls.size(), "(%d, %d, %d): table sizes", nc[0], nc[1], nc[2]);
    // first-seen z, y, x order: cell by cell, a class index is either known or the next new one; no neighbour mask: key == local
    int seen = 0;
    for (size_t cell = 0; cell < t.cls.size(); ++cell) {
      CHECK(t.cls[cell] <= seen, "(%d, %d, %d): class %d of cell %zu before class %d", nc[0], nc[1], nc[2], t.cls[cell], cell, seen);
      if (t.cls[cell] == seen) ++seen;
      CHECK(t.key[t.cls[cell]] == t.local[cell], "(%d, %d, %d): key of cell %zu", nc[0], nc[1], nc[2], cell);
    }
  }
  { // the explicit order on a 3 x 3 x 3 mesh: x fastest, bits (lower, upper) = 2 (first cell), 3 (middle), 1 (last)
    const int nc[3] = {3, 3, 3}, bits[3] = {2, 3, 1};
    const vanka::ClassTable t = vanka::class_table(nc, 0);
    for (int i = 0; i < 27 && t.key.size() == 27; ++i)
      CHECK(t.key[i] == (bits[i % 3] | (bits[(i / 3) % 3] << 2) | (bits[i / 9] << 4)), "key %d of (3, 3, 3) = %d", i, t.key[i]);
  }
  { // a slab with neighbour ranks below and above: its single z layer is an interior layer
    const int nc[3] = {3, 3, 1}, full[3] = {3, 3, 3};
    const vanka::ClassTable t = vanka::class_table(nc, 16 | 32), f = vanka::class_table(full, 0);
    CHECK(t.key.size() == 9, "(3, 3, 1) with mask 48: %zu classes", t.key.size());
    for (int cell = 0; cell < 9 && t.cls.size() == 9; ++cell) {
      CHECK(t.key[t.cls[cell]] == f.key[f.cls[9 + cell]], "cell %d of the slab: key %d, interior layer %d", cell, t.key[t.cls[cell]], f.key[f.cls[9 + cell]]);
      CHECK((t.local[cell] >> 4) == 0, "cell %d of the slab: local z pattern %d", cell, t.local[cell] >> 4);
    }
  }
}

static void test_cell_lists()
{
  const int meshes[3][3] = {{2, 1, 4}, {5, 4, 3}, {9, 9, 9}};
  for (const auto &nc : meshes) {
    const vanka::ClassTable t = vanka::class_table(nc, 0);
    const size_t ncells = t.cls.size();
    const vanka::CellList l = vanka::cell_list(t, -1);
    CHECK(l.order.size() % 64 == 0 && l.cls.size() == l.order.size() / 64, "flat list: %zu entries, %zu quads", l.order.size(), l.cls.size());
    // every class starts on a multiple of 64, classes ascend, cls[q] is the class of every real cell of quad q
    for (size_t q = 0; q < l.cls.size(); ++q) {
      CHECK(q == 0 || l.cls[q] >= l.cls[q - 1], "flat list: class %d after %d", l.cls[q], q ? l.cls[q - 1] : 0);
      if (q == 0 || l.cls[q] != l.cls[q - 1]) CHECK(l.order[64 * q] >= 0, "flat list: class %d starts with padding", l.cls[q]);
      for (int e = 0; e < 64; ++e)
        if (l.order[64 * q + e] >= 0) CHECK(t.cls[l.order[64 * q + e]] == l.cls[q], "flat list: quad %zu holds a cell of class %d", q, t.cls[l.order[64 * q + e]]);
    }
    std::vector<int> quads_of(t.key.size(), 0), cells_of(t.key.size(), 0);
    for (int c : l.cls) ++quads_of[c];
    for (int c : t.cls) ++cells_of[c];
    for (size_t c = 0; c < t.key.size(); ++c) CHECK(quads_of[c] == (cells_of[c] + 63) / 64, "flat list: class %zu has %d quads for %d cells", c, quads_of[c], cells_of[c]);
    // slot: injective, onto the non-padding entries
    CHECK(l.slot.size() == ncells, "flat list: slot table of %zu entries", l.slot.size());
    std::vector<char> used(l.order.size(), 0);
    for (size_t cell = 0; cell < ncells && l.slot.size() == ncells; ++cell) {
      const int s = l.slot[cell];
      CHECK(s >= 0 && size_t(s) < l.order.size() && l.order[s] == int(cell) && !used[s], "flat list: slot %d of cell %zu", s, cell);
      if (s >= 0 && size_t(s) < used.size()) used[s] = 1;
    }
    // what the kernels read: the cells' first DoFs in list order, the pad value elsewhere
    std::vector<int> first(ncells);
    for (size_t cell = 0; cell < ncells; ++cell) first[cell] = 1000 + 7 * int(cell);
    const std::vector<int> g = vanka::gather_cells(l.order, first, -1);
    for (size_t i = 0; i < g.size(); ++i) CHECK(g[i] == (l.order[i] < 0 ? -1 : first[l.order[i]]), "gather_cells: entry %zu", i);
    // the colour lists: every cell exactly once, in its colour, grouped by (class, local pattern)
    std::vector<int> count(ncells, 0);
    for (int colour = 0; colour < 8; ++colour) {
      const vanka::CellList cl = vanka::cell_list(t, colour);
      CHECK(cl.order.size() % 64 == 0 && cl.cls.size() == cl.order.size() / 64 && cl.slot.empty(), "colour %d: list sizes", colour);
      for (size_t i = 0; i < cl.order.size(); ++i) {
        const int cell = cl.order[i];
        if (cell < 0) continue;
        ++count[cell];
        const int cx = cell % nc[0], cy = (cell / nc[0]) % nc[1], cz = cell / (nc[0] * nc[1]);
        CHECK((cx & 1) + 2 * (cy & 1) + 4 * (cz & 1) == colour, "colour %d holds cell %d", colour, cell);
        CHECK(cl.cls[i / 64] == (t.cls[cell] | (t.local[cell] << 8)), "colour %d: quad %zu, cell %d", colour, i / 64, cell);
      }
    }
    for (size_t cell = 0; cell < ncells; ++cell) CHECK(count[cell] == 1, "cell %zu is in %d colour lists", cell, count[cell]);
  }
}

// (mtw, parts) for 1 .. 32 row tiles, recorded from the plans before they moved into the header
static const int PLAN64[32][2] = {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {1, 5}, {6, 1}, {1, 7}, {4, 2}, {3, 3}, {2, 5}, {4, 3}, {4, 3}, {1, 13}, {2, 7}, {4, 4}, {4, 4},
                                  {6, 3}, {6, 3}, {4, 5}, {4, 5}, {3, 7}, {4, 6}, {4, 6}, {4, 6}, {1, 25}, {4, 7}, {4, 7}, {4, 7}, {6, 5}, {6, 5}, {4, 8}, {4, 8}};
static const int PLAN32[32][2] = {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {1, 5}, {6, 1}, {1, 7}, {8, 1}, {3, 3}, {2, 5}, {4, 3}, {4, 3}, {1, 13}, {2, 7}, {8, 2}, {8, 2},
                                  {6, 3}, {6, 3}, {4, 5}, {4, 5}, {3, 7}, {8, 3}, {8, 3}, {8, 3}, {1, 25}, {4, 7}, {4, 7}, {4, 7}, {6, 5}, {6, 5}, {8, 4}, {8, 4}};
static const int PLAN_STOKES[32][2] = {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {1, 5}, {3, 2}, {1, 7}, {4, 2}, {3, 3}, {2, 5}, {1, 11}, {4, 3}, {1, 13}, {2, 7}, {3, 5}, {4, 4},
                                       {1, 17}, {3, 6}, {1, 19}, {4, 5}, {3, 7}, {2, 11}, {1, 23}, {4, 6}, {1, 25}, {2, 13}, {3, 9}, {4, 7}, {1, 29}, {3, 10}, {1, 31}, {4, 8}};

static void test_tile_plans()
{
  unsetenv("STFEM_VANKA_TILES");
  for (int tiles = 1; tiles <= 32; ++tiles) {
    const vanka::TilePlan d = vanka::scalar_tile_plan(tiles, false), f = vanka::scalar_tile_plan(tiles, true), s = vanka::stokes_tile_plan(tiles);
    CHECK(d.mtw == PLAN64[tiles - 1][0] && d.parts == PLAN64[tiles - 1][1], "fp64, %d tiles: (%d, %d)", tiles, d.mtw, d.parts);
    CHECK(f.mtw == PLAN32[tiles - 1][0] && f.parts == PLAN32[tiles - 1][1], "fp32, %d tiles: (%d, %d)", tiles, f.mtw, f.parts);
    CHECK(s.mtw == PLAN_STOKES[tiles - 1][0] && s.parts == PLAN_STOKES[tiles - 1][1], "Stokes, %d tiles: (%d, %d)", tiles, s.mtw, s.parts);
  }
}

// two blocks over three nodes, node 1 constrained, valences (2, 1, 4)
template <typename T> static void test_finish_block(double tol)
{
  const int nb = 2, nloc = 3, m = 6, mpad = 16, kpad = 8;
  const std::vector<double> K = {4.0, -1.0, 0.5, -1.0, 5.0, -2.0, 0.5, -2.0, 6.0}, M = {2.0, 0.5, 0.25, 0.5, 3.0, 0.75, 0.25, 0.75, 1.5};
  const double Alpha[4] = {0.5, -0.25, 0.125, 1.0}, Beta[4] = {1.0, 0.5, -0.5, 2.0};
  const std::vector<int> dof = {0, 1, 2, 0, 1, 2};
  const std::vector<char> con = {0, 1, 0};
  const std::vector<double> val = {2.0, 1.0, 4.0};
  std::vector<double> B;
  vanka::combine_scalar(nb, nloc, Alpha, Beta, K, M, B);
  CHECK(B.size() == size_t(m) * m && B[size_t(1) * m + 5] == Beta[1] * M[1 * 3 + 2] + Alpha[1] * K[1 * 3 + 2], "combine_scalar");
  // the same steps written out: constrain, scale the rows
  std::vector<double> want = B;
  for (int r = 0; r < m; ++r)
    for (int s = 0; s < m; ++s) {
      if (r % nloc != s % nloc && (r % nloc == 1 || s % nloc == 1)) want[size_t(r) * m + s] = 0.0;
      want[size_t(r) * m + s] *= val[r % nloc];
    }
  std::vector<T> out(size_t(kpad) * mpad, T(-7));
  CHECK(vanka::finish_block(m, B, dof, con, val, out.data(), mpad, kpad), "finish_block reported singular");
  std::vector<double> inv(size_t(m) * m);
  for (int k = 0; k < kpad; ++k)
    for (int r = 0; r < mpad; ++r) {
      const T e = out[size_t(k) * mpad + r];
      if (k >= m || r >= m) CHECK(e == T(0), "padding entry [%d][%d] = %g", k, r, double(e));
      else {
        inv[size_t(r) * m + k] = double(e); // stored transposed
        if (r % nloc != k % nloc && (r % nloc == 1 || k % nloc == 1)) CHECK(e == T(0), "constrained entry (%d, %d) = %g", r, k, double(e));
      }
    }
  const double defect = inverse_defect(m, want, inv);
  CHECK(defect <= tol, "finish_block: max |B B^-1 - I| = %.3e", defect);
  CHECK(inv[size_t(1) * m + 1] != 0.0 && inv[size_t(4) * m + 4] != 0.0, "the diagonal of the constrained node is gone");
  std::vector<double> Z(size_t(m) * m, 0.0);
  CHECK(!vanka::finish_block(m, Z, dof, con, val, out.data(), mpad, kpad), "a zero block was inverted");
}

static void test_combine_two_variable()
{
  // blocks (u, p, u) with nu = 2 first-variable DoFs of nl = 3; Beta only couples the u blocks, zero Alpha entries are skipped
  const int var[3] = {0, 1, 0}, rowbase[3] = {0, 2, 3}, m = 5;
  const std::vector<double> A = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0}, Mu = {10.0, 20.0, 30.0, 40.0};
  const double Alpha[9] = {1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 2.0, 0.0, 1.0}, Beta[9] = {1.0, 5.0, 0.5, 5.0, 5.0, 5.0, 0.0, 5.0, 1.0};
  std::vector<double> B;
  vanka::combine_two_variable(3, var, rowbase, m, 2, 3, Alpha, Beta, A, Mu, B);
  const double want[25] = {11.0, 22.0, 3.0, 5.0, 10.0, 34.0, 45.0, 6.0, 15.0, 20.0, 7.0, 8.0, 9.0, 7.0, 8.0, 2.0, 4.0, 0.0, 11.0, 22.0, 8.0, 10.0, 0.0, 34.0, 45.0};
  for (int i = 0; i < 25; ++i) CHECK(B[i] == want[i], "combine_two_variable: entry (%d, %d) = %g, expected %g", i / 5, i % 5, B[i], want[i]);
}

int main()
{
  test_inverse();
  test_class_table();
  test_cell_lists();
  test_tile_plans();
  // defect <= eps * sum_k |B(r, k)| |B^-1(k, c)| * growth: 6 terms of at most 40 * 1; eps = 1.1e-16 (a factor 100 for the
  // elimination) and 6e-8 (the stored inverse rounded to fp32)
  test_finish_block<double>(1e-12);
  test_finish_block<float>(1e-4);
  test_combine_two_variable();
  if (failures) printf("%d checks failed\n", failures);
  else printf("stfem_vanka_setup.h: all checks passed\n");
  return failures ? 1 : 0;
}
