// CPU self-test of the index helpers of the one-block-per-cell Stokes smoother in stfem_vanka_setup.h (the cell's DoFs and the cells
// that share them, rows of the block, distinct linearisation states): exit status 0 = all checks hold.  Built by
// `make test_stokes_vanka_setup` (host compiler only; HOSTFLAGS takes -fsanitize=address,undefined), run by
// tests/test_stokes_vanka_setup_cpu.py.
#include "stfem_vanka_setup.h"

#include <cstdio>

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

// global number of cell DoF k of cell (cx, cy, cz) on a mesh of nc cells: velocity component-major on the (2 nc + 1)^3 lattice, then
// the pressure: vertices of the (nc + 1)^3 lattice, or four functions per cell
static long long global_dof(const int nc[3], bool pdg, const int c[3], int k)
{
  const long long Nu = (long long)(2 * nc[0] + 1) * (2 * nc[1] + 1) * (2 * nc[2] + 1);
  if (k < 81) {
    const int comp = k / 27, n = k % 27;
    return comp * Nu + (2 * c[0] + n % 3) + (long long)(2 * nc[0] + 1) * ((2 * c[1] + (n / 3) % 3) + (long long)(2 * nc[1] + 1) * (2 * c[2] + n / 9));
  }
  const int l = k - 81;
  if (pdg) return 3 * Nu + 4ll * (c[0] + nc[0] * (c[1] + nc[1] * c[2])) + l;
  return 3 * Nu + (c[0] + (l & 1)) + (long long)(nc[0] + 1) * ((c[1] + ((l >> 1) & 1)) + (long long)(nc[1] + 1) * (c[2] + (l >> 2)));
}

// the neighbour table against the global numbering: DoF k of the middle cell of a 3 x 3 x 3 mesh is DoF nbr[k][s] of the cell at shift
// s, and of no other DoF of that cell; -1 exactly where the cell does not hold it
static void test_neighbour_table(bool pdg)
{
  const vanka::CellDofTables t = vanka::stokes_cell_dof_tables(pdg);
  const int nl = 81 + (pdg ? 4 : 8);
  CHECK(t.nl == nl && int(t.nbr.size()) == nl * 27 && int(t.face.size()) == nl, "sizes (pdg %d)", int(pdg));
  if (t.nl != nl) return;
  const int nc[3] = {3, 3, 3}, mid[3] = {1, 1, 1};
  for (int k = 0; k < nl; ++k) {
    const long long g = global_dof(nc, pdg, mid, k);
    int valence = 0;
    for (int s = 0; s < 27; ++s) {
      const int c[3] = {1 + s % 3 - 1, 1 + (s / 3) % 3 - 1, 1 + s / 9 - 1};
      int found = -1, count = 0;
      for (int k2 = 0; k2 < nl; ++k2)
        if (global_dof(nc, pdg, c, k2) == g) { found = k2; ++count; }
      CHECK(count <= 1, "DoF %d twice in the cell at shift %d", k, s);
      CHECK(t.nbr[size_t(k) * 27 + s] == found, "pdg %d DoF %d shift %d: table %d, numbering %d", int(pdg), k, s, t.nbr[size_t(k) * 27 + s], found);
      if (found >= 0) ++valence;
    }
    CHECK(t.nbr[size_t(k) * 27 + 13] == k, "DoF %d is not itself in its own cell", k);
    // valence of the numbering: velocity 1 / 2 / 4 / 8 by the faces the node lies on, vertices 8, cell functions 1
    int faces = 0;
    for (int b = 0; b < 6; ++b) faces += t.face[k] >> b & 1;
    const int want = k < 81 ? 1 << faces : (pdg ? 1 : 8);
    CHECK(valence == want, "pdg %d DoF %d: valence %d, expected %d", int(pdg), k, valence, want);
    if (k >= 81) CHECK(t.face[k] == 0, "pressure DoF %d carries face bits", k);
    else {
      const int n = k % 27, idx[3] = {n % 3, (n / 3) % 3, n / 9};
      for (int d = 0; d < 3; ++d) {
        CHECK((t.face[k] >> (2 * d) & 1) == (idx[d] == 0), "velocity DoF %d, lower face of direction %d", k, d);
        CHECK((t.face[k] >> (2 * d + 1) & 1) == (idx[d] == 2), "velocity DoF %d, upper face of direction %d", k, d);
      }
    }
  }
}

static void test_row_dofs()
{
  const int var[5] = {0, 1, 1, 0, 1};
  for (int npl : {4, 8}) {
    std::vector<int> blk, dof;
    vanka::stokes_row_dofs(5, var, npl, blk, dof);
    const int m = 2 * 81 + 3 * npl;
    CHECK(int(blk.size()) == m && int(dof.size()) == m, "row count %zu, expected %d", blk.size(), m);
    int r = 0;
    for (int i = 0; i < 5; ++i)
      for (int k = 0; k < (var[i] ? npl : 81); ++k, ++r) {
        if (r >= int(blk.size())) return;
        CHECK(blk[r] == i && dof[r] == (var[i] ? 81 + k : k), "row %d: block %d DoF %d", r, blk[r], dof[r]);
      }
  }
}

static void test_distinct_states()
{
  const double a[1] = {0}, b[1] = {0}, c[1] = {0};
  { // time-major cG(2): velocity blocks 0 and 2 with two states
    const int var[4] = {0, 1, 0, 1};
    const double *lin[4] = {a, nullptr, b, nullptr}, *state[8];
    int sel[4];
    CHECK(vanka::distinct_states(4, var, lin, sel, state) == 2, "two states");
    CHECK(sel[0] == 0 && sel[2] == 1 && sel[1] == 0 && sel[3] == 0 && state[0] == a && state[1] == b, "their order");
  }
  { // equal pointers are one state; a pressure entry is never read
    const int var[6] = {0, 0, 0, 1, 1, 1};
    const double *lin[6] = {c, a, c, b, b, b}, *state[8];
    int sel[6];
    CHECK(vanka::distinct_states(6, var, lin, sel, state) == 2, "equal pointers once");
    CHECK(sel[0] == 0 && sel[1] == 1 && sel[2] == 0 && state[0] == c && state[1] == a, "selection of equal pointers");
  }
  { // no linearisation: one state, the null one
    const int var[2] = {0, 1};
    const double *state[8];
    int sel[2] = {7, 7};
    CHECK(vanka::distinct_states(2, var, nullptr, sel, state) == 1 && state[0] == nullptr && sel[0] == 0 && sel[1] == 0, "mode 0");
  }
  { // eight velocity blocks, all different: the arrays of VK_MAX_BLOCKS entries are filled to the end and no further
    int var[8];
    double v[8];
    const double *lin[8], *state[8];
    int sel[8];
    for (int i = 0; i < 8; ++i) { var[i] = 0; lin[i] = &v[i]; }
    CHECK(vanka::distinct_states(8, var, lin, sel, state) == 8, "eight states");
    for (int i = 0; i < 8; ++i) CHECK(sel[i] == i && state[i] == &v[i], "state %d", i);
  }
}

int main()
{
  test_neighbour_table(false);
  test_neighbour_table(true);
  test_row_dofs();
  test_distinct_states();
  if (failures) printf("%d check(s) failed\n", failures);
  else printf("stokes vanka setup: all checks hold\n");
  return failures ? 1 : 0;
}
