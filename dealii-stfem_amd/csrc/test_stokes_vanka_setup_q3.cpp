// CPU self-test of the index helpers of the one-block-per-cell Stokes smoother at velocity degree 3 in stfem_vanka_setup.h (the cell's
// 192 + 27 / 10 DoFs and the cells that share them, the faces they lie on, rows of the block, the apply's row table) against a
// brute-force enumeration of the global numbering on a 3 x 3 x 3 patch: exit status 0 = all checks hold.  Built by
// `make test_stokes_vanka_setup_q3` (host compiler only; HOSTFLAGS takes -fsanitize=address,undefined), run by
// tests/test_stokes_vanka_setup_q3_cpu.py.  The degree-2 tables stay with test_stokes_vanka_setup.cpp; one check here holds the
// generalised functions to their defaults.
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

// global number of cell DoF k of cell (cx, cy, cz) on a mesh of nc cells: velocity component-major on the (3 nc + 1)^3 lattice, then
// the pressure: nodes of the (2 nc + 1)^3 lattice, or ten functions per cell
static long long global_dof(const int nc[3], bool pdg, const int c[3], int k)
{
  const long long ndx = 3 * nc[0] + 1, ndy = 3 * nc[1] + 1, ndz = 3 * nc[2] + 1, Nu = ndx * ndy * ndz;
  if (k < 192) {
    const int comp = k / 64, n = k % 64;
    return comp * Nu + (3 * c[0] + n % 4) + ndx * ((3 * c[1] + (n / 4) % 4) + ndy * (3 * c[2] + n / 16));
  }
  const int l = k - 192;
  if (pdg) return 3 * Nu + 10ll * (c[0] + nc[0] * (c[1] + nc[1] * c[2])) + l;
  return 3 * Nu + (2 * c[0] + l % 3) + (long long)(2 * nc[0] + 1) * ((2 * c[1] + (l / 3) % 3) + (long long)(2 * nc[1] + 1) * (2 * c[2] + l / 9));
}

// the neighbour table against the global numbering: DoF k of the middle cell of a 3 x 3 x 3 mesh is DoF nbr[k][s] of the cell at shift
// s, and of no other DoF of that cell; -1 exactly where the cell does not hold it
static void test_neighbour_table(bool pdg)
{
  const vanka::CellDofTables t = vanka::stokes_cell_dof_tables(pdg, 3);
  const int npl = pdg ? 10 : 27, nl = 192 + npl;
  CHECK(vanka::stokes_cell_velocity_dofs(3) == 192 && vanka::stokes_cell_pressure_dofs(3, pdg) == npl, "cell DoF counts (pdg %d)", int(pdg));
  CHECK(t.nl == nl && int(t.nbr.size()) == nl * 27 && int(t.face.size()) == nl, "sizes (pdg %d)", int(pdg));
  if (t.nl != nl) return;
  const int nc[3] = {3, 3, 3}, mid[3] = {1, 1, 1};
  for (int k = 0; k < nl; ++k) {
    const long long g = global_dof(nc, pdg, mid, k);
    int valence = 0;
    for (int s = 0; s < 27; ++s) {
      const int c[3] = {s % 3, (s / 3) % 3, s / 9};
      int found = -1, count = 0;
      for (int k2 = 0; k2 < nl; ++k2)
        if (global_dof(nc, pdg, c, k2) == g) { found = k2; ++count; }
      CHECK(count <= 1, "DoF %d twice in the cell at shift %d", k, s);
      CHECK(t.nbr[size_t(k) * 27 + s] == found, "pdg %d DoF %d shift %d: table %d, numbering %d", int(pdg), k, s, t.nbr[size_t(k) * 27 + s], found);
      if (found >= 0) ++valence;
    }
    CHECK(t.nbr[size_t(k) * 27 + 13] == k, "DoF %d is not itself in its own cell", k);
    if (k < 192) { // velocity: 1 / 2 / 4 / 8 cells by the faces the node lies on
      int faces = 0;
      for (int b = 0; b < 6; ++b) faces += t.face[k] >> b & 1;
      CHECK(valence == 1 << faces, "pdg %d velocity DoF %d: valence %d with %d faces", int(pdg), k, valence, faces);
      const int n = k % 64, idx[3] = {n % 4, (n / 4) % 4, n / 16};
      for (int d = 0; d < 3; ++d) {
        CHECK((t.face[k] >> (2 * d) & 1) == (idx[d] == 0), "velocity DoF %d, lower face of direction %d", k, d);
        CHECK((t.face[k] >> (2 * d + 1) & 1) == (idx[d] == 3), "velocity DoF %d, upper face of direction %d", k, d);
      }
    } else { // FE_Q(2) pressure: by the faces of the 3^3 node lattice; cell functions: the cell alone
      CHECK(t.face[k] == 0, "pressure DoF %d carries face bits", k);
      const int l = k - 192, idx[3] = {l % 3, (l / 3) % 3, l / 9};
      int want = 1;
      for (int d = 0; d < 3 && !pdg; ++d)
        if (idx[d] != 1) want *= 2;
      CHECK(valence == want, "pdg %d pressure DoF %d: valence %d, expected %d", int(pdg), k, valence, want);
    }
  }
}

// rows of the block and the apply's row table: row r of a block layout reads the global DoF that the brute-force numbering gives for
// (block, cell DoF) of every cell of a 2 x 3 x 2 mesh
static void test_rows(bool pdg)
{
  const int var[4] = {0, 1, 1, 0}, npl = pdg ? 10 : 27;
  std::vector<int> rowblk, rowdof;
  vanka::stokes_row_dofs(4, var, npl, rowblk, rowdof, 192);
  const int m = 2 * 192 + 2 * npl;
  CHECK(int(rowblk.size()) == m && int(rowdof.size()) == m, "row count %zu, expected %d", rowblk.size(), m);
  if (int(rowblk.size()) != m) return;
  int rowbase[4], at = 0;
  for (int i = 0; i < 4; ++i) { rowbase[i] = at; at += var[i] ? npl : 192; }
  for (int r = 0; r < m; ++r) {
    int i = 3;
    while (rowbase[i] > r) --i;
    CHECK(rowblk[r] == i, "row %d: block %d, expected %d", r, rowblk[r], i);
    CHECK(rowdof[r] == (var[i] ? 192 : 0) + r - rowbase[i], "row %d: cell DoF %d", r, rowdof[r]);
  }
  const int nc[3] = {2, 3, 2}, ndu[3] = {7, 10, 7}, ndp[3] = {5, 7, 5};
  const long long Nu = 7ll * 10 * 7;
  std::vector<int> xy;
  CHECK(vanka::stokes_row_table(3, pdg, 4, var, rowbase, Nu, ndu, ndp, xy), "row table refused");
  CHECK(int(xy.size()) == 2 * m, "row table size %zu", xy.size());
  if (int(xy.size()) != 2 * m) return;
  for (int cz = 0; cz < nc[2]; ++cz)
    for (int cy = 0; cy < nc[1]; ++cy)
      for (int cx = 0; cx < nc[0]; ++cx) {
        const int c[3] = {cx, cy, cz};
        // the cell's first DoF of each variable, as the apply and the collecting launch compute it
        const long long firstu = 3 * cx + (long long)ndu[0] * (3 * cy + (long long)ndu[1] * 3 * cz);
        const long long firstp = pdg ? 10ll * (cx + nc[0] * (cy + nc[1] * cz)) : 2 * cx + (long long)ndp[0] * (2 * cy + (long long)ndp[1] * 2 * cz);
        for (int r = 0; r < m; ++r) {
          const int blk = xy[2 * r] & 255, v = xy[2 * r] >> 8;
          CHECK(blk == rowblk[r] && v == var[blk], "row %d: table block %d variable %d", r, blk, v);
          const long long got = (v ? 3 * Nu + firstp : firstu) + xy[2 * r + 1];
          CHECK(got == global_dof(nc, pdg, c, rowdof[r]), "pdg %d cell (%d, %d, %d) row %d: element %lld, numbering %lld", int(pdg), cx, cy, cz, r, got,
                global_dof(nc, pdg, c, rowdof[r]));
        }
      }
  // an offset beyond 2^31 is refused, not wrapped
  const int big[3] = {3001, 3001, 3001};
  CHECK(!vanka::stokes_row_table(3, pdg, 4, var, rowbase, 3001ll * 3001 * 3001, big, ndp, xy), "an offset beyond 2^31 was accepted");
}

// the defaults of the generalised functions are the degree-2 tables
static void test_degree2_defaults(bool pdg)
{
  const vanka::CellDofTables a = vanka::stokes_cell_dof_tables(pdg), b = vanka::stokes_cell_dof_tables(pdg, 2);
  CHECK(a.nl == 81 + (pdg ? 4 : 8) && a.nl == b.nl && a.nbr == b.nbr && a.face == b.face, "degree-2 default tables (pdg %d)", int(pdg));
  const int var[2] = {0, 1};
  std::vector<int> b1, d1, b2, d2;
  vanka::stokes_row_dofs(2, var, pdg ? 4 : 8, b1, d1);
  vanka::stokes_row_dofs(2, var, pdg ? 4 : 8, b2, d2, 81);
  CHECK(b1 == b2 && d1 == d2 && int(b1.size()) == 81 + (pdg ? 4 : 8), "degree-2 default rows (pdg %d)", int(pdg));
}

int main()
{
  for (int pdg = 0; pdg < 2; ++pdg) {
    test_neighbour_table(pdg != 0);
    test_rows(pdg != 0);
    test_degree2_defaults(pdg != 0);
  }
  if (failures) printf("%d check(s) failed\n", failures);
  else printf("all checks hold\n");
  return failures ? 1 : 0;
}
