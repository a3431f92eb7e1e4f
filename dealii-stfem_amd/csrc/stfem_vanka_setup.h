// Host-side set-up steps shared by the cell-patch smoothers (stfem_vanka.hip: scalar systems; stfem_stokes_vanka.hip: the
// two-variable Stokes system): block classes of an axis-aligned uniform mesh, cell lists of the apply launches, tile plans, and
// the way from a combined cell matrix to the stored inverse, and the index tables of the one-block-per-cell Stokes layout
// (stfem_stokes_vanka_cell.hip), at velocity degree 2 and 3.  Plain C++17, no HIP: csrc/test_vanka_setup.cpp, csrc/test_stokes_vanka_setup.cpp and
// csrc/test_stokes_vanka_setup_q3.cpp run it on the CPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <utility>
#include <vector>

namespace stfem {
namespace vanka {

// in-place Gauss-Jordan inverse with partial pivoting (FullMatrix::gauss_jordan, stmg.h:828); false: singular (or a NaN pivot)
inline bool invert(int n, std::vector<double> &A)
{
  std::vector<int> piv(n);
  for (int c = 0; c < n; ++c) {
    int p = c;
    double best = std::abs(A[size_t(c) * n + c]);
    for (int r = c + 1; r < n; ++r)
      if (std::abs(A[size_t(r) * n + c]) > best) { best = std::abs(A[size_t(r) * n + c]); p = r; }
    if (!(best > 0.0)) return false;
    piv[c] = p;
    if (p != c)
      for (int k = 0; k < n; ++k) std::swap(A[size_t(c) * n + k], A[size_t(p) * n + k]);
    const double inv = 1.0 / A[size_t(c) * n + c];
    A[size_t(c) * n + c] = 1.0;
    for (int k = 0; k < n; ++k) A[size_t(c) * n + k] *= inv;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = A[size_t(r) * n + c];
      if (f == 0.0) continue;
      A[size_t(r) * n + c] = 0.0;
      for (int k = 0; k < n; ++k) A[size_t(r) * n + k] -= f * A[size_t(c) * n + k];
    }
  }
  for (int c = n - 1; c >= 0; --c)
    if (piv[c] != c)
      for (int r = 0; r < n; ++r) std::swap(A[size_t(r) * n + c], A[size_t(r) * n + piv[c]]);
  return true;
}

// ---- block classes ----
// The block of a cell depends only on which neighbours it has.  Key: per direction d bit 2d = has a lower neighbour, bit 2d + 1 =
// has an upper neighbour - on this rank or, across a face of neighbour_mask, on the rank next to it (valence and assembled entries
// count those cells too; what they add to the shared DoFs arrives with the caller's add-exchange of the interface planes).
// local: neighbours on this rank only - the first-touch rule of the scatter.
struct ClassTable {
  int nc[3];
  std::vector<int> cls, local; // [cell]: class index, local pattern
  std::vector<int> key;        // [class], in the order the cells meet them (z, y, x): fixes the layout of the blocks
};
inline ClassTable class_table(const int nc[3], int neighbour_mask)
{
  ClassTable t;
  std::map<int, int> class_id;
  int loc[3], key[3], c[3];
  for (int d = 0; d < 3; ++d) t.nc[d] = nc[d];
  for (c[2] = 0; c[2] < nc[2]; ++c[2])
    for (c[1] = 0; c[1] < nc[1]; ++c[1])
      for (c[0] = 0; c[0] < nc[0]; ++c[0]) {
        for (int d = 0; d < 3; ++d) {
          loc[d] = (c[d] > 0 ? 1 : 0) | (c[d] < nc[d] - 1 ? 2 : 0);
          key[d] = loc[d] | ((c[d] == 0 && (neighbour_mask & (1 << (2 * d)))) ? 1 : 0) | ((c[d] == nc[d] - 1 && (neighbour_mask & (2 << (2 * d)))) ? 2 : 0);
        }
        const int k = key[0] | (key[1] << 2) | (key[2] << 4);
        const auto it = class_id.emplace(k, int(t.key.size()));
        if (it.second) t.key.push_back(k);
        t.cls.push_back(it.first->second);
        t.local.push_back(loc[0] | (loc[1] << 2) | (loc[2] << 4));
      }
  return t;
}

// ---- cell lists of the apply launches: batches of 16 cells, four batches of one class per workgroup ----
struct CellList {
  std::vector<int> order; // [64 quads]: cell number, -1 = padding
  std::vector<int> cls;   // [quads]: class index (colour lists: | local pattern << 8)
  std::vector<int> slot;  // flat list: cell -> its position in order
};
// colour 0..7: the cells with (cx & 1) + 2 (cy & 1) + 4 (cz & 1) == colour, grouped by (class, local pattern); colour < 0: the flat
// list of the two-phase apply, all cells grouped by class.  Groups in ascending order, each padded to whole quads of 64.
inline CellList cell_list(const ClassTable &t, int colour)
{
  const bool flat = colour < 0;
  const int first[3] = {flat ? 0 : colour & 1, flat ? 0 : (colour >> 1) & 1, flat ? 0 : colour >> 2}, step = flat ? 1 : 2;
  std::map<std::pair<int, int>, std::vector<int>> groups;
  for (int cz = first[2]; cz < t.nc[2]; cz += step)
    for (int cy = first[1]; cy < t.nc[1]; cy += step)
      for (int cx = first[0]; cx < t.nc[0]; cx += step) {
        const int cell = cx + t.nc[0] * (cy + t.nc[1] * cz);
        groups[{t.cls[cell], flat ? 0 : t.local[cell]}].push_back(cell);
      }
  CellList l;
  if (flat) l.slot.assign(t.cls.size(), 0);
  for (const auto &g : groups) {
    for (int cell : g.second) {
      if (flat) l.slot[cell] = int(l.order.size());
      l.order.push_back(cell);
    }
    l.order.resize((l.order.size() + 63) / 64 * 64, -1);
    l.cls.resize(l.order.size() / 64, g.first.first | (g.first.second << 8));
  }
  return l;
}
// what the kernel reads per list entry: per_cell[cell] (the first DoF of the cell), pad for padding
inline std::vector<int> gather_cells(const std::vector<int> &order, const std::vector<int> &per_cell, int pad)
{
  std::vector<int> out(order.size());
  for (size_t i = 0; i < order.size(); ++i) out[i] = order[i] < 0 ? pad : per_cell[order[i]];
  return out;
}

// ---- tile plans: a cell block of `tiles` row tiles (16 rows each) is split into parts of mtw tiles, one workgroup each ----
// (smaller parts: more workgroups per launch and per CU; larger: less set-up per MFMA).  The two plans answer differently for
// the same tile count, and mtw picks the kernel instantiation.
struct TilePlan {
  int mtw = 0, parts = 0; // mtw == 0: no split
};
// scalar smoother.  Measured on cfg 1 (16 tiles; profiles/r2/vanka): fp64 1.16 / 1.25 ms with 4 / 8 tiles per workgroup, fp32
// 0.74 / 0.69; two or four 16-cell column batches per wave (one staged slab and one LDS read for 2 - 4 MFMAs) 1.19 - 1.47 ms:
// slower; capping the resident workgroups per CU changes nothing.
inline TilePlan scalar_tile_plan(int tiles, bool fp32)
{
  int env_tiles = 0;
  if (const char *e = getenv("STFEM_VANKA_TILES")) env_tiles = atoi(e); // (experiments)
  TilePlan plan;
  double best = 1e30;
  const int cand64[] = {4, 8, 6, 3, 2, 1}, cand32[] = {8, 4, 6, 3, 2, 1};
  for (int mtw : (fp32 ? cand32 : cand64)) {
    if (tiles <= 4 ? mtw != tiles : mtw > tiles) continue; // small blocks: one part
    if (env_tiles && mtw != env_tiles) continue;
    const int parts = (tiles + mtw - 1) / mtw;
    const double cost = double(parts * mtw) / tiles * (mtw >= 4 ? 1.0 : 1.1); // padded row tiles are computed too
    if (cost < best - 1e-9) {
      best = cost;
      plan.mtw = mtw; plan.parts = parts;
    }
  }
  return plan;
}
// Stokes smoother: the split with the fewest padded tiles (fp64: at most six per workgroup)
inline TilePlan stokes_tile_plan(int tiles)
{
  TilePlan plan;
  int best = 1 << 30;
  for (int mtw : {4, 3, 6, 2, 1}) {
    if (mtw > tiles && mtw != 1) continue;
    const int parts = (tiles + mtw - 1) / mtw;
    if (parts * mtw < best) { best = parts * mtw; plan.mtw = mtw; plan.parts = parts; }
  }
  return plan;
}

// ---- from the restricted assembled matrices of a cell to the stored inverse (stmg.h:806-829) ----
// scalar system: B(i nloc + r, j nloc + s) = Beta(i, j) M(r, s) + Alpha(i, j) K(r, s)
inline void combine_scalar(int nb, int nloc, const double *Alpha, const double *Beta, const std::vector<double> &K, const std::vector<double> &M,
                           std::vector<double> &B)
{
  const int m = nb * nloc;
  B.resize(size_t(m) * m);
  for (int i = 0; i < nb; ++i)
    for (int j = 0; j < nb; ++j)
      for (int r = 0; r < nloc; ++r)
        for (int s = 0; s < nloc; ++s)
          B[size_t(i * nloc + r) * m + j * nloc + s] = Beta[i * nb + j] * M[size_t(r) * nloc + s] + Alpha[i * nb + j] * K[size_t(r) * nloc + s];
}
// two variables: block i has variable var[i] (0: the first nu cell DoFs, 1: the other nl - nu) and starts at row rowbase[i];
// B((i, k), (j, l)) = Alpha(i, j) A(k, l) + [var i = var j = 0] Beta(i, j) Mu(k, l), A over all nl cell DoFs, Mu over the first nu
inline void combine_two_variable(int nblk, const int *var, const int *rowbase, int m, int nu, int nl, const double *Alpha, const double *Beta,
                                 const std::vector<double> &A, const std::vector<double> &Mu, std::vector<double> &B)
{
  B.assign(size_t(m) * m, 0.0);
  for (int i = 0; i < nblk; ++i)
    for (int j = 0; j < nblk; ++j) {
      const int ni = var[i] ? nl - nu : nu, nj = var[j] ? nl - nu : nu, ro = var[i] ? nu : 0, co = var[j] ? nu : 0;
      const double al = Alpha[i * nblk + j], be = Beta[i * nblk + j];
      for (int k = 0; k < ni; ++k)
        for (int l = 0; l < nj; ++l) {
          double e = 0.0;
          if (be != 0.0 && var[i] == 0 && var[j] == 0) e += be * Mu[size_t(k) * nu + l]; // M_mask(0, 0) only
          if (al != 0.0) e += al * A[size_t(ro + k) * nl + co + l];
          B[size_t(rowbase[i] + k) * m + rowbase[j] + l] = e;
        }
    }
}
// Row r of the m x m matrix B belongs to cell DoF dof[r].  Constrained DoFs (con): row and column dropped, the diagonal of the
// unconstrained assembly stays (the entries between one DoF and itself, in every block); rows scaled by the valence of their DoF
// (val, powers of two); Gauss-Jordan; the block in the apply's layout: out[k][r] = T(inverse(r, k)), [kpad][mpad], zero padding.
// false: singular.
template <typename T>
bool finish_block(int m, std::vector<double> &B, const std::vector<int> &dof, const std::vector<char> &con, const std::vector<double> &val, T *out,
                  int mpad, int kpad)
{
  for (int r = 0; r < m; ++r)
    for (int s = 0; s < m; ++s) {
      if (dof[r] != dof[s] && (con[dof[r]] || con[dof[s]])) B[size_t(r) * m + s] = 0.0;
      B[size_t(r) * m + s] *= val[dof[r]];
    }
  if (!invert(m, B)) return false;
  for (int k = 0; k < kpad; ++k)
    for (int r = 0; r < mpad; ++r) out[size_t(k) * mpad + r] = (k < m && r < m) ? T(B[size_t(r) * m + k]) : T(0);
  return true;
}

// ---- one block per cell of the two-variable (Stokes) system: the cell's DoFs and the cells that share them ----
// Velocity degree p (2 or 3): the cell holds nn = (p + 1)^3 velocity nodes per component.  Cell DoF k: 0 .. 3 nn - 1 velocity
// (component k / nn, node k % nn = a + (p + 1) (b + (p + 1) e) of the FE_Q(p) cell), from 3 nn the pressure DoFs: the FE_Q(p - 1)
// nodes a + p (b + p e), or the FE_DGP(p - 1) functions of the cell (4 at degree 2, 10 at degree 3), which no other cell holds.
inline int stokes_cell_velocity_dofs(int degree) { return 3 * (degree + 1) * (degree + 1) * (degree + 1); }
inline int stokes_cell_pressure_dofs(int degree, bool pdg) { return pdg ? (degree == 2 ? 4 : 10) : degree * degree * degree; }
struct CellDofTables {
  int nl = 0;            // velocity + pressure DoFs of a cell (degree 2: 81 + 8 or 4, degree 3: 192 + 27 or 10)
  std::vector<int> nbr;  // [nl][27]: the DoF's index in the neighbour cell at shift (sx + 1) + 3 (sy + 1) + 9 (sz + 1), -1: not held there
  std::vector<int> face; // [nl]: bit 2 d / 2 d + 1: a velocity DoF on the cell's lower / upper face of direction d (strong constraints)
};
inline CellDofTables stokes_cell_dof_tables(bool pdg, int degree = 2)
{
  CellDofTables t;
  const int nv = stokes_cell_velocity_dofs(degree), nn = nv / 3;
  t.nl = nv + stokes_cell_pressure_dofs(degree, pdg);
  t.nbr.assign(size_t(t.nl) * 27, -1);
  t.face.assign(t.nl, 0);
  for (int k = 0; k < t.nl; ++k) {
    const bool vel = k < nv;
    if (!vel && pdg) { // a cell function: the cell itself only
      t.nbr[size_t(k) * 27 + 13] = k;
      continue;
    }
    const int n1 = vel ? degree + 1 : degree, top = n1 - 1, n = vel ? k % nn : k - nv, base = vel ? k - n : nv;
    const int idx[3] = {n % n1, (n / n1) % n1, n / (n1 * n1)};
    for (int d = 0; d < 3; ++d)
      if (vel) t.face[k] |= (idx[d] == 0 ? 1 << (2 * d) : 0) | (idx[d] == top ? 2 << (2 * d) : 0);
    for (int s = 0; s < 27; ++s) {
      const int sh[3] = {s % 3 - 1, (s / 3) % 3 - 1, s / 9 - 1};
      int n2 = 0, mul = 1;
      bool held = true;
      for (int d = 0; d < 3; ++d) {
        // the cell below holds the DoFs of this cell's lower face on its upper face, and the other way round
        if (sh[d] == -1 && idx[d] != 0) held = false;
        if (sh[d] == 1 && idx[d] != top) held = false;
        n2 += (sh[d] == -1 ? top : (sh[d] == 1 ? 0 : idx[d])) * mul;
        mul *= n1;
      }
      if (held) t.nbr[size_t(k) * 27 + s] = base + n2;
    }
  }
  return t;
}
// row of the cell block -> (block of the BlockSlice, cell DoF): block i holds the nvel velocity or the npl pressure DoFs, the blocks
// one after the other
inline void stokes_row_dofs(int nblk, const int *var, int npl, std::vector<int> &rowblk, std::vector<int> &rowdof, int nvel = 81)
{
  rowblk.clear();
  rowdof.clear();
  for (int i = 0; i < nblk; ++i)
    for (int k = 0; k < (var[i] ? npl : nvel); ++k) {
      rowblk.push_back(i);
      rowdof.push_back((var[i] ? nvel : 0) + k);
    }
}
// The apply's row table of the one-block-per-cell layout: row -> (block | variable << 8, element offset from the cell's first DoF of
// the variable); velocity block: component c, node (a, b, e) at c Nu + a + ndu[0] (b + ndu[1] e); pressure block: node (a, b, e) at
// a + ndp[0] (b + ndp[1] e), or cell function n at n.  false: an offset beyond 2^31.
inline bool stokes_row_table(int degree, bool pdg, int nblk, const int *var, const int *rowbase, long long Nu, const int ndu[3], const int ndp[3],
                             std::vector<int> &rowtab_xy)
{
  const int n1 = degree + 1, nn = n1 * n1 * n1, npl = stokes_cell_pressure_dofs(degree, pdg);
  int m = 0;
  for (int i = 0; i < nblk; ++i) m = rowbase[i] + (var[i] ? npl : 3 * nn) > m ? rowbase[i] + (var[i] ? npl : 3 * nn) : m;
  rowtab_xy.assign(size_t(2) * m, 0);
  for (int i = 0; i < nblk; ++i) {
    if (var[i] == 0) {
      for (int c = 0; c < 3; ++c)
        for (int n = 0; n < nn; ++n) {
          const int a = n % n1, b = (n / n1) % n1, e = n / (n1 * n1);
          const long long off = c * Nu + a + (long long)ndu[0] * (b + (long long)ndu[1] * e);
          if (off > 0x7fffffffll) return false;
          rowtab_xy[2 * (rowbase[i] + c * nn + n)] = i;
          rowtab_xy[2 * (rowbase[i] + c * nn + n) + 1] = int(off);
        }
    } else {
      for (int n = 0; n < npl; ++n) {
        const int a = n % degree, b = (n / degree) % degree, e = n / (degree * degree);
        rowtab_xy[2 * (rowbase[i] + n)] = i | (1 << 8);
        rowtab_xy[2 * (rowbase[i] + n) + 1] = pdg ? n : a + ndp[0] * (b + ndp[1] * e);
      }
    }
  }
  return true;
}
// The distinct linearisation states of the velocity column blocks: sel[j] = position of lin[j] among the distinct pointers, in the
// order the blocks meet them (pressure blocks and a null `lin`: 0); returns their number (at least 1)
inline int distinct_states(int nblk, const int *var, const double *const *lin, int *sel, const double **state)
{
  int n = 0;
  for (int j = 0; j < nblk; ++j) {
    sel[j] = 0;
    if (var[j] != 0 || !lin) continue;
    int at = -1;
    for (int s = 0; s < n; ++s)
      if (state[s] == lin[j]) at = s;
    if (at < 0) { state[n] = lin[j]; at = n++; }
    sel[j] = at;
  }
  if (n == 0) { state[0] = nullptr; n = 1; }
  return n;
}

} // namespace vanka
} // namespace stfem
