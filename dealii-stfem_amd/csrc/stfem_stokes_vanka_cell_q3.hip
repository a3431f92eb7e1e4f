// Per-cell Vanka blocks of the Stokes system at velocity degree 3 (stfem_stokes_vanka_create_space, _create_linearised_space): the cell
// matrices of FE_Q(3)^3 x FE_Q(2) / FE_DGP(2) with QGauss(4).  The stage that stokes_cell_matrices_kernel (stfem_stokes_vanka_cell.hip) is at
// degree 2, for the assembled matrix the reference inverts per cell (stmg.h:704-742, compute_block_matrix.h:50-139); assembly,
// inversion and apply are the kernels of that file, which know the degree.
//   Ac[cell][219 or 202][.]: the cell's own matrix of [[nu K, -B^T], [B, 0]], rows / columns: 3 x 64 velocity DoFs (component-major,
//                            node a + 4 b + 16 c on the Gauss-Lobatto nodes), then the 27 FE_Q(2) nodes a + 3 b + 9 c or the ten FE_DGP(2)
//                            functions in the order include/stfem_stokes_space.h documents
//   Mc[cell][64][64]:        its scalar mass
// With a convection mode (template parameter MODE, the linearisation velocity b of the state in the parameters) the velocity-velocity
// entries are those of A(b): + C_form(b, .) (form) / + C_form(b, .) + C_form(., b) (jacobian), C_form(b, u)(v) = - int (u (x) b) : grad v
// (operators.h:1554-1567), the forms stokes_convection_kernel<3, ...> applies and phase 0 of stokes_cell_matrices_kernel holds at degree 2.
// b is read as read_dof_values reads it: an entry on a strongly constrained DoF is selected as 0, never loaded.  MODE 0 is the linear
// operator alone and holds none of this.  A degree-3 context has no weak faces and no CIP term.
//
// Plain matrix form, one workgroup per cell: the physical gradients, values and pressure functions of all 64 points are tabulated in
// LDS (G 96 KiB + PH 32 KiB + PS 13.5 KiB + geometry 5 KiB = 146.7 KiB of the 160 KiB a workgroup may declare on gfx950: one workgroup
// per CU; a mode adds b at the cell's nodes and at the points, 1.5 KiB each: 150 KiB) from the 1D tables of the context - the ones its
// cell kernel applies, no closed form typed again -, then every thread takes entries (row, column) and sums over the points in ascending
// order: a fixed summation order.  Set-up code, not tuned.
#include "stfem_stokes_internal.h"

#include <cstring>

#include "stfem_vanka_kernel.h"

namespace {

struct StokesCellMatQ3Params {
  const double *vertices; // (nc + 1)^3 x 3
  double *Ac, *Mc;        // [cell of the window][nl][nl], [cell of the window][64][64] (nullptr: not wanted)
  int ncx, ncy, ncz;
  long long cell0;        // first cell of the window
  double nu;
  double Su[16], Du[16], Sp[12]; // StokesParamsT<3>: [q*4+a], [q*4+a], [q*3+a]
  double xq[4], wq[4], l1q[4], l2q[4];
  // read with a convection mode only (behind everything the linear kernel reads)
  const double *b;        // linearisation velocity (3 Nu, component-major)
  long long Nu;
  int ndu[3], dmask;
};

template <bool PDG, int MODE>
__global__ __launch_bounds__(256) void stokes_cell_matrices_q3_kernel(const StokesCellMatQ3Params P)
{
  constexpr int NQ = 64, NN = 64, NV = 3 * NN, NPL = PDG ? 10 : 27, NL = NV + NPL;
  __shared__ double G[NQ][NN][3]; // physical gradient of velocity node n at point q
  __shared__ double PH[NQ][NN];   // its value
  __shared__ double PS[NQ][NPL];  // pressure functions
  __shared__ double JI[NQ][9], W[NQ];
  __shared__ double tS[16], tD[16], tP[12], tL[12], tX[4], tW[4]; // the 1D tables; Legendre [degree * 4 + q], degree 0 = 1
  const int tid = threadIdx.x;
  const long long cell = P.cell0 + blockIdx.x;
  const int cx = int(cell % P.ncx), cy = int((cell / P.ncx) % P.ncy), cz = int(cell / ((long long)P.ncx * P.ncy));
  if (tid < 16) { tS[tid] = P.Su[tid]; tD[tid] = P.Du[tid]; }
  if (tid < 12) tP[tid] = P.Sp[tid];
  if (tid < 4) { tL[tid] = 1.0; tL[4 + tid] = P.l1q[tid]; tL[8 + tid] = P.l2q[tid]; tX[tid] = P.xq[tid]; tW[tid] = P.wq[tid]; }
  __shared__ double bl[MODE ? NV : 1], BQ[MODE ? NQ : 1][3]; // b at the cell's nodes [component * 64 + n] and at the points
  if constexpr (MODE != 0) {
    if (tid < NV) { // read_dof_values: entries on strongly constrained DoFs read as 0
      const int comp = tid / NN, n = tid % NN;
      const int ix = 3 * cx + (n & 3), iy = 3 * cy + ((n >> 2) & 3), iz = 3 * cz + (n >> 4);
      const bool con = ((P.dmask & 1) && ix == 0) || ((P.dmask & 2) && ix == P.ndu[0] - 1) || ((P.dmask & 4) && iy == 0) ||
                       ((P.dmask & 8) && iy == P.ndu[1] - 1) || ((P.dmask & 16) && iz == 0) || ((P.dmask & 32) && iz == P.ndu[2] - 1);
      bl[tid] = con ? 0.0 : P.b[comp * P.Nu + ix + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz)];
    }
  }
  __syncthreads();
  // ---- geometry of the points: MappingQ1 from the eight vertices, point q = qa + 4 qb + 16 qc
  if (tid < NQ) {
    const double xi[3] = {tX[tid & 3], tX[(tid >> 2) & 3], tX[tid >> 4]};
    double Ji[3][3], det;
    cip_jacobian(P, cx, cy, cz, xi, Ji, det);
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
      for (int d = 0; d < 3; ++d) JI[tid][3 * e + d] = Ji[e][d]; // d xi_e / d x_d
    W[tid] = det * tW[tid & 3] * tW[(tid >> 2) & 3] * tW[tid >> 4];
  }
  __syncthreads();
  // ---- the functions at the points
  for (int e = tid; e < NQ * NN; e += 256) {
    const int q = e / NN, n = e % NN, a = n & 3, b = (n >> 2) & 3, c = n >> 4, qa = q & 3, qb = (q >> 2) & 3, qc = q >> 4;
    const double sx = tS[qa * 4 + a], sy = tS[qb * 4 + b], sz = tS[qc * 4 + c];
    const double gr[3] = {tD[qa * 4 + a] * sy * sz, sx * tD[qb * 4 + b] * sz, sx * sy * tD[qc * 4 + c]};
    const double *Ji = JI[q];
    PH[q][n] = sx * sy * sz;
#pragma unroll
    for (int d = 0; d < 3; ++d) G[q][n][d] = gr[0] * Ji[d] + gr[1] * Ji[3 + d] + gr[2] * Ji[6 + d];
  }
  for (int e = tid; e < NQ * NPL; e += 256) {
    const int q = e / NPL, l = e % NPL, qa = q & 3, qb = (q >> 2) & 3, qc = q >> 4;
    if (PDG) { // l_i(xi) l_j(eta) l_k(zeta), i + j + k <= 2, i fastest
      const int di = (l == 1 || l == 4 || l == 7) ? 1 : (l == 2 ? 2 : 0);
      const int dj = (l == 3 || l == 4 || l == 8) ? 1 : (l == 5 ? 2 : 0);
      const int dk = (l == 6 || l == 7 || l == 8) ? 1 : (l == 9 ? 2 : 0);
      PS[q][l] = tL[di * 4 + qa] * tL[dj * 4 + qb] * tL[dk * 4 + qc];
    } else {
      PS[q][l] = tP[qa * 3 + l % 3] * tP[qb * 3 + (l / 3) % 3] * tP[qc * 3 + l / 9];
    }
  }
  __syncthreads();
  if constexpr (MODE != 0) { // ---- b at the points, nodes ascending
    if (tid < NQ * 3) {
      const int q = tid / 3, comp = tid % 3;
      double s = 0.0;
      for (int n = 0; n < NN; ++n) s += PH[q][n] * bl[comp * NN + n];
      BQ[q][comp] = s;
    }
    __syncthreads();
  }
  // ---- the entries
  double *Ac = P.Ac + (size_t)blockIdx.x * NL * NL;
  for (int e = tid; e < NL * NL; e += 256) {
    const int r = e / NL, c = e % NL;
    double acc = 0.0;
    if (r < NV && c < NV) {
      const int ci = r / NN, a = r % NN, cj = c / NN, b = c % NN;
      if constexpr (MODE == 0) {
        if (ci == cj)
          for (int q = 0; q < NQ; ++q) {
            const double *ga = G[q][a], *gb = G[q][b];
            acc += W[q] * (P.nu * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]));
          }
      } else if (ci == cj) {
        for (int q = 0; q < NQ; ++q) {
          const double *ga = G[q][a], *gb = G[q][b], *bq = BQ[q];
          const double pb = PH[q][b];
          double t = P.nu * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]);
          t -= pb * (bq[0] * ga[0] + bq[1] * ga[1] + bq[2] * ga[2]); // - (u (x) b) : grad v
          if (MODE == 2) t -= bq[ci] * pb * ga[cj];                  // - (b (x) u) : grad v
          acc += W[q] * t;
        }
      } else if (MODE == 2) {
        for (int q = 0; q < NQ; ++q) acc += W[q] * -(BQ[q][ci] * PH[q][b] * G[q][a][cj]);
      }
    } else if (r < NV) { // - p div v
      const int ci = r / NN, a = r % NN, l = c - NV;
      for (int q = 0; q < NQ; ++q) acc += -W[q] * PS[q][l] * G[q][a][ci];
    } else if (c < NV) { // q div u
      const int cj = c / NN, b = c % NN, l = r - NV;
      for (int q = 0; q < NQ; ++q) acc += W[q] * PS[q][l] * G[q][b][cj];
    }
    Ac[e] = acc;
  }
  if (P.Mc) {
    double *Mc = P.Mc + (size_t)blockIdx.x * NN * NN;
    for (int e = tid; e < NN * NN; e += 256) {
      const int a = e / NN, b = e % NN;
      double s = 0.0;
      for (int q = 0; q < NQ; ++q) s += W[q] * PH[q][a] * PH[q][b];
      Mc[e] = s;
    }
  }
}

} // namespace

int stokes_cell_matrices_q3_launch(const stfem_stokes_ctx *c, double *Ac, double *Mc, long long cell0, unsigned count, int mode, const double *b)
{
  if (c->degree != 3) return stfem_set_error(STFEM_ERR_UNSUPPORTED, "stokes_cell_matrices_q3_kernel: a context of velocity degree %d", c->degree);
  // the window must lie in the mesh: the kernel reads the vertices of cells [cell0, cell0 + count)
  const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
  if (cell0 < 0 || cell0 + (long long)count > ncells)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stokes_cell_matrices_q3_kernel: cells [%lld, %lld) of %lld", cell0, cell0 + (long long)count, ncells);
  if (mode < 0 || mode > 2 || (mode != 0 && !b))
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stokes_cell_matrices_q3_kernel: mode %d%s", mode, mode >= 0 && mode <= 2 ? " without its linearisation velocity" : "");
  const StokesParamsT<3> &q = c->base3;
  StokesCellMatQ3Params p;
  std::memset(&p, 0, sizeof(p));
  p.vertices = c->d_vertices;
  p.Ac = Ac; p.Mc = Mc;
  p.ncx = c->nc[0]; p.ncy = c->nc[1]; p.ncz = c->nc[2];
  p.cell0 = cell0;
  p.nu = c->nu;
  for (int i = 0; i < 16; ++i) { p.Su[i] = q.Su[i]; p.Du[i] = q.Du[i]; }
  for (int i = 0; i < 12; ++i) p.Sp[i] = q.Sp[i];
  for (int i = 0; i < 4; ++i) { p.xq[i] = q.xq[i]; p.wq[i] = q.wq[i]; p.l1q[i] = q.lq[0][i]; p.l2q[i] = q.lq[1][i]; }
  p.b = mode ? b : nullptr;
  p.Nu = c->Nu; p.dmask = c->dmask;
  for (int i = 0; i < 3; ++i) p.ndu[i] = c->ndu[i];
  const void *const kernels[2][3] = {
    {reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<false, 0>), reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<false, 1>),
     reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<false, 2>)},
    {reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<true, 0>), reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<true, 1>),
     reinterpret_cast<const void *>(&stokes_cell_matrices_q3_kernel<true, 2>)}};
  const void *k = kernels[c->pspace ? 1 : 0][mode];
  return vk_launch(k, dim3(count), &p, nullptr, "stokes_cell_matrices_q3_kernel");
}
