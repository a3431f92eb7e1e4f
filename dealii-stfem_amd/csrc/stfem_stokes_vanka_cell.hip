// Cell-patch Vanka smoother of the two-variable Stokes system with ONE BLOCK PER CELL: general (perturbed) meshes and the linearised
// Navier-Stokes operator (stfem_stokes_vanka_create_linearised).
//
// Replaces the two steps of the reference's reinit_asm (include/stmg.h:929-965): space_operator_mf->set_data(mg_data[l]) followed by
// the assembly of the linearised matrix (compute_matrix_helper<OperatorMode::jacobian>, operators.h:1310-1318), and the construction of
// one inverted block per cell from that matrix (stmg.h:704-742, compute_block_matrix.h:50-139).  The block is the one of the header
// comment of stfem_stokes_vanka.hip with K = the assembled A(b_j) of the column block's linearisation state b_j (operators.h:835-866):
//   A(b) = [[nu K, -B^T], [B, 0]] + Nitsche terms of the weak faces + C_form(b, .) (form) / C_form(b, .) + C_form(., b) (jacobian),
//   C_form(b, u)(v) = - int (u (x) b) : grad v - int_{weak faces} min(b.n, 0) u.v            (operators.h:1554-1567, 1738-1743).
// Set-up on the device, a few cell layers at a time, in the stages of the scalar smoother (stfem_vanka.hip):
//   stokes_cell_matrices_kernel   the cell's own (81 + npl)^2 matrix of A(b) and its 27 x 27 scalar mass, in plain matrix form, a launch per state
//   stokes_vanka_assemble_kernel  restriction of the assembled matrices to the cell's DoFs, constraints, valence, Alpha / Beta
//   vanka_invert_kernel<double>   (stfem_vanka.hip) Gauss-Jordan, straight into the apply's layout
// Velocity degree 3 (stfem_stokes_vanka_create_space, _create_linearised_space; FE_Q(3)^3 x FE_Q(2) / FE_DGP(2) with QGauss(4), weak
// faces in the blocks of the linear operator alone, no CIP term): the same kernels - the cell matrices (192 + npl)^2 and 64 x 64 from the degree's instantiation of the one
// degree-templated kernel, the assembling kernel instantiated for 64 nodes per component, the apply told the degree.
// Apply: stokes_vanka_apply_percell_kernel streams every block from HBM once and leaves the rows in the scratch array; the collecting
// launch of stfem_stokes_vanka.hip sums them per DoF: two launches, no colours, no atomics, fixed summation order.
#include "stfem_stokes_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "stfem_vanka_kernel.h"
#include "stfem_vanka_setup.h"

namespace vanka = stfem::vanka;

namespace {

// The description of stokes_cell_matrices_kernel: geometry and 1D tables are copied from the context's StokesParamsT<DEG>
template <int DEG> struct StokesCellMatParamsT {
  const double *vertices; // (nc + 1)^3 x 3
  double *Ac, *Mc;        // [cell of the window][NL][NL], [cell of the window][NN][NN] (nullptr: not wanted)
  int ncx, ncy, ncz;
  long long cell0;        // first cell of the window
  double nu;
  double Su[(DEG + 1) * (DEG + 1)], Du[(DEG + 1) * (DEG + 1)], Sp[(DEG + 1) * DEG]; // [q*(DEG+1)+a], [q*(DEG+1)+a], [q*DEG+a]
  double xq[DEG + 1], wq[DEG + 1], lq[DEG - 1][DEG + 1];
  // read with a convection mode only (behind everything the linear kernel reads)
  const double *b;        // linearisation velocity (3 Nu, component-major)
  long long Nu;
  int ndu[3], dmask;
  // the weak faces (all zero until the context has some), behind the rest: where the description of degree 2 has always had them
  int weak_mask;
  double gamma1, gamma2;
  double Eu[2 * (DEG + 1)], EDu[2 * (DEG + 1)], Ep[2 * DEG]; // the end-point tables of BoundaryParams, [s * n + a]
};
template <int DEG> using StokesCellMat = StokesCellMatParamsT<DEG>;
static_assert(sizeof(StokesCellMat<2>) == 504, "the degree-2 description: the layout it had as a description of its own");

// Ac[cell][NL][NL]: the cell's own matrix of A(b), rows / columns: 3 x NN velocity DoFs (component-major, node a + N1 b + N1^2 c on the
// Gauss-Lobatto nodes), then the DEG^3 FE_Q(DEG - 1) nodes or the FE_DGP(DEG - 1) functions in the order include/stfem_stokes_space.h
// documents; Mc[cell][NN][NN]: its scalar mass.  MODE: 0 the linear operator alone, which holds nothing of b; 1 / 2 the forms
// stokes_convection_kernel applies, b read as read_dof_values reads it: an entry on a strongly constrained DoF is selected as 0.
// One workgroup per cell, plain matrix form: the physical gradients, values and pressure functions of all points are tabulated in LDS
// from the 1D tables of the context - the ones its cell kernel applies, no closed form typed again -, then every thread takes entries
// (row, column) and sums over the points in ascending order: a fixed summation order.  Degree 3: G 96 KiB + PH 32 KiB + PS 13.5 KiB +
// geometry 5 KiB + face normals and end-point tables 0.6 KiB = 147.5 KiB (150 992 B with FE_Q(2), the larger) of the 163 840 B a workgroup may declare on gfx950, one workgroup
// per CU; a mode adds b at the cell's nodes and at the points, 1.5 KiB each.  Phase 0: the cell term at the operator's N1^3 Gauss points
// (MappingQ1 Jacobian from the eight vertices); phases 1 - 6: the Nitsche and (degree 2 only: a degree-3 context with weak faces
// takes no mode) inflow terms of the cell's weak faces at their N1 x N1 points, lower tangential index fastest, h = sqrt(face area)
// (get_h_face, operators.h:184-209); there the 1D factor of the face's normal direction comes from the end-point tables, l_1 = -+ sqrt 3
// and l_2 = sqrt 5 for FE_DGP.
// Set-up code, not tuned.
template <int DEG, bool PDG, int MODE>
__global__ __launch_bounds__(256) void stokes_cell_matrices_kernel(const StokesCellMat<DEG> P)
{
  constexpr int N1 = DEG + 1, NQ = N1 * N1 * N1, NN = NQ, NV = 3 * NN;
  constexpr int NPL = PDG ? (DEG == 2 ? 4 : 10) : DEG * DEG * DEG, NL = NV + NPL;
  constexpr bool FACES = true;
  constexpr int NF = N1 * N1; // points of a face
  __shared__ double G[NQ][NN][3]; // physical gradient of velocity node n at point q
  __shared__ double PH[NQ][NN];   // its value
  __shared__ double PS[NQ][NPL];  // pressure functions
  __shared__ double JI[NQ][9], W[NQ];
  __shared__ double tS[N1 * N1], tD[N1 * N1], tP[N1 * DEG], tL[DEG * N1], tX[N1], tW[N1]; // the 1D tables; Legendre [degree * N1 + q], degree 0 = 1
  __shared__ double tE[2 * N1], tED[2 * N1], tEp[2 * DEG], NR[NF][3];   // end-point tables [s * n + a]; normals of a face
  __shared__ double bl[MODE ? NV : 1], BQ[MODE ? NQ : 1][3], INF[MODE ? NF : 1]; // b at the cell's nodes [component * NN + n] and at the points; inflow
  const int tid = threadIdx.x;
  const long long cell = P.cell0 + blockIdx.x;
  const int cx = int(cell % P.ncx), cy = int((cell / P.ncx) % P.ncy), cz = int(cell / ((long long)P.ncx * P.ncy));
  if (tid < N1 * N1) { tS[tid] = P.Su[tid]; tD[tid] = P.Du[tid]; }
  if (tid < N1 * DEG) tP[tid] = P.Sp[tid];
  if (tid < N1) {
    tL[tid] = 1.0;
#pragma unroll
    for (int k = 1; k < DEG; ++k) tL[k * N1 + tid] = P.lq[k - 1][tid];
    tX[tid] = P.xq[tid]; tW[tid] = P.wq[tid];
  }
  if constexpr (FACES) {
    if (tid < 2 * N1) { tE[tid] = P.Eu[tid]; tED[tid] = P.EDu[tid]; }
    if (tid < 2 * DEG) tEp[tid] = P.Ep[tid];
  }
  if constexpr (MODE != 0) {
    if (tid < NV) { // read_dof_values: entries on strongly constrained DoFs read as 0
      const int comp = tid / NN, n = tid % NN;
      const int ix = DEG * cx + n % N1, iy = DEG * cy + (n / N1) % N1, iz = DEG * cz + n / (N1 * N1);
      bl[tid] = constrained_u(P, ix, iy, iz) ? 0.0 : P.b[comp * P.Nu + ix + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz)];
    }
  }
  __syncthreads();
  double *Ac = P.Ac + (size_t)blockIdx.x * NL * NL;
  for (int phase = 0; phase < (FACES ? 7 : 1); ++phase) {
    const bool face = FACES && phase > 0;
    const int f = phase - 1, fd = f >> 1, fs = f & 1, t1 = fd == 0 ? 1 : 0; // the face of phases 1 - 6, its lower tangential direction
    if constexpr (FACES) {
      const int cd = fd == 0 ? cx : (fd == 1 ? cy : cz), ncd = fd == 0 ? P.ncx : (fd == 1 ? P.ncy : P.ncz);
      if (face && !((P.weak_mask >> f & 1) && cd == (fs ? ncd - 1 : 0))) continue; // (uniform)
    }
    // (the sums of the entries run to npts, not to NQ: at degree 2, where it is a run-time value, the compiler then leaves them rolled -
    // unrolled over the 27 points they take 256 VGPRs, one wave per SIMD for three or four, and an update of the blocks of 32^3 cells
    // 92 ms for 75: profiles/stokes_cell_matrices_merge.txt, section 3)
    const int npts = face ? NF : NQ;
    // direction k is the normal one of the face: the 1D factors there are the end-point tables'; in every other direction those of
    // the 1D Gauss point of point q, q = qa + N1 qb + N1^2 qc in the cell and lower tangential index fastest on a face
    auto normal = [&](int k) { return face && k == fd; };
    auto q1d = [&](int q, int k) {
      if (face) return k == t1 ? q % N1 : q / N1;
      return k == 0 ? q % N1 : (k == 1 ? (q / N1) % N1 : q / (N1 * N1));
    };
    auto su = [&](int q, int k, int a) { return normal(k) ? tE[fs * N1 + a] : tS[q1d(q, k) * N1 + a]; };
    auto du = [&](int q, int k, int a) { return normal(k) ? tED[fs * N1 + a] : tD[q1d(q, k) * N1 + a]; };
    auto sp = [&](int q, int k, int a) { return normal(k) ? tEp[fs * DEG + a] : tP[q1d(q, k) * DEG + a]; };
    // at the end points l_1(s) = sqrt 3 (2 s - 1), l_2(s) = sqrt 5
    auto lv = [&](int q, int k, int dg) { return normal(k) ? (dg ? (dg == 1 ? (fs ? sqrt(3.0) : -sqrt(3.0)) : sqrt(5.0)) : 1.0) : tL[dg * N1 + q1d(q, k)]; };
    // ---- geometry of the points: MappingQ1 from the eight vertices
    if (tid < npts) {
      double xi[3], Ji[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) xi[k] = normal(k) ? double(fs) : tX[q1d(tid, k)];
      const double det = mapping_q1_inverse(P.vertices, P.ncx, P.ncy, cx, cy, cz, xi, Ji);
#pragma unroll
      for (int e = 0; e < 3; ++e)
#pragma unroll
        for (int d = 0; d < 3; ++d) JI[tid][3 * e + d] = Ji[e][d]; // d xi_e / d x_d
      if (!face) {
        W[tid] = det * tW[q1d(tid, 0)] * tW[q1d(tid, 1)] * tW[q1d(tid, 2)];
      } else {
        double nrm[3];
        const double len = mapping_q1_face_normal(Ji, fd, fs ? 1 : -1, nrm);
        for (int k = 0; k < 3; ++k) NR[tid][k] = nrm[k];
        W[tid] = fabs(det) * len * tW[tid % N1] * tW[tid / N1];
      }
    }
    __syncthreads();
    // ---- the functions at the points
    for (int e = tid; e < npts * NN; e += 256) {
      const int q = e / NN, n = e % NN, a = n % N1, b = (n / N1) % N1, c = n / (N1 * N1);
      const double sx = su(q, 0, a), sy = su(q, 1, b), sz = su(q, 2, c);
      const double gr[3] = {du(q, 0, a) * sy * sz, sx * du(q, 1, b) * sz, sx * sy * du(q, 2, c)};
      const double *Ji = JI[q];
      PH[q][n] = sx * sy * sz;
#pragma unroll
      for (int d = 0; d < 3; ++d) G[q][n][d] = gr[0] * Ji[d] + gr[1] * Ji[3 + d] + gr[2] * Ji[6 + d];
    }
    for (int e = tid; e < npts * NPL; e += 256) {
      const int q = e / NPL, l = e % NPL;
      if (PDG) { // l_i(xi) l_j(eta) l_k(zeta), i + j + k <= DEG - 1, i fastest; degree 2: deal.II's basis 1, l_1(xi), l_1(eta), l_1(zeta)
        const int di = DEG == 2 ? l == 1 : ((l == 1 || l == 4 || l == 7) ? 1 : (l == 2 ? 2 : 0));
        const int dj = DEG == 2 ? l == 2 : ((l == 3 || l == 4 || l == 8) ? 1 : (l == 5 ? 2 : 0));
        const int dk = DEG == 2 ? l == 3 : ((l == 6 || l == 7 || l == 8) ? 1 : (l == 9 ? 2 : 0));
        PS[q][l] = lv(q, 0, di) * lv(q, 1, dj) * lv(q, 2, dk);
      } else {
        PS[q][l] = sp(q, 0, l % DEG) * sp(q, 1, (l / DEG) % DEG) * sp(q, 2, l / (DEG * DEG));
      }
    }
    __syncthreads();
    if constexpr (MODE != 0) { // ---- b at the points, nodes ascending
      if (tid < npts * 3) {
        const int q = tid / 3, comp = tid % 3;
        double s = 0.0;
        for (int n = 0; n < NN; ++n) s += PH[q][n] * bl[comp * NN + n];
        BQ[q][comp] = s;
      }
      __syncthreads();
    }
    double g1h = 0.0, g2h = 0.0;
    if constexpr (FACES) {
      if (face) {
        double area = 0.0;
        for (int q = 0; q < NF; ++q) area += W[q];
        const double h = sqrt(area);
        g1h = P.gamma1 / h;
        g2h = P.gamma2 / h;
        if constexpr (MODE != 0) {
          if (tid < NF) INF[tid] = -fmin(BQ[tid][0] * NR[tid][0] + BQ[tid][1] * NR[tid][1] + BQ[tid][2] * NR[tid][2], 0.0) * W[tid];
          __syncthreads();
        }
      }
    }
    // ---- the entries
    for (int e = tid; e < NL * NL; e += 256) {
      const int r = e / NL, c = e % NL;
      double acc = 0.0;
      if (r < NV && c < NV) {
        const int ci = r / NN, a = r % NN, cj = c / NN, b = c % NN;
        if (face) {
          for (int q = 0; q < npts; ++q) {
            const double *ga = G[q][a], *gb = G[q][b], *n = NR[q];
            const double pa = PH[q][a], pb = PH[q][b];
            double t = 0.0;
            if (ci == cj) {
              const double dna = ga[0] * n[0] + ga[1] * n[1] + ga[2] * n[2], dnb = gb[0] * n[0] + gb[1] * n[1] + gb[2] * n[2];
              t = -P.nu * dnb * pa + g1h * pa * pb - P.nu * pb * dna;
            }
            t += g2h * n[ci] * n[cj] * pa * pb;
            acc += W[q] * t;
            if (MODE != 0 && ci == cj) acc += INF[q] * pa * pb; // - min(b.n, 0) u.v
          }
        } else if constexpr (MODE == 0) {
          if (ci == cj)
            for (int q = 0; q < npts; ++q) {
              const double *ga = G[q][a], *gb = G[q][b];
              acc += W[q] * (P.nu * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]));
            }
        } else if (ci == cj) {
          for (int q = 0; q < npts; ++q) {
            const double *ga = G[q][a], *gb = G[q][b], *bq = BQ[q];
            const double pb = PH[q][b];
            const double visc = P.nu * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]), bga = bq[0] * ga[0] + bq[1] * ga[1] + bq[2] * ga[2];
            // - (u (x) b) : grad v.  Which of the two products is fused into the subtraction decides the last bit: left to the compiler it
            // is the first, and the blocks of degree 3 are those; the blocks of degree 2 have the second fused, and every result recorded
            // for them is compared bit for bit (profiles/stokes_cell_matrices_merge.txt, section 2)
            double t = DEG == 2 ? fma(-pb, bga, visc) : visc - pb * bga;
            if (MODE == 2) t -= bq[ci] * pb * ga[cj];                  // - (b (x) u) : grad v
            acc += W[q] * t;
          }
        } else if (MODE == 2) {
          for (int q = 0; q < npts; ++q) acc += W[q] * -(BQ[q][ci] * PH[q][b] * G[q][a][cj]);
        }
      } else if (r < NV) { // - p div v; faces: p n.v
        const int ci = r / NN, a = r % NN, l = c - NV;
        for (int q = 0; q < npts; ++q) acc += face ? W[q] * PS[q][l] * NR[q][ci] * PH[q][a] : -W[q] * PS[q][l] * G[q][a][ci];
      } else if (c < NV) { // q div u; faces: - q u.n
        const int cj = c / NN, b = c % NN, l = r - NV;
        for (int q = 0; q < npts; ++q) acc += face ? -W[q] * PS[q][l] * NR[q][cj] * PH[q][b] : W[q] * PS[q][l] * G[q][b][cj];
      }
      if (!face) Ac[e] = acc;
      else Ac[e] += acc; // (the same thread wrote the entry in the phases before)
    }
    if (!face && P.Mc) {
      double *Mc = P.Mc + (size_t)blockIdx.x * NN * NN;
      for (int e = tid; e < NN * NN; e += 256) {
        const int a = e / NN, b = e % NN;
        double s = 0.0;
        for (int q = 0; q < NQ; ++q) s += W[q] * PH[q][a] * PH[q][b];
        Mc[e] = s;
      }
    }
    if constexpr (FACES) __syncthreads(); // the next phase rewrites the tables
  }
}

constexpr int CIP_CELL = 27 * 7 * 27; // doubles of a cell's CIP matrix

struct StokesCipCellParams {
  const double *vertices; // (nc + 1)^3 x 3
  const double *w;        // weight velocity (3 Nu, component-major)
  double *Cc;             // [cell of the window][27 rows][7 column groups][27]
  int ncx, ncy, ncz, ndu[3];
  long long Nu, cell0;    // first cell of the window
  int dmask;
  double Su[9], Du[9], Eu[6], EDu[6]; // the 1D tables of CipParams
  double xq[3], wq[3];
  double hinv[3], detJ;   // CART
  double scale;           // delta0 / pa
  // a mesh that ends in a ghost cell layer of a z-slab (stokes_cell_vanka_desc::beyond): bit 4 / 5 - there are cells beyond the bottom /
  // top layer.  Its outer z face is then interior for column group 0 (the own-side term needs the cell's own geometry and the weight on
  // that plane alone); the group of the cell beyond stays zero and that cell is never evaluated: the mesh does not hold it.
  int beyond;
};

// The CIP term C(w; .) of stfem_stokes_cip.hip in plain matrix form, scalar (the term is component-diagonal), cell-centric like
// stokes_cip_kernel: one workgroup per cell; the rows are the cell's own 27 test functions ("adds only its own side's test
// contribution"), column group 0 the cell's own 27 nodes, summed over its interior faces in the order 0..5, column group 1 + f the 27
// nodes of the neighbour behind face f, with the minus sign of the jump (zeros behind a boundary face).  Geometry, normal, JxW, h_F
// and w are those of the cell's own side, exactly as stokes_cip_kernel takes them; entries of w on strongly constrained DoFs read as 0,
// u carries no constraint (the assembly applies them).  Per face: nine threads take the geometry of the nine points, 243 the normal
// derivatives of the 27 nodes of both sides, then every thread up to three of the 729 entries.  Set-up code: not tuned.
template <bool CART>
__global__ __launch_bounds__(256) void stokes_cip_cell_matrices_kernel(const StokesCipCellParams P)
{
  __shared__ double tS[9], tD[9], tE[6], tED[6];
  __shared__ double sW[81];
  __shared__ double sGO[9][3], sGN[9][3], sJxW[9], sWN[9]; // J^-1 n of this side and of the neighbour's, JxW, w.n
  __shared__ double sDO[9][27], sDN[9][27];                // d_n phi_n at the points: this side, the neighbour's
  const int tid = threadIdx.x;
  const long long cell = P.cell0 + blockIdx.x;
  const int cx = int(cell % P.ncx), cy = int((cell / P.ncx) % P.ncy), cz = int(cell / ((long long)P.ncx * P.ncy));
  double *Cc = P.Cc + (size_t)blockIdx.x * CIP_CELL;
  if (tid < 9) { tS[tid] = P.Su[tid]; tD[tid] = P.Du[tid]; }
  if (tid < 6) { tE[tid] = P.Eu[tid]; tED[tid] = P.EDu[tid]; }
  if (tid < 81) { // read_dof_values: entries on strongly constrained DoFs read as 0
    const int comp = tid / 27, n = tid % 27;
    const int ix = 2 * cx + n % 3, iy = 2 * cy + (n / 3) % 3, iz = 2 * cz + n / 9;
    sW[tid] = constrained_u(P, ix, iy, iz) ? 0.0 : P.w[comp * P.Nu + ix + (long long)P.ndu[0] * (iy + (long long)P.ndu[1] * iz)];
  }
  __syncthreads();
  double own0 = 0.0, own1 = 0.0, own2 = 0.0; // entries tid, tid + 256, tid + 512 of column group 0
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const int d = f >> 1, s = f & 1, t1 = d == 0 ? 1 : 0;
    const int cd = d == 0 ? cx : (d == 1 ? cy : cz), ncd = d == 0 ? P.ncx : (d == 1 ? P.ncy : P.ncz);
    const bool outer = d == 2 && !(s ? cd < ncd - 1 : cd > 0) && (P.beyond >> f & 1); // the face to the cells beyond a ghost layer
    if (!(s ? cd < ncd - 1 : cd > 0) && !outer) { // a boundary face (uniform)
      for (int e = tid; e < 729; e += 256) Cc[(e / 27) * 189 + (1 + f) * 27 + e % 27] = 0.0;
      continue;
    }
    if (tid < 9) { // the geometry of face point tid, both sides, and w.n
      const int q1 = tid % 3, q2 = tid / 3;
      double go[3] = {0, 0, 0}, gnb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, JxW;
      if constexpr (CART) {
        nrm[d] = 1.0;
        go[d] = P.hinv[d];
        gnb[d] = outer ? 0.0 : P.hinv[d];
        JxW = P.detJ * P.hinv[d] * P.wq[q1] * P.wq[q2];
      } else {
        double xi[3], Ji[3][3], det;
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[k] = k == d ? double(s) : P.xq[k == t1 ? q1 : q2];
        det = mapping_q1_inverse(P.vertices, P.ncx, P.ncy, cx, cy, cz, xi, Ji);
        const double len = mapping_q1_face_normal(Ji, d, 0, nrm); // J^-T e_d, unsigned
        JxW = fabs(det) * len * P.wq[q1] * P.wq[q2];
#pragma unroll
        for (int e = 0; e < 3; ++e) go[e] = Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2];
        // behind an outer face there is no cell in this mesh (cz -+ 1 would read vertex plane -1 or ncz + 1): the cell itself is
        // evaluated in its place, in bounds, and the result dropped (one call either way: a branch here cost 66 VGPRs)
        xi[d] = double(1 - s);
        det = mapping_q1_inverse(P.vertices, P.ncx, P.ncy, cx + (d == 0 ? (s ? 1 : -1) : 0), cy + (d == 1 ? (s ? 1 : -1) : 0), cz + (d == 2 && !outer ? (s ? 1 : -1) : 0), xi, Ji);
#pragma unroll
        for (int e = 0; e < 3; ++e) gnb[e] = outer ? 0.0 : Ji[e][0] * nrm[0] + Ji[e][1] * nrm[1] + Ji[e][2] * nrm[2];
      }
      double wval[3] = {0, 0, 0}; // w at the point: the nine nodes of the face
#pragma unroll
      for (int j2 = 0; j2 < 3; ++j2)
#pragma unroll
        for (int j1 = 0; j1 < 3; ++j1) {
          const int k0 = d == 0 ? 2 * s : (t1 == 0 ? j1 : j2), k1 = d == 1 ? 2 * s : (t1 == 1 ? j1 : j2), k2 = d == 2 ? 2 * s : j2;
          const double phi = tS[q1 * 3 + j1] * tS[q2 * 3 + j2];
#pragma unroll
          for (int c3 = 0; c3 < 3; ++c3) wval[c3] = fma(phi, sW[c3 * 27 + k0 + 3 * k1 + 9 * k2], wval[c3]);
        }
#pragma unroll
      for (int e = 0; e < 3; ++e) { sGO[tid][e] = go[e]; sGN[tid][e] = gnb[e]; }
      sJxW[tid] = JxW;
      sWN[tid] = wval[0] * nrm[0] + wval[1] * nrm[1] + wval[2] * nrm[2];
    }
    __syncthreads();
    if (tid < 243) { // the normal derivative of node n at point q: this side (face f) and the neighbour's (face f ^ 1)
      const int q = tid / 27, n = tid % 27;
      double g0, g1, g2;
      cip_face_gradient(tS, tD, tE, tED, f, q, n, g0, g1, g2);
      sDO[q][n] = sGO[q][0] * g0 + sGO[q][1] * g1 + sGO[q][2] * g2;
      cip_face_gradient(tS, tD, tE, tED, f ^ 1, q, n, g0, g1, g2);
      sDN[q][n] = sGN[q][0] * g0 + sGN[q][1] * g1 + sGN[q][2] * g2;
    }
    __syncthreads();
    double area = 0.0; // h_F^2 = the face's area: the nine JxW in point order
#pragma unroll
    for (int q = 0; q < 9; ++q) area += sJxW[q];
    double cq[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) cq[q] = P.scale * area * sWN[q] * sWN[q] * sJxW[q];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = tid + 256 * k;
      if (e < 729) {
        const int a = e / 27, b = e % 27;
        double so = 0.0, sn = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const double t = cq[q] * sDO[q][a];
          so = fma(t, sDO[q][b], so);
          sn = fma(t, sDN[q][b], sn);
        }
        if (k == 0) own0 += so;
        else if (k == 1) own1 += so;
        else own2 += so;
        Cc[a * 189 + (1 + f) * 27 + b] = outer ? 0.0 : -sn;
      }
    }
    __syncthreads(); // the next face rewrites the tables
  }
  Cc[(tid / 27) * 189 + tid % 27] = own0;
  Cc[((tid + 256) / 27) * 189 + (tid + 256) % 27] = own1;
  if (tid + 512 < 729) Cc[((tid + 512) / 27) * 189 + (tid + 512) % 27] = own2;
}

struct StokesAssembleParams {
  const double *Ac, *Mc;    // cell matrices of the cell layers [zw0, ...): Ac[state][cell of the window][nl][nl], Mc[cell][NN][NN]
  const double *Cc;         // CIP matrices Cc[state][cell of the window][27][7][27]; nullptr: no CIP term
  size_t cip_stride;        // doubles between the states of Cc
  int selc[VK_MAX_BLOCKS];  // the state of Cc of every column block
  size_t state_stride;      // doubles between the states of Ac
  double *B;                // [cell of the batch][m][m]
  const int *nbr, *face;    // vanka::CellDofTables
  const int *rowblk, *rowdof;
  int nc[3], dmask, nl, m, nblk;
  int zw0, z0;
  int var[VK_MAX_BLOCKS], sel[VK_MAX_BLOCKS];
  double Alpha[VK_MAX_BLOCKS * VK_MAX_BLOCKS], Beta[VK_MAX_BLOCKS * VK_MAX_BLOCKS];
};

// One workgroup per cell: entry (r, s) of the block = valence(r) (Alpha(i, j) A_j(k, l) + [velocity, velocity] Beta(i, j) M(k, l)) with the
// ASSEMBLED matrices restricted to the cell's DoFs k, l: the cell's own matrix + what the neighbours holding both DoFs add
// (compute_block_matrix.h:50-139; cells in z, y, x order); a strongly constrained DoF keeps only the entries with itself.
// NN: velocity nodes of a cell per component, 27 (FE_Q(2)) or 64 (FE_Q(3), no CIP term).
template <int NN>
__global__ __launch_bounds__(256) void stokes_vanka_assemble_kernel(const StokesAssembleParams P)
{
  constexpr int NV = 3 * NN;
  __shared__ double s_val[NV + 32]; // (nl <= NV + 27)
  __shared__ int s_con[NV + 32];
  const int lc = blockIdx.x, cpl = P.nc[0] * P.nc[1];
  const int cz = P.z0 + lc / cpl, cy = (lc % cpl) / P.nc[0], cx = lc % P.nc[0];
  const int cc[3] = {cx, cy, cz};
  auto has_cell = [&](int s) { // the neighbour at shift s exists
    const int sh[3] = {s % 3 - 1, (s / 3) % 3 - 1, s / 9 - 1};
    return cx + sh[0] >= 0 && cx + sh[0] < P.nc[0] && cy + sh[1] >= 0 && cy + sh[1] < P.nc[1] && cz + sh[2] >= 0 && cz + sh[2] < P.nc[2];
  };
  for (int k = threadIdx.x; k < P.nl; k += 256) {
    int val = 0;
    for (int s = 0; s < 27; ++s)
      if (P.nbr[k * 27 + s] >= 0 && has_cell(s)) ++val;
    bool con = false;
    for (int d = 0; d < 3; ++d) {
      if ((P.face[k] >> (2 * d) & 1) && cc[d] == 0 && (P.dmask >> (2 * d) & 1)) con = true;
      if ((P.face[k] >> (2 * d + 1) & 1) && cc[d] == P.nc[d] - 1 && (P.dmask >> (2 * d + 1) & 1)) con = true;
    }
    s_val[k] = double(val);
    s_con[k] = con;
  }
  __syncthreads();
  double *B = P.B + (size_t)lc * P.m * P.m;
  const size_t nl2 = size_t(P.nl) * P.nl;
  for (int e = threadIdx.x; e < P.m * P.m; e += 256) {
    const int r = e / P.m, s = e % P.m;
    const int i = P.rowblk[r], j = P.rowblk[s], a = P.rowdof[r], b = P.rowdof[s];
    double out = 0.0;
    if (a == b || !(s_con[a] || s_con[b])) {
      const bool mass = a < NV && b < NV && a / NN == b / NN;
      const double *A = P.Ac + size_t(P.sel[j]) * P.state_stride;
      double ks = 0.0, ms = 0.0;
      for (int sh = 0; sh < 27; ++sh) {
        const int a2 = P.nbr[a * 27 + sh], b2 = P.nbr[b * 27 + sh];
        if (a2 < 0 || b2 < 0 || !has_cell(sh)) continue;
        const size_t c2 = size_t(cx + sh % 3 - 1) + size_t(P.nc[0]) * (size_t(cy + (sh / 3) % 3 - 1) + size_t(P.nc[1]) * size_t(cz + sh / 9 - 1 - P.zw0));
        ks += A[c2 * nl2 + size_t(a2) * P.nl + b2];
        if (mass) ms += P.Mc[c2 * (NN * NN) + (a2 % NN) * NN + b2 % NN];
      }
      if (NN == 27 && P.Cc && mass) {
        // the assembled CIP matrix: every patch cell K' = K + sh holding a adds its own-side rows - its column group 0 when it holds b
        // too, and for each of its interior faces f the group 1 + f when the neighbour behind that face is a patch cell holding b
        // (only patch cells hold b).  Shifts ascending, group 0 first, faces 0..5: a fixed order.
        const double *Cs = P.Cc + size_t(P.selc[j]) * P.cip_stride;
        double cs = 0.0;
        for (int sh = 0; sh < 27; ++sh) {
          const int a2 = P.nbr[a * 27 + sh];
          if (a2 < 0 || !has_cell(sh)) continue;
          const int sx = sh % 3 - 1, sy = (sh / 3) % 3 - 1, sz = sh / 9 - 1;
          const size_t c2 = size_t(cx + sx) + size_t(P.nc[0]) * (size_t(cy + sy) + size_t(P.nc[1]) * size_t(cz + sz - P.zw0));
          const double *row = Cs + c2 * CIP_CELL + size_t(a2 % 27) * 189;
          const int b2 = P.nbr[b * 27 + sh];
          if (b2 >= 0) cs += row[b2 % 27];
          for (int f = 0; f < 6; ++f) {
            const int fd = f >> 1, e = (f & 1) ? 1 : -1;
            const int tx = sx + (fd == 0 ? e : 0), ty = sy + (fd == 1 ? e : 0), tz = sz + (fd == 2 ? e : 0);
            if (tx < -1 || tx > 1 || ty < -1 || ty > 1 || tz < -1 || tz > 1) continue;
            const int sh2 = (tx + 1) + 3 * (ty + 1) + 9 * (tz + 1);
            if (!has_cell(sh2)) continue;
            const int b3 = P.nbr[b * 27 + sh2];
            if (b3 >= 0) cs += row[(1 + f) * 27 + b3 % 27];
          }
        }
        ks += cs;
      }
      const double al = P.Alpha[i * P.nblk + j], be = P.Beta[i * P.nblk + j];
      if (be != 0.0 && P.var[i] == 0 && P.var[j] == 0) out += be * ms; // M_mask(0, 0) only
      if (al != 0.0) out += al * ks;
      out *= s_val[a];
    }
    B[e] = out;
  }
}

struct StokesCellApplyParams {
  const double *src[VK_MAX_BLOCKS];
  const double *blocks; // [cell][kpad][mpad], element (row r, column k) of the cell's inverse at [k][r]
  double *flat;         // Y[cell][mpad]
  const int2 *rowtab;   // row -> (vector | variable << 8, element offset from the cell's first DoF of the variable)
  int m, mpad, kpad, pdg;
  int nc[3], ndu[3], ndp[3];
  int pu, pp, npc; // velocity degree 2 / 3: cell steps of the velocity and the FE_Q pressure lattice (2, 1 / 3, 2), FE_DGP functions per cell (4 / 10)
};

typedef double double2_t __attribute__((ext_vector_type(2)));

// y = B_c^-1 gather(src) per cell, the block streamed from HBM once (the reference's apply: stmg.h:845-867): one workgroup per cell.
// HBM-bound: kpad * mpad doubles per cell (70 kB at m = 89, 1.3 - 1.6 MB at the 404 - 438 rows of degree 3, where the shape below is one
// group of mpad / 2 threads that walks all k) against 2 m of DoF traffic.  A thread holds a PAIR of rows (one 16-byte
// load per k) and the threads are dealt over 256 / (mpad / 2) groups that split k between them - at m = 89 five groups of 48 threads,
// 240 of 256 busy, each step of the k loop reading 5 consecutive k rows = 3840 contiguous bytes (thread r = row r with 8-byte loads,
// the scalar kernel's shape, would leave 167 threads idle there).  Four loads of a thread are in flight at a time.  The partial sums
// of the groups meet in LDS and are added in ascending group order: reproducible.
__global__ __launch_bounds__(256) void stokes_vanka_apply_percell_kernel(const StokesCellApplyParams P)
{
  __shared__ double xs[VK_MAX_ROWS];
  __shared__ double part[VK_MAX_ROWS]; // [group][mpad], groups * mpad <= 512
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const int cx = int(cell % P.nc[0]), cy = int((cell / P.nc[0]) % P.nc[1]), cz = int(cell / ((long long)P.nc[0] * P.nc[1]));
  const long long firstu = P.pu * cx + (long long)P.ndu[0] * (P.pu * cy + (long long)P.ndu[1] * P.pu * cz);
  const long long firstp = P.pdg ? P.npc * cell : P.pp * cx + (long long)P.ndp[0] * (P.pp * cy + (long long)P.ndp[1] * P.pp * cz);
  for (int r = tid; r < P.kpad; r += 256) {
    double v = 0.0;
    if (r < P.m) {
      const int2 e = P.rowtab[r];
      const int blk = e.x & 255;
      const double *sp = P.src[0];
#pragma unroll
      for (int b = 1; b < VK_MAX_BLOCKS; ++b)
        if (b == blk) sp = P.src[b];
      v = sp[((e.x >> 8) ? firstp : firstu) + e.y];
    }
    xs[r] = v;
  }
  __syncthreads();
  const int RP = P.mpad >> 1, KG = 256 / RP; // row pairs, k groups
  const int rp = tid % RP, kg = tid / RP;
  if (kg < KG) {
    const double2_t *B = reinterpret_cast<const double2_t *>(P.blocks + (size_t)cell * P.kpad * P.mpad) + rp;
    double2_t a0 = {0, 0}, a1 = {0, 0}, a2 = {0, 0}, a3 = {0, 0};
    int k = kg;
    for (; k + 3 * KG < P.kpad; k += 4 * KG) {
      const double2_t b0 = __builtin_nontemporal_load(B + (size_t)k * RP);
      const double2_t b1 = __builtin_nontemporal_load(B + (size_t)(k + KG) * RP);
      const double2_t b2 = __builtin_nontemporal_load(B + (size_t)(k + 2 * KG) * RP);
      const double2_t b3 = __builtin_nontemporal_load(B + (size_t)(k + 3 * KG) * RP);
      a0 += b0 * xs[k];
      a1 += b1 * xs[k + KG];
      a2 += b2 * xs[k + 2 * KG];
      a3 += b3 * xs[k + 3 * KG];
    }
    for (; k < P.kpad; k += KG) a0 += __builtin_nontemporal_load(B + (size_t)k * RP) * xs[k];
    const double2_t s = (a0 + a1) + (a2 + a3);
    part[kg * P.mpad + 2 * rp] = s.x;
    part[kg * P.mpad + 2 * rp + 1] = s.y;
  }
  __syncthreads();
  for (int r = tid; r < P.m; r += 256) {
    double s = part[r];
    for (int g = 1; g < KG; ++g) s += part[g * P.mpad + r];
    P.flat[(size_t)cell * P.mpad + r] = s;
  }
}

template <int DEG>
int cell_matrices_launch(const stfem_stokes_ctx *c, double *Ac, double *Mc, long long cell0, unsigned count, int mode, const double *b)
{
  // (the table names the kernels of both degrees, degree 2 first, whatever DEG: the order in which the host code first names the
  // kernels is the order in which they stand in the code object, which stays that of profiles/stokes_launch_set.txt)
#define STFEM_CELL_MATRICES(D, PDG) \
  {reinterpret_cast<const void *>(&stokes_cell_matrices_kernel<D, PDG, 0>), reinterpret_cast<const void *>(&stokes_cell_matrices_kernel<D, PDG, 1>), \
   reinterpret_cast<const void *>(&stokes_cell_matrices_kernel<D, PDG, 2>)}
  static const void *const kernels[2][2][3] = {{STFEM_CELL_MATRICES(2, false), STFEM_CELL_MATRICES(2, true)},
                                               {STFEM_CELL_MATRICES(3, false), STFEM_CELL_MATRICES(3, true)}}; // [degree - 2][pspace][mode]
#undef STFEM_CELL_MATRICES
  StokesCellMat<DEG> p;
  std::memset(&p, 0, sizeof(p));
  const StokesParamsT<DEG> &g = c->desc<DEG>();
  constexpr int N1 = DEG + 1;
  p.vertices = c->d_vertices;
  p.Ac = Ac; p.Mc = Mc;
  p.ncx = c->nc[0]; p.ncy = c->nc[1]; p.ncz = c->nc[2];
  p.cell0 = cell0;
  p.nu = c->nu;
  for (int i = 0; i < N1 * N1; ++i) { p.Su[i] = g.Su[i]; p.Du[i] = g.Du[i]; }
  for (int i = 0; i < N1 * DEG; ++i) p.Sp[i] = g.Sp[i];
  for (int i = 0; i < N1; ++i) {
    p.xq[i] = g.xq[i]; p.wq[i] = g.wq[i];
    for (int k = 0; k < DEG - 1; ++k) p.lq[k][i] = g.lq[k][i];
  }
  p.b = mode ? b : nullptr;
  p.Nu = c->Nu; p.dmask = c->dmask;
  for (int i = 0; i < 3; ++i) p.ndu[i] = c->ndu[i];
  const BoundaryParams &w = c->bnd; // (all zero until stfem_stokes_set_weak_boundaries or its _space form)
  p.weak_mask = w.weak_mask; p.gamma1 = w.gamma1; p.gamma2 = w.gamma2;
  for (int i = 0; i < 2 * N1; ++i) { p.Eu[i] = w.Eu[i]; p.EDu[i] = w.EDu[i]; }
  for (int i = 0; i < 2 * DEG; ++i) p.Ep[i] = w.Ep[i];
  return vk_launch(kernels[DEG - 2][c->pspace ? 1 : 0][mode], dim3(count), &p, nullptr, "stokes_cell_matrices_kernel");
}

} // namespace

int stokes_cell_matrices_launch(const stfem_stokes_ctx *c, double *Ac, double *Mc, long long cell0, unsigned count, int mode, const double *b)
{
  // the window must lie in the mesh: the kernel reads the vertices of cells [cell0, cell0 + count)
  const long long ncells = (long long)c->nc[0] * c->nc[1] * c->nc[2];
  if (cell0 < 0 || cell0 + (long long)count > ncells)
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stokes_cell_matrices_kernel: cells [%lld, %lld) of %lld", cell0, cell0 + (long long)count, ncells);
  if (mode < 0 || mode > 2 || (mode != 0 && !b))
    return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "stokes_cell_matrices_kernel: mode %d%s", mode, mode >= 0 && mode <= 2 ? " without its linearisation velocity" : "");
  return stokes_with_degree(c, [&](auto deg) { return cell_matrices_launch<deg()>(c, Ac, Mc, cell0, count, mode, b); });
}

struct stokes_cell_vanka {
  stfem_stokes_ctx *ctx = nullptr;   // the context of the apply: its cells index the blocks
  stfem_stokes_ctx *setup = nullptr; // the context of the set-up (ctx, or a slab's extended context); own layers [own0, own0 + ctx->nc[2])
  int own0 = 0;
  stokes_cell_vanka_desc d;
  int nl = 0, npl = 0, nn = 27; // cell DoFs, its pressure DoFs, velocity nodes per component (64 at degree 3)
  int setup_batches = 0; // batches of cell layers the last build_blocks took
  double *d_blocks = nullptr, *d_flat = nullptr;
  int2 *d_rowtab = nullptr;
  int *d_nbr = nullptr, *d_face = nullptr, *d_rowblk = nullptr, *d_rowdof = nullptr;
};

namespace {

// Stages 1 - 3 into v->d_blocks, a few cell layers at a time with a window of cell matrices (the batch's layers and one on either
// side), as vanka_create_per_cell_device does it.  fresh: the blocks are not allocated yet - they must fit beside the scratch.
int build_blocks(stokes_cell_vanka *v, const double *const *lin, bool fresh)
{
  // Geometry, masks and states are those of the set-up context c; on a slab that is the extended context, whose cell layers
  // [own0, own1) are the slab's own: only they get blocks, stored from cell 0 of the slab, and the window of cell matrices reaches
  // into the ghost layers.
  stfem_stokes_ctx *c = v->setup;
  const stokes_cell_vanka_desc &d = v->d;
  const int nl = v->nl, m = d.m;
  const int ncx = c->nc[0], ncy = c->nc[1], ncz = c->nc[2];
  const int own0 = v->own0, nown = v->ctx->nc[2], own1 = own0 + nown;
  const size_t cpl = size_t(ncx) * ncy, ncells = cpl * nown, bsz = size_t(d.kpad) * d.mpad;
  int sel[VK_MAX_BLOCKS];
  const double *state[VK_MAX_BLOCKS];
  const int nstates = vanka::distinct_states(d.nblk, d.var, d.mode ? lin : nullptr, sel, state);
  // the CIP term: a weight velocity per distinct state of `lin`, whatever the mode; a mesh without interior faces has none
  const bool cip = d.delta0 != 0.0 && (ncx > 1 || ncy > 1 || ncz > 1);
  int selc[VK_MAX_BLOCKS];
  const double *weight[VK_MAX_BLOCKS];
  const int ncip = cip ? vanka::distinct_states(d.nblk, d.var, lin, selc, weight) : 0;
  const size_t nl2 = size_t(nl) * nl, nn2 = size_t(v->nn) * v->nn;
  const size_t km_layer = (size_t(nstates) * nl2 + nn2 + size_t(ncip) * CIP_CELL) * cpl * sizeof(double), b_layer = cpl * size_t(m) * m * sizeof(double);
  STFEM_TRY(hipSetDevice(c->device));
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
  const double need = double(ncells) * double(bsz) * sizeof(double);
  // scratch of one batch of L cell layers: (L + 2) layers of cell matrices + L layers of blocks; at most 6 GB, and never more than
  // what is left beside the blocks themselves
  const double budget = std::min(6e9, 0.9 * double(free_b) - (fresh ? need : 0.0));
  if (budget < 3.0 * double(km_layer) + double(b_layer)) {
    return stfem_set_error(STFEM_ERR_OUT_OF_MEMORY, "per-cell Stokes blocks of %zu cells need %.2f GB and %.2f GB of set-up scratch (%.2f GB free)",
                           ncells, need * 1e-9, (3.0 * double(km_layer) + double(b_layer)) * 1e-9, double(free_b) * 1e-9);
  }
  int L = int((budget - 2.0 * double(km_layer)) / double(km_layer + b_layer));
  L = std::max(1, std::min(L, nown));
  if (const char *e = getenv("STFEM_VANKA_SETUP_LAYERS")) // at most this many cell layers per batch (tests: the batch loop on small meshes)
    if (atoi(e) > 0) L = std::min(L, atoi(e));
  if (fresh) {
    const int rc = vk_alloc(reinterpret_cast<void **>(&v->d_blocks), ncells * bsz * sizeof(double));
    if (rc != STFEM_OK) return rc;
  }
  const size_t win_cells = cpl * size_t(std::min(ncz, L + 2));
  double *d_A = nullptr, *d_M = nullptr, *d_B = nullptr, *d_C = nullptr;
  int *d_flag = nullptr;
  auto cleanup = [&]() {
    (void)hipFree(d_A);
    (void)hipFree(d_M);
    (void)hipFree(d_B);
    (void)hipFree(d_C);
    (void)hipFree(d_flag);
  };
  int rc = vk_alloc(reinterpret_cast<void **>(&d_A), size_t(nstates) * win_cells * nl2 * sizeof(double));
  if (rc == STFEM_OK) rc = vk_alloc(reinterpret_cast<void **>(&d_M), win_cells * nn2 * sizeof(double));
  if (rc == STFEM_OK) rc = vk_alloc(reinterpret_cast<void **>(&d_B), cpl * L * size_t(m) * m * sizeof(double));
  if (rc == STFEM_OK && cip) rc = vk_alloc(reinterpret_cast<void **>(&d_C), size_t(ncip) * win_cells * CIP_CELL * sizeof(double));
  if (rc == STFEM_OK) rc = vk_alloc(reinterpret_cast<void **>(&d_flag), sizeof(int));
  if (rc != STFEM_OK) {
    cleanup();
    return rc;
  }
  hipError_t e = hipMemset(d_flag, 0, sizeof(int));
  StokesAssembleParams ap;
  std::memset(&ap, 0, sizeof(ap));
  ap.Ac = d_A; ap.Mc = d_M; ap.state_stride = win_cells * nl2; ap.B = d_B;
  ap.nbr = v->d_nbr; ap.face = v->d_face; ap.rowblk = v->d_rowblk; ap.rowdof = v->d_rowdof;
  for (int k = 0; k < 3; ++k) ap.nc[k] = c->nc[k];
  ap.dmask = c->dmask; ap.nl = nl; ap.m = m; ap.nblk = d.nblk;
  for (int i = 0; i < d.nblk; ++i) { ap.var[i] = d.var[i]; ap.sel[i] = sel[i]; }
  for (int i = 0; i < d.nblk * d.nblk; ++i) { ap.Alpha[i] = d.Alpha[i]; ap.Beta[i] = d.Beta[i]; }
  StokesCipCellParams cp;
  std::memset(&cp, 0, sizeof(cp));
  if (cip) {
    const StokesParams &b = c->desc<2>(); // (the CIP term is built for degree 2)
    cp.vertices = c->d_vertices;
    cp.ncx = ncx; cp.ncy = ncy; cp.ncz = ncz;
    for (int k = 0; k < 3; ++k) { cp.ndu[k] = c->ndu[k]; cp.xq[k] = b.xq[k]; cp.wq[k] = b.wq[k]; cp.hinv[k] = c->hinv[k]; }
    for (int i = 0; i < 9; ++i) { cp.Su[i] = b.Su[i]; cp.Du[i] = b.Du[i]; }
    stokes_cip_end_tables(cp.Eu, cp.EDu);
    cp.Nu = c->Nu; cp.dmask = c->dmask; cp.detJ = c->detJ;
    cp.scale = d.delta0 / (8.0 * std::sqrt(2.0)); // pa = degree^3.5, degree 2 (operators.h:1614-1615)
    cp.beyond = d.beyond;
    ap.Cc = d_C; ap.cip_stride = win_cells * CIP_CELL;
    for (int i = 0; i < d.nblk; ++i) ap.selc[i] = selc[i];
  }
  const void *cipk = c->cart ? reinterpret_cast<const void *>(&stokes_cip_cell_matrices_kernel<true>) : reinterpret_cast<const void *>(&stokes_cip_cell_matrices_kernel<false>);
  // (64 named before 27: the order of the two kernels in the code object, see cell_matrices_launch; degree 3 has no CIP term)
  const void *asmk = reinterpret_cast<const void *>(&stokes_vanka_assemble_kernel<64>);
  if (d.degree == 2) asmk = reinterpret_cast<const void *>(&stokes_vanka_assemble_kernel<27>);
  stfem_launch_begin();
  v->setup_batches = 0;
  for (int z0 = own0; z0 < own1 && e == hipSuccess && rc == STFEM_OK; z0 += L) {
    ++v->setup_batches;
    const int z1 = std::min(own1, z0 + L), zw0 = std::max(0, z0 - 1), zw1 = std::min(ncz, z1 + 1);
    const size_t wcells = cpl * size_t(zw1 - zw0), bcells = cpl * size_t(z1 - z0);
    for (int s = 0; s < nstates && rc == STFEM_OK; ++s)
      rc = stokes_cell_matrices_launch(c, d_A + size_t(s) * ap.state_stride, s == 0 ? d_M : nullptr, (long long)cpl * zw0, (unsigned)wcells, d.mode, state[s]);
    for (int s = 0; s < ncip && rc == STFEM_OK; ++s) {
      cp.w = weight[s];
      cp.Cc = d_C + size_t(s) * ap.cip_stride;
      cp.cell0 = (long long)cpl * zw0;
      rc = vk_launch(cipk, dim3((unsigned)wcells), &cp, nullptr, "stokes_cip_cell_matrices_kernel");
    }
    ap.zw0 = zw0; ap.z0 = z0;
    if (rc == STFEM_OK) rc = vk_launch(asmk, dim3((unsigned)bcells), &ap, nullptr, "stokes_vanka_assemble_kernel");
    if (rc == STFEM_OK) rc = stfem_vanka_invert_launch(d_B, v->d_blocks, m, d.mpad, d.kpad, (long long)cpl * (z0 - own0), (unsigned)bcells, d_flag, nullptr);
    if (rc == STFEM_OK) e = hipDeviceSynchronize(); // (the next batch reuses the scratch)
  }
  int flag = 0;
  if (rc == STFEM_OK && e == hipSuccess) e = hipMemcpy(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost);
  cleanup();
  if (rc != STFEM_OK) return rc;
  if (e != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "per-cell Stokes block set-up: %s", hipGetErrorString(e));
  if (flag) return stfem_set_error(STFEM_ERR_INVALID_ARGUMENT, "singular cell block");
  return STFEM_OK;
}

} // namespace

void stokes_cell_vanka_destroy(stokes_cell_vanka *v)
{
  if (!v) return;
  (void)hipFree(v->d_blocks);
  (void)hipFree(v->d_flat);
  (void)hipFree(v->d_rowtab);
  (void)hipFree(v->d_nbr);
  (void)hipFree(v->d_face);
  (void)hipFree(v->d_rowblk);
  (void)hipFree(v->d_rowdof);
  delete v;
}

int stokes_cell_vanka_create(stfem_stokes_ctx *c, const stokes_cell_vanka_desc &d, const int *rowtab_xy, const double *const *lin,
                             stokes_cell_vanka **out)
{
  *out = nullptr;
  // the kernels know 27 and 64 velocity nodes per component, nothing else; and the degree is the context's
  const int degree = d.degree;
  if ((degree != 2 && degree != 3) || degree != c->degree)
    return stfem_set_error(STFEM_ERR_UNSUPPORTED, "per-cell Stokes blocks of velocity degree %d on a context of degree %d: built for 2 and 3", degree, c->degree);
  stokes_cell_vanka *v = new (std::nothrow) stokes_cell_vanka;
  if (!v) return STFEM_ERR_OUT_OF_MEMORY;
  v->ctx = c;
  v->setup = d.setup ? d.setup : c;
  v->own0 = d.setup ? d.own0 : 0;
  v->d = d;
  const int nvel = vanka::stokes_cell_velocity_dofs(degree);
  v->npl = vanka::stokes_cell_pressure_dofs(degree, c->pspace != 0);
  v->nn = nvel / 3;
  v->nl = nvel + v->npl;
  const vanka::CellDofTables t = vanka::stokes_cell_dof_tables(c->pspace != 0, degree);
  std::vector<int> rowblk, rowdof;
  vanka::stokes_row_dofs(d.nblk, d.var, v->npl, rowblk, rowdof, nvel);
  std::vector<int2> rowtab(d.m);
  for (int r = 0; r < d.m; ++r) rowtab[r] = make_int2(rowtab_xy[2 * r], rowtab_xy[2 * r + 1]);
  const size_t ncells = size_t(c->nc[0]) * c->nc[1] * c->nc[2];
  int rc = vk_upload(&v->d_nbr, t.nbr);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_face, t.face);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_rowblk, rowblk);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_rowdof, rowdof);
  if (rc == STFEM_OK) rc = vk_upload(&v->d_rowtab, rowtab);
  if (rc == STFEM_OK) rc = build_blocks(v, lin, true);
  if (rc == STFEM_OK) rc = vk_alloc(reinterpret_cast<void **>(&v->d_flat), ncells * d.mpad * sizeof(double));
  if (rc != STFEM_OK) {
    stokes_cell_vanka_destroy(v);
    return rc;
  }
  *out = v;
  return STFEM_OK;
}

int stokes_cell_vanka_update(stokes_cell_vanka *v, const double *const *lin) { return build_blocks(v, lin, false); }
int stokes_cell_vanka_setup_batches(const stokes_cell_vanka *v) { return v ? v->setup_batches : 0; }

int stokes_cell_vanka_apply(stokes_cell_vanka *v, const double *const *src_blocks, const double **rows, void *stream)
{
  const stfem_stokes_ctx *c = v->ctx;
  StokesCellApplyParams p;
  std::memset(&p, 0, sizeof(p));
  for (int i = 0; i < v->d.nblk; ++i) p.src[i] = src_blocks[i];
  p.blocks = v->d_blocks; p.flat = v->d_flat; p.rowtab = v->d_rowtab;
  p.m = v->d.m; p.mpad = v->d.mpad; p.kpad = v->d.kpad; p.pdg = c->pspace;
  for (int k = 0; k < 3; ++k) { p.nc[k] = c->nc[k]; p.ndu[k] = c->ndu[k]; p.ndp[k] = c->ndp[k]; }
  p.pu = v->d.degree; p.pp = v->d.degree - 1; p.npc = c->pspace ? v->npl : 0;
  *rows = v->d_flat;
  const size_t ncells = size_t(c->nc[0]) * c->nc[1] * c->nc[2];
  return vk_launch(reinterpret_cast<const void *>(&stokes_vanka_apply_percell_kernel), dim3((unsigned)ncells), &p, static_cast<hipStream_t>(stream),
                   "stokes_vanka_apply_percell_kernel");
}
