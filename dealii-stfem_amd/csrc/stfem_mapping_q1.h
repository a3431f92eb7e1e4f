// MappingQ1 of one cell of the structured block: the trilinear map of the reference cube onto the hexahedron of the cell's eight
// vertices, its Jacobian and what the kernels derive from it.  The one copy: every kernel and host loop that maps a cell calls these.
// Plain C++ that also compiles as HIP device code; nothing of the project is included.
//   vertices: [(ncz + 1)][(ncy + 1)][(ncx + 1)][3]; cell (cx, cy, cz) reads vertex (cx + i, cy + j, cz + k), i, j, k in {0, 1}.
// The order of every sum and product below is part of the interface: the results of the library are compared bit for bit.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define STFEM_MQ1 __host__ __device__ __forceinline__
#define STFEM_MQ1_UNROLL _Pragma("unroll")
#else
#define STFEM_MQ1 inline
#define STFEM_MQ1_UNROLL
#endif

// J[d][e] = d x_d / d xi_e at the reference point xi
STFEM_MQ1 void mapping_q1_jacobian(const double *vertices, int ncx, int ncy, int cx, int cy, int cz, const double xi[3], double J[3][3])
{
  const double fx[2] = {1 - xi[0], xi[0]}, fy[2] = {1 - xi[1], xi[1]}, fz[2] = {1 - xi[2], xi[2]}, dd[2] = {-1.0, 1.0};
  const long long nvx = ncx + 1, nvy = ncy + 1;
  STFEM_MQ1_UNROLL
  for (int d = 0; d < 3; ++d) J[d][0] = J[d][1] = J[d][2] = 0.0;
  STFEM_MQ1_UNROLL
  for (int k = 0; k < 2; ++k)
    STFEM_MQ1_UNROLL
    for (int j = 0; j < 2; ++j)
      STFEM_MQ1_UNROLL
      for (int i = 0; i < 2; ++i) {
        const double *V = vertices + 3 * ((cx + i) + nvx * ((cy + j) + nvy * (long long)(cz + k)));
        STFEM_MQ1_UNROLL
        for (int d = 0; d < 3; ++d) {
          const double Vd = V[d];
          J[d][0] += Vd * dd[i] * fy[j] * fz[k];
          J[d][1] += Vd * fx[i] * dd[j] * fz[k];
          J[d][2] += Vd * fx[i] * fy[j] * dd[k];
        }
      }
}

STFEM_MQ1 double mapping_q1_det(const double J[3][3])
{
  return J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
}

// Ji[e][d] = d xi_e / d x_d: the cofactors times 1 / det J; returns det J
STFEM_MQ1 double mapping_q1_inverse(const double J[3][3], double Ji[3][3])
{
  const double det = mapping_q1_det(J), id = 1.0 / det;
  Ji[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id;
  Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
  Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
  Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * id;
  Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
  Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
  Ji[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id;
  Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
  Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
  return det;
}
// the same of cell (cx, cy, cz) at the reference point xi
STFEM_MQ1 double mapping_q1_inverse(const double *vertices, int ncx, int ncy, int cx, int cy, int cz, const double xi[3], double Ji[3][3])
{
  double J[3][3];
  mapping_q1_jacobian(vertices, ncx, ncy, cx, cy, cz, xi, J);
  return mapping_q1_inverse(J, Ji);
}

// The normal of the face xi_d = const: nrm = +- J^-T e_d / len, returns len = |J^-T e_d|.  sign: +1 / -1 for the outward normal of the
// upper / lower face, 0 for J^-T e_d as it is, where the orientation does not matter.  The surface element of a face point with the
// weights w1, w2 is fabs(det) * len * w1 * w2.  (Selects among values read first: with a row of Ji indexed by d, or a select among
// the reads, the caller's array would live in scratch.)
STFEM_MQ1 double mapping_q1_face_normal(const double Ji[3][3], int d, int sign, double nrm[3])
{
  double len = 0.0;
  STFEM_MQ1_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double r0 = Ji[0][k], r1 = Ji[1][k], r2 = Ji[2][k];
    const double m = d == 0 ? r0 : (d == 1 ? r1 : r2);
    nrm[k] = sign == 0 ? m : (sign > 0 ? 1.0 : -1.0) * m;
    len += nrm[k] * nrm[k];
  }
  len = sqrt(len);
  STFEM_MQ1_UNROLL
  for (int k = 0; k < 3; ++k) nrm[k] /= len;
  return len;
}

// x = the image of the reference point xi
STFEM_MQ1 void mapping_q1_point(const double *vertices, int ncx, int ncy, int cx, int cy, int cz, const double xi[3], double x[3])
{
  const long long nvx = ncx + 1, nvy = ncy + 1;
  x[0] = x[1] = x[2] = 0.0;
  STFEM_MQ1_UNROLL
  for (int k = 0; k < 2; ++k)
    STFEM_MQ1_UNROLL
    for (int j = 0; j < 2; ++j)
      STFEM_MQ1_UNROLL
      for (int i = 0; i < 2; ++i) {
        const double w = (i ? xi[0] : 1 - xi[0]) * (j ? xi[1] : 1 - xi[1]) * (k ? xi[2] : 1 - xi[2]);
        const double *V = vertices + 3 * ((cx + i) + nvx * ((cy + j) + nvy * (long long)(cz + k)));
        STFEM_MQ1_UNROLL
        for (int d = 0; d < 3; ++d) x[d] += w * V[d];
      }
}
