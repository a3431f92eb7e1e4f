/* The pressure space by itself and the divergence functional for a Stokes context of velocity degree 2 or 3.  A companion of stfem.h,
 * which includes it (after stfem_stokes_vanka_linearised_space.h and the types it needs, inside its extern "C"): include stfem.h, not
 * this file. */
#ifndef STFEM_STOKES_PRESSURE_SPACE_H
#define STFEM_STOKES_PRESSURE_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_pressure_space.h where its types are declared"
#endif

/* What the context was made with: velocity degree, pressure space (0 = FE_Q, 1 = FE_DGP of degree - 1) and viscosity; reserved is
 * returned as 0.  It takes no device array and makes no device call.  A null argument: STFEM_ERR_INVALID_ARGUMENT. */
int stfem_stokes_get_space(const stfem_stokes_ctx *ctx, stfem_stokes_space_desc *out);

/* stfem_stokes_pressure_ctx, _pressure_mean_vectors, _pressure_quadrature_points, _pressure_difference, _dgp_prolongate, _dgp_restrict
 * and stfem_stokes_divergence of stfem.h for a context of either degree: the same argument lists and the same argument refusals in the
 * same order with the same statuses (a null context or array, nq outside 1..8: STFEM_ERR_INVALID_ARGUMENT), all decided before the
 * context is read or the device touched.
 *   velocity degree 2: exactly the entry of stfem.h without the suffix: same code path, same bits.
 *   velocity degree 3 (stfem_stokes_create_space), where the entries of stfem.h refuse:
 *     pressure_ctx:  FE_Q(2): a scalar degree-2 context on the mesh (with the vertices on a general mesh), no constraints - everything
 *       a FE_Q(2) function has in this library, the stfem_transfer_* between levels included.  FE_DGP(2): a CARRIER for the
 *       10 n_cells entries, a degree-1 context on 1 x 4 x (n_cells - 1) cells (2 x 5 x n_cells DoFs), good for the vector arithmetic
 *       only; it needs n_cells >= 2 (STFEM_ERR_UNSUPPORTED otherwise).  Owned by the Stokes context.
 *     pressure_mean_vectors (boxes):  FE_Q(2): ones = 1, weights = the tensor product of the assembled 1D integrals h (1/6, 4/6, 1/6)
 *       on the 2 nc + 1 lattice.  FE_DGP(2): ones and weights are non-zero at j = 0 of every ten alone (1 and the cell volume): the
 *       nine other functions have zero mean on a box.
 *     pressure_quadrature_points (boxes):  independent of the degree.
 *     pressure_difference (boxes):  p_h from the 27 FE_Q(2) nodes of the cell (Lagrange on 0, 1/2, 1) or from the ten Legendre
 *       products of stfem_stokes_space.h in its order; one workgroup per cell, a fixed summation order.
 *     dgp_prolongate / dgp_restrict:  the FE_DGP(2) embedding between a mesh and its 2 x 2 x 2 children, and its transpose.  On child
 *       s of a direction the parent's 1D functions are l_0 = l_0, l_1 = 1/2 l_1 + (2 s - 1) (sqrt 3 / 2) l_0,
 *       l_2 = 1/4 l_2 + (2 s - 1) (sqrt 15 / 4) l_1.  Both contexts must have a FE_DGP pressure and the same velocity degree:
 *       STFEM_ERR_UNSUPPORTED otherwise, with its reason in stfem_last_error; cell counts that are not 2 : 1: STFEM_ERR_SHAPE_MISMATCH.
 *     divergence:  cell[c] = sum_q (div u_h)^2 JxW at the operator's own 4 x 4 x 4 Gauss points, any mesh (MappingQ1 from the eight
 *       vertices), the velocity read plain (entries on constrained DoFs count as stored), total = sqrt of the fixed-order sum.  One
 *       wave per cell, no colours, no atomics: bitwise reproducible.
 * A degree-3 context has with these the linear cell operator, the convection modes, its per-cell Vanka smoother (linear and
 * linearised), the pressure space helpers and the divergence.  Not built at degree 3: weak faces, CIP, drag / lift, GMGStokes and
 * the drivers, slabs, fp32. */
int stfem_stokes_pressure_ctx_space(stfem_stokes_ctx *ctx, stfem_ctx **out);
int stfem_stokes_pressure_mean_vectors_space(stfem_stokes_ctx *ctx, double *ones, double *weights, double *volume);
int stfem_stokes_pressure_quadrature_points_space(const stfem_stokes_ctx *ctx, int nq, double *out);
int stfem_stokes_pressure_difference_space(stfem_stokes_ctx *ctx, int nq, const double *p, const double *exact_at_points, double out[2],
                                           void *stream);
int stfem_stokes_dgp_prolongate_space(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_fine, const double *src_coarse, int add,
                                      void *stream);
int stfem_stokes_dgp_restrict_space(stfem_stokes_ctx *fine, stfem_stokes_ctx *coarse, double *dst_coarse, const double *src_fine, int add,
                                    void *stream);
int stfem_stokes_divergence_space(stfem_stokes_ctx *ctx, const double *u, double *cell_out, double *total, void *stream);

/* Diagnostic of the divergence kernel, at either degree: out[0] = workgroups of the last divergence launch of the context, out[1] =
 * the longest run of cells one wave (degree 3) or half-wave (degree 2) walked in it.  STFEM_STOKES_Q3_WORKGROUPS=<n> in the
 * environment, read at every launch, caps the workgroups of the degree-3 launch (tests: several cells per wave on a small mesh); the
 * degree-2 launch is not changed by it.  STFEM_ERR_UNSUPPORTED, with its reason in stfem_last_error, on a context that has launched
 * no divergence kernel. */
int stfem_stokes_last_divergence_plan(const stfem_stokes_ctx *ctx, int32_t out[2]);

#endif /* STFEM_STOKES_PRESSURE_SPACE_H */
