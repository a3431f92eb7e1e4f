/* The weak (Nitsche) boundary faces of the Stokes operator at velocity degree 2 or 3.  A companion of stfem.h, which includes it (after
 * stfem_stokes_pressure_space.h and the types it needs, inside its extern "C"): include stfem.h, not this file. */
#ifndef STFEM_STOKES_BOUNDARY_SPACE_H
#define STFEM_STOKES_BOUNDARY_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_boundary_space.h where its types are declared"
#endif

/* stfem_stokes_set_weak_boundaries, _n_face_points, _face_points and _nitsche_rhs of stfem.h for a context of either degree: the same
 * argument lists and the same argument refusals (a null context or array, a mask outside 0..63: STFEM_ERR_INVALID_ARGUMENT).
 *   velocity degree 2: exactly the entry of stfem.h without the suffix: same code path, same bits.
 *   velocity degree 3 (stfem_stokes_create_space), where the entries of stfem.h refuse: the weak faces of FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)
 *     at the 4 x 4 Gauss points of a face (QGauss(4), lower tangential direction fastest), 16 points per face cell:
 *       v <- -nu grad u n + p n + gamma1/h u + gamma2/h n (u.n),  dv/dn <- -nu u,  q <- -u.n
 *     with gamma1 = viscosity penalty1, gamma2 = penalty2, h = sqrt(face area) (operators.h:1720-1739), and for _nitsche_rhs the
 *     functional of the Dirichlet data g at those points (operators.h:1921-1932).  The face points are listed faces ascending, the
 *     cells of a face with the lower tangential direction fastest, 16 points per cell; g is indexed the same way.
 *     A face in both the weak and the outflow set takes the outflow branch and adds no linear term; mask 0 is the state of a context
 *     that never had faces.  With weak faces set, stfem_stokes_vmult, _st_vmult, _st_vmult_slice_add and their _convection_space forms
 *     with STFEM_CONVECTION_NONE include the face launches: one wave per boundary cell (a cell on several weak faces is handled once),
 *     eight colour launches after the cell operator's on the same stream, plain read-add-write: no atomics, bitwise reproducible.  A
 *     context without weak faces launches nothing more than before.  stfem_stokes_vanka_create_space over such a context builds blocks
 *     that hold the Nitsche terms.
 * Refused at degree 3 with weak faces, STFEM_ERR_UNSUPPORTED with the reason in stfem_last_error, before the device is touched and with
 * the operands untouched: a convection mode (form / jacobian) of the _convection_space entries and of
 * stfem_stokes_vanka_create_linearised_space - the inflow term - min(b.n, 0) u of the faces is not built.  Not built at degree 3 at
 * all: CIP in the Vanka blocks and on slabs (the operator's term: stfem_stokes_cip_space.h), drag / lift, GMGStokes and the drivers,
 * slabs, fp32. */
int stfem_stokes_set_weak_boundaries_space(stfem_stokes_ctx *ctx, int weak_mask, int outflow_mask, double penalty1, double penalty2);
int64_t stfem_stokes_n_face_points_space(const stfem_stokes_ctx *ctx);
int stfem_stokes_face_points_space(const stfem_stokes_ctx *ctx, double *out_xyz);
int stfem_stokes_nitsche_rhs_space(stfem_stokes_ctx *ctx, const double *g_at_face_points, double *dst_u, double *dst_p, void *stream);

/* Diagnostic of the boundary kernel, at either degree: out[0] = workgroups of the last boundary colour launch of the context,
 * out[1] = the longest run of items (boundary cells of the weak faces) one wave (degree 3) or half-wave (degree 2) walked in it.
 * STFEM_STOKES_FACE_WORKGROUPS=<n> in the environment, read at every launch, caps the workgroups of the boundary colour launches at
 * either degree (tests: several items per wave on a small mesh).  STFEM_ERR_UNSUPPORTED, with its reason in stfem_last_error, on a
 * context that has not launched the boundary kernel. */
int stfem_stokes_last_face_plan(const stfem_stokes_ctx *ctx, int32_t out[2]);

#endif /* STFEM_STOKES_BOUNDARY_SPACE_H */
