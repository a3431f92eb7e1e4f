/* The Navier-Stokes modes (form / jacobian) of the Stokes operator at velocity degree 2 or 3.  A companion of stfem.h, which includes it
 * (after stfem_stokes_vanka_space.h and the types it needs, inside its extern "C"): include stfem.h, not this file. */
#ifndef STFEM_STOKES_CONVECTION_SPACE_H
#define STFEM_STOKES_CONVECTION_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_convection_space.h where its types are declared"
#endif

/* stfem_stokes_vmult_convection, _st_vmult_convection and _st_vmult_slice_add_convection of stfem.h for a context of either degree:
 * the same argument lists, and the same argument and alias refusals in the same order with the same statuses (a null context or array,
 * a mode outside 0..2, a mode other than 0 without its linearisation: STFEM_ERR_INVALID_ARGUMENT; a destination that is a source or a
 * linearisation velocity: STFEM_ERR_ALIAS), all decided before the context is read or the device touched.
 *   velocity degree 2: exactly the entry of stfem.h without the suffix: same code path, same bits - weak faces and their inflow term,
 *     CIP and slabs included.
 *   velocity degree 3 (stfem_stokes_create_space), where the entries of stfem.h refuse every mode but STFEM_CONVECTION_NONE: every mode
 *     runs.  After the linear cell launches of the same set, at the operator's own 4 x 4 x 4 Gauss points, with u and the linearisation
 *     velocity b read as read_dof_values reads them (entries on strongly constrained DoFs as 0):
 *       STFEM_CONVECTION_FORM:      dst_u += - int (u (x) b) : grad v
 *       STFEM_CONVECTION_JACOBIAN:  dst_u += - int (b (x) u + u (x) b) : grad v
 *     (operators.h:1554-1567).  A degree-3 context has no weak faces: there is no inflow term.  Pressure rows and constrained velocity
 *     rows are those of the linear operator, bit for bit.  One wave per cell, eight colour launches, plain loads and stores: no atomics,
 *     bitwise reproducible.  STFEM_CONVECTION_NONE: the entry of stfem.h, launch for launch.
 * The Vanka blocks of the operator in these modes: stfem_stokes_vanka_create_linearised_space (stfem_stokes_vanka_linearised_space.h;
 * stfem_stokes_vanka_create_space stays linear).
 * The pressure space helpers and the divergence of such a context: stfem_stokes_pressure_space.h.
 * Not built at degree 3: weak faces with their inflow term, CIP, GMGStokes and the drivers, slabs, fp32. */
int stfem_stokes_vmult_convection_space(stfem_stokes_ctx *ctx, int mode, double *dst_u, double *dst_p, const double *src_u,
                                        const double *src_p, const double *lin_u, void *stream);
int stfem_stokes_st_vmult_convection_space(stfem_stokes_ctx *ctx, int mode, int n_timesteps_at_once, int n_timedofs,
                                           int variable_major, const double *Alpha, const double *Beta,
                                           double *const *dst_blocks, const double *const *src_blocks,
                                           const double *const *lin_blocks, void *stream);
int stfem_stokes_st_vmult_slice_add_convection_space(stfem_stokes_ctx *ctx, int mode, int n_timesteps_at_once, int n_timedofs,
                                                     int variable_major, const double *Gamma, const double *Zeta,
                                                     double *const *dst_blocks, const double *src_u,
                                                     const double *src_p, const double *lin_u, void *stream);

/* Diagnostic of the convection cell kernel, at either degree: out[0] = workgroups of the last convection colour launch of the context,
 * out[1] = the longest run of cells one wave (degree 3) or half-wave (degree 2) walked in it.  STFEM_STOKES_Q3_WORKGROUPS=<n> in the
 * environment, read at every launch, caps the workgroups of the convection colour launches at either degree (tests: several cells per
 * wave or half-wave on a small mesh).  STFEM_ERR_UNSUPPORTED, with its reason in stfem_last_error, on a context that has launched no
 * convection kernel. */
int stfem_stokes_last_convection_plan(const stfem_stokes_ctx *ctx, int32_t out[2]);

#endif /* STFEM_STOKES_CONVECTION_SPACE_H */
