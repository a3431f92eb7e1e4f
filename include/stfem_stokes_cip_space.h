/* The CIP interior-face stabilisation (delta0) of the Stokes operator at velocity degree 2 or 3.  A companion of stfem.h, which includes
 * it (after stfem_stokes_boundary_space.h and the types it needs, inside its extern "C"): include stfem.h, not this file. */
#ifndef STFEM_STOKES_CIP_SPACE_H
#define STFEM_STOKES_CIP_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_cip_space.h where its types are declared"
#endif

/* stfem_stokes_set_cip and stfem_stokes_cip_add of stfem.h for a context of either degree: the same argument lists, the same contracts
 * (STFEM_CIP_WEIGHT_SOURCE / _LINEARISATION, delta0 == 0: no launch) and the same argument refusals, status for status (a null context
 * or array, a non-finite delta0, a weight outside the two: STFEM_ERR_INVALID_ARGUMENT; dst_u equal to src_u or weight_u:
 * STFEM_ERR_ALIAS).
 *   velocity degree 2: exactly the entry of stfem.h without the suffix: same code path, same bits.
 *   velocity degree 3 (stfem_stokes_create_space), where the entries of stfem.h refuse:
 *       C(w; u)(v) = sum_F int_F delta0 h_F^2 / 3^3.5 (w.n)^2 [d_n u] . [d_n v] dA     (operators.h:1605-1633, pa = degree^3.5)
 *     on the interior faces of FE_Q(3)^3 at the 4 x 4 Gauss points of a face (QGauss(4), lower tangential direction fastest), MappingQ1,
 *     h_F = sqrt(sum of the face's 16 JxW); entries of u and w on strongly constrained DoFs read as 0, constrained rows and the pressure
 *     rows receive nothing.  One wave per cell, which computes the jump on its up to six interior faces from its own and the
 *     neighbour's 3 x 64 source values and adds its own side's test contribution to its own 64 nodes; eight colour launches after every
 *     other launch of the same set on the same stream, plain read-add-write, faces and points ascending: no atomics, bitwise
 *     reproducible.
 *   set_cip_space: every later stfem_stokes_vmult, _st_vmult, _st_vmult_slice_add and the three _convection_space forms add the term
 *     last (cell operator, boundary launches of the weak faces, convection colours, CIP colours).  With STFEM_CIP_WEIGHT_LINEARISATION
 *     and a convection mode w is the linearisation velocity of the source's block, otherwise the source.  stfem_stokes_mass_vmult
 *     never gets the term.  Weak faces and CIP together run in the linear entries; a convection mode on a degree-3 context with weak
 *     faces stays STFEM_ERR_UNSUPPORTED (the inflow term), with or without CIP.
 *   cip_add_space: dst_u += C(weight_u; src_u) with the given delta0, independent of set_cip_space: the term by itself.
 * Still refused at degree 3, STFEM_ERR_UNSUPPORTED with the reason in stfem_last_error, before the device is touched: the entries of
 * stfem.h without the suffix, the slab entries (stfem_stokes_set_cip_neighbours, the ghost planes, _cip_pack, _cip_add_slab,
 * _cip_bind_ghosts) and a non-zero delta0 in the Vanka constructors. */
int stfem_stokes_set_cip_space(stfem_stokes_ctx *ctx, double delta0, int weight);
int stfem_stokes_cip_add_space(stfem_stokes_ctx *ctx, double *dst_u, const double *src_u, const double *weight_u, double delta0,
                               void *stream);

/* Diagnostic of the CIP kernel, at either degree: out[0] = workgroups of the last CIP colour launch of the context, out[1] = the
 * number of passes of its grid-stride loop, i.e. the longest run of cells one wave (degree 3) or half-wave (degree 2) walked in it.
 * STFEM_STOKES_CIP_WORKGROUPS=<n> in the environment, read at every launch, caps the workgroups of the CIP colour launches at either
 * degree (tests: several cells per wave on a small mesh); a value that is not a positive whole number is no cap.  STFEM_ERR_UNSUPPORTED, with its reason in stfem_last_error, on a context
 * that has not launched the CIP kernel (delta0 == 0 and a mesh without interior faces launch nothing). */
int stfem_stokes_last_cip_plan(const stfem_stokes_ctx *ctx, int32_t out[2]);

#endif /* STFEM_STOKES_CIP_SPACE_H */
