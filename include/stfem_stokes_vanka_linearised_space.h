/* The cell-patch Vanka smoother of the LINEARISED Stokes (Navier-Stokes) operator by descriptor: velocity degree 2 or 3.  A companion of
 * stfem.h, which includes it (after stfem_stokes_convection_space.h and the types it needs, inside its extern "C"): include stfem.h, not
 * this file. */
#ifndef STFEM_STOKES_VANKA_LINEARISED_SPACE_H
#define STFEM_STOKES_VANKA_LINEARISED_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_vanka_linearised_space.h where its types are declared"
#endif

/* One inverted block per cell of the operator linearised about lin_blocks, on boxes and general meshes alike: the block of
 * stfem_stokes_vanka_create_space with K of column block j = the assembled A(b_j), b_j = lin_blocks[j], as the comment of
 * stfem_stokes_vanka_create_linearised in stfem.h defines it (reinit_asm, include/stmg.h:929-965; operators.h:835-866, 1554-1567).
 *   velocity degree 2: exactly stfem_stokes_vanka_create_linearised(ctx, n_blocks, block_variable, Alpha, Beta, mode, lin_blocks, out):
 *     same code path, same bits - weak faces and their inflow term included.
 *   velocity degree 3 (stfem_stokes_create_space), STFEM_CONVECTION_NONE: the blocks of stfem_stokes_vanka_create_space, bit for bit;
 *     lin_blocks is not read.
 *   velocity degree 3, STFEM_CONVECTION_FORM / _JACOBIAN: the velocity-velocity entries of the cell matrices hold, at the operator's own
 *     4 x 4 x 4 Gauss points and with b_j read as read_dof_values reads it (an entry on a strongly constrained DoF counts as 0 and is
 *     never loaded: it may hold anything),
 *       form:      + ( - int (u (x) b) : grad v )                      (same component only)
 *       jacobian:  + ( - int (u (x) b) : grad v - int (b (x) u) : grad v )
 *     the forms stfem_stokes_st_vmult_convection_space applies.  A degree-3 context has no weak faces: there is no inflow term.
 *     Pressure rows and columns and the mass are those of the linear operator.  Equal pointers in lin_blocks are one state: the cell
 *     matrices are computed once per distinct state and batch of cell layers (153 600 B of LDS per workgroup, one cell per workgroup);
 *     assembly, constraints, valence, Alpha / Beta, Gauss-Jordan, block layout and the apply are those of
 *     stfem_stokes_vanka_create_space, and so are the row counts (219 / 202 per time dof), the limit of 512 rows (STFEM_ERR_UNSUPPORTED
 *     with the row count and the limit in stfem_last_error), the batching (STFEM_VANKA_SETUP_LAYERS) and STFEM_ERR_OUT_OF_MEMORY.
 * Refusals, all decided on the arguments in this order before the context is read or the device touched, each with its reason in
 * stfem_last_error and *out = NULL: a null out, ctx or desc, a non-zero reserved, n_blocks outside 1..8, a null block_variable, Alpha
 * or Beta, a block_variable outside 0..1, a mode outside 0..2, a null lin_blocks with a mode other than 0, a null entry of lin_blocks
 * for a velocity block with a mode other than 0: STFEM_ERR_INVALID_ARGUMENT.
 * The handle is an ordinary stfem_stokes_vanka.  stfem_stokes_vanka_update(v, lin_blocks) on a handle created with a mode rebuilds the
 * blocks about the new states into the same storage (a null lin_blocks or velocity entry: STFEM_ERR_INVALID_ARGUMENT, as at degree 2);
 * on a handle created with STFEM_CONVECTION_NONE lin_blocks is not read.
 * Not built at degree 3: the CIP term in the blocks, weak faces and their inflow term (a degree-3 context has neither), class blocks,
 * blocks beyond 512 rows, slabs, fp32. */
typedef struct {
  int32_t n_blocks;
  const int32_t *block_variable;   /* n_blocks entries, 0 velocity / 1 pressure, BlockSlice order */
  const double *Alpha, *Beta;      /* host, n_blocks x n_blocks, row-major, in that block order */
  int32_t mode;                    /* STFEM_CONVECTION_NONE / _FORM / _JACOBIAN */
  const double *const *lin_blocks; /* n_blocks DEVICE pointers in BlockSlice order; only velocity entries are read, pressure entries
                                      may be null; may be null altogether with mode 0; equal pointers = one state */
  int32_t reserved[4];             /* must be 0 */
} stfem_stokes_vanka_linearised_space_desc;
int stfem_stokes_vanka_create_linearised_space(stfem_stokes_ctx *ctx, const stfem_stokes_vanka_linearised_space_desc *desc,
                                               stfem_stokes_vanka **out);

#endif /* STFEM_STOKES_VANKA_LINEARISED_SPACE_H */
