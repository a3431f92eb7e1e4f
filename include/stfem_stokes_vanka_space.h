/* The cell-patch Vanka smoother of the Stokes system by descriptor: velocity degree 2 or 3.  A companion of stfem.h, which includes it
 * (after stfem_stokes_space.h and the types it needs, inside its extern "C"): include stfem.h, not this file.  Its entry point takes
 * no device array. */
#ifndef STFEM_STOKES_VANKA_SPACE_H
#define STFEM_STOKES_VANKA_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_vanka_space.h where its types are declared"
#endif

/* One inverted block per cell of the LINEAR operator of the context, on boxes and general meshes alike: what the reference builds per
 * cell from its assembled matrix (include/stmg.h:704-742, compute_block_matrix.h:50-139) and applies in PreconditionVanka::vmult
 * (stmg.h:832-872), as tests/tp_03stokes.cc:714-726 sets it up over a two-variable BlockSlice:
 *     B_c((i, k), (j, l)) = valence(k) (Alpha(i, j) A(k, l) + [velocity, velocity] Beta(i, j) M(k, l)),
 * A = the assembled [[nu K, -B^T], [B, 0]] and M the assembled vector mass, restricted to the cell's DoFs, a strongly constrained DoF
 * keeping only the entries with itself; inverted by Gauss-Jordan with partial pivoting.
 *   velocity degree 2: exactly stfem_stokes_vanka_create_linearised(ctx, n_blocks, block_variable, Alpha, Beta, STFEM_CONVECTION_NONE,
 *     NULL, out): same code path, same bits (weak faces of the context included).
 *   velocity degree 3 (stfem_stokes_create_space): per time dof 192 velocity rows (3 components x 64 nodes a + 4 b + 16 c) and 27
 *     (FE_Q(2), nodes a + 3 b + 9 c) or 10 (FE_DGP(2), p[10 cell + j]) pressure rows: 219 / 202 rows for one time dof, 438 / 404 for two
 *     (cG(2), dG(1), or cG(1) with two time steps).  More than 512 rows (dG(2): 657 / 606): STFEM_ERR_UNSUPPORTED with the row count and
 *     the limit in stfem_last_error.  There are no class blocks at degree 3: a box gets one block per cell too.  The cell matrices are
 *     integrated at the operator's 4 x 4 x 4 Gauss points from its own 1D tables, MappingQ1 from the mesh vertices; the set-up runs on
 *     the device in batches of cell layers sized from the free memory (STFEM_VANKA_SETUP_LAYERS=<n> caps a batch); blocks that do not fit:
 *     STFEM_ERR_OUT_OF_MEMORY with the needed and free gigabytes in stfem_last_error.  The apply streams every block from HBM once
 *     (kpad * mpad * 8 bytes per cell: 1.57 MB at 438 rows), rows to a scratch array, then one collecting launch: two launches, no
 *     colours, no atomics, a fixed summation order.  fp64.
 * Refusals, all decided on the arguments before the context or the device is touched, each with its reason in stfem_last_error and
 * *out = NULL: a null ctx, desc, out, block_variable, Alpha or Beta, a non-zero reserved, n_blocks outside 1..8, a block_variable
 * outside 0..1: STFEM_ERR_INVALID_ARGUMENT.
 * The handle is an ordinary stfem_stokes_vanka: stfem_stokes_vanka_step, _vmult, _update (lin_blocks is not read: the same blocks again,
 * bit for bit), _setup_batches, _n_classes (the cell count) and _destroy work on it unchanged.
 * The blocks of the operator linearised about a velocity (the convection modes) come from the companion
 * stfem_stokes_vanka_linearised_space.h (stfem_stokes_vanka_create_linearised_space); this entry stays linear.
 * Not built at degree 3: class blocks, the CIP term, weak faces (a degree-3 context has neither), slabs, fp32. */
typedef struct {
  int32_t n_blocks;
  const int32_t *block_variable; /* n_blocks entries, 0 velocity / 1 pressure, BlockSlice order */
  const double *Alpha, *Beta;    /* host, n_blocks x n_blocks, row-major, in that block order */
  int32_t reserved[4];           /* must be 0 */
} stfem_stokes_vanka_space_desc;
int stfem_stokes_vanka_create_space(stfem_stokes_ctx *ctx, const stfem_stokes_vanka_space_desc *desc, stfem_stokes_vanka **out);

#endif /* STFEM_STOKES_VANKA_SPACE_H */
