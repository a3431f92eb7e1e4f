/* The Stokes operator by descriptor: velocity degree 2 or 3.  A companion of stfem.h, which includes it (after the types it needs,
 * inside its extern "C"): include stfem.h, not this file.  Its entry points take no device array. */
#ifndef STFEM_STOKES_SPACE_H
#define STFEM_STOKES_SPACE_H
#ifndef STFEM_H
#error "include stfem.h: it includes stfem_stokes_space.h where its types are declared"
#endif

/* The constructor by descriptor (like stfem_ctx_create on the scalar side).  reserved must be 0.
 *   velocity_degree 2: exactly the context of stfem_stokes_create_ex(mesh, 2, pressure_space, viscosity): same code path, same bits.
 *   velocity_degree 3: the pair the reference runs for time degree 2 (tests/tp_03stokes.cc:79-86: FE_Q(k+1)^dim x FE_DGP(k) or FE_Q(k),
 *     QGauss(k+2)).  Velocity FE_Q(3)^3 on Gauss-Lobatto nodes in the scalar FE_Q(3) numbering, ndu[d] = 3 ncell[d] + 1, component-
 *     major; pressure_space 0: FE_Q(2), ndp[d] = 2 ncell[d] + 1; pressure_space 1: FE_DGP(2), ten DoFs per cell, p[10 cell + j], cells
 *     lexicographic, deal.II's basis: the products l_i(xi) l_j(eta) l_k(zeta), i + j + k <= 2, of the orthonormal Legendre polynomials
 *     l_0 = 1, l_1 = sqrt 3 (2 x - 1), l_2 = sqrt 5 (6 x^2 - 6 x + 1) on [0, 1], i fastest: (0,0,0), (1,0,0), (2,0,0), (0,1,0),
 *     (1,1,0), (0,2,0), (0,0,1), (1,0,1), (0,1,1), (0,0,2).  QGauss(4), MappingQ1 from the mesh vertices (a constant diagonal
 *     Jacobian without vertices); dirichlet_mask constrains the velocity, the pressure is free; fp64.
 *     A degree-3 context has the LINEAR CELL OPERATOR and its per-cell Vanka smoother (stfem_stokes_vanka_create_space,
 *     stfem_stokes_vanka_space.h: the one Vanka constructor that serves it), and of the entries declared in stfem.h itself nothing else: n_velocity_dofs / n_pressure_dofs, the vector functions,
 *     stfem_stokes_vmult, _mass_vmult, _st_vmult, _st_vmult_slice_add (and with them the reference's Tvmult) and their _convection
 *     forms with STFEM_CONVECTION_NONE, all through one cell kernel (one wave per cell, eight colour launches, bitwise reproducible;
 *     boxes included: no Kronecker path).  Every other entry point that takes a Stokes context - weak / outflow faces, the convection
 *     modes, CIP, divergence, drag / lift, the face-point and Nitsche functions, the pressure helpers, the FE_DGP transfers, the Vanka
 *     constructors of stfem.h itself (stfem_stokes_vanka_create and the three _create_linearised forms) - returns STFEM_ERR_UNSUPPORTED with "<entry> is built for velocity degree 2 only" in stfem_last_error, before it
 *     touches the device and with its operands untouched (the int64_t counts return that status as their value).  The convection
 *     modes at degree 3 run through entries of their own, the _space forms of the three _convection entries
 *     (stfem_stokes_convection_space.h), and the Vanka smoother of the linear and of the linearised operator through
 *     stfem_stokes_vanka_create_space and _create_linearised_space (stfem_stokes_vanka_space.h, stfem_stokes_vanka_linearised_space.h);
 *     the pressure helpers, the FE_DGP transfers and the divergence likewise through the _space forms of their entries, with the
 *     getter stfem_stokes_get_space (stfem_stokes_pressure_space.h); the weak (Nitsche) / outflow faces of the linear operator, the
 *     face points and the Nitsche functional through the _space forms of theirs (stfem_stokes_boundary_space.h) - once weak faces
 *     are set there, the vmult entries above include the face launches and stfem_stokes_vanka_create_space builds blocks with the
 *     Nitsche terms.
 *     Not built at degree 3 either: with weak faces the inflow term of the convection modes and the linearised Vanka blocks (refused
 *     with their reason), CIP in the Vanka blocks, drag / lift, GMGStokes and the drivers, fp32.
 *     On z-slabs (a z-slab is a mesh of its own, the caller leaves its interface faces out of the masks; the interface planes of the
 *     velocity and of the FE_Q(2) pressure hold partial sums) the degree-3 context is held against the whole mesh for vmult, the
 *     modes without weak faces, st_vmult, st_vmult_slice_add, Tvmult, mass_vmult, the Nitsche functional, the divergence and the
 *     CIP term WITHOUT the interface faces (tests/test_gpu_stokes_q3_slabs.py).  Still missing there: stfem_stokes_set_cip_neighbours
 *     (the interface faces of the CIP term), the partitioned Vanka blocks, StokesSpaces::set_partition, GMGStokes.
 *   Any other degree: STFEM_ERR_UNSUPPORTED; non-zero reserved or a pressure_space outside 0..1: STFEM_ERR_INVALID_ARGUMENT; both
 *   with their reason in stfem_last_error. */
typedef struct {
  int32_t velocity_degree;
  int32_t pressure_space; /* 0 = FE_Q(degree - 1), 1 = FE_DGP(degree - 1) */
  double viscosity;
  int32_t reserved[4];
} stfem_stokes_space_desc;
int stfem_stokes_create_space(const stfem_mesh_desc *mesh, const stfem_stokes_space_desc *space, stfem_stokes_ctx **out);

/* Diagnostic of the cell kernel, at either degree: out[0] = workgroups of the last colour launch, out[1] = the longest run of cells
 * one wave (degree 3) or half-wave (degree 2) walked in it.  STFEM_STOKES_Q3_WORKGROUPS=<n> in the environment, read at every launch,
 * caps the workgroups of the colour launches of the cell kernel at either degree (tests: several cells per wave on a small mesh).
 * STFEM_ERR_UNSUPPORTED on a context that has never launched that kernel (a degree-2 box runs the Kronecker path instead). */
int stfem_stokes_last_cell_plan(const stfem_stokes_ctx *ctx, int32_t out[2]);

#endif /* STFEM_STOKES_SPACE_H */
