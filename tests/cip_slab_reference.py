"""Plain numpy restatement of the CIP interior-face term on ONE z-slab of a partitioned mesh, written from the formulas of
tests/cip_reference.py, not from the kernel.  The slab rule: every cell adds, per interior face, only its OWN side's test
contribution to its own 27 nodes,
  + delta_F ([d_n u]_own - [d_n u]_other) d_n v_own JxW,
with the normal, the face JxW, h_F and the weight velocity of its own side (the face is one bilinear patch: both sides compute the
same surface element and the same normal up to its sign, which enters squared).  Face 4 of the bottom cell layer / face 5 of the top
one is interior where the slab has a neighbour there; the neighbour cell is read through TWO ghost DoF planes per side (what `pack`
makes on the sender: its two planes next to the interface plane, zeros on the DoFs the sender constrains strongly) and ONE ghost
vertex plane per side.  The interface planes of the result hold partial sums; stokes_slab_cases.assemble completes them.

A helper of tests/test_cip_slab_contract_cpu.py and tests/test_gpu_stokes_cip_slabs.py, not a test module.  Vectors and vertices as in
tests/navier_reference.py; slabs as stokes_slab_cases.Slab."""
import numpy as np

import cip_reference as cref
import navier_reference as nref

LOWER, UPPER = 16, 32  # neighbour_mask bits: face 4 / face 5 is shared with a neighbour slab

# The cases of the per-cell two-variable Vanka blocks on slabs, specs as stokes_vanka_cip_reference.CASES, with their cuts in cell
# layers ("box224_jac_dg1" is a case of that table).  tests/test_cip_slab_contract_cpu.py records their conditioning, which is what a
# bound of 1e-10 on the applied smoother rests on.
VANKA_SLAB_SPECS = {
    "pert224_jac": ((2, 2, 4), True, 2, False, 0, 1, 1, 63, 0, True),
    "pert223_form_dgp_cg2_tm": ((2, 2, 3), True, 1, True, 0, 2, 1, 63, 0, False),
    "pert323_jac_weakx": ((3, 2, 3), True, 2, True, 0, 1, 1, 0b111100, 0b000011, True),  # weak x faces cut by the interface
}
VANKA_SLAB_CUTS = {
    "box224_jac_dg1": ((0, 2, 4), (0, 1, 4), (0, 1, 2, 4)),
    "pert224_jac": ((0, 2, 4), (0, 1, 3, 4)),
    "pert223_form_dgp_cg2_tm": ((0, 1, 3),),
    "pert323_jac_weakx": ((0, 2, 3),),
}


def plane_size(ncell):
    return (2 * ncell[0] + 1) * (2 * ncell[1] + 1)


def pack(u, ncell, strong, side):
    """[3][2][plane], flat: what the neighbour on `side` (0 lower, 1 upper) needs of u - this slab's DoF planes 1, 2 (side 0) or
    ndz - 3, ndz - 2 (side 1), ascending z, entries on this slab's strongly constrained DoFs as 0"""
    ndz = 2 * ncell[2] + 1
    U = nref._read(u, ncell, strong).reshape(3, ndz, plane_size(ncell))
    return (U[:, 1:3] if side == 0 else U[:, ndz - 3:ndz - 1]).reshape(-1).copy()


def neighbour_mask(slab):
    return (LOWER if slab.has_lower else 0) | (UPPER if slab.has_upper else 0)


def ghost_vertex_planes(verts, nc, slab):
    """(lower, upper): the global vertex planes one cell layer beyond the slab's interfaces, [(ncx + 1)(ncy + 1)][3], or None"""
    V = np.asarray(verts).reshape(nc[2] + 1, -1, 3)
    return (V[slab.z0 - 1].copy() if slab.has_lower else None, V[slab.z1 + 1].copy() if slab.has_upper else None)


def cip_slab(delta0, w, u, ncell, vertices, strong, mask=0, lower_ghost=None, upper_ghost=None, lower_vertices=None,
             upper_vertices=None, nq=3):
    """flat [3 n_u] of the slab: the own-side contributions of all its cells; mask 0 is the term on the slab's inner faces alone"""
    ndz, plane = 2 * ncell[2] + 1, plane_size(ncell)
    vplane = (ncell[0] + 1) * (ncell[1] + 1)
    # the slab with two DoF planes and one vertex plane on either side: DoF plane jz at jz + 2, cell layer cz at cz + 1
    U = np.zeros((3, ndz + 4, plane))
    U[:, 2:ndz + 2] = nref._read(u, ncell, strong).reshape(3, ndz, plane)
    V = np.zeros((ncell[2] + 3, vplane, 3))
    V[1:ncell[2] + 2] = np.asarray(vertices, dtype=np.float64).reshape(ncell[2] + 1, vplane, 3)
    if mask & LOWER:
        U[:, 0:2] = np.asarray(lower_ghost).reshape(3, 2, plane)
        V[0] = np.asarray(lower_vertices).reshape(vplane, 3)
    if mask & UPPER:
        U[:, ndz + 2:ndz + 4] = np.asarray(upper_ghost).reshape(3, 2, plane)
        V[ncell[2] + 2] = np.asarray(upper_vertices).reshape(vplane, 3)
    next_ = (ncell[0], ncell[1], ncell[2] + 2)  # the extended mesh: cells and DoFs addressed with the helpers of the whole-mesh code
    U = U.reshape(3, -1)
    W = nref._read(w, ncell, strong)
    con = nref.constrained(ncell, strong)
    out = np.zeros((3, nref.n_velocity(ncell)))
    for d in range(3):
        for s in (0, 1):
            pts_own, wts = cref.face_rule(d, float(s), nq)
            pts_nb, _ = cref.face_rule(d, float(1 - s), nq)
            phi, dphi_own, _, dN_own = nref.tables_3d(pts_own)
            _, dphi_nb, _, dN_nb = nref.tables_3d(pts_nb)
            for cz in range(ncell[2]):
                for cy in range(ncell[1]):
                    for cx in range(ncell[0]):
                        own = [cx, cy, cz]
                        nb = list(own); nb[d] += 1 if s else -1
                        inside = 0 <= nb[d] < ncell[d]
                        if not inside and not (d == 2 and mask & (UPPER if s else LOWER)):
                            continue  # a boundary face
                        dofs = nref._cell_dofs(ncell, *own)
                        dofs_own = nref._cell_dofs(next_, cx, cy, cz + 1)
                        dofs_nb = nref._cell_dofs(next_, nb[0], nb[1], nb[2] + 1)
                        J_own = np.einsum("vd,qve->qde", nref._cell_vertices(next_, V, cx, cy, cz + 1), dN_own)
                        J_nb = np.einsum("vd,qve->qde", nref._cell_vertices(next_, V, nb[0], nb[1], nb[2] + 1), dN_nb)
                        Ji_own, Ji_nb = np.linalg.inv(J_own), np.linalg.inv(J_nb)
                        m = Ji_own[:, d, :]                                        # J^-T e_d of the cell's own side
                        length = np.linalg.norm(m, axis=1)
                        normal = m / length[:, None]
                        JxW = np.abs(np.linalg.det(J_own)) * length * wts
                        h2 = JxW.sum()
                        dn_own = np.einsum("qne,qej,qj->qn", dphi_own, Ji_own, normal)
                        dn_nb = np.einsum("qne,qej,qj->qn", dphi_nb, Ji_nb, normal)
                        wn = np.einsum("iq,qi->q", W[:, dofs] @ phi.T, normal)
                        delta = delta0 * (h2 / cref.PA) * wn * wn
                        jump = U[:, dofs_own] @ dn_own.T - U[:, dofs_nb] @ dn_nb.T  # [3][q]
                        out[:, dofs] += np.einsum("q,iq,qn->in", delta * JxW, jump, dn_own)
    out[:, con] = 0.0
    return out.reshape(-1)


def slab_ghosts(parts, slabs_):
    """per slab (lower_ghost, upper_ghost): what its neighbours pack of their cut of a whole-mesh field; parts[r]: slab r's cut"""
    out = []
    for r, s in enumerate(slabs_):
        lo = pack(parts[r - 1], slabs_[r - 1].ncell, slabs_[r - 1].strong, 1) if s.has_lower else None
        up = pack(parts[r + 1], slabs_[r + 1].ncell, slabs_[r + 1].strong, 0) if s.has_upper else None
        out.append((lo, up))
    return out
