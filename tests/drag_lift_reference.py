"""Plain numpy restatement of StokesMatrixFreeOperator::compute_drag_lift (reference include/operators.h:1344-1389),
    f = scale sum_{faces of the mask} sum_{boundary cells} sum_{q < 9} ( p n - nu (grad u + grad u^T) n ) JxW_face,
written independently of the kernel's staging: dense per-cell tables of tests/navier_reference.py evaluated at the nine face points
(no end-point tables, no sum factorisation), the MappingQ1 Jacobian from the eight vertices, the outward normal and the area element
from the CROSS PRODUCT of the two face tangents (not from J^-T e_d).  A helper of tests/test_drag_lift_reference_cpu.py,
tests/test_gpu_stokes_drag_lift.py and tests/test_host_drag_lift.py, not a test module.

Vectors: velocity 3 * n_u doubles, component-major, every component lexicographic on the (2 ncell + 1)^3 lattice (x fastest); pressure
FE_Q(1) lexicographic on the (ncell + 1)^3 lattice, or FE_DGP(1): p[4 cell + j] with the basis 1, l(xi), l(eta), l(zeta),
l(x) = sqrt 3 (2 x - 1); vertices [(ncell + 1)^3][3].  Faces f = 2 d + s.  Items: faces ascending, the cells of a face lexicographic
with the lower tangential axis fastest."""
import numpy as np

import navier_reference as nref


def face_cells(ncell, face_mask):
    """[(face, (cx, cy, cz))] in item order"""
    out = []
    for f in range(6):
        if not face_mask >> f & 1:
            continue
        d, s = f // 2, f % 2
        t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
        for c2 in range(ncell[t2]):
            for c1 in range(ncell[t1]):
                cc = [0, 0, 0]
                cc[d], cc[t1], cc[t2] = (ncell[d] - 1 if s else 0), c1, c2
                out.append((f, tuple(cc)))
    return out


def n_items(ncell, face_mask):
    return len(face_cells(ncell, face_mask))


def _pressure_at(p, ncell, cc, pts, N, dg_pressure):
    """the pressure of cell cc at the reference points pts"""
    if dg_pressure:
        cell = cc[0] + ncell[0] * (cc[1] + ncell[1] * cc[2])
        leg = np.sqrt(3.0) * (2.0 * pts - 1.0)
        c = p[4 * cell:4 * cell + 4]
        return c[0] + leg @ c[1:4]
    nd = [n + 1 for n in ncell]
    dofs = np.array([(cc[0] + i) + nd[0] * ((cc[1] + j) + nd[1] * (cc[2] + k)) for k in range(2) for j in range(2) for i in range(2)])
    return N @ p[dofs]


def drag_lift(u, p, ncell, vertices, viscosity, face_mask, dirichlet_mask=0, plain=False, dg_pressure=False, scale=1.0, nq=3):
    """-> (force [3], items [n_items][3] (unscaled), A = sum |tau_k| JxW over all contributing points and components (unscaled): the
    scale of a rounding bound).  plain=False: velocity entries on the strongly constrained DoFs of dirichlet_mask read as 0."""
    ncell = tuple(int(n) for n in ncell)
    U = np.array(u, dtype=np.float64).reshape(3, nref.n_velocity(ncell))
    if not plain:
        U[:, nref.constrained(ncell, dirichlet_mask)] = 0.0
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    xq, wq = nref.gauss01(nq)
    items, A = [], 0.0
    tables = {}
    for f, cc in face_cells(ncell, face_mask):
        d, s = f // 2, f % 2
        t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
        if f not in tables:
            pts = np.zeros((nq * nq, 3)); wts = np.zeros(nq * nq)
            for q2 in range(nq):
                for q1 in range(nq):
                    pts[q1 + nq * q2, d], pts[q1 + nq * q2, t1], pts[q1 + nq * q2, t2] = s, xq[q1], xq[q2]
                    wts[q1 + nq * q2] = wq[q1] * wq[q2]
            tables[f] = (pts, wts) + tuple(nref.tables_3d(pts))
        pts, wts, phi, dphi, N, dN = tables[f]
        dofs = nref._cell_dofs(ncell, *cc)
        V = nref._cell_vertices(ncell, vertices, *cc)
        J = np.einsum("vd,qve->qde", V, dN)                    # dx_d / dxi_e
        Jinv = np.linalg.inv(J)                                # dxi_e / dx_j
        # the face is xi_d = s: its tangents are the columns t1, t2 of J; t1 x t2 points along +e_d for d = 0, 2 and -e_d for d = 1
        cross = np.cross(J[:, :, t1], J[:, :, t2])
        area = np.linalg.norm(cross, axis=1)
        normal = cross / area[:, None] * ((1.0 if s else -1.0) * (-1.0 if d == 1 else 1.0))
        JxW = area * wts
        grad = np.einsum("in,qne,qej->qij", U[:, dofs], dphi, Jinv)   # d u_i / d x_j
        pq = _pressure_at(p, ncell, cc, pts, N, dg_pressure)
        tau = pq[:, None] * normal - viscosity * np.einsum("qij,qj->qi", grad + np.swapaxes(grad, 1, 2), normal)
        items.append(np.einsum("qi,q->i", tau, JxW))
        A += float(np.sum(np.abs(tau) * JxW[:, None]))
    items = np.array(items).reshape(-1, 3)
    return scale * items.sum(axis=0), items, A


# ---- fields that lie exactly in the spaces


def velocity_lattice(ncell, vertices):
    """[n_u][3]: the positions of the velocity DoFs under MappingQ1 (vertices, edge / face / cell midpoints of the trilinear map)"""
    nd = [2 * n + 1 for n in ncell]
    nv = [n + 1 for n in ncell]
    V = np.asarray(vertices, dtype=np.float64).reshape(nv[2], nv[1], nv[0], 3)
    X = np.zeros((nd[2], nd[1], nd[0], 3))
    for k in range(nd[2]):
        for j in range(nd[1]):
            for i in range(nd[0]):
                ks, js, is_ = ({k // 2, (k + 1) // 2}, {j // 2, (j + 1) // 2}, {i // 2, (i + 1) // 2})
                X[k, j, i] = np.mean([V[c, b, a] for c in ks for b in js for a in is_], axis=0)
    return X.reshape(-1, 3)


def pressure_lattice(ncell, vertices):
    return np.asarray(vertices, dtype=np.float64).reshape(-1, 3)


def poiseuille(ncell, L, viscosity, c, dg_pressure=False):
    """u = (y (1 - y), 0, 0), p = -2 nu x + c on the box [0, Lx] x [0, 1] x [0, Lz] -> (u, p, vertices)"""
    verts = nref.perturbed_vertices(ncell, 0.0, 0, (0, 0, 0), (L[0], 1.0, L[2]))
    X = velocity_lattice(ncell, verts)
    u = np.concatenate([X[:, 1] * (1 - X[:, 1]), 0 * X[:, 0], 0 * X[:, 0]])
    if not dg_pressure:
        return u, -2 * viscosity * verts[:, 0] + c, verts
    p = np.zeros(4 * int(np.prod(ncell)))
    hx = L[0] / ncell[0]
    for cell in range(int(np.prod(ncell))):
        cx = cell % ncell[0]
        # -2 nu (x0 + hx xi) + c = [c - 2 nu (x0 + hx / 2)] 1 + [-nu hx / sqrt 3] l(xi)
        p[4 * cell] = c - 2 * viscosity * (cx + 0.5) * hx
        p[4 * cell + 1] = -viscosity * hx / np.sqrt(3.0)
    return u, p, verts


def poiseuille_forces(L, viscosity, c):
    """the closed forms of the six faces"""
    Lx, Lz, nu = L[0], L[2], viscosity
    return {0: (-c * Lz, 0, 0), 1: ((c - 2 * nu * Lx) * Lz, 0, 0),
            2: (nu * Lx * Lz, (nu * Lx ** 2 - c * Lx) * Lz, 0), 3: (nu * Lx * Lz, (c * Lx - nu * Lx ** 2) * Lz, 0),
            4: (0, 0, -(c * Lx - nu * Lx ** 2)), 5: (0, 0, c * Lx - nu * Lx ** 2)}
