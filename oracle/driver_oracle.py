"""CPU restatement (numpy, fp64) of what the slab drivers need around the operator (include/stfem.h: stfem_support_points,
stfem_quadrature_points, stfem_integrate_rhs, stfem_integrate_difference, and the pressure helpers of the Stokes context):
nodal points, Gauss points, load vectors, error norms, the FE_DGP(1) / FE_Q(1) pressure functions and their transfers.
TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product path, and it never calls the product library.

Everything is built here from the formulas: Lagrange polynomials on the Gauss-Lobatto nodes of oracle.gauss_lobatto, the
trilinear (MappingQ1) map and its Jacobian from the vertex array, the Gauss rule of numpy.polynomial.legendre.leggauss mapped
to [0, 1].  Numbering as in include/stfem.h: DoF index = ix + nx (iy + ny iz), nx = p ncell[0] + 1; cells lexicographic, x
fastest; points of a cell q = qx + nq (qy + nq qz); vertices [(ncell + 1)^3][3], x fastest.  Arrays over the points of a cell
are kept as [cell, qz, qy, qx] and arrays over its DoFs as [cell, az, ay, ax], which flatten to that numbering.

Checked by tests/test_driver_oracle_cpu.py against facts that do not come from it (volumes, exact integrals of polynomials,
affine functions on perturbed meshes)."""
import numpy as np

from . import oracle as _o

SQRT3 = np.sqrt(3.0)


def gauss_rule(nq):
    """QGauss(nq) on [0, 1]: (points ascending, weights)"""
    x, w = np.polynomial.legendre.leggauss(nq)
    return 0.5 * (x + 1.0), 0.5 * w


def lagrange_tables(nodes, x):
    """S[q, a] = l_a(x_q), D[q, a] = l_a'(x_q) for the Lagrange polynomials on `nodes`"""
    nodes, x = np.asarray(nodes, float), np.asarray(x, float)
    n = len(nodes)
    S, D = np.ones((len(x), n)), np.zeros((len(x), n))
    for a in range(n):
        for m in range(n):
            if m == a:
                continue
            S[:, a] *= (x - nodes[m]) / (nodes[a] - nodes[m])
            term = np.full(len(x), 1.0 / (nodes[a] - nodes[m]))
            for k in range(n):
                if k != a and k != m:
                    term *= (x - nodes[k]) / (nodes[a] - nodes[k])
            D[:, a] += term
    return S, D


def box_vertices(ncell, lower, upper):
    """vertex array of the axis-aligned box [lower, upper] with ncell cells"""
    ax = [np.linspace(lower[d], upper[d], ncell[d] + 1) for d in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3)


def _cell_corners(ncell, vertices):
    """[cell, k, j, i, 3]: the eight vertices of every cell"""
    nx, ny, nz = ncell
    V = np.asarray(vertices, float).reshape(nz + 1, ny + 1, nx + 1, 3)
    out = np.empty((nz, ny, nx, 2, 2, 2, 3))
    for k in range(2):
        for j in range(2):
            for i in range(2):
                out[:, :, :, k, j, i] = V[k:k + nz, j:j + ny, i:i + nx]
    return out.reshape(nx * ny * nz, 2, 2, 2, 3)


def _geometry(ncell, vertices, xi):
    """the trilinear map at the tensor points xi x xi x xi of every cell: x [cell, qz, qy, qx, 3] and
    J [cell, qz, qy, qx, d, e] = d x_d / d xi_e"""
    xi = np.asarray(xi, float)
    C = _cell_corners(ncell, vertices)
    N = np.stack([1.0 - xi, xi], axis=1)                      # [q, corner]
    dN = np.stack([-np.ones_like(xi), np.ones_like(xi)], axis=1)
    x = np.einsum("ckjid,xi,yj,zk->czyxd", C, N, N, N)
    J = np.empty(x.shape + (3,))
    J[..., 0] = np.einsum("ckjid,xi,yj,zk->czyxd", C, dN, N, N)
    J[..., 1] = np.einsum("ckjid,xi,yj,zk->czyxd", C, N, dN, N)
    J[..., 2] = np.einsum("ckjid,xi,yj,zk->czyxd", C, N, N, dN)
    return x, J


def _cell_dofs(p, ncell):
    """[cell, az, ay, ax] -> global DoF index"""
    nx, ny, nz = ncell
    ndx, ndy = p * nx + 1, p * ny + 1
    a = np.arange(p + 1)
    cx, cy, cz = np.arange(nx), np.arange(ny), np.arange(nz)
    ix = (p * cx[:, None] + a[None, :])                       # [cx, ax]
    iy = (p * cy[:, None] + a[None, :])
    iz = (p * cz[:, None] + a[None, :])
    idx = (ix[None, None, :, None, None, :] + ndx * (iy[None, :, None, None, :, None] + ndy * iz[:, None, None, :, None, None]))
    return idx.reshape(nx * ny * nz, p + 1, p + 1, p + 1)


def n_dofs(p, ncell):
    return int(np.prod([p * c + 1 for c in ncell]))


def constrained(p, ncell, dirichlet_mask):
    """bool [ndofs]: bit 2 d = lower, 2 d + 1 = upper face of direction d"""
    nd = [p * c + 1 for c in ncell]
    con = np.zeros((nd[2], nd[1], nd[0]), bool)
    for d in range(3):
        for side in range(2):
            if dirichlet_mask >> (2 * d + side) & 1:
                idx = [slice(None)] * 3
                idx[2 - d] = -1 if side else 0
                con[tuple(idx)] = True
    return con.ravel()


def support_points(p, ncell, vertices):
    """[ndofs, 3]: the nodes in the order of the vectors"""
    nodes = _o.gauss_lobatto(p + 1)
    x, _ = _geometry(ncell, vertices, nodes)
    out = np.zeros((n_dofs(p, ncell), 3))
    out[_cell_dofs(p, ncell).ravel()] = x.reshape(-1, 3)      # shared nodes: the cells agree up to round-off
    return out


def quadrature_points(p, ncell, vertices, nq):
    """[cell, nq^3, 3]"""
    xq, _ = gauss_rule(nq)
    x, _ = _geometry(ncell, vertices, xq)
    return x.reshape(x.shape[0], nq ** 3, 3)


def _jxw(ncell, vertices, nq):
    xq, wq = gauss_rule(nq)
    _, J = _geometry(ncell, vertices, xq)
    W = wq[:, None, None] * wq[None, :, None] * wq[None, None, :]
    return np.linalg.det(J) * W[None], J


def load_vector(p, ncell, vertices, nq, f_at_points, dirichlet_mask=0):
    """rhs_a = sum_q JxW f_q phi_a(x_q), constrained rows 0; f_at_points [cell, nq^3]"""
    xq, _ = gauss_rule(nq)
    S, _ = lagrange_tables(_o.gauss_lobatto(p + 1), xq)
    JxW, _ = _jxw(ncell, vertices, nq)
    F = JxW * np.asarray(f_at_points, float).reshape(JxW.shape)
    local = np.einsum("czyx,zk,yj,xi->ckji", F, S, S, S)
    out = np.zeros(n_dofs(p, ncell))
    np.add.at(out, _cell_dofs(p, ncell).ravel(), local.ravel())
    out[constrained(p, ncell, dirichlet_mask)] = 0.0
    return out


def difference(p, ncell, vertices, nq, u, exact, exact_grad=None):
    """(sum JxW (u_h - exact)^2, max |u_h - exact|, sum JxW |J^-T grad_ref u_h - exact_grad|^2) over QGauss(nq)^3 of the cells;
    exact [cell, nq^3], exact_grad [cell, nq^3, 3] or None (third entry 0)"""
    xq, _ = gauss_rule(nq)
    S, D = lagrange_tables(_o.gauss_lobatto(p + 1), xq)
    JxW, J = _jxw(ncell, vertices, nq)
    ul = np.asarray(u, float)[_cell_dofs(p, ncell)]
    val = np.einsum("ckji,zk,yj,xi->czyx", ul, S, S, S)
    e = val - np.asarray(exact, float).reshape(val.shape)
    l2 = float(np.sum(JxW * e * e))
    linf = float(np.abs(e).max())
    if exact_grad is None:
        return l2, linf, 0.0
    gref = np.stack([np.einsum("ckji,zk,yj,xi->czyx", ul, S, S, D),
                     np.einsum("ckji,zk,yj,xi->czyx", ul, S, D, S),
                     np.einsum("ckji,zk,yj,xi->czyx", ul, D, S, S)], axis=-1)     # d / d xi_e
    Jinv = np.linalg.inv(J)                                                        # [.., e, d] = d xi_e / d x_d
    g = np.einsum("...ed,...e->...d", Jinv, gref)                                  # J^-T grad_ref
    dg = g - np.asarray(exact_grad, float).reshape(g.shape)
    return l2, linf, float(np.sum(JxW[..., None] * dg * dg))


# ------------------------------------------------------------------------------------------------ pressure spaces

def _tensor_xi(nq):
    """[nq^3, 3] reference points of QGauss(nq)^3, q = qx + nq (qy + nq qz)"""
    xq, _ = gauss_rule(nq)
    Z, Y, X = np.meshgrid(xq, xq, xq, indexing="ij")
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3)


def dgp_values(ncell, coeffs, xi):
    """FE_DGP(1): p_h = c0 + c1 l(xi) + c2 l(eta) + c3 l(zeta), l(x) = sqrt 3 (2 x - 1), four coefficients per cell
    (coeffs[4 cell + j]); xi: reference points [npts, 3] (the same in every cell) or [cell, npts, 3] -> [cell, npts]"""
    c = np.asarray(coeffs, float).reshape(int(np.prod(ncell)), 4)
    xi = np.asarray(xi, float)
    if xi.ndim == 2:
        xi = np.broadcast_to(xi[None], (c.shape[0],) + xi.shape)
    leg = SQRT3 * (2.0 * xi - 1.0)
    return c[:, None, 0] + c[:, None, 1] * leg[..., 0] + c[:, None, 2] * leg[..., 1] + c[:, None, 3] * leg[..., 2]


def q1_values(ncell, nodal, xi):
    """FE_Q(1) with nodal values in the scalar degree-1 numbering; xi as in dgp_values -> [cell, npts]"""
    ul = np.asarray(nodal, float)[_cell_dofs(1, ncell)]       # [cell, k, j, i]
    xi = np.asarray(xi, float)
    if xi.ndim == 2:
        xi = np.broadcast_to(xi[None], (ul.shape[0],) + xi.shape)
    N = np.stack([1.0 - xi, xi], axis=-1)                     # [cell, pt, d, corner]
    return np.einsum("ckji,cqi,cqj,cqk->cq", ul, N[..., 0, :], N[..., 1, :], N[..., 2, :])


def pressure_values(ncell, p, xi, dg):
    return dgp_values(ncell, p, xi) if dg else q1_values(ncell, p, xi)


def pressure_quadrature_points(ncell, vertices, nq):
    return quadrature_points(1, ncell, vertices, nq)


def pressure_difference(ncell, vertices, nq, p, exact, dg):
    """(sum JxW (p_h - exact)^2, max |p_h - exact|) over QGauss(nq)^3 of the cells; exact [cell, nq^3]"""
    JxW, _ = _jxw(ncell, vertices, nq)
    e = pressure_values(ncell, p, _tensor_xi(nq), dg) - np.asarray(exact, float).reshape(JxW.shape[0], -1)
    return float(np.sum(JxW.reshape(e.shape) * e * e)), float(np.abs(e).max())


def pressure_mean(ncell, vertices, p, dg, nq=2):
    """(mean value of p_h, volume) by quadrature (QGauss(2) integrates both spaces exactly on a box)"""
    JxW, _ = _jxw(ncell, vertices, nq)
    v = pressure_values(ncell, p, _tensor_xi(nq), dg)
    vol = float(JxW.sum())
    return float(np.sum(JxW.reshape(v.shape) * v)) / vol, vol


def dgp_parent(ncell_fine):
    """for every fine cell: (index of its parent in the mesh with half the cells, child position [3] in {0, 1})"""
    nx, ny, nz = ncell_fine
    assert nx % 2 == 0 and ny % 2 == 0 and nz % 2 == 0
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    parent = (cx // 2) + (nx // 2) * ((cy // 2) + (ny // 2) * (cz // 2))
    return parent.ravel(), np.stack([cx % 2, cy % 2, cz % 2], axis=-1).reshape(-1, 3)


def dgp_coarse_values_on_fine(ncell_fine, coarse_coeffs, xi):
    """the coarse FE_DGP(1) function at the reference points xi [npts, 3] of every FINE cell -> [fine cell, npts]"""
    parent, child = dgp_parent(ncell_fine)
    c = np.asarray(coarse_coeffs, float).reshape(-1, 4)[parent]
    xi_parent = 0.5 * (child[:, None, :] + np.asarray(xi, float)[None])
    return dgp_values(ncell_fine, c.ravel(), xi_parent)


def dgp_prolongate(ncell_fine, coarse_coeffs):
    """embedding of the coarse FE_DGP(1) function into the mesh with twice the cells: the L2 projection on every child (the basis
    is orthonormal on the reference cell), by QGauss(2)^3, which is exact for the products of two linear functions"""
    xi = _tensor_xi(2)
    _, w = gauss_rule(2)
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    v = dgp_coarse_values_on_fine(ncell_fine, coarse_coeffs, xi)               # [fine cell, 8]
    leg = SQRT3 * (2.0 * xi - 1.0)
    basis = np.concatenate([np.ones((len(xi), 1)), leg], axis=1)               # [pt, 4]
    return np.einsum("cq,q,qj->cj", v, W, basis).ravel()
