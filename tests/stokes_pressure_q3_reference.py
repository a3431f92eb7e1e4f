"""Plain numpy restatement of the pressure space helpers and of the divergence functional of the Stokes operator for pressure degree
d = 1 or 2 (velocity degree d + 1), written independently of the kernels: function values of FE_Q(d) / FE_DGP(d) at QGauss(nq)^3,
the mean weights, the dense embedding of a FE_DGP(d) function into the 2 x 2 x 2 children of its cell (an L2 projection by
quadrature, not the closed 1D formulas the library uses), and compute_divergence (reference include/operators.h:1391-1439) for a
velocity of degree 2 or 3 on any MappingQ1 mesh with the full 3D tables of tests/navier_q3_reference.py.  A helper of
tests/test_stokes_pressure_q3_reference_cpu.py, tests/test_gpu_stokes_q3_pressure.py, tests/test_gpu_stokes_q3_divergence.py and
tests/test_gpu_guard_bands_stokes_q3_pressure.py, not a test module.

Vectors: FE_Q(d) pressure on the (d ncell + 1)^3 lattice, x fastest; FE_DGP(d) pressure p[n cell + j], cells lexicographic, the
functions l_i(xi) l_j(eta) l_k(zeta), i + j + k <= d, i fastest, of the orthonormal Legendre polynomials on [0, 1]; velocity 3 * n_u
doubles, component-major; vertices [(ncell + 1)^3][3], x fastest.  Boxes are given by (lower, upper)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_q3_reference as nq3  # noqa: E402

gauss01 = nq3.gauss01


def legendre01(x):
    """[..., 3]: l_0 = 1, l_1 = sqrt 3 (2 x - 1), l_2 = sqrt 5 (6 x^2 - 6 x + 1)"""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([np.ones_like(x), np.sqrt(3.0) * (2 * x - 1), np.sqrt(5.0) * (6 * x * x - 6 * x + 1)], axis=-1)


def dgp_functions(d):
    """the (i, j, k) of the FE_DGP(d) functions in their order: i fastest"""
    return [(i, j, k) for k in range(d + 1) for j in range(d + 1) for i in range(d + 1) if i + j + k <= d]


def n_pressure(d, ncell, dg):
    return len(dgp_functions(d)) * int(np.prod(ncell)) if dg else int(np.prod([d * n + 1 for n in ncell]))


def tensor_xi(nq):
    """[nq^3, 3] reference points of QGauss(nq)^3, q = qx + nq (qy + nq qz), and their weights [nq^3]"""
    x, w = gauss01(nq)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    WZ, WY, WX = np.meshgrid(w, w, w, indexing="ij")
    return np.stack([X, Y, Z], axis=-1).reshape(-1, 3), (WX * WY * WZ).reshape(-1)


def dgp_basis(d, xi):
    """[..., n]: the FE_DGP(d) functions at the reference points xi [..., 3]"""
    L = legendre01(xi)  # [..., 3 (direction), 3 (function)]
    return np.stack([L[..., 0, i] * L[..., 1, j] * L[..., 2, k] for i, j, k in dgp_functions(d)], axis=-1)


def q_basis(d, xi):
    """[..., (d + 1)^3]: the FE_Q(d) functions on the nodes m / d at xi [..., 3], function a + (d + 1) (b + (d + 1) c)"""
    nodes = np.linspace(0.0, 1.0, d + 1)
    xi = np.asarray(xi, dtype=np.float64)
    one = []
    for e in range(3):
        S, _ = nq3.lagrange_1d(nodes, xi[..., e].reshape(-1))
        one.append(S.reshape(xi.shape[:-1] + (d + 1,)))
    return np.stack([one[0][..., a] * one[1][..., b] * one[2][..., c] for c in range(d + 1) for b in range(d + 1) for a in range(d + 1)], axis=-1)


def q_cell_dofs(d, ncell):
    """[cell, (d + 1)^3] lattice indices of the FE_Q(d) nodes of every cell"""
    nd = [d * n + 1 for n in ncell]
    return np.array([[(d * cx + a) + nd[0] * ((d * cy + b) + nd[1] * (d * cz + c)) for c in range(d + 1) for b in range(d + 1) for a in range(d + 1)]
                     for cz in range(ncell[2]) for cy in range(ncell[1]) for cx in range(ncell[0])])


def pressure_values(d, ncell, p, xi, dg):
    """p_h at the reference points xi ([npts, 3], the same in every cell, or [cell, npts, 3]) -> [cell, npts]"""
    ncells = int(np.prod(ncell))
    xi = np.asarray(xi, dtype=np.float64)
    if xi.ndim == 2:
        xi = np.broadcast_to(xi[None], (ncells,) + xi.shape)
    p = np.asarray(p, dtype=np.float64)
    if dg:
        return np.einsum("cqn,cn->cq", dgp_basis(d, xi), p.reshape(ncells, -1))
    return np.einsum("cqn,cn->cq", q_basis(d, xi), p[q_cell_dofs(d, ncell)])


def quadrature_points(ncell, lower, upper, nq):
    """[cell, nq^3, 3] on the box"""
    xi, _ = tensor_xi(nq)
    lower, upper = np.asarray(lower, float), np.asarray(upper, float)
    h = (upper - lower) / np.asarray(ncell)
    cells = np.array([[cx, cy, cz] for cz in range(ncell[2]) for cy in range(ncell[1]) for cx in range(ncell[0])], dtype=np.float64)
    return lower + h * (cells[:, None, :] + xi[None])


def pressure_difference(d, ncell, lower, upper, nq, p, exact, dg):
    """(sum JxW (p_h - exact)^2, max |p_h - exact|) over QGauss(nq)^3 of the cells of the box; exact [cell, nq^3]"""
    xi, w = tensor_xi(nq)
    vol = float(np.prod((np.asarray(upper, float) - np.asarray(lower, float)) / np.asarray(ncell)))
    e = pressure_values(d, ncell, p, xi, dg) - np.asarray(exact, dtype=np.float64).reshape(int(np.prod(ncell)), -1)
    return float(np.sum(vol * w[None] * e * e)), float(np.abs(e).max())


def mean_vectors(d, ncell, lower, upper, dg):
    """(ones, weights, volume) on the box: coefficients of p = 1 and (1, psi_j), by QGauss(d + 1)^3"""
    xi, w = tensor_xi(d + 1)
    ncells = int(np.prod(ncell))
    cell = float(np.prod((np.asarray(upper, float) - np.asarray(lower, float)) / np.asarray(ncell)))
    n = n_pressure(d, ncell, dg)
    if dg:
        integrals = cell * (w @ dgp_basis(d, xi))
        per = len(integrals)
        ones = np.zeros(n)
        ones[::per] = 1.0
        return ones, np.tile(integrals, ncells), cell * ncells
    integrals = cell * (w @ q_basis(d, xi))
    weights = np.zeros(n)
    np.add.at(weights, q_cell_dofs(d, ncell).reshape(-1), np.tile(integrals, ncells))
    return np.ones(n), weights, cell * ncells


# ---------------------------------------------------------------------------------------------- FE_DGP(d) between two meshes

def dgp_child_matrix(d, child):
    """[n, n]: M[m'][m] = (psi_m of the parent, psi_m' of the child) on child (sx, sy, sz): the parent's function m has the
    coefficients M[:, m] there - the L2 projection (the basis is orthonormal), exact with QGauss(d + 1)^3"""
    xi, w = tensor_xi(d + 1)
    parent = dgp_basis(d, 0.5 * (np.asarray(child, float)[None] + xi))
    return np.einsum("q,qa,qb->ab", w, dgp_basis(d, xi), parent)


def dgp_parent(ncell_fine):
    """for every fine cell: (index of its parent in the mesh with half the cells, child position [3] in {0, 1})"""
    nx, ny, nz = ncell_fine
    assert nx % 2 == 0 and ny % 2 == 0 and nz % 2 == 0
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    parent = (cx // 2) + (nx // 2) * ((cy // 2) + (ny // 2) * (cz // 2))
    return parent.ravel(), np.stack([cx % 2, cy % 2, cz % 2], axis=-1).reshape(-1, 3)


def dgp_embedding(d, ncell_fine):
    """the dense [n_fine, n_coarse] embedding"""
    n = len(dgp_functions(d))
    parent, child = dgp_parent(ncell_fine)
    P = np.zeros((n * len(parent), n * len(parent) // 8))
    M = {(sx, sy, sz): dgp_child_matrix(d, (sx, sy, sz)) for sx in range(2) for sy in range(2) for sz in range(2)}
    for f, (pc, ch) in enumerate(zip(parent, child)):
        P[n * f:n * (f + 1), n * pc:n * (pc + 1)] = M[tuple(int(v) for v in ch)]
    return P


def dgp_prolongate(d, ncell_fine, coarse_coeffs):
    return dgp_embedding(d, ncell_fine) @ np.asarray(coarse_coeffs, dtype=np.float64)


def dgp_restrict(d, ncell_fine, fine_coeffs):
    return dgp_embedding(d, ncell_fine).T @ np.asarray(fine_coeffs, dtype=np.float64)


def dgp_coarse_values_on_fine(d, ncell_fine, coarse_coeffs, xi):
    """the coarse FE_DGP(d) function at the reference points xi ([npts, 3] or [fine cell, npts, 3]) of every FINE cell"""
    n = len(dgp_functions(d))
    parent, child = dgp_parent(ncell_fine)
    c = np.asarray(coarse_coeffs, dtype=np.float64).reshape(-1, n)[parent]
    xi = np.asarray(xi, dtype=np.float64)
    if xi.ndim == 2:
        xi = np.broadcast_to(xi[None], (len(parent),) + xi.shape)
    return np.einsum("cqn,cn->cq", dgp_basis(d, 0.5 * (child[:, None, :] + xi)), c)


# ---------------------------------------------------------------------------------------------- compute_divergence

def divergence_cells(degree, u, ncell, vertices):
    """([n_cells] sum_q (div u_h)^2 JxW at QGauss(degree + 1)^3, sqrt of their sum); the velocity read plain"""
    xi, w = tensor_xi(degree + 1)
    _, dphi = nq3.tables_3d(nq3.gauss_lobatto01(degree), xi)
    _, dN = nq3.tables_3d(np.array([0.0, 1.0]), xi)
    U = np.asarray(u, dtype=np.float64).reshape(3, nq3.n_velocity(degree, ncell))
    cells = []
    for cz in range(ncell[2]):
        for cy in range(ncell[1]):
            for cx in range(ncell[0]):
                dofs = nq3._cell_dofs(degree, ncell, cx, cy, cz)
                V = nq3._cell_vertices(ncell, vertices, cx, cy, cz)
                J = np.einsum("vd,qve->qde", V, dN)
                grad = np.einsum("qne,qej->qnj", dphi, np.linalg.inv(J))  # d phi_n / dx_j
                div = np.einsum("in,qni->q", U[:, dofs], grad)
                cells.append(np.sum(div * div * np.linalg.det(J) * w))
    cells = np.array(cells)
    return cells, float(np.sqrt(cells.sum()))


def box_node_coordinates(degree, ncell, lower, upper):
    """[n_u][3]: the velocity DoF positions on the box"""
    lower, upper = np.asarray(lower, float), np.asarray(upper, float)
    return lower + (upper - lower) * nq3.node_coordinates(degree, ncell)


def solenoidal_cubic(x):
    """[3 n] component-major: the curl of (x y^2 z^3, 0, x^2 y^2 z^3) at the points x [n][3]; its components lie in Q3"""
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    return np.concatenate([2 * X * X * Y * Z ** 3, 3 * X * Y * Y * Z * Z - 2 * X * Y * Y * Z ** 3, -2 * X * Y * Z ** 3])
