"""oracle/driver_oracle.py (the numpy reference of the load-vector, error-norm and pressure helpers) against facts that do
not come from it, and the host-only entry points stfem_gauss_rule / stfem_fe_time_points through the library.  No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
from numpy.polynomial import polynomial as P

from oracle import driver_oracle as D

# the perturbed meshes of the configuration grid of tests/test_gpu_driver_kernels.py
PERTURBED = [(2, (7, 3, 2), 0.15), (3, (3, 4, 2), 0.2), (5, (2, 2, 3), 0.1)]
AFFINE = (0.3, np.array([1.1, -0.7, 0.45]))  # a + b . x


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    mod.lib()
    return mod


def perturbed_vertices(stfem, nc, distort, lower=(0, 0, 0), upper=(1, 1, 1)):
    return stfem.mesh_vertices(nc, lower, upper, distort, 5489)


def hexahedron_volume(c):
    """exact volume of a trilinear hexahedron with corners c[k, j, i]: det J is a polynomial of degree <= 2 per reference
    direction, integrated exactly here from its coefficients (numpy.polynomial), not by a Gauss rule"""
    # x(xi) = sum_ijk c_kji N_i(xi) N_j(eta) N_k(zeta): coefficients T[d][a, b, c] of xi^a eta^b zeta^c
    N = [np.array([1.0, -1.0]), np.array([0.0, 1.0])]  # 1 - t, t
    T = np.zeros((3, 2, 2, 2))
    for k in range(2):
        for j in range(2):
            for i in range(2):
                T += c[k, j, i][:, None, None, None] * np.einsum("a,b,c->abc", N[i], N[j], N[k])[None]

    def deriv(t, axis):
        out = np.zeros((3, 3, 3))
        sl = [slice(0, 2)] * 3
        sl[axis] = slice(0, 1)
        out[tuple(sl)] = np.take(t, [1], axis=axis)
        return out

    def mul(a, b):
        out = np.zeros(tuple(sa + sb - 1 for sa, sb in zip(a.shape, b.shape)))
        for ia in np.ndindex(a.shape):
            if a[ia] != 0.0:
                out[ia[0]:ia[0] + b.shape[0], ia[1]:ia[1] + b.shape[1], ia[2]:ia[2] + b.shape[2]] += a[ia] * b
        return out

    Jp = [[deriv(T[d], e) for e in range(3)] for d in range(3)]
    det = (mul(Jp[0][0], mul(Jp[1][1], Jp[2][2])) - mul(Jp[0][0], mul(Jp[1][2], Jp[2][1]))
           - mul(Jp[0][1], mul(Jp[1][0], Jp[2][2])) + mul(Jp[0][1], mul(Jp[1][2], Jp[2][0]))
           + mul(Jp[0][2], mul(Jp[1][0], Jp[2][1])) - mul(Jp[0][2], mul(Jp[1][1], Jp[2][0])))
    vol = 0.0
    for ia in np.ndindex(det.shape):
        vol += det[ia] / ((ia[0] + 1) * (ia[1] + 1) * (ia[2] + 1))
    return vol


def test_gauss_rule_and_lagrange_tables():
    for n in range(1, 9):
        x, w = D.gauss_rule(n)
        assert np.all(np.diff(x) > 0) and x[0] > 0 and x[-1] < 1
        for k in range(2 * n):
            assert abs(np.dot(w, x ** k) - 1.0 / (k + 1)) < 1e-15
    nodes = np.array([0.0, 0.2, 0.55, 1.0])
    xs = np.linspace(0, 1, 7)
    S, Dv = D.lagrange_tables(nodes, xs)
    for k in range(4):  # polynomials up to degree 3 are reproduced, with their derivative
        np.testing.assert_allclose(S @ nodes ** k, xs ** k, atol=1e-14)
        np.testing.assert_allclose(Dv @ nodes ** k, k * xs ** max(k - 1, 0) if k else 0 * xs, atol=1e-13)


def test_load_vector_of_one_is_the_volume(stfem):
    for p, nc, lower, upper in [(1, (1, 1, 1), (0, 0, 0), (2, 1, 0.5)), (4, (3, 2, 2), (-1, -1, -1), (1, 2, 1))]:
        v = D.box_vertices(nc, lower, upper)
        for nq in (1, 2, p + 1, 8):
            if nq < (p + 2) // 2:
                continue  # the rule must integrate the basis itself: degree p per direction
            rhs = D.load_vector(p, nc, v, nq, np.ones((int(np.prod(nc)), nq ** 3)), 0)
            assert abs(rhs.sum() - np.prod(np.subtract(upper, lower))) < 1e-13 * np.prod(np.subtract(upper, lower))
    for p, nc, distort in PERTURBED:
        v = perturbed_vertices(stfem, nc, distort, (0, 0, 0), (1.5, 1, 2))
        assert np.abs(v - D.box_vertices(nc, (0, 0, 0), (1.5, 1, 2))).max() > 0.01
        corners = D._cell_corners(nc, v)
        exact = sum(hexahedron_volume(c) for c in corners)
        assert abs(exact - 3.0) < 1e-13  # the perturbation moves interior vertices only
        for nq in (p + 1, p + 2):  # det J has degree 2 per direction, the basis degree p
            ones = np.ones((len(corners), nq ** 3))
            rhs = D.load_vector(p, nc, v, nq, ones, 0)
            assert abs(rhs.sum() - exact) < 1e-13 * exact
            # cell by cell too: the integral of 1 over one cell (f = indicator of the cell)
            for cell in (0, len(corners) - 1):
                ind = np.zeros_like(ones)
                ind[cell] = 1.0
                assert abs(D.load_vector(p, nc, v, nq, ind, 0).sum() - hexahedron_volume(corners[cell])) < 1e-14


def test_load_vector_of_a_polynomial_on_a_box(oracle_mod):
    """rhs_a = prod_d int f_d(x_d) phi_{a_d}(x_d) dx_d for f = f_x f_y f_z: 1D integrals from polynomial coefficients"""
    lower, upper = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 2.0, 1.0])
    f1d = [np.array([0.5, -1.0, 0.25, 2.0]), np.array([1.0, 0.3, -0.4]), np.array([-0.2, 0.0, 0.0, 1.5])]  # coefficients in x_d
    for p, nc, mask in [(4, (3, 2, 2), 0b010101), (2, (2, 1, 3), 0), (1, (1, 1, 1), 0)]:
        nq = p + 3  # integrand degree p + 3 per direction <= 2 nq - 1
        v = D.box_vertices(nc, lower, upper)
        nodes = oracle_mod.gauss_lobatto(p + 1)
        line = []
        for d in range(3):
            h = (upper[d] - lower[d]) / nc[d]
            out = np.zeros(p * nc[d] + 1)
            for c in range(nc[d]):
                x0 = lower[d] + c * h
                # in the cell's own coordinate t in [0, 1] (x = x0 + h t), where the monomial basis is well conditioned
                ft = np.zeros(1)
                for k, ck in enumerate(f1d[d]):
                    ft = P.polyadd(ft, ck * P.polypow(np.array([x0, h]), k))
                for a in range(p + 1):
                    poly = np.array([1.0])
                    for m in range(p + 1):
                        if m != a:
                            poly = P.polymul(poly, np.array([-nodes[m], 1.0]) / (nodes[a] - nodes[m]))
                    out[p * c + a] += h * P.polyval(1.0, P.polyint(P.polymul(poly, ft)))
            line.append(out)
        exact = np.einsum("k,j,i->kji", line[2], line[1], line[0]).ravel()
        exact[D.constrained(p, nc, mask)] = 0.0
        pts = D.quadrature_points(p, nc, v, nq)
        f = P.polyval(pts[..., 0], f1d[0]) * P.polyval(pts[..., 1], f1d[1]) * P.polyval(pts[..., 2], f1d[2])
        got = D.load_vector(p, nc, v, nq, f, mask)
        assert np.abs(got - exact).max() < 1e-13 * np.abs(exact).max(), np.abs(got - exact).max() / np.abs(exact).max()
        assert np.all(got[D.constrained(p, nc, mask)] == 0.0)
        nd = [p * c + 1 for c in nc]
        assert D.constrained(p, nc, mask).sum() == (0 if mask == 0 else D.n_dofs(p, nc) - (nd[0] - 1) * (nd[1] - 1) * (nd[2] - 1))


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5])
def test_affine_function_on_perturbed_meshes(stfem, degree):
    """MappingQ1 reproduces affine functions: a + b . x interpolated at the support points has value and gradient error 0 at
    every point of every rule; with J^-1 used transposed the gradient error is O(1).  Also pins the residual the GPU tests
    scale their round-off bounds with."""
    a, b = AFFINE
    meshes = [(nc, dist) for _, nc, dist in PERTURBED]
    for nc, distort in meshes:
        v = perturbed_vertices(stfem, nc, distort)
        sp = D.support_points(degree, nc, v)
        u = a + sp @ b
        scale = np.abs(u).max()
        for nq in (degree, degree + 1, degree + 2):
            pts = D.quadrature_points(degree, nc, v, nq)
            ex = a + pts @ b
            grad = np.broadcast_to(b, pts.shape)
            l2, linf, h1 = D.difference(degree, nc, v, nq, u, ex, grad)
            assert linf < 1e-12 * scale and l2 < 1e-24 * scale ** 2 and h1 < 1e-24 * scale ** 2, (degree, nc, nq, l2, linf, h1)
            assert D.difference(degree, nc, v, nq, u, ex)[2] == 0.0
        # the check bites: the transposed inverse does not give 0 on a perturbed mesh
        xq, _ = D.gauss_rule(degree + 1)
        _, J = D._geometry(nc, v, xq)
        assert np.abs(J - np.swapaxes(J, -1, -2)).max() > 1e-2


def test_support_and_quadrature_points_layout():
    nc, lower, upper = (2, 3, 1), (0, 0, 0), (2.0, 3.0, 0.5)
    v = D.box_vertices(nc, lower, upper)
    sp = D.support_points(2, nc, v).reshape(3, 7, 5, 3)
    np.testing.assert_allclose(sp[0, 0, :, 0], np.linspace(0, 2, 5), atol=1e-15)
    np.testing.assert_allclose(sp[0, :, 0, 1], np.linspace(0, 3, 7), atol=1e-15)
    np.testing.assert_allclose(sp[:, 0, 0, 2], np.linspace(0, 0.5, 3), atol=1e-15)
    x, _ = D.gauss_rule(3)
    qp = D.quadrature_points(2, nc, v, 3)
    assert qp.shape == (6, 27, 3)
    cell = 1 + 2 * (2 + 3 * 0)  # cx = 1, cy = 2, cz = 0
    q = 2 + 3 * (0 + 3 * 1)     # qx = 2, qy = 0, qz = 1
    np.testing.assert_allclose(qp[cell, q], [1 + x[2], 2 + x[0], 0.5 * x[1]], atol=1e-15)


def test_pressure_spaces():
    nc, lower, upper = (4, 2, 6), (0, 0, 0), (1.0, 0.7, 1.3)
    v = D.box_vertices(nc, lower, upper)
    ncells = int(np.prod(nc))
    rng = np.random.default_rng(11)
    # FE_DGP(1): orthonormal on the reference cell
    xi = D._tensor_xi(2)
    _, w = D.gauss_rule(2)
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    G = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            ei, ej = np.zeros(4 * ncells), np.zeros(4 * ncells)
            ei[i], ej[j] = 1.0, 1.0
            G[i, j] = np.dot(W, D.dgp_values(nc, ei, xi)[0] * D.dgp_values(nc, ej, xi)[0])
    np.testing.assert_allclose(G, np.eye(4), atol=1e-15)
    # an affine function in both spaces: zero difference, mean = value at the centre, volume 0.91
    a, b = AFFINE
    centres = D.quadrature_points(1, nc, v, 1)[:, 0, :]
    h = np.array([1.0 / 4, 0.7 / 2, 1.3 / 6])
    dgp = np.concatenate([(a + centres @ b)[:, None], np.broadcast_to(b * h / (2 * D.SQRT3), (ncells, 3))], axis=1).ravel()
    q1 = a + D.support_points(1, nc, v) @ b
    for dg, coeffs in ((True, dgp), (False, q1)):
        for nq in (1, 3, 8):
            ex = a + D.pressure_quadrature_points(nc, v, nq) @ b
            l2, linf = D.pressure_difference(nc, v, nq, coeffs, ex, dg)
            assert linf < 1e-14 and l2 < 1e-28
            ex[3, 0] += 0.5  # one point off: seen by both outputs with that point's weight
            l2, linf = D.pressure_difference(nc, v, nq, coeffs, ex, dg)
            x1, w1 = D.gauss_rule(nq)
            assert abs(linf - 0.5) < 1e-14 and abs(l2 - 0.25 * w1[0] ** 3 * np.prod(h)) < 1e-15
        mean, vol = D.pressure_mean(nc, v, coeffs, dg)
        assert abs(vol - 0.91) < 1e-14 and abs(mean - (a + b @ (np.array(upper) / 2))) < 1e-14
    # the embedding into the refined mesh describes the same function, and it is what the projection of a random one gives
    coarse_nc = (2, 1, 3)
    c = rng.uniform(-1, 1, 4 * 6)
    fine = D.dgp_prolongate(nc, c)
    for nq in (2, 3):
        ex = D.dgp_coarse_values_on_fine(nc, c, D._tensor_xi(nq))
        l2, linf = D.pressure_difference(nc, v, nq, fine, ex, True)
        assert linf < 1e-12 * np.abs(c).max() and l2 < 1e-24 * np.abs(c).max() ** 2
    # the same function seen from the coarse mesh: values at physical points agree
    pts_f = D.pressure_quadrature_points(nc, v, 2)
    hc = 2 * h
    cell_c = np.floor(pts_f / hc).astype(int)
    xi_c = pts_f / hc - cell_c
    idx = cell_c[..., 0] + 2 * (cell_c[..., 1] + 1 * cell_c[..., 2])
    direct = np.array([[D.dgp_values((1, 1, 1), c.reshape(-1, 4)[idx[f, q]], xi_c[f, q][None])[0, 0] for q in range(8)] for f in range(ncells)])
    np.testing.assert_allclose(D.dgp_values(nc, fine, D._tensor_xi(2)), direct, atol=1e-14)


# ------------------------------------------------------------------ host-only entry points of the library

def test_library_gauss_rule(stfem):
    L = stfem.lib()
    for n in range(1, 17):
        x, w = stfem.gauss_rule(n)
        xr, wr = np.polynomial.legendre.leggauss(n)
        np.testing.assert_allclose(x, 0.5 * (xr + 1), rtol=0, atol=2e-15)
        np.testing.assert_allclose(w, 0.5 * wr, rtol=0, atol=2e-15)
        for k in range(2 * n):
            assert abs(np.dot(w, x ** k) - 1.0 / (k + 1)) < 5e-15, (n, k)
    buf = np.zeros(32)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    for n in (0, 17, -1):
        assert L.stfem_gauss_rule(n, ptr, ptr) == -1  # STFEM_ERR_INVALID_ARGUMENT
        with pytest.raises(stfem.StfemError):
            stfem.gauss_rule(n)
    assert L.stfem_gauss_rule(3, None, ptr) == -1 and L.stfem_gauss_rule(3, ptr, None) == -1
    assert np.all(buf == 0.0)


def test_library_fe_time_points(stfem, oracle_mod):
    L = stfem.lib()
    for r in range(0, 9):
        if r >= 1:
            np.testing.assert_allclose(stfem.fe_time_points(stfem.CGP, r), oracle_mod.gauss_lobatto(r + 1), rtol=0, atol=2e-15)
        np.testing.assert_allclose(stfem.fe_time_points(stfem.DG, r), oracle_mod.gauss_radau_right(r + 1), rtol=0, atol=2e-15)
    # independent facts: Lobatto contains both ends and is symmetric; right Radau ends at 1 and is exact to degree 2 r
    for r in range(1, 9):
        x = stfem.fe_time_points(stfem.CGP, r)
        assert x[0] == 0.0 and x[-1] == 1.0 and np.all(np.diff(x) > 0)
        np.testing.assert_allclose(x + x[::-1], 1.0, atol=2e-15)
    for r in range(0, 9):
        x = stfem.fe_time_points(stfem.DG, r)
        assert x[-1] == 1.0 and np.all(np.diff(x) > 0) and x[0] > 0
        V = np.vander(x, r + 1, increasing=True).T
        w = np.linalg.solve(V, 1.0 / np.arange(1, r + 2))  # interpolatory weights
        for k in range(2 * r + 1):
            assert abs(np.dot(w, x ** k) - 1.0 / (k + 1)) < 1e-12, (r, k)
    buf = np.zeros(16)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.stfem_fe_time_points(0, 0, ptr) == -1   # cG(0) does not exist
    assert L.stfem_fe_time_points(2, 1, ptr) == -1   # unknown type
    assert L.stfem_fe_time_points(0, 9, ptr) == -1 and L.stfem_fe_time_points(1, -1, ptr) == -1
    assert L.stfem_fe_time_points(0, 2, None) == -1 and L.stfem_fe_time_points(1, 2, None) == -1
    assert np.all(buf == 0.0)
    with pytest.raises(stfem.StfemError):
        stfem.fe_time_points(2, 1)
