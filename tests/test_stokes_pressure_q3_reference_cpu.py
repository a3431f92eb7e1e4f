"""Pins tests/stokes_pressure_q3_reference.py, the numpy restatement the degree-3 pressure and divergence GPU tests compare with, against
what is known by itself: the mean weights sum to the volume, a quadratic polynomial is represented exactly by both degree-2 spaces, the
embedding of a FE_DGP function into the children of its cell is the same function at random points and its restriction the transpose, at
pressure degree 1 the restatement is the one the existing FE_DGP(1) tests use (oracle/driver_oracle.py), the divergence at velocity
degree 2 is tests/navier_slab_reference.py::divergence_cells, and a solenoidal cubic field has none.  The closed 1D formulas of the
library's embedding (include/stfem_stokes_pressure_space.h) are checked here against the projection too.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_slab_reference as nsr  # noqa: E402
import stokes_pressure_q3_reference as R  # noqa: E402
from oracle import driver_oracle as D  # noqa: E402

LOWER, UPPER = (0.0, -0.5, 0.25), (1.0, 0.2, 1.55)  # volume 0.91
MESHES = [(2, 1, 1), (3, 2, 2)]


def quadratic(x):
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    return 0.3 + X - 2 * Y + 0.5 * Z + X * X - 0.7 * Y * Y + 1.1 * Z * Z + 0.9 * X * Y - 1.3 * Y * Z + 0.4 * X * Z


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("nc", MESHES)
def test_mean_weights(nc, d, dg):
    ones, weights, volume = R.mean_vectors(d, nc, LOWER, UPPER, dg)
    assert ones.shape == weights.shape == (R.n_pressure(d, nc, dg),)
    assert abs(volume - 0.91) <= 1e-14
    assert abs(weights @ ones - volume) <= 1e-14
    # p = 1 is the function 1
    assert np.abs(R.pressure_values(d, nc, ones, R.tensor_xi(3)[0], dg) - 1.0).max() <= 1e-14
    if dg:  # only the first function of a cell has a mean: the others are the rounding of a sum of (d + 1)^3 products of size <= 5
        per = len(R.dgp_functions(d))
        assert np.abs(np.delete(weights.reshape(-1, per), 0, axis=1)).max() <= 27 * 5 * np.finfo(float).eps
    elif d == 2:  # the tensor product of the assembled h (1/6, 4/6, 1/6)
        h = (np.array(UPPER) - np.array(LOWER)) / np.array(nc)
        one = []
        for e in range(3):
            w = np.zeros(2 * nc[e] + 1)
            for c in range(nc[e]):
                w[2 * c:2 * c + 3] += h[e] * np.array([1, 4, 1]) / 6
            one.append(w)
        closed = np.einsum("k,j,i->kji", one[2], one[1], one[0]).ravel()
        assert np.abs(weights - closed).max() <= 1e-15


def representation(d, nc, dg):
    """the coefficients of `quadratic` in the space: nodal values, or the L2 projection per cell"""
    if not dg:
        ax = [np.linspace(LOWER[e], UPPER[e], d * nc[e] + 1) for e in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return quadratic(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))
    xi, w = R.tensor_xi(3)
    vals = quadratic(R.quadrature_points(nc, LOWER, UPPER, 3))
    return np.einsum("cq,q,qn->cn", vals, w, R.dgp_basis(d, xi)).ravel()


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("nq", [1, 3, 4])
@pytest.mark.parametrize("nc", MESHES)
def test_quadratic_is_exact_at_degree_2(nc, nq, dg):
    coeffs = representation(2, nc, dg)
    exact = quadratic(R.quadrature_points(nc, LOWER, UPPER, nq))
    scale = np.abs(exact).max()
    l2, linf = R.pressure_difference(2, nc, LOWER, UPPER, nq, coeffs, exact, dg)
    assert l2 < 1e-24 * scale ** 2 and linf < 1e-12 * scale, (l2, linf)
    # and the mean of the function through the weights
    _, weights, volume = R.mean_vectors(2, nc, LOWER, UPPER, dg)
    xi, w = R.tensor_xi(3)
    mean = np.sum(quadratic(R.quadrature_points(nc, LOWER, UPPER, 3)) * w[None]) * (volume / np.prod(nc)) / volume
    assert abs(weights @ coeffs / volume - mean) <= 1e-13 * scale


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("nf", [(2, 2, 2), (4, 2, 6)])
def test_embedding_is_the_same_function(nf, d):
    rng = np.random.default_rng([d, *nf])
    n = len(R.dgp_functions(d))
    c = rng.uniform(-1, 1, n * int(np.prod(nf)) // 8)
    Pc = R.dgp_prolongate(d, nf, c)
    xi = rng.uniform(0, 1, (int(np.prod(nf)), 5, 3))
    assert np.abs(R.pressure_values(d, nf, Pc, xi, True) - R.dgp_coarse_values_on_fine(d, nf, c, xi)).max() <= 1e-14
    f = rng.uniform(-1, 1, n * int(np.prod(nf)))
    P = R.dgp_embedding(d, nf)
    assert np.array_equal(R.dgp_restrict(d, nf, f), P.T @ f)
    assert abs(R.dgp_restrict(d, nf, f) @ c - f @ Pc) <= 1e-13 * np.linalg.norm(f) * np.linalg.norm(Pc)


def test_degree_1_is_the_existing_restatement():
    nf = (4, 2, 6)
    rng = np.random.default_rng(3)
    c = rng.uniform(-1, 1, 4 * 6)
    assert np.abs(R.dgp_prolongate(1, nf, c) - D.dgp_prolongate(nf, c)).max() <= 1e-14
    # the formulas of the FE_DGP(1) kernel: c0 + sqrt 3 ((sx - 1/2) c1 + ...), c1 / 2, c2 / 2, c3 / 2
    for child in [(0, 0, 0), (1, 0, 1), (1, 1, 1)]:
        M = np.zeros((4, 4))
        M[0, 0] = 1.0
        for e in range(3):
            M[0, 1 + e] = np.sqrt(3.0) * (child[e] - 0.5)
            M[1 + e, 1 + e] = 0.5
        assert np.abs(R.dgp_child_matrix(1, child) - M).max() <= 1e-15
    verts = D.box_vertices(nf, LOWER, UPPER)
    for dg in (False, True):
        p = rng.uniform(-1, 1, R.n_pressure(1, nf, dg))
        for nq in (1, 3):
            exact = rng.uniform(-1, 1, (48, nq ** 3))
            got, ref = R.pressure_difference(1, nf, LOWER, UPPER, nq, p, exact, dg), D.pressure_difference(nf, verts, nq, p, exact, dg)
            assert abs(got[0] - ref[0]) <= 1e-13 * ref[0] and abs(got[1] - ref[1]) <= 1e-14 * ref[1]
            assert np.abs(R.quadrature_points(nf, LOWER, UPPER, nq) - D.pressure_quadrature_points(nf, verts, nq)).max() <= 1e-14
        mean_ref, vol_ref = D.pressure_mean(nf, verts, p, dg)
        _, weights, volume = R.mean_vectors(1, nf, LOWER, UPPER, dg)
        assert abs(volume - vol_ref) <= 1e-14 and abs(weights @ p / volume - mean_ref) <= 1e-13


def closed_child_matrix(child):
    """the 10 x 10 matrix from the 1D tables of include/stfem_stokes_pressure_space.h"""
    fn = R.dgp_functions(2)
    T = []
    for s in child:
        sg = 2 * s - 1
        T.append(np.array([[1, 0, 0], [sg * np.sqrt(3) / 2, 0.5, 0], [0, sg * np.sqrt(15) / 4, 0.25]]))  # T[i][j]: parent l_i, child l_j
    return np.array([[T[0][m[0], n[0]] * T[1][m[1], n[1]] * T[2][m[2], n[2]] for m in fn] for n in fn])


def test_closed_1d_formulas_of_the_degree_2_embedding():
    assert R.dgp_functions(2) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 2)]
    for child in [(sx, sy, sz) for sz in range(2) for sy in range(2) for sx in range(2)]:
        assert np.abs(closed_child_matrix(child) - R.dgp_child_matrix(2, child)).max() <= 1e-14


def test_divergence_at_degree_2_is_the_existing_restatement():
    nc = (3, 2, 2)
    stfem = __import__("importlib").import_module("dealii-stfem_amd")
    verts = stfem.mesh_vertices(nc, distort=0.15, seed=77)
    u = np.random.default_rng(5).uniform(-1, 1, 3 * 7 * 5 * 5)
    cells, total = R.divergence_cells(2, u, nc, verts)
    ref_cells, ref_total = nsr.divergence_cells(u, nc, verts)
    assert np.abs(cells - ref_cells).max() <= 1e-13 * ref_cells.max() and abs(total - ref_total) <= 1e-13 * ref_total


@pytest.mark.parametrize("degree", [2, 3])
def test_divergence_of_known_fields(degree):
    nc = (2, 3, 2)
    verts = R.nq3.box_vertices(nc, LOWER, UPPER)
    x = R.box_node_coordinates(degree, nc, LOWER, UPPER)
    # (x, y, z) has divergence 3
    _, total = R.divergence_cells(degree, x.T.ravel(), nc, verts)
    assert abs(total - 3 * np.sqrt(0.91)) <= 1e-13 * 3
    if degree == 3:  # the solenoidal cubic lies in the space: nothing but rounding
        u = R.solenoidal_cubic(x)
        cells, total = R.divergence_cells(3, u, nc, verts)
        assert np.all(cells >= 0.0) and total <= 1e-13 * np.linalg.norm(u), (total, np.linalg.norm(u))
