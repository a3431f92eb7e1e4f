"""The numpy restatement of the convection term for a velocity of any degree (tests/navier_q3_reference.py), pinned without a GPU: at
degree 2 against the closed-form FE_Q(2) restatement tests/navier_reference.py, and at degree 3 against what it must satisfy by
construction.  Bounds 1e-13 rel-L2: two restatements of the same dense sums in fp64."""
import numpy as np
import pytest

import navier_q3_reference as q3
import navier_reference as nref

TOL = 1e-13


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


@pytest.mark.parametrize("mode", [q3.FORM, q3.JACOBIAN])
@pytest.mark.parametrize("distort", [0.0, 0.1], ids=["box", "perturbed"])
def test_degree_2_equals_the_q2_restatement(distort, mode):
    """a 2 x 3 x 2 mesh, a mask that leaves the faces 2 and 5 free"""
    nc, mask = (2, 3, 2), 0b011011
    verts = nref.perturbed_vertices(nc, distort, 7)
    rng = np.random.default_rng(5)
    u, b = rng.uniform(-1, 1, 3 * nref.n_velocity(nc)), rng.uniform(-1, 1, 3 * nref.n_velocity(nc))
    assert np.allclose(q3.gauss_lobatto01(2), [0.0, 0.5, 1.0], rtol=0, atol=1e-16)
    assert q3.n_velocity(2, nc) == nref.n_velocity(nc) and np.array_equal(q3.constrained(2, nc, mask), nref.constrained(nc, mask))
    want = nref.convection_cells(mode, b, u, nc, verts, mask)
    got = q3.convection_cells(2, mode, b, u, nc, verts, mask)
    err = rel(got, want)
    print("degree 2", distort, mode, "%.2e" % err)
    assert np.linalg.norm(want) > 0 and err < TOL


@pytest.mark.parametrize("distort", [0.0, 0.1], ids=["box", "perturbed"])
def test_jacobian_is_the_sum_of_the_two_forms(distort):
    nc, mask = (2, 2, 2), 0b100110
    verts = nref.perturbed_vertices(nc, distort, 3)
    rng = np.random.default_rng(6)
    n = 3 * q3.n_velocity(3, nc)
    u, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    jac = q3.convection_cells(3, q3.JACOBIAN, b, u, nc, verts, mask)
    both = q3.convection_cells(3, q3.FORM, b, u, nc, verts, mask) + q3.convection_cells(3, q3.FORM, u, b, nc, verts, mask)
    assert np.linalg.norm(both) > 0 and rel(jac, both) < TOL


@pytest.mark.parametrize("mode", [q3.FORM, q3.JACOBIAN])
def test_four_point_rule_is_exact_for_quadratic_fields(mode):
    """u, b nodal interpolants of polynomials of degree <= 2 per variable on a box: FE_Q(3) holds them exactly, the integrand
    (u (x) b) : grad v has degree <= 2 + 2 + 3 = 7 per variable with a constant Jacobian - the exactness of Gauss(4) - so Gauss(4)
    and Gauss(6) agree to rounding"""
    nc = (2, 1, 2)
    verts = q3.box_vertices(nc)
    xyz = q3.node_coordinates(3, nc)
    rng = np.random.default_rng(3)

    def quadratic():
        c = rng.uniform(-1, 1, (3, 3, 3, 3))
        px = np.stack([xyz[:, 0] ** i for i in range(3)])
        py = np.stack([xyz[:, 1] ** i for i in range(3)])
        pz = np.stack([xyz[:, 2] ** i for i in range(3)])
        return np.einsum("cijk,in,jn,kn->cn", c, px, py, pz).reshape(-1)

    u, b = quadratic(), quadratic()
    r4 = q3.convection_cells(3, mode, b, u, nc, verts, 0, nq=4)
    r6 = q3.convection_cells(3, mode, b, u, nc, verts, 0, nq=6)
    assert np.linalg.norm(r6) > 0 and rel(r4, r6) < TOL
    # (and the rule is needed: three points do not integrate degree 7)
    assert rel(q3.convection_cells(3, mode, b, u, nc, verts, 0, nq=3), r6) > 1e-8


@pytest.mark.parametrize("mode", [q3.FORM, q3.JACOBIAN])
def test_constrained_rows_and_entries(mode):
    """constrained rows of the result are exactly 0; entries of u and b on constrained DoFs are not read"""
    nc, mask = (2, 3, 2), 0b010110
    verts = nref.perturbed_vertices(nc, 0.1, 4)
    con = np.tile(q3.constrained(3, nc, mask), 3)
    assert con.any() and not con.all()
    rng = np.random.default_rng(8)
    u, b = rng.uniform(-1, 1, con.size), rng.uniform(-1, 1, con.size)
    r = q3.convection_cells(3, mode, b, u, nc, verts, mask).reshape(-1)
    assert np.all(r[con] == 0.0) and np.all(r[~con] != 0.0)
    u2, b2 = u.copy(), b.copy()
    u2[con] = 1e30
    b2[con] = 1e30
    assert np.all(q3.convection_cells(3, mode, b2, u2, nc, verts, mask).reshape(-1) == r)
