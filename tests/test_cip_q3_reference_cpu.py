"""The general-degree numpy restatement of the CIP interior-face term (tests/cip_q3_reference.py): pinned at degree 2 against the
closed-form FE_Q(2) restatement (tests/cip_reference.py), held at degree 3 by the properties the form has by construction - no
reference-held number reaches this term -, and the guard that keeps the degree-3 GPU tests from being hollow.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_q3_reference as c3  # noqa: E402
import cip_reference as cref  # noqa: E402
import navier_q3_reference as qref  # noqa: E402

EPS = np.finfo(np.float64).eps
PERT = ((3, 2, 4), 0.15)


def _fields(nc, seed, n=1, degree=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, 3 * qref.n_velocity(degree, nc)) for _ in range(n)]


def _meshes():
    return [((3, 2, 4), c3.mesh_vertices("pert"), 0b111011), ((4, 3, 2), qref.box_vertices((4, 3, 2), upper=(1.0, 1.5, 0.6)), 0),
            ((2, 2, 2), qref.box_vertices((2, 2, 2)), 63)]


@pytest.mark.parametrize("mesh", ["pair", "pert", "box"])
def test_degree_2_equals_the_closed_form_restatement(mesh):
    """The general-degree module at degree 2 against the closed-form FE_Q(2) module: different tables (product formulas on the
    Gauss-Lobatto nodes against closed forms), different node and vertex bookkeeping, the same loop over face pairs and the same
    einsum contractions - so this pins tables, numbering, face rule and pa, not two independent summation orders (the absolute scale
    is held by the closed form and the properties below).  Bound: an entry is a sum over at most 6 faces x 9 points of delta JxW jump
    d_n phi, the jump a sum of 2 x 27 products, w.n of 27: ~10^3 rounded operations whose errors add at worst linearly, with
    cancellation of at most ~10: 1e4 eps = 2.2e-12 of max |C|.  Measured (printed): 0 on all nine cases - the tables of the two
    modules agree to the last bit at these points and the contractions run in the same order."""
    nc = cref.MESHES[mesh][0]
    verts = cref.mesh_vertices(mesh)
    for mask in cref.MASKS:
        u, w = _fields(nc, 11 + mask, 2, degree=2)
        old = cref.cip(1.7, w, u, nc, verts, mask)
        new = c3.cip(2, 1.7, w, u, nc, verts, mask)
        dev = np.abs(new - old).max() / np.abs(old).max()
        print(f"{mesh} mask {mask}: max deviation {dev:.2e} of max |C| = {np.abs(old).max():.3e}")
        assert np.abs(old).max() > 0 and dev <= 1e4 * EPS
        assert np.array_equal(new == 0.0, old == 0.0)  # the same empty rows
    assert abs(c3.pa(2) - cref.PA) <= 4 * EPS * cref.PA and abs(c3.pa(3) - 27.0 * np.sqrt(3.0)) <= 4 * EPS * 47


@pytest.mark.parametrize("case", range(3))
def test_symmetric_and_semidefinite_for_a_fixed_weight(case):
    """x . C(w; u) = u . C(w; x) and u . C(w; u) >= 0: the form is sum delta_F [d_n u] [d_n x] with delta_F >= 0.  Rounding of sums of
    O(10^5) products: 1e-13 relative to |x| |C(w; u)|"""
    nc, verts, mask = _meshes()[case]
    u, x, w = _fields(nc, 3, 3)
    cu, cx = c3.cip(3, 1.0, w, u, nc, verts, mask), c3.cip(3, 1.0, w, x, nc, verts, mask)
    free = ~np.tile(qref.constrained(3, nc, mask), 3)
    assert np.linalg.norm(cu) > 0
    assert abs(x[free] @ cu[free] - u[free] @ cx[free]) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(cu)
    assert u[free] @ cu[free] > 0


def test_homogeneity():
    """C(a w; u) = a^2 C(w; u), C(w; a u) = a C(w; u), and linear in delta0"""
    nc, verts, mask = _meshes()[0]
    u, w = _fields(nc, 4, 2)
    c = c3.cip(3, 1.0, w, u, nc, verts, mask)
    for a in (-2.0, 0.5, 3.0):
        assert np.linalg.norm(c3.cip(3, 1.0, a * w, u, nc, verts, mask) - a * a * c) <= 8 * EPS * a * a * np.linalg.norm(c)
        assert np.linalg.norm(c3.cip(3, 1.0, w, a * u, nc, verts, mask) - a * c) <= 8 * EPS * abs(a) * np.linalg.norm(c)
        assert np.linalg.norm(c3.cip(3, a, w, u, nc, verts, mask) - a * c) <= 8 * EPS * abs(a) * np.linalg.norm(c)


def test_vanishes_without_a_gradient_jump():
    """the nodal interpolant of a global cubic on a Cartesian mesh is that cubic in every cell: the gradient is continuous, the term
    rounding.  |u| ~ 10, gradients O(1 / h) ~ 10 with table entries up to ~10, sums of ~200 products: 1e-11 absolute.  The same
    coefficients with one quartic monomial added jump: the check can fail"""
    nc = (3, 2, 2)
    verts = qref.box_vertices(nc, upper=(1.0, 1.5, 0.6))
    X = c3.dof_points(3, nc, verts)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    mono = np.stack([x ** i * y ** j * z ** k for i in range(4) for j in range(4) for k in range(4) if i + j + k <= 3])
    rng = np.random.default_rng(8)
    cubic = (rng.uniform(-1, 1, (3, len(mono))) @ mono).reshape(-1)
    w = rng.uniform(-1, 1, cubic.size)
    assert np.linalg.norm(cubic) > 1
    assert np.max(np.abs(c3.cip(3, 1.0, w, cubic, nc, verts, 0))) <= 1e-11
    quartic = cubic + np.concatenate([x ** 4, y ** 4, z ** 4])
    assert np.max(np.abs(c3.cip(3, 1.0, w, quartic, nc, verts, 0))) > 1e-6


def test_vanishes_for_a_tangential_weight():
    """w . n = 0 on every interior face: one face direction only (1 x 1 x 3, w_z = 0), and on a Cartesian 2 x 2 x 2 mesh w_d = 0 on
    the DoFs of the faces of direction d.  The normal of the numerically inverted Jacobian is e_d up to O(eps), so w . n is O(eps) and
    the term, which carries its square, O(eps^2) times gradients and sums of O(10^4): 1e-27 absolute"""
    nc = (1, 1, 3)
    verts = qref.box_vertices(nc)
    u, w = _fields(nc, 6, 2)
    assert np.linalg.norm(c3.cip(3, 1.0, w, u, nc, verts, 0)) > 0
    w.reshape(3, -1)[2] = 0.0
    assert np.max(np.abs(c3.cip(3, 1.0, w, u, nc, verts, 0))) <= 1e-27
    nc = (2, 2, 2)
    verts = qref.box_vertices(nc)
    u, w = _fields(nc, 6, 2)
    iz, iy, ix = np.meshgrid(*[np.arange(7)] * 3, indexing="ij")
    for d, idx in enumerate((ix, iy, iz)):
        w.reshape(3, -1)[d][(idx % 3 == 0).reshape(-1)] = 0.0
    assert np.linalg.norm(w) > 1
    assert np.max(np.abs(c3.cip(3, 1.0, w, u, nc, verts, 0))) <= 1e-27


def test_closed_form_on_two_cells():
    """[0, 2] x [0, 1]^2, 2 x 1 x 1 cells, u = (|x - 1|, 0, 0), w = (0.7, 0, 0), delta0 = 3: one face of area 1, the jump of d_x u is
    2, u . C(w; u) = 3 / 3^3.5 * 0.49 * 4.  (|x - 1| is linear in each cell: in the space.)"""
    nc = (2, 1, 1)
    verts = qref.box_vertices(nc, upper=(2, 1, 1))
    X = c3.dof_points(3, nc, verts)
    z = np.zeros(len(X))
    u = np.concatenate([np.abs(X[:, 0] - 1.0), z, z])
    w = np.concatenate([np.full(len(X), 0.7), z, z])
    val = u @ c3.cip(3, 3.0, w, u, nc, verts, 0)
    exact = 3.0 / (27.0 * np.sqrt(3.0)) * 0.49 * 4.0
    print(f"closed form: {val!r} against {exact!r}")
    assert abs(val - exact) <= 64 * EPS * exact


def test_constraints():
    """constrained rows are exactly 0, and the constrained entries of u and w are not read"""
    nc, verts, mask = _meshes()[0]
    u, w, junk = _fields(nc, 7, 3)
    con = np.tile(qref.constrained(3, nc, mask), 3)
    c = c3.cip(3, 1.0, w, u, nc, verts, mask)
    assert con.any() and np.all(c[con] == 0.0) and np.linalg.norm(c) > 0
    u2, w2 = u.copy(), w.copy()
    u2[con], w2[con] = 1e6 * junk[con], -1e6 * junk[con]
    assert np.array_equal(c3.cip(3, 1.0, w2, u2, nc, verts, mask), c)
    assert not np.array_equal(c3.cip(3, 1.0, w, u, nc, verts, 0), c)


def test_a_lone_cell_has_no_face():
    nc = (1, 1, 1)
    u, w = _fields(nc, 2, 2)
    assert np.array_equal(c3.cip(3, 1.0, w, u, nc, qref.box_vertices(nc), 0), np.zeros(192))


@pytest.mark.parametrize("mask", c3.MASKS)
@pytest.mark.parametrize("mesh", list(c3.MESHES))
def test_gpu_cases_are_not_hollow(mesh, mask):
    """for every (mesh, mask) the GPU tests use, with its delta0, nu = 0.3 and their fields (w = u): the term is at least a tenth of
    the linear operator's velocity result - the threshold of tests/test_cip_reference_cpu.py - so an error in it cannot hide behind
    the 1e-12 of the sum; the separate-weight term of the same case is no smaller than a third of it"""
    from oracle import oracle
    nc = c3.MESHES[mesh][0]
    orc = oracle.StokesOracle(nc, c3.mesh_vertices(mesh), mask, c3.NU, pu=3)
    U = c3.fields(mesh)[0]
    P = np.random.default_rng(c3.FIELD_SEED + 1).uniform(-1, 1, orc.n_p)
    ku, _ = orc.apply(U, P)
    c = c3.delta0_of(mesh, mask) * c3.term(mesh, mask, 0, 0)
    ratio = np.linalg.norm(c) / np.linalg.norm(ku)
    print(f"{mesh} mask {mask}: delta0 {c3.delta0_of(mesh, mask)}, |C(u; u)| / |nu K u - B^T p| = {ratio:.3f}")
    assert ratio >= 0.1
    assert np.linalg.norm(c3.term(mesh, mask, 1, 0)) >= np.linalg.norm(c3.term(mesh, mask, 0, 0)) / 3


def test_library_vertices_of_the_boxes_are_the_plain_grid():
    """the Cartesian meshes run without vertices on the device: the restatement's vertices are that grid"""
    for mesh, (nc, lower, upper, distort) in c3.MESHES.items():
        if distort == 0.0:
            assert np.allclose(np.reshape(c3.mesh_vertices(mesh), (-1, 3)), qref.box_vertices(nc, lower, upper), rtol=0, atol=1e-15)
