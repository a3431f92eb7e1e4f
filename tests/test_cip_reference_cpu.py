"""The numpy restatement of the CIP interior-face term (tests/cip_reference.py) held by the properties it must have by construction -
no reference-held number reaches this term -, the guard that keeps the GPU test from being hollow, and the C-ABI of the term checked
without a GPU: the symbols exist and refuse bad arguments before anything touches a device."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import navier_reference as nref  # noqa: E402

EPS = np.finfo(np.float64).eps
PERT = ((3, 2, 4), 0.15)


def _fields(nc, seed, n=1):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, 3 * nref.n_velocity(nc)) for _ in range(n)]


def _meshes():
    nc, distort = PERT
    return [(nc, nref.perturbed_vertices(nc, distort, 77), 0b111011), ((4, 3, 2), cref.box_vertices((4, 3, 2), upper=(1.0, 1.5, 0.6)), 0),
            ((2, 2, 2), cref.box_vertices((2, 2, 2)), 63)]


@pytest.mark.parametrize("case", range(3))
def test_symmetric_and_semidefinite_for_a_fixed_weight(case):
    """x . C(w; u) = u . C(w; x) and u . C(w; u) >= 0: the form is sum delta_F [d_n u] [d_n x] with delta_F >= 0.  Rounding of sums of
    O(10^4) products: 1e-13 relative to |x| |C(w; u)|"""
    nc, verts, mask = _meshes()[case]
    u, x, w = _fields(nc, 3, 3)
    cu, cx = cref.cip(1.0, w, u, nc, verts, mask), cref.cip(1.0, w, x, nc, verts, mask)
    # (the rows of constrained DoFs are zero and the constrained entries of the arguments are not read: compare on the free ones)
    free = ~np.tile(nref.constrained(nc, mask), 3)
    assert np.linalg.norm(cu) > 0
    assert abs(x[free] @ cu[free] - u[free] @ cx[free]) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(cu)
    assert u[free] @ cu[free] > 0


def test_homogeneity():
    """C(a w; u) = a^2 C(w; u), C(w; a u) = a C(w; u), and linear in delta0"""
    nc, verts, mask = _meshes()[0]
    u, w = _fields(nc, 4, 2)
    c = cref.cip(1.0, w, u, nc, verts, mask)
    for a in (-2.0, 0.5, 3.0):
        assert np.linalg.norm(cref.cip(1.0, a * w, u, nc, verts, mask) - a * a * c) <= 8 * EPS * a * a * np.linalg.norm(c)
        assert np.linalg.norm(cref.cip(1.0, w, a * u, nc, verts, mask) - a * c) <= 8 * EPS * abs(a) * np.linalg.norm(c)
        assert np.linalg.norm(cref.cip(a, w, u, nc, verts, mask) - a * c) <= 8 * EPS * abs(a) * np.linalg.norm(c)


def test_vanishes_without_a_gradient_jump():
    """physical-space linear fields on a perturbed mesh (in the isoparametric-free FE_Q(2) space through the trilinear map: a linear
    function of x is trilinear in xi) and quadratic fields on a Cartesian mesh, mask 0: the gradient is continuous, the term is
    rounding.  |u| ~ 10, gradients O(1 / h) ~ 10, sums of ~100 products: 1e-12 absolute"""
    nc, distort = PERT
    verts = nref.perturbed_vertices(nc, distort, 77)
    X = cref.dof_points(nc, verts)
    rng = np.random.default_rng(8)
    w = rng.uniform(-1, 1, 3 * nref.n_velocity(nc))
    lin = np.concatenate([X @ rng.uniform(-1, 1, 3) + rng.uniform(-1, 1) for _ in range(3)])
    assert np.linalg.norm(lin) > 1
    assert np.max(np.abs(cref.cip(1.0, w, lin, nc, verts, 0))) <= 1e-12
    # the same field is seen to jump once the mesh-linear (not physically linear) one is taken: the check can fail
    xi = cref.dof_points(nc, cref.box_vertices(nc))
    notlin = np.concatenate([xi @ np.array([1.0, -2.0, 0.5])] * 3)
    assert np.max(np.abs(cref.cip(1.0, w, notlin, nc, verts, 0))) > 1e-6
    nc = (3, 2, 2)
    verts = cref.box_vertices(nc, upper=(1.0, 1.5, 0.6))
    X = cref.dof_points(nc, verts)
    mono = np.stack([np.ones(len(X)), X[:, 0], X[:, 1], X[:, 2], X[:, 0] ** 2, X[:, 1] ** 2, X[:, 2] ** 2, X[:, 0] * X[:, 1],
                     X[:, 1] * X[:, 2], X[:, 0] * X[:, 2]])
    quad = (rng.uniform(-1, 1, (3, 10)) @ mono).reshape(-1)
    w = rng.uniform(-1, 1, quad.size)
    assert np.linalg.norm(quad) > 1
    assert np.max(np.abs(cref.cip(1.0, w, quad, nc, verts, 0))) <= 1e-12


def test_vanishes_for_a_tangential_weight():
    """w . n = 0 on every interior face: one face direction only (1 x 1 x 3, w_z = 0), and on a Cartesian 2 x 2 x 2 mesh w_d = 0 on
    the DoFs of the faces of direction d.  The normal of the numerically inverted Jacobian is e_d up to O(eps), so w . n is O(eps) and
    the term, which carries its square, O(eps^2) times gradients and sums of O(10^3): 1e-28 absolute"""
    nc = (1, 1, 3)
    verts = cref.box_vertices(nc)
    u, w = _fields(nc, 6, 2)
    assert np.linalg.norm(cref.cip(1.0, w, u, nc, verts, 0)) > 0
    w.reshape(3, -1)[2] = 0.0
    assert np.max(np.abs(cref.cip(1.0, w, u, nc, verts, 0))) <= 1e-28
    nc = (2, 2, 2)
    verts = cref.box_vertices(nc)
    u, w = _fields(nc, 6, 2)
    nd = [5, 5, 5]
    iz, iy, ix = np.meshgrid(*[np.arange(n) for n in nd[::-1]], indexing="ij")
    for d, idx in enumerate((ix, iy, iz)):
        w.reshape(3, -1)[d][(idx % 2 == 0).reshape(-1)] = 0.0
    assert np.linalg.norm(w) > 1
    assert np.max(np.abs(cref.cip(1.0, w, u, nc, verts, 0))) <= 1e-28


def test_closed_form_on_two_cells():
    """[0, 2] x [0, 1]^2, 2 x 1 x 1 cells, u = (|x - 1|, 0, 0), w = (0.7, 0, 0), delta0 = 3: one face of area 1, the jump of d_x u is
    2, u . C(w; u) = 3 / 2^3.5 * 0.49 * 4"""
    nc = (2, 1, 1)
    verts = cref.box_vertices(nc, upper=(2, 1, 1))
    X = cref.dof_points(nc, verts)
    z = np.zeros(len(X))
    u = np.concatenate([np.abs(X[:, 0] - 1.0), z, z])
    w = np.concatenate([np.full(len(X), 0.7), z, z])
    val = u @ cref.cip(3.0, w, u, nc, verts, 0)
    exact = 3.0 / 2 ** 3.5 * 0.49 * 4.0
    assert abs(exact - 0.519723484172112) < 1e-15
    print(f"closed form: {val!r} against {exact!r}")
    assert abs(val - exact) <= 16 * EPS * exact


def test_constraints():
    """constrained rows are exactly 0, and the constrained entries of u and w are not read"""
    nc, verts, mask = _meshes()[0]
    u, w, junk = _fields(nc, 7, 3)
    con = np.tile(nref.constrained(nc, mask), 3)
    c = cref.cip(1.0, w, u, nc, verts, mask)
    assert con.any() and np.all(c[con] == 0.0) and np.linalg.norm(c) > 0
    u2, w2 = u.copy(), w.copy()
    u2[con], w2[con] = 1e6 * junk[con], -1e6 * junk[con]
    assert np.array_equal(cref.cip(1.0, w2, u2, nc, verts, mask), c)
    assert not np.array_equal(cref.cip(1.0, w, u, nc, verts, 0), c)


def test_a_lone_cell_has_no_face():
    nc = (1, 1, 1)
    u, w = _fields(nc, 2, 2)
    assert np.array_equal(cref.cip(1.0, w, u, nc, cref.box_vertices(nc), 0), np.zeros(81))


def test_wrappers_add_the_term_with_the_skip_rule():
    """vmult / st_vmult = navier_reference's plus the term; an Alpha entry below 10 eps moves nothing"""
    class Zero:  # (a linear part of zero: the wrappers' additions alone)
        def apply(self, u, p):
            return np.zeros_like(u), np.zeros_like(p)

        def st_vmult(self, Alpha, Beta, ns, nt, blocks, variable_major=True):
            return [np.zeros_like(b) for b in blocks]

    nc, verts, mask = (2, 1, 2), cref.box_vertices((2, 1, 2)), 0
    u, b, u2, b2 = _fields(nc, 9, 4)
    p = np.zeros(4)
    ku, _ = cref.vmult(Zero(), 2.0, cref.SOURCE, nref.FORM, b, u, p, nc, verts, mask)
    assert np.allclose(ku, nref.convection(nref.FORM, b, u, nc, verts, mask) + cref.cip(2.0, u, u, nc, verts, mask), rtol=0, atol=1e-13)
    ku, _ = cref.vmult(Zero(), 2.0, cref.LINEARISATION, nref.FORM, b, u, p, nc, verts, mask)
    assert np.allclose(ku, nref.convection(nref.FORM, b, u, nc, verts, mask) + cref.cip(2.0, b, u, nc, verts, mask), rtol=0, atol=1e-13)
    ku, _ = cref.vmult(Zero(), 2.0, cref.LINEARISATION, 0, b, u, p, nc, verts, mask)  # mode 0: falls back to the source
    assert np.array_equal(ku, cref.cip(2.0, u, u, nc, verts, mask))
    index = lambda it, v, d: v * 2 + d  # noqa: E731
    Alpha = np.zeros((4, 4)); Alpha[0, 0], Alpha[1, 0], Alpha[1, 1], Alpha[0, 1] = 1.5, -0.5, 2.0, 5 * EPS
    dst = cref.st_vmult(Zero(), 1.0, cref.SOURCE, 0, Alpha, np.zeros((4, 4)), 1, 2, [u, u2, p, p], None, index, nc, verts, mask)
    c0, c1 = cref.cip(1.0, u, u, nc, verts, mask), cref.cip(1.0, u2, u2, nc, verts, mask)
    assert np.array_equal(dst[0], 1.5 * c0) and np.allclose(dst[1], -0.5 * c0 + 2.0 * c1, rtol=0, atol=1e-14)
    assert not dst[2].any() and not dst[3].any()


@pytest.mark.parametrize("mask", cref.MASKS)
@pytest.mark.parametrize("mesh", [m for m in cref.MESHES if m != "cell"])
def test_gpu_cases_are_not_hollow(mesh, mask):
    """for every mesh / mask the GPU test uses, with its delta0, nu = 0.3, fields uniform in [-1, 1] and w = u: the term is at least a
    tenth of the linear operator's velocity result, so an error in it cannot hide behind the 1e-12 of the sum"""
    from oracle import oracle
    nc = cref.MESHES[mesh][0]
    verts = cref.mesh_vertices(mesh)
    orc = oracle.StokesOracle(nc, verts, mask, cref.NU)
    rng = np.random.default_rng(cref.FIELD_SEED)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, _ = orc.apply(U, P)
    c = cref.cip(cref.delta0_of(mesh, mask), U, U, nc, verts, mask)
    ratio = np.linalg.norm(c) / np.linalg.norm(ku)
    print(f"{mesh} mask {mask}: |C(u; u)| / |nu K u - B^T p| = {ratio:.3f}")
    assert ratio >= 0.1


def test_library_vertices_of_the_boxes_are_the_plain_grid():
    """the Cartesian meshes run without vertices on the device: the restatement's vertices are that grid"""
    for mesh, (nc, lower, upper, distort) in cref.MESHES.items():
        if distort == 0.0:
            assert np.allclose(np.reshape(cref.mesh_vertices(mesh), (-1, 3)), cref.box_vertices(nc, lower, upper), rtol=0, atol=1e-15)


NEW = ["stfem_stokes_set_cip", "stfem_stokes_cip_add"]


def test_symbols_and_refusals_without_a_device():
    """both symbols are exported and in the veneer's table; every argument refusal is decided before anything touches the device, so it
    is the same with and without a GPU (the context pointer is never dereferenced on these paths except by set_cip, given NULL)"""
    stfem = importlib.import_module("dealii-stfem_amd")
    L = stfem.lib()
    for name in NEW:
        assert name in stfem.SIGNATURES and hasattr(L, name)
    assert (stfem.CIP_WEIGHT_SOURCE, stfem.CIP_WEIGHT_LINEARISATION) == (0, 1)
    buf = (C.c_double * 4)()
    a, b, c = C.addressof(buf), C.addressof(buf) + 8, C.addressof(buf) + 16
    ctx = C.c_void_p(C.addressof(buf) + 24)  # (never dereferenced: the refusals come first)
    assert L.stfem_stokes_set_cip(None, 1.0, 0) == -1
    assert L.stfem_stokes_set_cip(ctx, float("nan"), 0) == -1
    assert L.stfem_stokes_set_cip(ctx, float("inf"), 0) == -1
    assert L.stfem_stokes_set_cip(ctx, 1.0, 2) == -1
    assert L.stfem_stokes_set_cip(ctx, 1.0, -1) == -1
    assert L.stfem_stokes_cip_add(None, a, b, c, 1.0, None) == -1
    assert L.stfem_stokes_cip_add(ctx, None, b, c, 1.0, None) == -1
    assert L.stfem_stokes_cip_add(ctx, a, None, c, 1.0, None) == -1
    assert L.stfem_stokes_cip_add(ctx, a, b, None, 1.0, None) == -1
    assert L.stfem_stokes_cip_add(ctx, a, b, c, float("nan"), None) == -1
    assert L.stfem_stokes_cip_add(ctx, a, a, c, 1.0, None) == -6
    assert L.stfem_stokes_cip_add(ctx, a, b, a, 1.0, None) == -6
