"""The pressure space helpers and the FE_DGP transfers of include/stfem_stokes_pressure_space.h at velocity degree 3 (FE_Q(2) /
FE_DGP(2)), each called through the C-ABI and compared with the numpy restatement tests/stokes_pressure_q3_reference.py (checked by
itself in tests/test_stokes_pressure_q3_reference_cpu.py) - test_pressure_helpers / test_dgp_transfers of
tests/test_gpu_driver_kernels.py one degree up, with its bars: sums rel 1e-12, maxima 1e-13, points 1e-14, the mean of a random vector
1e-12; quantities that are zero in exact arithmetic are bounded by 100 x what the restatement leaves on the same input (floor 1e-12
scale for maxima, 1e-24 scale^2 for squared sums).  A degree-2 context through every _space entry gives the bits of the entry without
the suffix."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stokes_pressure_q3_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL, TOL_MAX = 1e-12, 1e-13
INVALID, UNSUPPORTED, SHAPE_MISMATCH = -1, -2, -5
LOWER, UPPER = (0.0, 0.0, 0.0), (1.0, 0.7, 1.3)  # unequal edge lengths in every mesh below; volume 0.91
MESHES = [(2, 1, 1), (3, 2, 2), (2, 3, 4)]
NQS = (1, 3, 4)
SPACES = pytest.mark.parametrize("dg", [False, True], ids=["FE_Q2", "FE_DGP2"])


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


def op3(stfem, nc, dg, degree=3, **kw):
    return stfem.StokesMatrixFreeOperator.with_degree(degree, nc, lower=LOWER, upper=UPPER, dg_pressure=dg, **kw)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def roundoff_bound(reference_value, floor):
    """100 x the reference's own residual on the same input; the floor where that residual is exactly 0"""
    return 100.0 * reference_value if reference_value > 0.0 else floor


def quadratic(x):
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    return 0.3 + X - 2 * Y + 0.5 * Z + X * X - 0.7 * Y * Y + 1.1 * Z * Z + 0.9 * X * Y - 1.3 * Y * Z + 0.4 * X * Z


def representation(nc, dg):
    """the coefficients of `quadratic` in the degree-2 space: nodal values, or the L2 projection per cell"""
    if not dg:
        ax = [np.linspace(LOWER[e], UPPER[e], 2 * nc[e] + 1) for e in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return quadratic(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))
    xi, w = R.tensor_xi(3)
    return np.einsum("cq,q,qn->cn", quadratic(R.quadrature_points(nc, LOWER, UPPER, 3)), w, R.dgp_basis(2, xi)).ravel()


@SPACES
@pytest.mark.parametrize("nc", MESHES, ids=["2x1x1", "3x2x2", "2x3x4"])
def test_pressure_helpers(stfem, nc, dg):
    op = op3(stfem, nc, dg)
    ncells = int(np.prod(nc))
    assert op.space() == (3, int(dg), 1.0)
    assert op.n_pressure == R.n_pressure(2, nc, dg) == (10 * ncells if dg else int(np.prod([2 * n + 1 for n in nc])))
    rng = np.random.default_rng([nc[0], nc[2], int(dg)])
    coeffs = rng.uniform(-1, 1, op.n_pressure)
    p = op.initialize_dof_vector(1, coeffs)
    ones, weights, volume = op.pressure_mean_vectors()
    ones_ref, weights_ref, volume_ref = R.mean_vectors(2, nc, LOWER, UPPER, dg)
    assert abs(volume - 0.91) <= 1e-14 * 0.91 and abs(volume_ref - 0.91) <= 1e-14
    assert np.array_equal(ones, ones_ref)
    # a sum of n_pressure products of O(1) numbers
    mean_ref = weights_ref @ coeffs / volume_ref
    assert abs(np.dot(weights, coeffs) / volume - mean_ref) <= 1e-12 * np.abs(coeffs).max(), (np.dot(weights, coeffs) / volume, mean_ref)
    assert abs(np.dot(weights, ones) / volume - 1.0) <= 1e-14
    if dg:
        assert np.all(weights.reshape(-1, 10)[:, 1:] == 0.0) and np.all(ones.reshape(-1, 10)[:, 1:] == 0.0)
    p_one, quad = op.initialize_dof_vector(1, ones), representation(nc, dg)
    p_quad = op.initialize_dof_vector(1, quad)
    for nq in NQS + (8, 2):  # one context: the buffer the library keeps across calls grows, and is reused when nq shrinks
        pts = op.pressure_quadrature_points(nq)
        pts_ref = R.quadrature_points(nc, LOWER, UPPER, nq)
        assert pts.shape == pts_ref.shape and np.abs(pts - pts_ref).max() <= 1e-14 * np.abs(pts_ref).max()
        exact = rng.uniform(-1, 1, (ncells, nq ** 3))
        got, ref = op.pressure_difference(nq, p, exact), R.pressure_difference(2, nc, LOWER, UPPER, nq, coeffs, exact, dg)
        print(f"pressure_difference {nc} dg {dg} nq {nq}: got {got} ref {ref}")
        assert abs(got[0] - ref[0]) <= TOL * ref[0] and abs(got[1] - ref[1]) <= TOL_MAX * ref[1], (nq, got, ref)
        # the constant 1 against itself
        got1 = op.pressure_difference(nq, p_one, np.ones((ncells, nq ** 3)))
        ref1 = R.pressure_difference(2, nc, LOWER, UPPER, nq, ones, np.ones((ncells, nq ** 3)), dg)
        assert ref1[0] < 1e-24 and ref1[1] < 1e-12
        assert got1[0] <= roundoff_bound(ref1[0], 1e-24) and got1[1] <= roundoff_bound(ref1[1], 1e-12), (nq, got1, ref1)
        # a quadratic polynomial is in both spaces
        exact = quadratic(pts_ref)
        scale = np.abs(exact).max()
        got2, ref2 = op.pressure_difference(nq, p_quad, exact), R.pressure_difference(2, nc, LOWER, UPPER, nq, quad, exact, dg)
        print(f"quadratic {nc} dg {dg} nq {nq}: got {got2} reference residual {ref2}")
        assert ref2[0] < 1e-24 * scale ** 2 and ref2[1] < 1e-12 * scale
        assert got2[0] <= roundoff_bound(ref2[0], 1e-24 * scale ** 2) and got2[1] <= roundoff_bound(ref2[1], 1e-12 * scale), (nq, got2, ref2)


@SPACES
def test_pressure_context(stfem, dg):
    """FE_Q(2): a scalar degree-2 context on the mesh; FE_DGP(2): a carrier of 10 n_cells DoFs; both serve stfem_dot / axpby on the
    operator's pressure vectors"""
    nc = (3, 2, 2)
    op = op3(stfem, nc, dg)
    L = stfem.lib()
    h = op.pressure_ctx()
    assert h.value and op.pressure_ctx().value == h.value  # made once, owned by the operator
    assert L.stfem_n_dofs(h) == op.n_pressure == (120 if dg else 7 * 5 * 5)
    old = C.c_void_p(5)
    assert L.stfem_stokes_pressure_ctx(op._h, C.byref(old)) == UNSUPPORTED  # the entry of stfem.h: degree 2 only
    rng = np.random.default_rng(8)
    x, y = rng.uniform(-1, 1, op.n_pressure), rng.uniform(-1, 1, op.n_pressure)
    dx, dy = op.initialize_dof_vector(1, x), op.initialize_dof_vector(1, y)
    vx, vy = C.c_void_p(), C.c_void_p()
    for v, d in ((vx, dx), (vy, dy)):
        stfem._check(L.stfem_vector_wrap(h, 1, (C.c_void_p * 1)(d.ptr), C.byref(v)), "stfem_vector_wrap")
    try:
        out = C.c_double(0.0)
        stfem._check(L.stfem_dot(h, vx, vy, 0, C.byref(out), None), "stfem_dot")
        assert abs(out.value - x @ y) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(y)
        stfem._check(L.stfem_vector_axpby(h, 0.5, vx, -2.0, vy, None), "stfem_vector_axpby")
        assert np.abs(dy.download() - (0.5 * x - 2.0 * y)).max() <= 4 * np.finfo(float).eps * 3
        assert np.array_equal(dx.download(), x)
    finally:
        L.stfem_vector_destroy(vx)
        L.stfem_vector_destroy(vy)
    if dg:  # the carrier needs two cells
        lone = op3(stfem, (1, 1, 1), True)
        with pytest.raises(stfem.StfemError) as err:
            lone.pressure_ctx()
        assert err.value.status == UNSUPPORTED and b"n_cells" in L.stfem_last_error()


@SPACES
def test_pressure_helpers_refuse_a_perturbed_mesh(stfem, dg):
    nc = (3, 2, 2)
    verts = stfem.mesh_vertices(nc, LOWER, UPPER, 0.1, 5489)
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=verts, dg_pressure=dg)
    p = op.initialize_dof_vector(1)
    for call in (lambda: op.pressure_quadrature_points(2), lambda: op.pressure_difference(2, p, np.zeros((12, 8))), op.pressure_mean_vectors):
        with pytest.raises(stfem.StfemError) as err:
            call()
        assert err.value.status == UNSUPPORTED and stfem.lib().stfem_last_error()
    if not dg:  # the FE_Q(2) context takes the vertices
        assert stfem.lib().stfem_is_cartesian(op.pressure_ctx()) == 0


@pytest.mark.parametrize("nf,ncoarse", [((2, 2, 2), (1, 1, 1)), ((4, 2, 6), (2, 1, 3))], ids=["2x2x2", "4x2x6"])
def test_dgp_transfers(stfem, nf, ncoarse):
    fine, coarse = op3(stfem, nf, True), op3(stfem, ncoarse, True)
    rng = np.random.default_rng(nf)
    c, f = rng.uniform(-1, 1, coarse.n_pressure), rng.uniform(-1, 1, fine.n_pressure)
    src_c = coarse.initialize_dof_vector(1, c)
    dst_f = fine.initialize_dof_vector(1, np.full(fine.n_pressure, np.nan))
    stfem.stokes_dgp_prolongate(fine, coarse, dst_f, src_c, add=False)  # overwrites NaN
    Pc = dst_f.download()
    assert np.isfinite(Pc).all()
    Pc_ref = R.dgp_prolongate(2, nf, c)
    assert rel(Pc, Pc_ref) < TOL and relmax(Pc, Pc_ref) < TOL
    # the prolongated coefficients describe the same function: at the Gauss points through the library ...
    for nq in (1, 3, 4):
        exact = R.dgp_coarse_values_on_fine(2, nf, c, R.tensor_xi(nq)[0])
        scale = np.abs(exact).max()
        got = fine.pressure_difference(nq, dst_f, exact)
        ref = R.pressure_difference(2, nf, LOWER, UPPER, nq, Pc_ref, exact, True)
        print(f"embedding {nf} nq {nq}: got {got} reference residual {ref}")
        assert ref[0] < 1e-24 * scale ** 2 and ref[1] < 1e-12 * scale
        assert got[0] <= roundoff_bound(ref[0], 1e-24 * scale ** 2) and got[1] <= roundoff_bound(ref[1], 1e-12 * scale), (got, ref)
    # ... and at random points of every child
    xi = rng.uniform(0, 1, (fine.n_cells, 6, 3))
    assert np.abs(R.pressure_values(2, nf, Pc, xi, True) - R.dgp_coarse_values_on_fine(2, nf, c, xi)).max() <= 1e-13
    # restriction = transpose
    src_f = fine.initialize_dof_vector(1, f)
    dst_c = coarse.initialize_dof_vector(1, np.full(coarse.n_pressure, np.nan))
    stfem.stokes_dgp_restrict(fine, coarse, dst_c, src_f, add=False)
    Rf = dst_c.download()
    assert np.isfinite(Rf).all()
    assert rel(Rf, R.dgp_restrict(2, nf, f)) < TOL
    assert abs(np.dot(Rf, c) - np.dot(f, Pc)) <= 1e-13 * np.linalg.norm(f) * np.linalg.norm(Pc)
    # add = 1 adds to what was there: one more rounding per entry
    y_f, y_c = rng.uniform(-1, 1, fine.n_pressure), rng.uniform(-1, 1, coarse.n_pressure)
    dst_f.upload(y_f)
    stfem.stokes_dgp_prolongate(fine, coarse, dst_f, src_c, add=True)
    assert np.all(np.abs(dst_f.download() - (y_f + Pc)) <= 2 * np.finfo(float).eps * (np.abs(y_f) + np.abs(Pc)))
    dst_c.upload(y_c)
    stfem.stokes_dgp_restrict(fine, coarse, dst_c, src_f, add=True)
    assert np.all(np.abs(dst_c.download() - (y_c + Rf)) <= 2 * np.finfo(float).eps * (np.abs(y_c) + np.abs(Rf)))


def test_dgp_transfer_argument_errors(stfem):
    """differing cell counts, a continuous pressure, mixed velocity degrees; the entries of stfem.h refuse degree 3"""
    fine, wrong, cont = op3(stfem, (4, 2, 6), True), op3(stfem, (2, 2, 3), True), op3(stfem, (2, 1, 3), False)
    low = op3(stfem, (2, 1, 3), True, degree=2)
    good = op3(stfem, (2, 1, 3), True)
    f = fine.initialize_dof_vector(1, np.full(fine.n_pressure, 2.0))
    w, c, l, g = (o.initialize_dof_vector(1) for o in (wrong, cont, low, good))
    L = stfem.lib()
    for fn, raw in ((stfem.stokes_dgp_prolongate, L.stfem_stokes_dgp_prolongate), (stfem.stokes_dgp_restrict, L.stfem_stokes_dgp_restrict)):
        up = fn is stfem.stokes_dgp_prolongate
        for other, vec, status, reason in ((wrong, w, SHAPE_MISMATCH, None), (cont, c, UNSUPPORTED, b"FE_DGP"), (low, l, UNSUPPORTED, b"velocity degrees")):
            dst, src = (f, vec) if up else (vec, f)
            with pytest.raises(stfem.StfemError) as err:
                fn(fine, other, dst, src)
            assert err.value.status == status
            if reason:
                assert reason in L.stfem_last_error()
        dst, src = (f, g) if up else (g, f)
        assert raw(fine._h, good._h, dst.ptr, src.ptr, 0, None) == UNSUPPORTED and b"velocity degree 2 only" in L.stfem_last_error()
    assert np.all(f.download() == 2.0)


@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q1", "FE_DGP1"])
def test_degree_2_through_space_entries_is_bit_identical(stfem, dg):
    """a degree-2 context made by descriptor: every _space entry gives the bits of the entry without the suffix"""
    nc, ncoarse = (4, 2, 6), (2, 1, 3)
    old, new = stfem.StokesMatrixFreeOperator(nc, lower=LOWER, upper=UPPER, dg_pressure=dg), op3(stfem, nc, dg, degree=2)
    assert new.space() == (2, int(dg), 1.0)
    rng = np.random.default_rng(17)
    coeffs = rng.uniform(-1, 1, old.n_pressure)
    for a, b in zip(old.pressure_mean_vectors(), new.pressure_mean_vectors()):
        assert np.array_equal(a, b)
    L = stfem.lib()
    assert L.stfem_n_dofs(new.pressure_ctx()) == L.stfem_n_dofs(old.pressure_ctx()) == old.n_pressure
    for nq in NQS:
        assert np.array_equal(old.pressure_quadrature_points(nq), new.pressure_quadrature_points(nq))
        exact = rng.uniform(-1, 1, (old.n_cells, nq ** 3))
        a = old.pressure_difference(nq, old.initialize_dof_vector(1, coeffs), exact)
        b = new.pressure_difference(nq, new.initialize_dof_vector(1, coeffs), exact)
        assert np.array_equal(a, b), (a, b)
    if dg:
        old_c = stfem.StokesMatrixFreeOperator(ncoarse, lower=LOWER, upper=UPPER, dg_pressure=True)
        new_c = op3(stfem, ncoarse, True, degree=2)
        c, y = rng.uniform(-1, 1, old_c.n_pressure), rng.uniform(-1, 1, old.n_pressure)
        for add in (False, True):
            res = []
            for fine, coarse in ((old, old_c), (new, new_c)):
                df, dc = fine.initialize_dof_vector(1, y), coarse.initialize_dof_vector(1, c)
                stfem.stokes_dgp_prolongate(fine, coarse, df, dc, add=add)
                back = coarse.initialize_dof_vector(1, c)
                stfem.stokes_dgp_restrict(fine, coarse, back, df, add=add)
                res.append((df.download(), back.download()))
            assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
