"""The entry points around the operator, each called on its own through the C-ABI and compared with the plain numpy reference
oracle/driver_oracle.py (checked by itself in tests/test_driver_oracle_cpu.py): stfem_support_points, stfem_quadrature_points,
stfem_integrate_rhs(_product), stfem_integrate_difference(_product), stfem_vector_axpby, stfem_vector_set_zero, and on the Stokes
context stfem_stokes_pressure_quadrature_points, stfem_stokes_pressure_difference, stfem_stokes_pressure_mean_vectors,
stfem_stokes_dgp_prolongate, stfem_stokes_dgp_restrict.  (stfem_gauss_rule and stfem_fe_time_points are host code: CPU file.)

Inputs are random per point / per DoF.  Tolerances: fp64 vectors rel-L2 and max-norm 1e-12 (the project's parity bar), fp64 sums
1e-12, maxima 1e-13; the fp32 load vector 1e-5 (TOL32 of test_gpu_parity.py).  Quantities that are zero in exact arithmetic are
bounded by 100 x what the reference itself leaves on the same input (floor: 1e-12 scale for maxima, 1e-24 scale^2 for squared sums,
which is also the ceiling tests/test_driver_oracle_cpu.py holds the reference to).

Measured on an MI355X, fp32 load vector (each cell's value formed in double, the sum over the cells of a DoF in fp32): the largest
rel-L2 error over the grid's fp32 cases is 3.5e-8 (Q2 on 7 x 3 x 2 perturbed cells, nq = 2; max |diff| / max |ref| 4.0e-8), the
fp64 cases stay below 5e-15; test_integrate_rhs prints both figures of every case and keeps them in its assertion message."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from oracle import driver_oracle as D

pytestmark = pytest.mark.gpu
TOL, TOL_MAX, TOL32 = 1e-12, 1e-13, 1e-5
INVALID, UNSUPPORTED, SHAPE_MISMATCH = -1, -2, -5

# p, ncell, geometry ("box", lower, upper) or ("perturbed", distortion), dirichlet mask, nq
GRID = [
    (1, (1, 1, 1), ("box", (0, 0, 0), (2, 1, 0.5)), 0, (1, 2, 8)),
    (2, (7, 3, 2), ("perturbed", 0.15), 0b100110, (2, 3, 4)),
    (3, (3, 4, 2), ("perturbed", 0.2), 63, (3, 4, 7)),  # 7^3 = 343 > 256 points: the strided loops
    (4, (3, 2, 2), ("box", (-1, -1, -1), (1, 2, 1)), 0b010101, (5, 6)),
    (5, (2, 2, 3), ("perturbed", 0.1), 63, (6, 8)),
]
CASES = [pytest.param(i, nq, id=f"Q{g[0]}-{'x'.join(map(str, g[1]))}-{g[2][0]}-nq{nq}") for i, g in enumerate(GRID) for nq in g[4]]
PERTURBED_CASES = [c for c in CASES if GRID[c.values[0]][2][0] == "perturbed"]
NUMBERS = ["double", "float"]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def make_ctx(stfem, cfg, number):
    """(context, the vertex array the reference works on)"""
    p, nc, geo, mask, _ = GRID[cfg]
    if geo[0] == "box":
        ctx = stfem.MatrixFreeOperator(p, nc, lower=geo[1], upper=geo[2], dirichlet_mask=mask, number=number)
        return ctx, D.box_vertices(nc, geo[1], geo[2])
    verts = stfem.mesh_vertices(nc, (0, 0, 0), (1, 1, 1), geo[1], 5489)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, dirichlet_mask=mask, number=number)
    assert not ctx.is_cartesian
    return ctx, verts


def rng_for(cfg, nq, salt):
    return np.random.default_rng([cfg, nq, salt])


@functools.lru_cache(maxsize=None)
def reference_load_vector(cfg, nq):
    p, nc, geo, mask, _ = GRID[cfg]
    verts = D.box_vertices(nc, geo[1], geo[2]) if geo[0] == "box" else None
    if verts is None:
        verts = importlib.import_module("dealii-stfem_amd").mesh_vertices(nc, (0, 0, 0), (1, 1, 1), geo[1], 5489)
    f = rng_for(cfg, nq, 1).uniform(-1, 1, (int(np.prod(nc)), nq ** 3))
    return f, D.load_vector(p, nc, verts, nq, f, mask)


def roundoff_bound(reference_value, floor):
    """100 x the reference's own residual on the same input; the floor where that residual is exactly 0"""
    return 100.0 * reference_value if reference_value > 0.0 else floor


# ------------------------------------------------------------------------------------------------ (a) points

@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("cfg,nq", CASES)
def test_points(stfem, cfg, nq, number):
    p, nc, _, _, _ = GRID[cfg]
    ctx, verts = make_ctx(stfem, cfg, number)
    sp, sp_ref = stfem.support_points(ctx), D.support_points(p, nc, verts)
    assert sp.shape == sp_ref.shape == (ctx.n_dofs, 3)
    assert np.abs(sp - sp_ref).max() <= 1e-14 * np.abs(sp_ref).max()
    qp, qp_ref = stfem.quadrature_points(ctx, nq), D.quadrature_points(p, nc, verts, nq)
    assert qp.shape == qp_ref.shape == (ctx.n_cells, nq ** 3, 3)
    assert np.abs(qp - qp_ref).max() <= 1e-14 * np.abs(qp_ref).max()


# ------------------------------------------------------------------------------------------------ (b) load vector

@pytest.mark.parametrize("own_stream", [False, True], ids=["null-stream", "own-stream"])
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("cfg,nq", CASES)
def test_integrate_rhs(stfem, cfg, nq, number, own_stream):
    p, nc, _, mask, _ = GRID[cfg]
    ctx, _ = make_ctx(stfem, cfg, number)
    f, ref = reference_load_vector(cfg, nq)
    dst = stfem.BlockVector(ctx, 3).upload(np.full((3, ctx.n_dofs), np.nan))
    stream = None
    if own_stream:
        stream = C.c_void_p()
        assert stfem.lib().stfem_stream_create(C.byref(stream)) == 0
    try:
        stfem.integrate_rhs(ctx, nq, f, dst, block=1, stream=stream)  # synchronous
    finally:
        if own_stream:
            stfem.lib().stfem_stream_destroy(stream)
    got = dst.download()
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all()          # the other blocks are not touched
    assert np.isfinite(got[1]).all()                                   # block 1 is overwritten, not accumulated into
    con = D.constrained(p, nc, mask)
    assert np.all(got[1][con] == 0.0) and (con.sum() == 0) == (mask == 0)  # rows named by the mask are exactly 0
    e2, emax = rel(got[1], ref), relmax(got[1], ref)
    print(f"integrate_rhs cfg {cfg} nq {nq} {number}: rel-L2 {e2:.3e} max {emax:.3e}")
    tol = TOL32 if number == "float" else TOL
    assert e2 < tol and emax < tol, f"rel-L2 {e2:.3e}, max |diff| / max |ref| {emax:.3e} ({number})"


# ------------------------------------------------------------------------------------------------ (c) error norms

def check_difference(got, ref, what):
    print(f"{what}: got {got} ref {ref}")
    assert abs(got[0] - ref[0]) <= TOL * abs(ref[0]), (what, got, ref)
    assert abs(got[1] - ref[1]) <= TOL_MAX * abs(ref[1]), (what, got, ref)
    assert abs(got[2] - ref[2]) <= TOL * abs(ref[2]), (what, got, ref)


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("cfg,nq", CASES)
def test_integrate_difference(stfem, cfg, nq, number):
    p, nc, _, _, _ = GRID[cfg]
    ctx, verts = make_ctx(stfem, cfg, number)
    rng = rng_for(cfg, nq, 2)
    U = rng.uniform(-1, 1, (3, ctx.n_dofs))
    exact = rng.uniform(-1, 1, (ctx.n_cells, nq ** 3))
    grad = rng.uniform(-5, 5, (ctx.n_cells, nq ** 3, 3))
    u = stfem.BlockVector(ctx, 3).upload(U)
    # the kernel's arithmetic is double in both instantiations: the fp32 case differs by the rounding of u only
    u_ref = U[2].astype(np.float32).astype(np.float64) if number == "float" else U[2]
    ref = D.difference(p, nc, verts, nq, u_ref, exact, grad)
    check_difference(stfem.integrate_difference(ctx, nq, u, 2, exact, grad), ref, f"cfg {cfg} nq {nq} {number}")
    got = stfem.integrate_difference(ctx, nq, u, 2, exact)
    check_difference(got, (ref[0], ref[1], 0.0), "without gradient")
    assert got[2] == 0.0
    # another block of the same vector is another function
    ref0 = D.difference(p, nc, verts, nq, U[0].astype(np.float32).astype(np.float64) if number == "float" else U[0], exact, grad)
    check_difference(stfem.integrate_difference(ctx, nq, u, 0, exact, grad), ref0, "block 0")


@pytest.mark.parametrize("cfg,nq", PERTURBED_CASES)
def test_integrate_difference_affine_is_exact(stfem, cfg, nq):
    """MappingQ1 reproduces affine functions: all three outputs at round-off, everything taken from the library itself (its
    support points, its quadrature points); J^-1 used transposed would leave an O(1) gradient error on these meshes"""
    p, nc, _, _, _ = GRID[cfg]
    ctx, verts = make_ctx(stfem, cfg, "double")
    a, b = 0.3, np.array([1.1, -0.7, 0.45])
    u_host = a + stfem.support_points(ctx) @ b
    pts = stfem.quadrature_points(ctx, nq)
    exact, grad = a + pts @ b, np.broadcast_to(b, pts.shape)
    got = stfem.integrate_difference(ctx, nq, stfem.BlockVector(ctx, 1).upload(u_host[None]), 0, exact, grad)
    ref = D.difference(p, nc, verts, nq, u_host, exact, grad)
    scale = np.abs(u_host).max()
    print(f"affine cfg {cfg} nq {nq}: got {got} reference residual {ref}")
    assert ref[1] < 1e-12 * scale and ref[0] < 1e-24 * scale ** 2 and ref[2] < 1e-24 * scale ** 2, ref
    assert got[0] <= roundoff_bound(ref[0], 1e-24 * scale ** 2), (got, ref)
    assert got[1] <= roundoff_bound(ref[1], 1e-12 * scale), (got, ref)
    assert got[2] <= roundoff_bound(ref[2], 1e-24 * scale ** 2), (got, ref)


# ------------------------------------------------------------------------------------------------ (d) product variants

def product_function(pts, amplitude, frequency):
    w = 2.0 * np.pi * frequency
    s, c = np.sin(w * pts), np.cos(w * pts)
    val = amplitude * s[..., 0] * s[..., 1] * s[..., 2]
    grad = amplitude * w * np.stack([c[..., 0] * s[..., 1] * s[..., 2], s[..., 0] * c[..., 1] * s[..., 2], s[..., 0] * s[..., 1] * c[..., 2]], axis=-1)
    return val, grad


@pytest.mark.parametrize("frequency", [1.0, 2.5])
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("cfg,nq", [(3, 5), (3, 6), (1, 2), (1, 4)], ids=["box-nq5", "box-nq6", "perturbed-nq2", "perturbed-nq4"])
def test_product_variants(stfem, cfg, nq, number, frequency):
    """the device-evaluated f(x) = amplitude prod sin(2 pi frequency x_d) against the host-array entry points fed with the same
    function, evaluated by numpy at the library's quadrature points"""
    amplitude = -0.7
    ctx, _ = make_ctx(stfem, cfg, number)
    val, grad = product_function(stfem.quadrature_points(ctx, nq), amplitude, frequency)
    a, b = stfem.BlockVector(ctx, 2), stfem.BlockVector(ctx, 2)
    stfem.integrate_rhs(ctx, nq, val, a, block=1)
    stfem.integrate_rhs_product(ctx, nq, amplitude, frequency, b, block=1)
    A, B = a.download(), b.download()
    assert np.all(A[0] == 0.0) and np.all(B[0] == 0.0) and np.abs(A[1]).max() > 0
    tol = TOL32 if number == "float" else TOL
    assert rel(B[1], A[1]) < tol and relmax(B[1], A[1]) < tol, (rel(B[1], A[1]), relmax(B[1], A[1]))
    U = rng_for(cfg, nq, 3).uniform(-1, 1, (2, ctx.n_dofs))
    u = stfem.BlockVector(ctx, 2).upload(U)
    check_difference(stfem.integrate_difference_product(ctx, nq, u, 1, amplitude, frequency),
                     stfem.integrate_difference(ctx, nq, u, 1, val, grad), f"product cfg {cfg} nq {nq} {number} f {frequency}")


# ------------------------------------------------------------------------------------------------ (e) vector arithmetic

@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("nb", [1, 8, 9, 12])  # more than eight blocks: the second launch
def test_vector_axpby_and_set_zero(stfem, nb, number):
    ctx = stfem.MatrixFreeOperator(2, (5, 4, 3), number=number)
    T = np.float32 if number == "float" else np.float64
    wide = np.float64 if number == "float" else np.longdouble   # holds a product of two T exactly (fp32) or to 64 bits (fp64)
    eps = np.finfo(T).eps
    rng = np.random.default_rng(nb)
    X = rng.uniform(-2, 2, (nb, ctx.n_dofs)).astype(T)
    Y = rng.uniform(-2, 2, (nb, ctx.n_dofs)).astype(T)
    bad = np.full((nb, ctx.n_dofs), np.nan)
    bad[:, ::3] = np.inf
    bad[:, 1::3] = -np.inf
    a, b = 1.7, -0.3
    aT, bT = T(a), T(b)  # the library converts the factors to the element type

    def run(fa, x_host, fb, y_host, same=False):
        y = stfem.BlockVector(ctx, nb).upload(y_host)
        x = y if same else stfem.BlockVector(ctx, nb).upload(x_host)
        stfem.vector_axpby(ctx, fa, x, fb, y)
        out = y.download()
        if not same:
            assert np.array_equal(x.download(), np.asarray(x_host, dtype=np.float64), equal_nan=True)  # x is read only
        return out

    def close(got, x, y):
        """a x + b y with or without contraction to an fma: both lie within one ulp (at the size of the terms) of the exact value"""
        ax, by = wide(aT) * x.astype(wide), wide(bT) * y.astype(wide)
        assert np.all(np.abs(got.astype(wide) - (ax + by)) <= eps * (np.abs(ax) + np.abs(by)))

    close(run(a, X, b, Y), X, Y)
    assert np.array_equal(run(a, X, 0.0, bad), (aT * X).astype(np.float64))          # b = 0: y is not read
    assert np.array_equal(run(0.0, bad, b, Y), (bT * Y).astype(np.float64))          # a = 0: x is not read
    assert np.array_equal(run(0.0, bad, 0.0, bad), np.zeros((nb, ctx.n_dofs)))       # both: assigns zero
    close(run(a, None, b, Y, same=True), Y, Y)                                        # x and y the same vector
    assert np.array_equal(run(a, None, 0.0, Y, same=True), (aT * Y).astype(np.float64))
    y = stfem.BlockVector(ctx, nb).upload(bad)
    stfem.vector_set_zero(ctx, y)
    assert np.array_equal(y.download(), np.zeros((nb, ctx.n_dofs)))
    # argument errors: vectors of another context or with another number of blocks
    other = stfem.MatrixFreeOperator(2, (5, 4, 3), number=number)
    L = stfem.lib()
    x = stfem.BlockVector(ctx, nb).upload(X)
    assert L.stfem_vector_axpby(ctx._h, 1.0, stfem.BlockVector(other, nb)._h, 1.0, x._h, None) == INVALID
    assert L.stfem_vector_axpby(ctx._h, 1.0, stfem.BlockVector(ctx, nb + 1)._h, 1.0, x._h, None) == INVALID
    assert L.stfem_vector_set_zero(other._h, x._h, None) == INVALID
    assert np.array_equal(x.download(), X.astype(np.float64))


# ------------------------------------------------------------------------------------------------ (f) pressure helpers

P_LOWER, P_UPPER = (0.0, 0.0, 0.0), (1.0, 0.7, 1.3)


def stokes_op(stfem, nc, dg, **kw):
    return stfem.StokesMatrixFreeOperator(nc, lower=P_LOWER, upper=P_UPPER, dg_pressure=dg, **kw)


@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q1", "FE_DGP1"])
@pytest.mark.parametrize("nc", [(4, 2, 6), (1, 1, 2)], ids=["4x2x6", "1x1x2"])
def test_pressure_helpers(stfem, nc, dg):
    op = stokes_op(stfem, nc, dg)
    verts = D.box_vertices(nc, P_LOWER, P_UPPER)
    ncells = int(np.prod(nc))
    assert op.n_pressure == (4 * ncells if dg else D.n_dofs(1, nc))
    rng = np.random.default_rng([nc[0], nc[2], int(dg)])
    coeffs = rng.uniform(-1, 1, op.n_pressure)
    p = op.initialize_dof_vector(1, coeffs)
    ones, weights, volume = op.pressure_mean_vectors()
    p_one = op.initialize_dof_vector(1, ones)
    assert abs(volume - 0.91) <= 1e-14 * 0.91
    mean_ref, vol_ref = D.pressure_mean(nc, verts, coeffs, dg)
    assert abs(vol_ref - 0.91) <= 1e-14
    # a sum of n_pressure products of O(1) numbers
    assert abs(np.dot(weights, coeffs) / volume - mean_ref) <= 1e-12 * np.abs(coeffs).max(), (np.dot(weights, coeffs) / volume, mean_ref)
    assert abs(np.dot(weights, ones) / volume - 1.0) <= 1e-14
    for nq in (2, 5, 1, 8, 3):  # one context: the buffer the library keeps across calls grows, and is reused when nq shrinks
        pts = op.pressure_quadrature_points(nq)
        pts_ref = D.pressure_quadrature_points(nc, verts, nq)
        assert pts.shape == pts_ref.shape and np.abs(pts - pts_ref).max() <= 1e-14 * np.abs(pts_ref).max()
        exact = rng.uniform(-1, 1, (ncells, nq ** 3))
        got, ref = op.pressure_difference(nq, p, exact), D.pressure_difference(nc, verts, nq, coeffs, exact, dg)
        print(f"pressure_difference {nc} dg {dg} nq {nq}: got {got} ref {ref}")
        assert abs(got[0] - ref[0]) <= TOL * ref[0] and abs(got[1] - ref[1]) <= TOL_MAX * ref[1], (nq, got, ref)
        # the constant 1 against itself
        got1 = op.pressure_difference(nq, p_one, np.ones((ncells, nq ** 3)))
        ref1 = D.pressure_difference(nc, verts, nq, ones, np.ones((ncells, nq ** 3)), dg)
        assert ref1[0] < 1e-24 and ref1[1] < 1e-12
        assert got1[0] <= roundoff_bound(ref1[0], 1e-24) and got1[1] <= roundoff_bound(ref1[1], 1e-12), (nq, got1, ref1)


@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q1", "FE_DGP1"])
def test_pressure_helpers_refuse_a_perturbed_mesh(stfem, dg):
    nc = (4, 2, 6)
    verts = stfem.mesh_vertices(nc, P_LOWER, P_UPPER, 0.1, 5489)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts, dg_pressure=dg)
    p = op.initialize_dof_vector(1)
    for call in (lambda: op.pressure_quadrature_points(2), lambda: op.pressure_difference(2, p, np.zeros((48, 8))), op.pressure_mean_vectors):
        with pytest.raises(stfem.StfemError) as err:
            call()
        assert err.value.status == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ (g) FE_DGP(1) transfers

@pytest.mark.parametrize("nf,ncoarse", [((4, 2, 6), (2, 1, 3)), ((2, 2, 2), (1, 1, 1))], ids=["4x2x6", "2x2x2"])
def test_dgp_transfers(stfem, nf, ncoarse):
    fine, coarse = stokes_op(stfem, nf, True), stokes_op(stfem, ncoarse, True)
    verts = D.box_vertices(nf, P_LOWER, P_UPPER)
    rng = np.random.default_rng(nf)
    c, f = rng.uniform(-1, 1, coarse.n_pressure), rng.uniform(-1, 1, fine.n_pressure)
    src_c = coarse.initialize_dof_vector(1, c)
    dst_f = fine.initialize_dof_vector(1, np.full(fine.n_pressure, np.nan))
    stfem.stokes_dgp_prolongate(fine, coarse, dst_f, src_c, add=False)  # overwrites NaN
    Pc = dst_f.download()
    assert np.isfinite(Pc).all()
    Pc_ref = D.dgp_prolongate(nf, c)
    assert rel(Pc, Pc_ref) < TOL and relmax(Pc, Pc_ref) < TOL
    # the prolongated coefficients describe the same function
    for nq in (2, 3):
        exact = D.dgp_coarse_values_on_fine(nf, c, D._tensor_xi(nq))
        scale = np.abs(exact).max()
        got = fine.pressure_difference(nq, dst_f, exact)
        ref = D.pressure_difference(nf, verts, nq, Pc_ref, exact, True)
        print(f"embedding {nf} nq {nq}: got {got} reference residual {ref}")
        assert ref[0] < 1e-24 * scale ** 2 and ref[1] < 1e-12 * scale
        assert got[0] <= roundoff_bound(ref[0], 1e-24 * scale ** 2) and got[1] <= roundoff_bound(ref[1], 1e-12 * scale), (got, ref)
    # restriction = transpose
    src_f = fine.initialize_dof_vector(1, f)
    dst_c = coarse.initialize_dof_vector(1, np.full(coarse.n_pressure, np.nan))
    stfem.stokes_dgp_restrict(fine, coarse, dst_c, src_f, add=False)
    Rf = dst_c.download()
    assert np.isfinite(Rf).all()
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
    fine, wrong, cont = stokes_op(stfem, (4, 2, 6), True), stokes_op(stfem, (2, 2, 3), True), stokes_op(stfem, (2, 1, 3), False)
    f = fine.initialize_dof_vector(1, np.full(fine.n_pressure, 2.0))
    w, c = wrong.initialize_dof_vector(1), cont.initialize_dof_vector(1)
    for fn in (stfem.stokes_dgp_prolongate, stfem.stokes_dgp_restrict):
        dst, src = (f, w) if fn is stfem.stokes_dgp_prolongate else (w, f)
        with pytest.raises(stfem.StfemError) as err:
            fn(fine, wrong, dst, src)
        assert err.value.status == SHAPE_MISMATCH
        dst, src = (f, c) if fn is stfem.stokes_dgp_prolongate else (c, f)
        with pytest.raises(stfem.StfemError) as err:
            fn(fine, cont, dst, src)
        assert err.value.status == UNSUPPORTED
    assert np.all(f.download() == 2.0)


# ------------------------------------------------------------------------------------------------ (h) argument errors

@pytest.mark.parametrize("number", NUMBERS)
def test_argument_errors_on_a_live_context(stfem, number):
    cfg, nq = 1, 3
    ctx, _ = make_ctx(stfem, cfg, number)
    other, _ = make_ctx(stfem, cfg, number)
    keep = np.random.default_rng(5).uniform(-1, 1, (3, ctx.n_dofs)).astype(np.float32).astype(np.float64)
    dst, foreign = stfem.BlockVector(ctx, 3).upload(keep), stfem.BlockVector(other, 3)
    f = np.ones((ctx.n_cells, nq ** 3))
    grad = np.ones((ctx.n_cells, nq ** 3, 3))

    def refused(call):
        with pytest.raises(stfem.StfemError) as err:
            call()
        assert err.value.status == INVALID
        assert np.array_equal(dst.download(), keep)

    for bad_nq in (0, 9):
        refused(lambda: stfem.integrate_rhs(ctx, bad_nq, f, dst, 1))
        refused(lambda: stfem.integrate_rhs_product(ctx, bad_nq, 1.0, 1.0, dst, 1))
        refused(lambda: stfem.integrate_difference(ctx, bad_nq, dst, 1, f, grad))
        refused(lambda: stfem.integrate_difference_product(ctx, bad_nq, dst, 1, 1.0, 1.0))
        refused(lambda: stfem.quadrature_points(ctx, bad_nq))
    for bad_block in (-1, 3):
        refused(lambda: stfem.integrate_rhs(ctx, nq, f, dst, bad_block))
        refused(lambda: stfem.integrate_rhs_product(ctx, nq, 1.0, 1.0, dst, bad_block))
        refused(lambda: stfem.integrate_difference(ctx, nq, dst, bad_block, f, grad))
        refused(lambda: stfem.integrate_difference_product(ctx, nq, dst, bad_block, 1.0, 1.0))
    refused(lambda: stfem.integrate_rhs(ctx, nq, f, foreign, 1))
    refused(lambda: stfem.integrate_rhs(other, nq, f, dst, 1))
    refused(lambda: stfem.integrate_difference(ctx, nq, foreign, 1, f, grad))
    refused(lambda: stfem.integrate_rhs(ctx, nq, None, dst, 1))
    refused(lambda: stfem.integrate_difference(ctx, nq, dst, 1, None, grad))
    L = stfem.lib()
    assert L.stfem_support_points(ctx._h, None) == INVALID and L.stfem_support_points(None, None) == INVALID
    assert L.stfem_integrate_difference(ctx._h, nq, dst._h, 1, f.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) == INVALID
    assert np.all(foreign.download() == 0.0)
    # and the context still works
    stfem.integrate_rhs(ctx, nq, f, dst, 1)
    assert np.array_equal(dst.download()[[0, 2]], keep[[0, 2]]) and not np.array_equal(dst.download()[1], keep[1])
