"""The Krylov and plane entry points, each called on its own through the C-ABI and compared with the exact reference
oracle/krylov_oracle.py (checked by itself in tests/test_krylov_oracle_cpu.py): stfem_dot, stfem_multi_dot, stfem_multi_axpy,
stfem_orthogonalize, stfem_tensorproduct_add, stfem_plane_pack, stfem_plane_unpack, stfem_planes_move.

The meshes only carry a vector length.  Inputs: seeded uniform values scaled by position, rounded to float on the host for the
float contexts (the reference sees what the device sees), and one cancellation case per reduction.  Every bound is computed from
the inputs; U64 = 2^-53 and U32 = 2^-24 are the unit roundoffs, `magnitude` the sum of the absolute values of the terms.

 inner products   |got - exact| <= (m + 18) U64 sum |a_i b_i|, m = nb ceil(n_own / (grid 256)), grid = min(ceil(n_own / 256), 512):
                  m fused multiply-adds per thread, then 6 shuffle steps, 2 adds over the four waves, at most 2 strided adds
                  and 8 tree steps in the finishing kernel.  The same for float: a product of two floats is exact in double.
 multi_axpy       elementwise (k + 1) U64 (|y| + sum |c_v x_v|); float: plus ceil(k / 8) U32 (...), one rounding per launch.
 tensorproduct    elementwise (ncols + 1) U_T (|c_i| + sum_j |A_ij| |b_j|), A converted to T first.
 orthogonalize    h, <w, w> before and after: the inner-product bound; the projected vector: multi_axpy's bound around the
                  reference projection with the h the library returned.
 planes           copies and single additions in T: bitwise.

Measured on an MI355X, the largest error / bound over all cases (every test prints its own figure, "RATIO ..." with -s):
                              double   float
 dot                          0.056    0.032
 multi_dot                    0.079    0.011
 multi_axpy                   0.496    0.989   (float, k = 1: one rounding to float of a sum with little cancellation)
 orthogonalize h              0.024    0.011
 orthogonalize <w, w>         0.092    0.096
 orthogonalize w              0.466    0.927
 second pass |h| / its bound  0.011    0.032
 tensorproduct_add            0.634    0.645
Every context, the 2 M-DoF ones included, is created in 0.1 ms (nothing is built on the device before the first operator apply);
the first one of a process takes 0.06 s.  The slowest case (test_dot on Q2 26^3, nb = 3) takes 0.6 s, most of it the reference."""
import ctypes as C
import gc
import importlib
import time

import numpy as np
import pytest

from oracle import krylov_oracle as K

pytestmark = pytest.mark.gpu
NUMBERS = ["double", "float"]
INVALID, UNSUPPORTED, SHAPE_MISMATCH, ALIAS = -1, -2, -5, -6
U64, U32 = 2.0 ** -53, 2.0 ** -24
# DOT_GRID (csrc/stfem_internal.h) and the workgroup size of multi_dot_kernel (csrc/stfem_vector.hip): the inner-product bound depends on them
DOT_GRID, WORKGROUP = 512, 256

MESHES = {  # name: (degree, cells): DoFs per block, purpose
    "q1_1": (1, (1, 1, 1)),        # 8: the smallest vector
    "q2_322": (2, (3, 2, 2)),      # 175: shorter than one workgroup
    "q1_377": (1, (3, 7, 7)),      # 256: exactly one workgroup
    "q2_975": (2, (9, 7, 5)),      # 3 135: several workgroups, a ragged last one
    "q2_26": (2, (26, 26, 26)),    # 148 877 > 512 x 256: the stride loop of the dot
    "q2_40": (2, (40, 40, 40)),    # 531 441 > 2048 x 256: the stride loop of multi_axpy
    "q2_51": (2, (51, 51, 51)),    # 1 092 727 > 4096 x 256: the stride loop of tensorproduct_add
    "q1_512": (1, (512, 512, 1)),  # plane 513^2 > 1024 x 256: the stride loop of planes_move
    "q1_1023": (1, (1023, 1023, 1)),  # plane 1024^2 = 4096 x 256: plane_unpack's grid cap exactly
    "q1_373": (1, (3, 7, 3)),      # the plane of q1_377 with another nz
}
SMALL = ["q1_1", "q2_322", "q1_377"]
_ratios = {}


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


LARGE = {"q2_26", "q2_40", "q2_51", "q1_512", "q1_1023"}  # created for the test that needs them and released with it
_contexts = {}


def context(mesh, number, instance=0):
    """one context per (mesh, precision) for the small meshes; instance 1 is a second context of the same mesh (the 'foreign'
    vectors).  Prints how long the creation took."""
    key = (mesh, number, int(instance))
    if key in _contexts:
        return _contexts[key]
    p, nc = MESHES[mesh]
    t0 = time.perf_counter()
    ctx = importlib.import_module("dealii-stfem_amd").MatrixFreeOperator(p, nc, number=number)
    print(f"CONTEXT {mesh} {number}: created in {time.perf_counter() - t0:.4f} s")
    if mesh not in LARGE:
        _contexts[key] = ctx
    return ctx


@pytest.fixture(scope="module", autouse=True)
def release_contexts():
    yield
    _contexts.clear()
    gc.collect()


def dims(mesh):
    p, nc = MESHES[mesh]
    nd = [p * c + 1 for c in nc]
    return nd[0] * nd[1], nd[2]  # plane, nz


def record(entry, number, err, bound):
    """err / bound (arrays: the largest), kept per entry point and precision and printed"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1e-300)))) if err.size else 0.0
    _ratios[(entry, number)] = max(_ratios.get((entry, number), 0.0), ratio)
    print(f"RATIO {entry} {number}: {ratio:.3f} (largest so far {_ratios[(entry, number)]:.3f})")
    return ratio


def err_of(got, exact):
    return np.abs((np.asarray(got) - exact.value) - exact.residual)


def inner_product_bound(nb, n_own, magnitude):
    grid = min(-(-n_own // WORKGROUP), DOT_GRID)
    m = nb * -(-n_own // (grid * WORKGROUP))
    return (m + 18) * U64 * magnitude


def axpy_bound(k, number, magnitude):
    return (k + 1) * U64 * magnitude + (-(-k // 8) * U32 * magnitude if number == "float" else 0.0)


def n_owns(n, plane):
    return [v for v in (0, 1, 255, 256, 257, n - plane, n, n + 1, -3) if v <= n + 1]


def nan_beyond(a, n_own, n):
    a = a.copy()
    a[:, K.owned(n, n_own):] = np.nan
    return a


def status_of(stfem, call):
    with pytest.raises(stfem.StfemError) as e:
        call()
    return e.value.status


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------- dot

@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh,nb", [(m, nb) for m in SMALL for nb in (1, 3, 8, 9, 12)] + [("q2_26", 1), ("q2_26", 3)])
def test_dot(stfem, mesh, nb, number):
    ctx = context(mesh, number)
    n, plane = ctx.n_dofs, dims(mesh)[0]
    A = K.seeded_blocks(1, nb, n, number)
    B = K.seeded_blocks(2, nb, n, number)
    a, b = stfem.BlockVector(ctx, nb).upload(A), stfem.BlockVector(ctx, nb)
    big = mesh == "q2_26"
    for n_own in ((0, n - plane) if big and nb > 1 else n_owns(n, plane)):
        no = K.owned(n, n_own)
        b.upload(nan_beyond(B, n_own, n))  # the entries at and beyond n_own are not read
        want = K.dot(A, B, n_own)
        got = stfem.dot(ctx, a, b, n_own)
        bound = inner_product_bound(nb, no, want.magnitude)
        record("dot", number, err_of(got, want), bound)
        assert err_of(got, want) <= bound, (n_own, got, want, bound)
        assert got == stfem.dot(ctx, a, b, n_own)  # a second call returns the same bits
    for n_own in (0, n - plane):  # the cancellation case: the exact product is about 1e-12 of the absolute sum
        Bc = K.cancelling_partner(A, 3, number, n_own)
        b.upload(nan_beyond(Bc, n_own, n))
        want = K.dot(A, Bc, n_own)
        got = stfem.dot(ctx, a, b, n_own)
        bound = inner_product_bound(nb, K.owned(n, n_own), want.magnitude)
        record("dot", number, err_of(got, want), bound)
        assert err_of(got, want) <= bound, ("cancelling", n_own, got, want, bound)


# ----------------------------------------------------------------------------------------------- multi_dot

MULTI_DOT = [(m, 3, k) for m in ("q2_322", "q2_975") for k in (1, 7, 8, 9, 16, 17, 33)] + [("q2_322", 1, 248), ("q2_26", 1, 9)]


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh,nb,k", MULTI_DOT)
def test_multi_dot(stfem, mesh, nb, k, number):
    ctx = context(mesh, number)
    n, plane = ctx.n_dofs, dims(mesh)[0]
    distinct = min(k, 10)  # k = 248, the limit: the handles repeat
    V = [K.seeded_blocks(10 + v, nb, n, number) for v in range(distinct)]
    W = K.seeded_blocks(2, nb, n, number)
    V[distinct // 2] = K.cancelling_partner(W, 3, number)  # one cancellation case (over the whole vector)
    vecs = [stfem.BlockVector(ctx, nb).upload(v) for v in V]
    vs = [vecs[i % distinct] for i in range(k)]
    w = stfem.BlockVector(ctx, nb)
    stream = C.c_void_p()
    assert stfem.lib().stfem_stream_create(C.byref(stream)) == 0
    try:
        for n_own in ((0, n - plane) if mesh == "q2_26" else n_owns(n, plane)):
            no = K.owned(n, n_own)
            w.upload(nan_beyond(W, n_own, n))
            got = stfem.multi_dot(ctx, vs, w, n_own)
            want = [K.dot(v, W, n_own) for v in V]
            err = np.array([err_of(got[i], want[i % distinct]) for i in range(k)])
            bound = np.array([inner_product_bound(nb, no, want[i % distinct].magnitude) for i in range(k)])
            record("multi_dot", number, err, bound)
            assert (err <= bound).all(), (n_own, err / bound)
            # every entry is stfem_dot's, a second call and a call on a stream of its own return the same bits
            singles = np.array([stfem.dot(ctx, vecs[i], w, n_own) for i in range(distinct)])
            assert same_bits(got, singles[np.arange(k) % distinct]), n_own
            assert same_bits(got, stfem.multi_dot(ctx, vs, w, n_own))
            assert same_bits(got, stfem.multi_dot(ctx, vs, w, n_own, stream=stream))
    finally:
        stfem.lib().stfem_stream_destroy(stream)


# ----------------------------------------------------------------------------------------------- multi_axpy

@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh,nb,k", [(m, nb, k) for m in ("q2_322", "q2_975") for nb in (1, 8) for k in (1, 8, 9, 17)] + [("q2_40", 1, 9)])
def test_multi_axpy(stfem, mesh, nb, k, number):
    ctx = context(mesh, number)
    n = ctx.n_dofs
    X = [K.seeded_blocks(10 + v, nb, n, number) for v in range(k)]
    Y = K.seeded_blocks(2, nb, n, number)
    coef = np.random.default_rng(k).uniform(-1, 1, k)
    if k > 1:
        coef[k // 2] = 0.0  # a coefficient of 0
    xs = [stfem.BlockVector(ctx, nb).upload(x) for x in X]
    y = stfem.BlockVector(ctx, nb).upload(Y)
    stfem.multi_axpy(ctx, coef, xs, y)
    got = y.download()
    want = K.multi_axpy(coef, X, Y)
    bound = axpy_bound(k, number, want.magnitude)
    record("multi_axpy", number, err_of(got, want), bound)
    assert (err_of(got, want) <= bound).all()
    for x, v in zip(X, xs):
        assert same_bits(v.download(), x)  # the x vectors are unchanged


# ----------------------------------------------------------------------------------------------- orthogonalize

def call_orthogonalize(stfem, ctx, vs, w, n_own, with_before, with_after):
    k = len(vs)
    h = np.zeros(k)
    before, after = C.c_double(np.nan), C.c_double(np.nan)
    arr = (C.c_void_p * k)(*[v._h for v in vs])
    rc = stfem.lib().stfem_orthogonalize(ctx._h, k, arr, w._h, n_own, h.ctypes.data_as(C.POINTER(C.c_double)),
                                         C.byref(before) if with_before else None, C.byref(after) if with_after else None, None)
    assert rc == 0, rc
    return h, before.value, after.value


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("own_plane", [False, True], ids=["all", "owned"])
@pytest.mark.parametrize("k", [1, 8, 9, 17, 247])
def test_orthogonalize(stfem, k, own_plane, number):
    mesh, nb = "q2_322", (1 if k == 247 else 3)
    ctx = context(mesh, number)
    n, plane = ctx.n_dofs, dims(mesh)[0]
    n_own = n - plane if own_plane else 0
    no = K.owned(n, n_own)
    distinct = min(k, 12)  # k = 247, the limit: the handles repeat
    V = [0.25 * K.seeded_blocks(10 + v, nb, n, number) for v in range(distinct)]  # (a power of two: floats stay floats)
    W = K.seeded_blocks(2, nb, n, number)
    vecs = [stfem.BlockVector(ctx, nb).upload(v) for v in V]
    vs = [vecs[i % distinct] for i in range(k)]
    Vk = [V[i % distinct] for i in range(k)]
    w = stfem.BlockVector(ctx, nb)
    forms = []
    for with_before, with_after in ((True, True), (False, True), (False, False)):  # the second is the driver's second pass
        w.upload(W)
        h, before, after = call_orthogonalize(stfem, ctx, vs, w, n_own, with_before, with_after)
        forms.append((h, before, after, w.download()))
    h, before, after, got = forms[0]
    for h2, _, _, w2 in forms[1:]:  # what is not asked for changes nothing else
        assert same_bits(h, h2) and same_bits(got, w2)
    assert same_bits(after, forms[1][2]) and np.isnan(forms[1][1]) and np.isnan(forms[2][1]) and np.isnan(forms[2][2])
    # the inner products are over the owned range ...
    want_h = [K.dot(v, W, n_own) for v in V]
    err = np.array([err_of(h[i], want_h[i % distinct]) for i in range(k)])
    bound = np.array([inner_product_bound(nb, no, want_h[i % distinct].magnitude) for i in range(k)])
    record("orthogonalize_h", number, err, bound)
    assert (err <= bound).all(), err / bound
    for name, value, exact in (("before", before, K.dot(W, W, n_own)), ("after", after, K.dot(got, got, n_own))):
        b = inner_product_bound(nb, no, exact.magnitude)
        record("orthogonalize_norm2", number, err_of(value, exact), b)
        assert err_of(value, exact) <= b, (name, value, exact)
    # ... the update over the whole vector, with the coefficients the library returned
    want = K.multi_axpy(-h, Vk, W)
    vbound = axpy_bound(k, number, want.magnitude)
    record("orthogonalize_w", number, err_of(got, want), vbound)
    assert (err_of(got, want) <= vbound).all()
    for x, v in zip(V, vecs):
        assert same_bits(v.download(), x)


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("own_plane", [False, True], ids=["all", "owned"])
@pytest.mark.parametrize("k", [1, 8, 9, 17])
def test_orthogonalize_second_pass_on_an_orthonormal_basis(stfem, k, own_plane, number):
    """V from a host QR (orthonormal over the owned range up to the rounding of Number).  After one pass the exact <v_i, w> is
    (<v_i, W> - h_i) - sum_j (G_ij - delta_ij) h_j + <v_i, d> with G the Gram matrix of V and d the rounding error of the update,
    so the second pass returns at most: its own inner-product bound, plus the first pass's, plus sum_j |G_ij - delta_ij| |h_j|,
    plus sum |v_i| x the update's bound - all computed here from the inputs."""
    mesh, nb = "q2_322", 3
    ctx = context(mesh, number)
    n, plane = ctx.n_dofs, dims(mesh)[0]
    n_own = n - plane if own_plane else 0
    no = K.owned(n, n_own)
    Q = np.linalg.qr(np.random.default_rng(k).uniform(-1, 1, (nb * no, k)))[0]
    V = []
    for v in range(k):
        x = K.seeded_blocks(10 + v, nb, n, number)  # (the entries beyond the owned range: anything)
        x[:, :no] = Q[:, v].reshape(nb, no)
        V.append(K.round_to(number, x))
    W = K.seeded_blocks(2, nb, n, number)
    vs = [stfem.BlockVector(ctx, nb).upload(v) for v in V]
    w = stfem.BlockVector(ctx, nb).upload(W)
    h1, _, _ = call_orthogonalize(stfem, ctx, vs, w, n_own, True, True)
    W1 = w.download()
    h2, before2, after2 = call_orthogonalize(stfem, ctx, vs, w, n_own, False, True)
    first = [K.dot(v, W, n_own) for v in V]
    second = [K.dot(v, W1, n_own) for v in V]
    update = axpy_bound(k, number, K.multi_axpy(-h1, V, W).magnitude)
    for i in range(k):
        own = inner_product_bound(nb, no, second[i].magnitude)
        assert err_of(h2[i], second[i]) <= own
        gram = sum(abs(K.dot(V[i], V[j], n_own).value - (i == j)) * abs(h1[j]) for j in range(k))
        around_zero = own + inner_product_bound(nb, no, first[i].magnitude) + gram + float(np.sum(np.abs(V[i][:, :no]) * update[:, :no]))
        record("orthogonalize_second_pass", number, abs(h2[i]), around_zero)
        assert abs(h2[i]) <= around_zero, (i, h2[i], around_zero)


# ----------------------------------------------------------------------------------------------- tensorproduct_add

def tensor_bound(ncols, number, magnitude):
    return (ncols + 1) * (U32 if number == "float" else U64) * magnitude


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh,shape", [(m, s) for m in ("q2_322", "q2_975") for s in ((1, 1), (2, 3), (3, 2), (8, 8), (2, 9), (12, 12))]
                         + [("q2_51", (1, 2))])
def test_tensorproduct_add(stfem, mesh, shape, number):
    ctx = context(mesh, number)
    n = ctx.n_dofs
    A = np.random.default_rng(shape[0] * 16 + shape[1]).uniform(-2, 2, shape)
    Bm, Cm = K.seeded_blocks(20, shape[1], n, number), K.seeded_blocks(21, shape[0], n, number)
    b, c = stfem.BlockVector(ctx, shape[1]).upload(Bm), stfem.BlockVector(ctx, shape[0]).upload(Cm)
    stfem.tensorproduct_add(ctx, c, A, b)
    got = c.download()
    want = K.tensorproduct_add(Cm, A, Bm, number)
    bound = tensor_bound(shape[1], number, want.magnitude)
    record("tensorproduct_add", number, err_of(got, want), bound)
    assert (err_of(got, want) <= bound).all()
    assert same_bits(b.download(), Bm)


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("shape", [(2, 3), (3, 9), (12, 12)])
def test_tensorproduct_add_skips_exact_zeros(stfem, shape, number):
    """A(i, j) == 0: b_j is not read (a column of NaN and Inf under a zero column of A does not spread); a zero row of A leaves
    its destination block bitwise as it was"""
    ctx = context("q2_322", number)
    n = ctx.n_dofs
    A = np.random.default_rng(shape[0] + 100 * shape[1]).uniform(-2, 2, shape)
    dead_col, dead_row = shape[1] - 1, shape[0] - 1
    A[:, dead_col] = 0.0
    A[dead_row, :] = 0.0
    Bm, Cm = K.seeded_blocks(20, shape[1], n, number), K.seeded_blocks(21, shape[0], n, number)
    Bm[dead_col, 0::2] = np.nan
    Bm[dead_col, 1::2] = np.inf
    b, c = stfem.BlockVector(ctx, shape[1]).upload(Bm), stfem.BlockVector(ctx, shape[0]).upload(Cm)
    stfem.tensorproduct_add(ctx, c, A, b)
    got = c.download()
    assert np.isfinite(got).all()
    want = K.tensorproduct_add(Cm, A, Bm, number)
    assert (err_of(got, want) <= tensor_bound(shape[1], number, want.magnitude)).all()
    assert same_bits(got[dead_row], Cm[dead_row])


# ----------------------------------------------------------------------------------------------- planes

def pattern(nb, n, number, salt=0):
    """a known pattern, exact in float: every entry differs from its neighbours"""
    return K.round_to(number, ((np.arange(nb * n, dtype=np.float64).reshape(nb, n) * 7 + salt) % 1021) / 8.0 + 1.0)


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh,nb", [("q1_1", 1), ("q2_322", 3), ("q1_377", 2), ("q1_512", 1), ("q1_1023", 1)])
def test_plane_pack_unpack(stfem, mesh, nb, number):
    ctx = context(mesh, number)
    L = stfem.lib()
    n, (plane, nz) = ctx.n_dofs, dims(mesh)
    assert nb * plane <= n
    S = K.seeded_blocks(1, nb, n, number)
    src = stfem.BlockVector(ctx, nb).upload(S)
    dst, hold = stfem.BlockVector(ctx, nb), stfem.BlockVector(ctx, 1)
    buf = hold.block_ptr(0)  # nb planes fit into one block
    for iz in sorted({0, 1, nz - 1}):
        for add in (0, 1):
            D0 = pattern(nb, n, number, iz)
            dst.upload(D0)
            hold.upload(np.full((1, n), -77.0))
            assert L.stfem_plane_pack(ctx._h, src._h, iz, buf, None) == 0
            packed = K.round_to(number, hold.download())  # (the buffer holds Numbers: read it back through the vector)
            assert same_bits(packed[0, :nb * plane], K.plane_pack(S, iz, plane).ravel()) and (packed[0, nb * plane:] == -77.0).all()
            assert L.stfem_plane_unpack(ctx._h, dst._h, nz - 1 - iz, buf, add, None) == 0
            want = K.plane_unpack(D0, nz - 1 - iz, K.plane_pack(S, iz, plane), add, plane, number)
            assert same_bits(dst.download(), want), (iz, add)  # the plane, and everything outside it bitwise as it was
            assert same_bits(src.download(), S)


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("src_mesh,dst_mesh,nb", [("q1_1", "q1_1", 1), ("q2_322", "q2_322", 3), ("q1_377", "q1_373", 8), ("q1_373", "q1_377", 2),
                                                  ("q1_512", "q1_512", 1)])
def test_planes_move(stfem, src_mesh, dst_mesh, nb, number):
    cs, cd = context(src_mesh, number), context(dst_mesh, number, 1 if src_mesh == dst_mesh else 0)
    L = stfem.lib()
    (plane, nzs), (plane_d, nzd) = dims(src_mesh), dims(dst_mesh)
    assert plane == plane_d
    S = K.seeded_blocks(1, nb, cs.n_dofs, number)
    src, dst = stfem.BlockVector(cs, nb).upload(S), stfem.BlockVector(cd, nb)
    nzmin = min(nzs, nzd)
    for nplanes in sorted({1, 2, nzmin}):
        for add_mask in (0, 1, 2, 3):
            iz_src, iz_dst = nzs - nplanes, (nzd - nplanes) // 2
            D0 = pattern(nb, cd.n_dofs, number, add_mask)
            dst.upload(D0)
            assert L.stfem_planes_move(cs._h, src._h, iz_src, cd._h, dst._h, iz_dst, nplanes, add_mask, None) == 0
            want = K.planes_move(S, iz_src, D0, iz_dst, nplanes, add_mask, plane, number)
            assert same_bits(dst.download(), want), (nplanes, add_mask)
            assert same_bits(src.download(), S)


# ----------------------------------------------------------------------------------------------- argument errors
# Every refused call leaves every operand bitwise unchanged.  Foreign vectors come from a second context of the same mesh and
# precision, so that nothing is read out of range whatever a call does with them.

class Operands:
    def __init__(self, stfem, number, mesh="q2_322"):
        self.stfem, self.ctx, self.other = stfem, context(mesh, number), context(mesh, number, 1)
        self.n = self.ctx.n_dofs
        self.held = []

    def vec(self, nb, seed, ctx=None):
        host = K.seeded_blocks(seed, nb, self.n, self.ctx.number)
        v = self.stfem.BlockVector(ctx or self.ctx, nb).upload(host)
        self.held.append((v, host))
        return v

    def unchanged(self):
        return all(same_bits(v.download(), host) for v, host in self.held)


@pytest.mark.parametrize("number", NUMBERS)
def test_multi_dot_refuses(stfem, number):
    o = Operands(stfem, number)
    L, ctx = stfem.lib(), o.ctx
    vs = [o.vec(2, 10 + i) for i in range(12)]
    w = o.vec(2, 2)
    out = np.full(256, 5.0)
    po = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(handles, k=None, wv=w):
        arr = (C.c_void_p * max(len(handles), 1))(*handles)
        return L.stfem_multi_dot(ctx._h, len(handles) if k is None else k, arr, wv._h, 0, po, None)

    hs = [v._h for v in vs]
    assert call(hs, k=0) == INVALID
    assert call([hs[i % 12] for i in range(249)]) == INVALID
    assert call([hs[i % 12] for i in range(248)]) == 0
    out[:] = 5.0
    assert call(hs[:9] + [None] + hs[10:]) == INVALID
    assert call(hs[:9] + [o.vec(2, 30, o.other)._h] + hs[10:]) == INVALID
    assert call(hs[:9] + [o.vec(3, 31)._h] + hs[10:]) == INVALID
    w9, v9 = o.vec(9, 3), o.vec(9, 4)
    assert call([v9._h], wv=w9) == UNSUPPORTED
    assert (out == 5.0).all() and o.unchanged()


@pytest.mark.parametrize("number", NUMBERS)
def test_orthogonalize_refuses(stfem, number):
    o = Operands(stfem, number)
    L, ctx = stfem.lib(), o.ctx
    vs = [o.vec(2, 10 + i) for i in range(12)]
    w = o.vec(2, 2)
    h = np.full(256, 5.0)
    before, after = C.c_double(5.0), C.c_double(5.0)

    def call(handles, wv=w):
        arr = (C.c_void_p * len(handles))(*handles)
        return L.stfem_orthogonalize(ctx._h, len(handles), arr, wv._h, 0, h.ctypes.data_as(C.POINTER(C.c_double)), C.byref(before), C.byref(after), None)

    hs = [v._h for v in vs]
    assert call([hs[i % 12] for i in range(248)]) == INVALID
    assert call(hs[:9] + [o.vec(2, 30, o.other)._h] + hs[10:]) == INVALID
    assert call(hs[:9] + [o.vec(3, 31)._h] + hs[10:]) == INVALID
    assert call(hs[:9] + [None] + hs[10:]) == INVALID
    assert call(hs[:9] + [w._h] + hs[10:]) == ALIAS  # v[9] == w: refused before the first group of eight is projected out
    assert call([o.vec(9, 4)._h], wv=o.vec(9, 3)) == UNSUPPORTED
    assert (h == 5.0).all() and before.value == 5.0 and after.value == 5.0 and o.unchanged()


@pytest.mark.parametrize("number", NUMBERS)
def test_multi_axpy_refuses(stfem, number):
    o = Operands(stfem, number)
    ctx = o.ctx
    xs = [o.vec(2, 10 + i) for i in range(12)]
    y = o.vec(2, 2)
    coef = np.linspace(0.5, 1.5, 12)
    for bad in (y, o.vec(2, 30, o.other), o.vec(3, 31)):  # x[9] == y, foreign, another block count: y is unchanged
        assert status_of(stfem, lambda: stfem.multi_axpy(ctx, coef, xs[:9] + [bad] + xs[10:], y)) == INVALID
        assert o.unchanged()
    assert status_of(stfem, lambda: stfem.multi_axpy(ctx, coef[:1], [o.vec(9, 4)], o.vec(9, 3))) == UNSUPPORTED
    assert o.unchanged()


@pytest.mark.parametrize("number", NUMBERS)
def test_tensorproduct_add_refuses(stfem, number):
    o = Operands(stfem, number)
    ctx = o.ctx
    A = np.random.default_rng(1).uniform(0.5, 1.5, (3, 2))
    c, b = o.vec(3, 1), o.vec(2, 2)
    for cc, bb in ((o.vec(2, 3), b), (o.vec(4, 4), b), (c, o.vec(3, 5)), (c, o.vec(1, 6))):
        assert status_of(stfem, lambda: stfem.tensorproduct_add(ctx, cc, A, bb)) == SHAPE_MISMATCH
    assert status_of(stfem, lambda: stfem.tensorproduct_add(ctx, o.vec(3, 7, o.other), A, b)) == INVALID
    assert status_of(stfem, lambda: stfem.tensorproduct_add(ctx, c, A, o.vec(2, 8, o.other))) == INVALID
    assert o.unchanged()
    # c and b share a block in row 1 under a non-zero coefficient: refused before row 0 is updated; under a zero one: allowed
    shared = stfem.BlockVector(ctx, device_ptrs=[b.block_ptr(0), c.block_ptr(1)])
    assert status_of(stfem, lambda: stfem.tensorproduct_add(ctx, c, A, shared)) == ALIAS
    assert o.unchanged()
    A0 = A.copy()
    A0[1:, 1] = 0.0  # (row 2 neither: it would read block 1 of c after row 1 has updated it)
    stfem.tensorproduct_add(ctx, c, A0, shared)
    C0, B0 = o.held[0][1], o.held[1][1]
    want = K.tensorproduct_add(C0, A0, np.stack([B0[0], C0[1]]), number)
    assert (err_of(c.download(), want) <= tensor_bound(2, number, want.magnitude)).all()


@pytest.mark.parametrize("number", NUMBERS)
def test_dot_refuses(stfem, number):
    o = Operands(stfem, number)
    L, ctx = stfem.lib(), o.ctx
    a, b = o.vec(2, 1), o.vec(2, 2)
    out = C.c_double(5.0)
    for x, y in ((o.vec(2, 3, o.other), b), (a, o.vec(2, 4, o.other)), (a, o.vec(3, 5)), (o.vec(1, 6), b)):
        assert L.stfem_dot(ctx._h, x._h, y._h, 0, C.byref(out), None) == INVALID
    assert L.stfem_dot(ctx._h, None, b._h, 0, C.byref(out), None) == INVALID
    assert L.stfem_dot(ctx._h, a._h, b._h, 0, None, None) == INVALID
    assert out.value == 5.0 and o.unchanged()


@pytest.mark.parametrize("number", NUMBERS)
def test_planes_move_refuses(stfem, number):
    o = Operands(stfem, number, "q1_377")
    L, cs = stfem.lib(), o.ctx
    cd = context("q1_373", number)
    nzs, nzd = dims("q1_377")[1], dims("q1_373")[1]
    src = o.vec(2, 1)
    D0 = K.seeded_blocks(2, 2, cd.n_dofs, number)
    dst = stfem.BlockVector(cd, 2).upload(D0)

    def move(iz_src, iz_dst, nplanes, s=src, d=dst, csx=cs, cdx=cd):
        return L.stfem_planes_move(csx._h, s._h, iz_src, cdx._h, d._h, iz_dst, nplanes, 3, None)

    assert move(0, 0, 0) == INVALID
    assert move(nzs - 1, 0, 2) == INVALID and move(0, nzd - 1, 2) == INVALID  # past either end
    assert move(-1, 0, 1) == INVALID and move(0, -1, 1) == INVALID
    assert move(0, 0, 1, d=src) == INVALID  # a vector of the other context
    other_plane = context("q2_322", number)
    assert move(0, 0, 1, d=stfem.BlockVector(other_plane, 2), cdx=other_plane) == SHAPE_MISMATCH
    other_number = context("q1_373", "float" if number == "double" else "double")
    assert move(0, 0, 1, d=stfem.BlockVector(other_number, 2), cdx=other_number) == SHAPE_MISMATCH
    assert move(0, 0, 1, d=stfem.BlockVector(cd, 3)) == SHAPE_MISMATCH
    assert move(0, 0, 1, s=o.vec(9, 3), d=stfem.BlockVector(cd, 9)) == UNSUPPORTED
    assert move(0, 0, nzd) == 0  # (and the longest range that fits is taken)
    assert o.unchanged() and same_bits(dst.download(), K.planes_move(o.held[0][1], 0, D0, 0, nzd, 3, dims("q1_377")[0], number))
