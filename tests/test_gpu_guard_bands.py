"""Guard-band tests of the scalar side: every device entry point on packed caller-owned views.

include/stfem.h puts no condition on where a caller's device arrays lie.  Each case runs one call twice - on arrays in allocations
of their own, as the library hands them out (`plain`), and on views of one guarded arena (tests/guard_arena.py: `guard | view |
guard | ...`, every byte classified) - and asserts
  1. plain agrees with the CPU reference of the operation, within the bound the entry point's existing parity test uses;
  2. the arena result equals plain bit for bit (every kernel is bitwise reproducible and nothing documented makes a result depend
     on an address);
  3. all guards and all sources of the arena are bit-identical to before the call.
Placements: `aligned` (256-byte boundaries), `packed` (8 mod 16 for fp64, 4 mod 8 for fp32), for the Vanka and transfer cases also
`descending` (later blocks at lower addresses).  Destinations start as a poison NaN where the call overwrites and as seeded values
where it accumulates.  Shapes are the smallest with a ragged edge of the path in question; the diagnostics (last_kernel_name,
last_sweep_plan, last_tile_plan, MGTwoLevelTransfer.last_path, setup_batches) prove the path ran."""
import collections
import functools
import importlib

import numpy as np
import pytest

import transfer_line_reference as tlr
from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
NUMBERS = ["double", "float"]
TOL, TOL32 = 1e-12, 1e-5  # the operators' parity bounds (test_gpu_parity.py)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for knob in ("STFEM_TILE_LZ", "STFEM_VARIANT", "STFEM_EXP", "STFEM_VANKA_COLOURS", "STFEM_VANKA_HOST_SETUP"):
        monkeypatch.delenv(knob, raising=False)


def T(number):
    return np.float32 if number == "float" else np.float64


def f32(a):
    """values both precisions hold exactly: one reference serves a case's double and float run"""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def dims(ctx):
    return tuple(ctx.degree * n + 1 for n in ctx.ncell)


def sources(prefix, X, number, shape):
    return [Spec(f"{prefix}{b}", X[b].astype(T(number)), "source", shape) for b in range(len(X))]


def destinations(prefix, n_blocks, n, number, shape, seeded=None):
    """poison where the call overwrites, seeded values where it accumulates"""
    return [Spec(f"{prefix}{b}", poison(n, T(number)) if seeded is None else seeded[b].astype(T(number)), "destination", shape)
            for b in range(n_blocks)]


def view(stfem, ctx, ptr, prefix, n_blocks):
    return stfem.BlockVector(ctx, device_ptrs=[ptr[f"{prefix}{b}"] for b in range(n_blocks)])


def refs(prefix, Y, tol):
    return {f"{prefix}{b}": (Y[b], tol) for b in range(len(Y))}


def scaled_like(ref, seed=3):
    """D0 of an add: random, of the increment's size (test_gpu_tile_layers.py)"""
    return f32(np.random.default_rng(seed).uniform(-1, 1, ref.shape) * np.sqrt(np.mean(np.square(ref))))


# ------------------------------------------------------------------------------------------ the scalar operator

# time: (type, r, steps at once, tau); coef: None or "cell" (per-cell coefficients on K and M); path: the sweep both precisions run;
# tile_lz: STFEM_TILE_LZ when the context is created
Sweep = collections.namedtuple("Sweep", "degree cells lower upper mask time distort coef path tile_lz")
SWEEPS = {
    # pencil sweep (Cartesian meshes; test_gpu_parity.py CASES)
    "q1_9x7x5_1":      Sweep(1, (9, 7, 5), (0, 0, 0), (1, 1, 1), 63, ("DG", 0, 1, 0.2), 0.0, None, "pencil", None),
    "q2_4x4x3_12":     Sweep(2, (4, 4, 3), (0, 0, 0), (1, 1, 1), 63, ("CGP", 3, 4, 0.05), 0.0, None, "pencil", None),      # panels
    "q3_5x4x6_dg2":    Sweep(3, (5, 4, 6), (-1, -1, -1), (1, 1, 1), 63, ("DG", 2, 1, 1 / 64), 0.0, None, "pencil", None),
    "q4_7x3x2_4":      Sweep(4, (7, 3, 2), (0, 0, 0), (2, 1, 0.5), 0, ("CGP", 2, 2, 0.01), 0.0, None, "pencil", None),     # ragged in x, fewer rows than a tile
    "q4_13x5x9_3":     Sweep(4, (13, 5, 9), (0, 0, 0), (1, 1, 1), 63, ("DG", 2, 1, 0.02), 0.0, None, "pencil", None),      # two cell groups per wave
    "q4_5x9x3_8":      Sweep(4, (5, 9, 3), (0, 0, 0), (1, 1, 1), 63, ("CGP", 4, 2, 0.02), 0.0, None, "pencil", None),
    "q2_11x6x5_4_coef": Sweep(2, (11, 6, 5), (0, 0, 0), (1.0, 0.7, 1.3), 0b011011, ("CGP", 1, 4, 0.03), 0.0, "cell", "pencil", None),
    # tile sweep (perturbed meshes, test_gpu_parity.py GENERAL_CASES; degree 5, test_gpu_degree5.py)
    "pert_q4_7x6x5":   Sweep(4, (7, 6, 5), (0, 0, 0), (1, 1, 1), 63, ("CGP", 2, 1, 0.02), 0.15, None, "tile", None),
    "pert_q2_9x5x4_4": Sweep(2, (9, 5, 4), (0, 0, 0), (1, 1, 1), 0, ("CGP", 1, 4, 0.02), 0.15, None, "tile", None),
    "pert_q1_4x3x3":   Sweep(1, (4, 3, 3), (0, 0, 0), (1, 1, 1), 0b101010, ("DG", 1, 2, 0.02), 0.2, None, "tile", None),
    "q5_4x3x2":        Sweep(5, (4, 3, 2), (0, 0, 0), (1, 1, 1), 63, ("CGP", 2, 1, 0.03), 0.0, None, "tile", None),
    "q5_1x1x1":        Sweep(5, (1, 1, 1), (0, 0, 0), (1, 2, 3), 63, ("CGP", 1, 1, 0.03), 0.0, None, "tile", None),           # its smallest: a single cell
    "pert_q4_7x6x5_lz2": Sweep(4, (7, 6, 5), (0, 0, 0), (1, 1, 1), 63, ("CGP", 2, 1, 0.02), 0.15, None, "tile", 2),        # chunks of 2, 2 and 1 layers
}


def sweep_setup(stfem, name):
    s = SWEEPS[name]
    tt, r, ns, tau = s.time
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(stfem.CGP if tt == "CGP" else stfem.DG, r, tau, ns)
    verts = stfem.mesh_vertices(s.cells, s.lower, s.upper, s.distort, 5489) if s.distort else stfem.mesh_vertices(s.cells, s.lower, s.upper)
    cl = cm = None
    if s.coef == "cell":
        rng = np.random.default_rng(17)
        cl, cm = rng.uniform(0.5, 3.0, int(np.prod(s.cells))), rng.uniform(0.5, 2.0, int(np.prod(s.cells)))
    return s.degree, s.cells, s.mask, Alpha, Beta, verts, cl, cm


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """inputs and the oracle's results of one case, shared by its precisions, placements and operations (read-only)"""
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, mask, Alpha, Beta, verts, cl, cm = sweep_setup(stfem, name)
    orc = oracle.Oracle(p, nc, verts, mask)
    if cl is not None:
        orc.set_coefficient(1, np.repeat(cl, (p + 1) ** 3))
        orc.set_coefficient(0, np.repeat(cm, (p + 1) ** 3))
    n = int(np.prod([p * c + 1 for c in nc]))
    X = f32(np.stack([np.random.default_rng(1234 + b).uniform(-1, 1, n) for b in range(Alpha.shape[0])]))
    out = dict(X=X, Y=orc.st_vmult(Alpha, Beta, X), YT=orc.st_vmult(Alpha, Beta, X, transpose=True))
    for v in out.values():
        v.setflags(write=False)
    return out


def sweep_context(stfem, name, number, monkeypatch):
    p, nc, mask, Alpha, Beta, verts, cl, cm = sweep_setup(stfem, name)
    lz = SWEEPS[name].tile_lz
    if lz:
        monkeypatch.setenv("STFEM_TILE_LZ", str(lz))  # read when the context is created
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, dirichlet_mask=mask, number=number)
    monkeypatch.delenv("STFEM_TILE_LZ", raising=False)
    if cl is not None:
        ctx.evaluate_coefficient(cl, which=1)
        ctx.evaluate_coefficient(cm, which=0)
    return ctx, Alpha, Beta


def assert_sweep_path(ctx, name):
    """the sweep the case is named for ran, in either precision (the kernel is chosen by degree, block count and geometry)"""
    path, lz = SWEEPS[name].path, SWEEPS[name].tile_lz
    if path == "pencil":
        assert ctx.last_kernel_name.startswith("st_sweep_pencil"), ctx.last_kernel_name
        assert ctx.last_sweep_plan[0] > 0 and ctx.last_tile_plan == (0, 0, 0, 0)
    else:
        assert ctx.last_kernel_name.startswith("st_sweep_cart_tile"), ctx.last_kernel_name
        plan = ctx.last_tile_plan
        assert plan[0] > 0 and ctx.last_sweep_plan == (0, 0), plan
        if lz:
            ncz = SWEEPS[name].cells[2]
            assert plan[2] == -(-ncz // lz) and plan[3] == lz >= 2, plan  # a z-chunk marches several layers


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("op", ["vmult", "Tvmult", "vmult_add"])
@pytest.mark.parametrize("name", list(SWEEPS))
def test_st_vmult(name, op, number, placement, stfem, oracle_mod, monkeypatch):
    """stfem_st_vmult: the space-time operator, its transpose and its add form"""
    ref = sweep_reference(name)
    ctx, Alpha, Beta = sweep_context(stfem, name, number, monkeypatch)
    nb, n, shape = Alpha.shape[0], ctx.n_dofs, dims(ctx)
    A = stfem.SystemMatrix(ctx, Alpha, Beta)
    Y = ref["YT"] if op == "Tvmult" else ref["Y"]
    D0 = scaled_like(Y) if op == "vmult_add" else None
    specs = sources("src", ref["X"], number, shape) + destinations("dst", nb, n, number, shape, seeded=D0)

    def call(ptr):
        A._apply(view(stfem, ctx, ptr, "dst", nb), view(stfem, ctx, ptr, "src", nb), op == "Tvmult", op == "vmult_add", None)

    guard_case(stfem, placement, specs, call, refs("dst", Y if D0 is None else D0 + Y, TOL32 if number == "float" else TOL),
               check=lambda: assert_sweep_path(ctx, name))


@functools.lru_cache(maxsize=None)
def space_reference(name):
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, mask, _, _, verts, cl, cm = sweep_setup(stfem, name)
    orc = oracle.Oracle(p, nc, verts, mask)
    if cl is not None:
        orc.set_coefficient(1, np.repeat(cl, (p + 1) ** 3))
        orc.set_coefficient(0, np.repeat(cm, (p + 1) ** 3))
    X = sweep_reference(name)["X"][:1]
    one = np.ones((1, 1))
    out = dict(KX=orc.st_vmult(one, 0 * one, X), MX=orc.st_vmult(0 * one, one, X), dK=orc.diagonal(0.0, 1.0), dM=orc.diagonal(1.0, 0.0))
    for v in out.values():
        v.setflags(write=False)
    return out


SPACE = ["q1_9x7x5_1", "q4_7x3x2_4", "q2_11x6x5_4_coef", "pert_q1_4x3x3", "pert_q4_7x6x5"]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("name", SPACE)
def test_space_vmult(name, number, placement, stfem, oracle_mod, monkeypatch):
    """stfem_space_vmult: dst = (mass M + laplace K) src on one block"""
    X, sp = sweep_reference(name)["X"][:1], space_reference(name)
    ctx, _, _ = sweep_context(stfem, name, number, monkeypatch)
    ctx.mass_matrix_scaling, ctx.laplace_matrix_scaling = 0.75, 1.5
    specs = sources("src", X, number, dims(ctx)) + destinations("dst", 1, ctx.n_dofs, number, dims(ctx))

    def call(ptr):
        ctx.vmult(view(stfem, ctx, ptr, "dst", 1), view(stfem, ctx, ptr, "src", 1))

    ms, ls = (1.0, 1.0) if SWEEPS[name].coef else (0.75, 1.5)  # operators.h:1152-1162: a coefficient table replaces the scaling
    guard_case(stfem, placement, specs, call, refs("dst", ms * sp["MX"] + ls * sp["KX"], TOL32 if number == "float" else TOL))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("name", SPACE)
def test_diagonals(name, number, placement, stfem, oracle_mod, monkeypatch):
    """stfem_diagonal, stfem_diagonal_inverse, stfem_st_diagonal (plain and inverse) into arena views"""
    sp = space_reference(name)
    ctx, Alpha, Beta = sweep_context(stfem, name, number, monkeypatch)
    n, shape, L = ctx.n_dofs, dims(ctx), stfem.lib()
    tol, tol_inv = (TOL32, TOL32) if number == "float" else (TOL, 1e-11)  # test_gpu_diagonal.py
    guard = np.sqrt(np.finfo(T(number)).eps)

    def inv(d):  # operators.h:1106-1109: 1 / d where |d| > sqrt(eps) of the Number, 1 elsewhere (test_gpu_diagonal.py)
        return np.where(np.abs(d) > guard, 1.0 / np.where(d == 0, 1.0, d), 1.0)

    ms, ls = (1.0, 1.0) if SWEEPS[name].coef else (0.5, 2.0)  # operators.h:1152-1162: a coefficient table replaces the scaling
    combined = ms * sp["dM"] + ls * sp["dK"]
    # The branch of the inverse is the same on the device as in the reference: no entry lies next to the guard.  The closest of these
    # meshes is diag M of q2_11x6x5_4_coef in float, 5.3e-4 of the guard (3.45e-4) away from it, where fp32 rounding moves an
    # entry by 6e-8 of its size; in double everything is more than a hundred times the guard
    for d in (sp["dK"], sp["dM"], combined):
        assert np.min(np.abs(np.abs(d[d != 0]) - guard)) > 1e-4 * guard

    def diagonal(ptr):
        d = view(stfem, ctx, ptr, "d", 1)
        stfem._check(L.stfem_diagonal(ctx._h, 0.5, 2.0, d._h, None), "stfem_diagonal")

    def diagonal_inverse(ptr):
        d = view(stfem, ctx, ptr, "d", 1)
        stfem._check(L.stfem_diagonal_inverse(ctx._h, 0.5, 2.0, d._h, None), "stfem_diagonal_inverse")

    guard_case(stfem, placement, destinations("d", 1, n, number, shape), diagonal, {"d0": (combined, tol)})
    guard_case(stfem, placement, destinations("d", 1, n, number, shape), diagonal_inverse, {"d0": (inv(combined), tol_inv)})
    nb = Alpha.shape[0]
    A, B = np.ascontiguousarray(Alpha), np.ascontiguousarray(Beta)
    for inverse in (0, 1):
        def st_diagonal(ptr):
            d = view(stfem, ctx, ptr, "d", nb)
            stfem._check(L.stfem_st_diagonal(ctx._h, nb, stfem._p(A), stfem._p(B), inverse, d._h, None), "stfem_st_diagonal")
        want = [(inv(sp["dK"]) / A[i, i] + inv(sp["dM"]) / B[i, i]) if inverse else (A[i, i] * sp["dK"] + B[i, i] * sp["dM"]) for i in range(nb)]
        guard_case(stfem, placement, destinations("d", nb, n, number, shape), st_diagonal, refs("d", want, tol_inv if inverse else tol))


# ------------------------------------------------------------------------------------------ vector and plane kernels

# n = 343 and n = 3465, neither a multiple of 256: one and fourteen workgroups, a ragged last one
MESHES = {"n343": (2, (3, 3, 3)), "n3465": (2, (10, 7, 5))}


def vector_ctx(stfem, mesh, number):
    p, nc = MESHES[mesh]
    ctx = stfem.MatrixFreeOperator(p, nc, number=number)
    assert ctx.n_dofs == int(mesh[1:]) and ctx.n_dofs % 256 != 0
    return ctx


def blocks(rng, nb, n, number):
    return rng.uniform(-1, 1, (nb, n)).astype(T(number)).astype(np.float64)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_tensorproduct_add(mesh, number, placement, stfem):
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(1)
    A = np.array([[1.5, 0.0, -2.0], [0.0, 0.25, 1.0]])
    X, Y = blocks(rng, 3, n, number), blocks(rng, 2, n, number)
    specs = sources("b", X, number, shape) + destinations("c", 2, n, number, shape, seeded=Y)

    def call(ptr):
        stfem.tensorproduct_add(ctx, view(stfem, ctx, ptr, "c", 2), A, view(stfem, ctx, ptr, "b", 3))

    guard_case(stfem, placement, specs, call, refs("c", Y + A @ X, 1e-15 if number == "double" else 1e-6))  # test_blas1_and_planes


def own_inside_last_plane(ctx):
    nx, ny, nz = dims(ctx)
    return nx * ny * (nz - 1) + (nx * ny) // 2 + 1


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_dot_and_multi_dot(mesh, number, placement, stfem):
    """stfem_dot, stfem_multi_dot with n_own inside the last plane: the entries behind n_own are NaN, as are the guards"""
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(2)
    nb, k, own = 3, 11, own_inside_last_plane(ctx)
    V, W = [blocks(rng, nb, n, number) for _ in range(k)], blocks(rng, nb, n, number)
    want = np.array([np.sum(v[:, :own] * W[:, :own]) for v in V])
    for a in V + [W]:
        a[:, own:] = np.nan
    specs = [s for i, v in enumerate(V) for s in sources(f"v{i}_", v, number, shape)] + sources("w", W, number, shape)
    tol = 1e-13 if number == "double" else 1e-6  # test_gram_schmidt_step_on_the_device

    def call(ptr):
        vs = [view(stfem, ctx, ptr, f"v{i}_", nb) for i in range(k)]
        w = view(stfem, ctx, ptr, "w", nb)
        return np.concatenate([stfem.multi_dot(ctx, vs, w, n_own=own), [stfem.dot(ctx, vs[0], w, n_own=own)]])

    def returned(got):
        assert np.allclose(got[:k], want, rtol=tol, atol=tol * np.abs(want).max()), (got, want)
        assert got[k] == got[0]

    guard_case(stfem, placement, specs, call, {}, returned=returned)


@pytest.fixture(scope="module")
def one_rank():
    """a communicator of one rank (tests/test_gpu_comm.py): stfem_dot_global is then stfem_dot without a reduction"""
    dmod = importlib.import_module("dealii-stfem_amd.distributed")
    comm = dmod.Communicator(0, 1, 0, lambda raw: raw)
    yield comm
    comm.close()


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
def test_dot_global_on_one_rank(number, placement, stfem, one_rank):
    """stfem_dot_global reads the caller's blocks like stfem_dot: n_own inside the last plane, NaN behind it"""
    ctx = vector_ctx(stfem, "n3465", number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(13)
    nb, own = 2, own_inside_last_plane(ctx)
    V, W = blocks(rng, nb, n, number), blocks(rng, nb, n, number)
    want = np.sum(V[:, :own] * W[:, :own])
    V[:, own:], W[:, own:] = np.nan, np.nan

    def returned(got):
        assert abs(got - want) <= (1e-12 if number == "double" else 1e-5) * abs(want)  # test_self_loop_exchange

    guard_case(stfem, placement, sources("v", V, number, shape) + sources("w", W, number, shape),
               lambda ptr: one_rank.dot(ctx, view(stfem, ctx, ptr, "v", nb), view(stfem, ctx, ptr, "w", nb), own), {}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_multi_axpy(mesh, number, placement, stfem):
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(3)
    nb, k = 3, 11
    V, W, coef = [blocks(rng, nb, n, number) for _ in range(k)], blocks(rng, nb, n, number), rng.uniform(-1, 1, k)
    specs = [s for i, v in enumerate(V) for s in sources(f"v{i}_", v, number, shape)] + destinations("w", nb, n, number, shape, seeded=W)

    def call(ptr):
        stfem.multi_axpy(ctx, coef, [view(stfem, ctx, ptr, f"v{i}_", nb) for i in range(k)], view(stfem, ctx, ptr, "w", nb))

    guard_case(stfem, placement, specs, call, refs("w", W + sum(c * v for c, v in zip(coef, V)), 1e-14 if number == "double" else 1e-6))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_orthogonalize(mesh, number, placement, stfem):
    """stfem_orthogonalize: inner products over n_own inside the last plane, the update over the whole of w"""
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(4)
    nb, k, own = 3, 11, own_inside_last_plane(ctx)
    V, W = [blocks(rng, nb, n, number) for _ in range(k)], blocks(rng, nb, n, number)
    h = np.array([np.sum(v[:, :own] * W[:, :own]) for v in V])
    W1 = W - sum(c * v for c, v in zip(h, V))
    specs = [s for i, v in enumerate(V) for s in sources(f"v{i}_", v, number, shape)] + destinations("w", nb, n, number, shape, seeded=W)
    tol = 1e-13 if number == "double" else 1e-6  # test_gram_schmidt_step_on_the_device

    def call(ptr):
        hh, n2, b2 = stfem.orthogonalize(ctx, [view(stfem, ctx, ptr, f"v{i}_", nb) for i in range(k)], view(stfem, ctx, ptr, "w", nb), n_own=own)
        return np.concatenate([hh, [n2, b2]])

    def returned(got):
        assert np.allclose(got[:k], h, rtol=tol, atol=tol * np.abs(h).max())
        before, after = np.sum(W[:, :own] ** 2), np.sum(T(number)(W1).astype(np.float64)[:, :own] ** 2)
        assert abs(got[k + 1] - before) <= (1e-12 if number == "double" else 1e-5) * before
        assert abs(got[k] - after) <= (1e-12 if number == "double" else 1e-4) * after  # (w itself is only known to 2e-6 in fp32)

    guard_case(stfem, placement, specs, call, refs("w", W1, 1e-13 if number == "double" else 2e-6), returned=returned)


def within_one_ulp(a, x, b, y, number):
    """a x + b y with or without contraction to an fma: within one ulp, at the size of the terms, of the exact value
    (test_vector_axpby_and_set_zero)"""
    t = T(number)
    wide = np.float64 if number == "float" else np.longdouble
    ax, by = wide(t(a)) * x.astype(t).astype(wide), wide(t(b)) * y.astype(t).astype(wide)

    def check(got):
        assert np.all(np.abs(got.astype(wide) - (ax + by)) <= np.finfo(t).eps * (np.abs(ax) + np.abs(by)))
    return check


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_vector_axpby_and_set_zero(mesh, number, placement, stfem):
    """stfem_vector_axpby on nine blocks (two launches), its zero-factor forms on NaN, stfem_vector_set_zero"""
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(5)
    nb, a, b = 9, 1.7, -0.3
    X, Y = blocks(rng, nb, n, number), blocks(rng, nb, n, number)

    def axpby(fa, fb):
        return lambda ptr: stfem.vector_axpby(ctx, fa, view(stfem, ctx, ptr, "x", nb), fb, view(stfem, ctx, ptr, "y", nb))

    guard_case(stfem, placement, sources("x", X, number, shape) + destinations("y", nb, n, number, shape, seeded=Y), axpby(a, b),
               {f"y{j}": within_one_ulp(a, X[j], b, Y[j], number) for j in range(nb)})
    # b = 0: y's poison is not read
    guard_case(stfem, placement, sources("x", X, number, shape) + destinations("y", nb, n, number, shape), axpby(a, 0.0),
               {f"y{j}": within_one_ulp(a, X[j], 0.0, 0 * Y[j], number) for j in range(nb)})
    # a = 0: x, all NaN, is not read
    guard_case(stfem, placement, sources("x", np.full_like(X, np.nan), number, shape) + destinations("y", nb, n, number, shape, seeded=Y), axpby(0.0, b),
               {f"y{j}": within_one_ulp(0.0, 0 * X[j], b, Y[j], number) for j in range(nb)})
    guard_case(stfem, placement, destinations("y", nb, n, number, shape), lambda ptr: stfem.vector_set_zero(ctx, view(stfem, ctx, ptr, "y", nb)),
               refs("y", np.zeros((nb, n)), 1e-300))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
def test_axpby_many(number, placement, stfem):
    """stfem_axpby_many: one launch over views of different lengths, nine arrays (a second launch)"""
    ctx = vector_ctx(stfem, "n343", number)
    rng, a, b = np.random.default_rng(6), 1.7, -0.3
    lens = [343, 3465, 1, 257, 3 * 125, 256, 36, 1029, 2]
    X, Y = [blocks(rng, 1, ln, number)[0] for ln in lens], [blocks(rng, 1, ln, number)[0] for ln in lens]
    specs = [Spec(f"x{j}", x.astype(T(number))) for j, x in enumerate(X)] + [Spec(f"y{j}", y.astype(T(number)), "destination") for j, y in enumerate(Y)]

    def call(ptr):
        stfem.axpby_many(ctx, a, [(ptr[f"x{j}"], ln) for j, ln in enumerate(lens)], b, [(ptr[f"y{j}"], ln) for j, ln in enumerate(lens)])

    guard_case(stfem, placement, specs, call, {f"y{j}": within_one_ulp(a, X[j], b, Y[j], number) for j in range(len(lens))})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("direction", ["to_float", "to_double"])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_vector_convert(mesh, direction, placement, stfem):
    """stfem_vector_convert in both directions: fp64 and fp32 views in one arena"""
    cd, cf = vector_ctx(stfem, mesh, "double"), vector_ctx(stfem, mesh, "float")
    n, shape, nb = cd.n_dofs, dims(cd), 2
    X = np.random.default_rng(7).uniform(-1, 1, (nb, n))
    src_number, dst_number, cs, ct = ("double", "float", cd, cf) if direction == "to_float" else ("float", "double", cf, cd)
    specs = sources("s", X, src_number, shape) + destinations("d", nb, n, dst_number, shape)

    def call(ptr):
        stfem.vector_convert(view(stfem, ct, ptr, "d", nb), view(stfem, cs, ptr, "s", nb))

    def exact(j):
        return lambda got: np.testing.assert_array_equal(got.astype(np.float64), X[j].astype(np.float32).astype(np.float64))  # test_vector_convert

    guard_case(stfem, placement, specs, call, {f"d{j}": exact(j) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_plane_pack_unpack(mesh, number, placement, stfem):
    """stfem_plane_pack / stfem_plane_unpack (plane_copy_kernel) with the plane buffer itself an arena view; the last plane, where one
    element too many leaves the block"""
    ctx = vector_ctx(stfem, mesh, number)
    n, shape, L, rng = ctx.n_dofs, dims(ctx), stfem.lib(), np.random.default_rng(8)
    nb, plane, nz = 3, shape[0] * shape[1], shape[2]
    S, D0, B = blocks(rng, nb, n, number), blocks(rng, nb, n, number), blocks(rng, 1, nb * plane, number)
    same = lambda want: (lambda got: np.testing.assert_array_equal(got.astype(np.float64), want))  # noqa: E731  (copies, one rounding of a sum)
    for iz in (nz - 1, 0):
        def pack(ptr):
            s = view(stfem, ctx, ptr, "s", nb)
            stfem._check(L.stfem_plane_pack(ctx._h, s._h, iz, ptr["buf"], None), "stfem_plane_pack")
        guard_case(stfem, placement, sources("s", S, number, shape) + [Spec("buf", poison(nb * plane, T(number)), "destination", (shape[0], shape[1], nb))],
                   pack, {"buf": same(S[:, iz * plane:(iz + 1) * plane].ravel())})
        for add in (0, 1):
            def unpack(ptr):
                d = view(stfem, ctx, ptr, "d", nb)
                stfem._check(L.stfem_plane_unpack(ctx._h, d._h, iz, ptr["buf"], add, None), "stfem_plane_unpack")
            want = D0.copy()
            part = B.reshape(nb, plane)
            want[:, iz * plane:(iz + 1) * plane] = T(number)(want[:, iz * plane:(iz + 1) * plane] + part) if add else part
            guard_case(stfem, placement, [Spec("buf", B.astype(T(number)), "source", (shape[0], shape[1], nb))] + destinations("d", nb, n, number, shape, seeded=D0),
                       unpack, {f"d{j}": same(want[j]) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_planes_move(mesh, number, placement, stfem):
    """stfem_planes_move between contexts of different height: the last planes of the source onto the last planes of the destination,
    the first and the last plane added"""
    cs = vector_ctx(stfem, mesh, number)
    p, nc = MESHES[mesh]
    cd = stfem.MatrixFreeOperator(p, (nc[0], nc[1], nc[2] - 1), number=number)
    ss, sd, L, rng = dims(cs), dims(cd), stfem.lib(), np.random.default_rng(9)
    nb, plane, nplanes = 3, ss[0] * ss[1], 3
    S, D0 = blocks(rng, nb, cs.n_dofs, number), blocks(rng, nb, cd.n_dofs, number)
    for add_mask in (0, 3):
        def move(ptr):
            s, d = view(stfem, cs, ptr, "s", nb), view(stfem, cd, ptr, "d", nb)
            stfem._check(L.stfem_planes_move(cs._h, s._h, ss[2] - nplanes, cd._h, d._h, sd[2] - nplanes, nplanes, add_mask, None), "stfem_planes_move")
        want = D0.copy()
        for q in range(nplanes):
            src = S[:, (ss[2] - nplanes + q) * plane:(ss[2] - nplanes + q + 1) * plane]
            sl = slice((sd[2] - nplanes + q) * plane, (sd[2] - nplanes + q + 1) * plane)
            add = (q == 0 and add_mask & 1) or (q == nplanes - 1 and add_mask & 2)
            want[:, sl] = T(number)(want[:, sl] + src) if add else src
        guard_case(stfem, placement, sources("s", S, number, ss) + destinations("d", nb, cd.n_dofs, number, sd, seeded=D0), move,
                   {f"d{j}": (lambda got, j=j, want=want: np.testing.assert_array_equal(got.astype(np.float64), want[j])) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
def test_upload_download_rebind_on_views(number, placement, stfem):
    """stfem_vector_wrap / rebind / n_blocks / block / upload / download: a view's own copies stay inside its blocks"""
    ctx = vector_ctx(stfem, "n343", number)
    n, shape, L, nb = ctx.n_dofs, dims(ctx), stfem.lib(), 2
    X, Y = blocks(np.random.default_rng(10), nb, n, number), blocks(np.random.default_rng(11), nb, n, number)

    def call(ptr):
        v = view(stfem, ctx, ptr, "s", nb)
        assert L.stfem_vector_n_blocks(v._h) == nb and [v.block_ptr(b) for b in range(nb)] == [ptr[f"s{b}"] for b in range(nb)]
        got = v.download()
        v.rebind([ptr[f"d{b}"] for b in range(nb)])
        assert [v.block_ptr(b) for b in range(nb)] == [ptr[f"d{b}"] for b in range(nb)]
        v.upload(Y)
        return got.ravel()

    guard_case(stfem, placement, sources("s", X, number, shape) + destinations("d", nb, n, number, shape), call,
               {f"d{j}": (lambda got, j=j: np.testing.assert_array_equal(got.astype(np.float64), Y[j])) for j in range(nb)},
               returned=lambda got: np.testing.assert_array_equal(got, X.ravel()))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("number", NUMBERS)
def test_integrate_rhs_and_difference(number, placement, stfem):
    """stfem_integrate_rhs(_product) into one block of a three-block view, stfem_integrate_difference(_product) of one block of it: Q2
    on 7 x 3 x 2 perturbed cells, nq = 3 (test_gpu_driver_kernels.py)"""
    from oracle import driver_oracle as D
    p, nc, mask, nq = 2, (7, 3, 2), 0b100110, 3
    verts = stfem.mesh_vertices(nc, (0, 0, 0), (1, 1, 1), 0.15, 5489)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, dirichlet_mask=mask, number=number)
    n, shape, rng = ctx.n_dofs, dims(ctx), np.random.default_rng(12)
    f = rng.uniform(-1, 1, (ctx.n_cells, nq ** 3))
    U = blocks(rng, 3, n, number)
    tol = TOL32 if number == "float" else TOL

    def rhs(ptr):
        stfem.integrate_rhs(ctx, nq, f, stfem.BlockVector(ctx, device_ptrs=[ptr["a"], ptr["dst"], ptr["b"]]), block=1)

    load = D.load_vector(p, nc, verts, nq, f, mask)
    guard_case(stfem, placement, [Spec("a", U[0].astype(T(number)), "source", shape), Spec("dst", poison(n, T(number)), "destination", shape),
                                  Spec("b", U[2].astype(T(number)), "source", shape)], rhs, {"dst": (load, tol)})
    amplitude, frequency = -0.7, 2.5
    w = 2.0 * np.pi * frequency
    pts = stfem.quadrature_points(ctx, nq)
    s, c = np.sin(w * pts), np.cos(w * pts)
    val = amplitude * s[..., 0] * s[..., 1] * s[..., 2]
    grad = amplitude * w * np.stack([c[..., 0] * s[..., 1] * s[..., 2], s[..., 0] * c[..., 1] * s[..., 2], s[..., 0] * s[..., 1] * c[..., 2]], axis=-1)

    def rhs_product(ptr):
        stfem.integrate_rhs_product(ctx, nq, amplitude, frequency, stfem.BlockVector(ctx, device_ptrs=[ptr["a"], ptr["dst"], ptr["b"]]), block=1)

    guard_case(stfem, placement, [Spec("a", U[0].astype(T(number)), "source", shape), Spec("dst", poison(n, T(number)), "destination", shape),
                                  Spec("b", U[2].astype(T(number)), "source", shape)], rhs_product, {"dst": (D.load_vector(p, nc, verts, nq, val, mask), tol)})
    exact, egrad = rng.uniform(-1, 1, (ctx.n_cells, nq ** 3)), rng.uniform(-5, 5, (ctx.n_cells, nq ** 3, 3))

    def difference(ptr):
        u = view(stfem, ctx, ptr, "u", 3)
        return np.concatenate([stfem.integrate_difference(ctx, nq, u, 2, exact, egrad), stfem.integrate_difference_product(ctx, nq, u, 2, amplitude, frequency)])

    def returned(got):
        for g, r in ((got[:3], D.difference(p, nc, verts, nq, U[2], exact, egrad)), (got[3:], D.difference(p, nc, verts, nq, U[2], val, grad))):
            assert abs(g[0] - r[0]) <= 1e-12 * abs(r[0]) and abs(g[1] - r[1]) <= 1e-13 * abs(r[1]) and abs(g[2] - r[2]) <= 1e-12 * abs(r[2]), (g, r)

    guard_case(stfem, placement, sources("u", U, number, shape), difference, {}, returned=returned)


# ------------------------------------------------------------------------------------------ space transfers

# name: (fine degree, fine cells, coarse degree, coarse cells, mask, blocks, fused y-z prolongation (double, float), restriction marches)
TRANSFERS = {
    "h_q2":     (2, (4, 4, 4), 2, (2, 2, 2), 63, 3, (False, False), False),     # test_space_transfer_vs_oracle
    "p_q3_q1":  (3, (3, 2, 2), 1, (3, 2, 2), 63, 3, (False, False), False),
    "hp_q2_q1": (2, (4, 2, 2), 1, (2, 1, 1), 0, 3, (False, False), False),      # its smallest: 225 fine DoFs, no constraints
    # test_gpu_transfer_large.py's smallest: 160 867 y-z threads fuse, the restriction marches several coarse cells along z
    "p_q2_q1_large": (2, (33, 49, 49), 1, (33, 49, 49), 0, 1, (True, True), True),
}
TRANSFER_PLACEMENTS = [("h_q2", "aligned"), ("h_q2", "packed"), ("h_q2", "descending"), ("p_q3_q1", "aligned"), ("p_q3_q1", "packed"),
                       ("hp_q2_q1", "packed"), ("p_q2_q1_large", "aligned"), ("p_q2_q1_large", "packed")]
TRANSFER_OPS = ["prolongate", "prolongate_and_add", "restrict", "restrict_and_add", "interpolate"]
# (interpolate is checked against the dense matrix of the restatement: on the small shapes)
TRANSFER_CASES = [(n, pl, op) for n, pl in TRANSFER_PLACEMENTS for op in TRANSFER_OPS if not (op == "interpolate" and n.endswith("_large"))]


@functools.lru_cache(maxsize=2)
def transfer_reference(name):
    from oracle import stmg_oracle
    pf, ncf, pc, ncc, mask, nb = TRANSFERS[name][:6]
    F = tlr.line_factors(pf, ncf, mask, pc, ncc, mask)
    n_f, n_c = int(np.prod([f.shape[0] for f in F])), int(np.prod([f.shape[1] for f in F]))
    rng = np.random.default_rng(11)
    Uc, Uf = f32(rng.uniform(-1, 1, (nb, n_c))), f32(rng.uniform(-1, 1, (nb, n_f)))
    out = dict(Uc=Uc, Uf=Uf, PUc=tlr.prolongate(F, Uc), RUf=tlr.restrict(F, Uf))
    if n_f * n_c < 1 << 22:  # the dense interpolation matrix of the small shapes
        out["IUf"] = (stmg_oracle.space_interpolation(pf, ncf, mask, pc, ncc, mask) @ Uf.T).T
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("name,placement,op", TRANSFER_CASES)
def test_space_transfer(name, placement, op, number, stfem):
    """stfem_transfer_prolongate / restrict (overwrite and add) / interpolate"""
    pf, ncf, pc, ncc, mask, nb, fused, marches = TRANSFERS[name]
    ref = transfer_reference(name)
    tol = 1e-13 if number == "double" else 2e-6  # test_space_transfer_vs_oracle, test_gpu_transfer_large.py
    fine = stfem.MatrixFreeOperator(pf, ncf, dirichlet_mask=mask, number=number)
    coarse = stfem.MatrixFreeOperator(pc, ncc, dirichlet_mask=mask, number=number)
    Tr = stfem.MGTwoLevelTransfer(fine, coarse)
    up = op.startswith("prolongate")
    (cs, S), (cd, D0) = ((coarse, ref["Uc"]), (fine, ref["Uf"])) if up else ((fine, ref["Uf"]), (coarse, ref["Uc"]))
    result = ref["PUc"] if up else (ref["IUf"] if op == "interpolate" else ref["RUf"])
    add = op.endswith("_and_add")
    specs = sources("s", S, number, dims(cs)) + destinations("d", nb, cd.n_dofs, number, dims(cd), seeded=D0 if add else None)

    def call(ptr):
        getattr(Tr, op)(view(stfem, cd, ptr, "d", nb), view(stfem, cs, ptr, "s", nb))

    def check():
        path = Tr.last_path
        if up:
            assert path[0] == int(fused[number == "float"]), path
        elif op != "interpolate":
            assert (path[2] >= 2) == marches, path

    guard_case(stfem, placement, specs, call, refs("d", D0 + result if add else result, tol), check=check)


# ------------------------------------------------------------------------------------------ the cell-patch smoother

# name: (degree, cells, time type, r, mask, distortion, coefficient, one block per cell, bounds (double, float) of test_gpu_vanka.py)
VANKA = {
    "classes_q2":  (2, (3, 2, 3), 0, 2, 63, 0.0, None, False, (1e-10, 2e-4)),
    "cells_q2":    (2, (3, 2, 2), 0, 2, 63, 0.12, None, True, (1e-10, 5e-4)),
    "cells_q3":    (3, (3, 2, 3), 1, 1, 63 & ~12, 0.0, "cell", True, (1e-10, 5e-4)),  # test_vanka_per_cell_blocks_vs_oracle
}


def vanka_setup(stfem, name, number):
    p, nc, ttype, r, mask, distort, coef, per_cell, _ = VANKA[name]
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(ttype, r, 0.05, 1)
    verts = stfem.mesh_vertices(nc, distort=distort, seed=11)
    cc = np.random.default_rng(2).choice([1.0, 9.0, 16.0], int(np.prod(nc))) if coef == "cell" else None
    return p, nc, mask, Alpha, Beta, verts, cc


@functools.lru_cache(maxsize=None)
def vanka_reference(name):
    from oracle import vanka_oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, mask, Alpha, Beta, verts, cc = vanka_setup(stfem, name, "double")
    orc = vanka_oracle.VankaOracle(p, nc, verts, mask, Alpha, Beta, coef_lap=None if cc is None else np.repeat(cc, (p + 1) ** 3))
    n = int(np.prod([p * c + 1 for c in nc]))
    rng = np.random.default_rng(7)
    X, D0 = f32(rng.uniform(-1, 1, (Alpha.shape[0], n))), f32(rng.uniform(-1, 1, (Alpha.shape[0], n)))
    out = dict(X=X, D0=D0, Y=orc.vmult(X))
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("placement", ["aligned", "packed", "descending"])
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("scheme", ["two-phase", "colours"])
@pytest.mark.parametrize("name", list(VANKA))
def test_vanka(name, scheme, number, placement, stfem, monkeypatch):
    """stfem_vanka_vmult and stfem_vanka_step (overwriting and accumulating), class blocks and one block per cell, both apply schemes"""
    if scheme == "colours":
        monkeypatch.setenv("STFEM_VANKA_COLOURS", "1")  # read when the smoother is created
    p, nc, mask, Alpha, Beta, verts, cc = vanka_setup(stfem, name, number)
    per_cell, tol = VANKA[name][7], VANKA[name][8][number == "float"]
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts if VANKA[name][5] else None, dirichlet_mask=mask, number=number)
    if cc is not None:
        ctx.evaluate_coefficient(cc, which=1)
    V = stfem.PreconditionVanka(ctx, Alpha, Beta)
    ncells = int(np.prod(nc))
    assert V.n_classes == (ncells if per_cell else int(np.prod([min(c, 3) for c in nc])))
    assert (V.setup_batches > 0) == per_cell  # the device set-up of the per-cell blocks ran
    ref = vanka_reference(name)
    nb, n, shape = Alpha.shape[0], ctx.n_dofs, dims(ctx)
    src = sources("s", ref["X"], number, shape)

    def args(ptr):
        return view(stfem, ctx, ptr, "d", nb), view(stfem, ctx, ptr, "s", nb)

    guard_case(stfem, placement, src + destinations("d", nb, n, number, shape), lambda ptr: V.vmult(*args(ptr)), refs("d", ref["Y"], tol))
    guard_case(stfem, placement, src + destinations("d", nb, n, number, shape), lambda ptr: V.step(args(ptr)[0], 0.7, False, args(ptr)[1]),
               refs("d", 0.7 * ref["Y"], tol))
    guard_case(stfem, placement, src + destinations("d", nb, n, number, shape, seeded=ref["D0"]),
               lambda ptr: V.step(args(ptr)[0], 0.7, True, args(ptr)[1]), refs("d", ref["D0"] + 0.7 * ref["Y"], tol))
