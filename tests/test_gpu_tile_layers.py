"""The tile sweep (csrc/stfem_tile.hip: st_sweep_cart_tile + st_tile_fixup) marching through several cell layers per z-chunk.
The planner (plan_chunks, csrc/stfem_capi.hip) gives every mesh of the other exact tests one layer per chunk, so nothing of the
march ran under an exact check: the top DoF plane carried to the next layer in LDS, the next layer's source planes fetched
during the store phase, x-slabs and y-halo addressed by plane within the chunk, plane k = P stored on the last layer only,
metric records and per-cell coefficients indexed by cz0 + layer, and the fix-up's top_below with chunks of unequal length.
Here every case runs with two or more layers per chunk, asserted through MatrixFreeOperator.last_tile_plan (so a changed
planner or switch fails the test instead of emptying it), against the CPU oracle: 1e-12 (fp64) / 1e-5 (fp32) rel-L2, the
bounds of test_gpu_parity.py and test_gpu_degree5.py - the number of terms per entry does not grow with the layers.

Forced cases: STFEM_TILE_LZ=<n> (read once per context) caps the layers per chunk on small meshes.  ncz = 5 gives chunks of
(1, 2, 2), (2, 3) and (5,) layers for n = 2, 3, 5; ncz = 7 gives (2, 2, 3) for n = 3.  Every mesh has three or more x-tiles
(both colours; an even tile with odd neighbours on both sides), two or more y-tiles with a ragged last row, and a full
interior tile (the straight-line store phase); one_chunk_no_fixup has one y-tile and one chunk, so no fix-up launch.

Natural cases: no switch; meshes with twice as many (tile column, layer) pairs of the larger colour (10 x 103) as the planner
has slots (256 CUs x max(2, resident workgroups); STFEM_DEBUG_OCC=1 reports one resident workgroup per CU for the general
FE_Q(4) two-block kernel and two for the FE_Q(2) one: 512 slots), so plan_chunks itself chooses 35 chunks of two or three
layers - with three, a layer both receives and hands on a carried plane; up to 1024 slots it would still choose two.  ncz is
prime: the chunks are of unequal length whatever their number.  The cost is the oracle, on eight threads: 0.4 s for an apply on the FE_Q(4) mesh (22 763 cells;
1.4 s with its set-up), 0.1 s on the FE_Q(2) mesh (36 771 cells); two applies per mesh."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL, TOL32 = 1e-12, 1e-5
UPPER = (1.0, 0.7, 1.3)
ROWS = 4  # cell rows of a tile

# cells per wave = cells per tile row: (degree, blocks of the launch) -> tile_cells_per_wave (csrc/stfem_tile.hip)
TILE_WIDTH = {(4, 2): 6, (2, 4): 5, (3, 3): 5, (1, 6): 5, (5, 1): 10, (5, 2): 5, (5, 4): 2, (5, 8): 1, (2, 2): 10}

# name: (degree, cells, distort (0: the box UPPER, given as vertices), time type, r, steps at once, Dirichlet mask,
#        coefficients on K and M (None, "q": per quadrature point, "cell": per cell), blocks of the last launch, STFEM_TILE_LZ values)
CASES = {
    "gen_q4_2":           (4, (14, 6, 5), 0.15, "CGP", 2, 1, 63, None, 2, (2, 3, 5)),
    "gen_q2_4":           (2, (12, 7, 7), 0.15, "CGP", 1, 4, 0, None, 4, (3,)),
    "gen_q3_3":           (3, (12, 6, 5), 0.1, "DG", 2, 1, 0b101010, None, 3, (2,)),
    "gen_q1_6":           (1, (12, 9, 7), 0.2, "DG", 1, 3, 0b010101, None, 6, (3,)),
    "gen_q5_2":           (5, (12, 6, 5), 0.12, "CGP", 2, 1, 63, None, 2, (2, 5)),
    "perq_q2_2":          (2, (23, 6, 5), 0.0, "CGP", 2, 1, 0b011011, "q", 2, (2,)),
    "cart_q5_1":          (5, (23, 6, 5), 0.0, "DG", 0, 1, 0b011011, None, 1, (2, 5)),
    "cart_q5_4_coef":     (5, (5, 6, 5), 0.0, "DG", 1, 2, 63, "cell", 4, (3,)),
    # twelve blocks: panels of 8 + 4 (later column panels add); the last launch is the 4 x 4 panel, two cells wide
    "cart_q5_12":         (5, (3, 6, 5), 0.0, "CGP", 3, 4, 63, None, 4, (2,)),
    "one_chunk_no_fixup": (4, (14, 4, 5), 0.15, "CGP", 2, 1, 0b110011, None, 2, (5,)),
}
FORCED = [(name, lz) for name, c in CASES.items() for lz in c[9]]
FP32 = [(name, lz) for name, lz in FORCED if name in ("gen_q4_2", "gen_q5_2", "cart_q5_1", "cart_q5_4_coef")]

# perturbed meshes, two blocks (cG(2)); no switch set
NATURAL = {
    "q4_cg2": (4, (13, 17, 103), 0.15, "CGP", 2, 1, 0b100111, None, 2, ()),  # the element of BASELINE's perturbed hypercube
    "q2_cg2": (2, (21, 17, 103), 0.15, "CGP", 2, 1, 0b011011, None, 2, ()),
}


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for knob in ("STFEM_TILE_LZ", "STFEM_VARIANT", "STFEM_EXP"):
        monkeypatch.delenv(knob, raising=False)


def _case(name):
    return CASES[name] if name in CASES else NATURAL[name]


def _setup(stfem, name):
    p, nc, distort, tt, r, ns, mask, coef, _, _ = _case(name)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(stfem.CGP if tt == "CGP" else stfem.DG, r, 0.02, ns)
    verts = stfem.mesh_vertices(nc, (0, 0, 0), (1, 1, 1), distort, 5489) if distort else stfem.mesh_vertices(nc, (0, 0, 0), UPPER)
    rng = np.random.default_rng(17)
    ncells = int(np.prod(nc))
    cl = cm = None
    if coef == "q":
        cl, cm = rng.uniform(0.5, 3.0, (ncells, (p + 1) ** 3)), rng.uniform(0.5, 2.0, (ncells, (p + 1) ** 3))
    elif coef == "cell":
        cl, cm = rng.uniform(0.5, 3.0, ncells), rng.uniform(0.5, 2.0, ncells)
    X = rng.uniform(-1, 1, (Alpha.shape[0], int(np.prod([p * c + 1 for c in nc]))))
    return p, nc, mask, Alpha, Beta, verts, cl, cm, X


def _oracle_apply(name, transpose, leading=None):
    from oracle import oracle  # (built, and its thread count set, by the oracle_mod fixture the tests ask for)
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, mask, Alpha, Beta, verts, cl, cm, X = _setup(stfem, name)
    orc = oracle.Oracle(p, nc, verts, mask)
    if cl is not None:
        per_q = cl.ndim == 2
        orc.set_coefficient(1, cl if per_q else np.repeat(cl, (p + 1) ** 3))
        orc.set_coefficient(0, cm if per_q else np.repeat(cm, (p + 1) ** 3))
    n = leading or Alpha.shape[0]
    Y = orc.st_vmult(Alpha[:n, :n], Beta[:n, :n], X[:n], transpose=transpose)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=6)
def _reference(name, transpose, leading=None):
    """the oracle's result, shared by the tests of a case (read-only); it does not depend on STFEM_TILE_LZ"""
    return _oracle_apply(name, transpose, leading)


def _context(stfem, name, number, lz, monkeypatch):
    """the switch is read when the context is created"""
    if lz:
        monkeypatch.setenv("STFEM_TILE_LZ", str(lz))
    p, nc, mask, Alpha, Beta, verts, cl, cm, X = _setup(stfem, name)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, dirichlet_mask=mask, number=number)
    monkeypatch.delenv("STFEM_TILE_LZ", raising=False)
    if cl is not None:
        ctx.evaluate_coefficient(cl, which=1)
        ctx.evaluate_coefficient(cm, which=0)
    return ctx, Alpha, Beta, X


def _constrained(name):
    """the DoFs of the faces in the Dirichlet mask (bits: x lower, x upper, y lower, y upper, z lower, z upper)"""
    p, nc, mask = _case(name)[0], _case(name)[1], _case(name)[6]
    c = np.zeros([p * n + 1 for n in nc[::-1]], dtype=bool)  # [z][y][x]
    for bit, index in enumerate([(..., 0), (..., -1), (slice(None), 0), (slice(None), -1), (0,), (-1,)]):
        if mask >> bit & 1:
            c[index] = True
    return c.ravel()


def _run(stfem, ctx, Alpha, Beta, X, transpose=False, add_to=None):
    n = Alpha.shape[0]
    src = stfem.BlockVector(ctx, n).upload(X)
    dst = stfem.BlockVector(ctx, n).upload(np.full(X.shape, np.nan) if add_to is None else add_to)  # every DoF is stored unless add
    stfem.SystemMatrix(ctx, Alpha, Beta)._apply(dst, src, transpose, add_to is not None, None)
    assert ctx.last_kernel_name.startswith("st_sweep_cart_tile"), ctx.last_kernel_name
    assert ctx.last_sweep_plan == (0, 0)
    return dst.download()


def _random_destination(ref, number="double"):
    """D0 of an add: random, of the increment's size (the stored D0 + increment is rounded once more, eps |D0 + increment|
    per entry; with |D0| ~ 1 and increments of 1e-2 that rounding alone would be a third of the fp32 bound)"""
    D0 = np.random.default_rng(3).uniform(-1, 1, ref.shape) * np.sqrt(np.mean(np.square(ref)))
    return D0.astype(np.float32).astype(np.float64) if number == "float" else D0


def _chunks(ncz, ntc):
    return tuple((c + 1) * ncz // ntc - c * ncz // ntc for c in range(ntc))


def _assert_forced_plan(name, lz_switch, plan, blocks, what):
    """the plan the case is named for: ntc = ceil(ncz / STFEM_TILE_LZ) chunks, the longest of lz = ceil(ncz / ntc) >= 2 layers"""
    p, nc = CASES[name][0], CASES[name][1]
    ntx, nty, ntc, lz = plan
    print(f"{what}: plan (ntx, nty, ntc, lz) = {plan}, chunks {_chunks(nc[2], ntc) if ntc > 0 else ()}")
    cw = TILE_WIDTH[(p, blocks)]
    assert ntc == -(-nc[2] // lz_switch) and lz == -(-nc[2] // ntc) and lz >= 2, plan
    assert ntx == -(-nc[0] // cw) and nty == -(-nc[1] // ROWS), plan
    if name == "one_chunk_no_fixup":
        assert nty == 1 and ntc == 1, plan  # the condition of the fix-up launch
    else:
        assert nty >= 2 and nc[1] % ROWS != 0 and nc[1] > ROWS, plan  # a full and a ragged tile row
    if name != "cart_q5_12":  # (its last launch, the 4 x 4 panel: two tiles; the 8 x 8 panel is checked on its own)
        assert ntx >= 3 and nc[0] >= cw, plan
    return plan


def _check(got, ref, zero_rows, tol, what, base=None):
    """finite everywhere, the constrained rows exactly zero (untouched by an add), within tol of the oracle"""
    assert np.all(np.isfinite(got)), f"{what}: {np.count_nonzero(~np.isfinite(got))} entries not finite"
    if base is None:
        assert np.all(got[:, zero_rows] == 0), what
    else:
        assert np.array_equal(got[:, zero_rows], base[:, zero_rows]), what
    err = rel(got if base is None else got - base, ref)
    print(f"{what}: rel-L2 {err:.3e}")
    assert err < tol, (what, err)


def _all_checks(stfem, name, lz, monkeypatch, plan_assert):
    """vmult into NaN (and a second one, bitwise equal: the summation order is fixed, the carried plane included), Tvmult, add"""
    ctx, Alpha, Beta, X = _context(stfem, name, "double", lz, monkeypatch)
    rows = _constrained(name)
    tag = f"{name} lz={lz or 'planned'}"
    got = _run(stfem, ctx, Alpha, Beta, X)
    plan_assert(ctx.last_tile_plan, tag)
    _check(got, _reference(name, False), rows, TOL, tag + " vmult")
    again = _run(stfem, ctx, Alpha, Beta, X)
    assert np.array_equal(again, got), tag
    _check(_run(stfem, ctx, Alpha, Beta, X, transpose=True), _reference(name, True), rows, TOL, tag + " Tvmult")
    plan_assert(ctx.last_tile_plan, tag + " Tvmult")
    D0 = _random_destination(_reference(name, False))
    _check(_run(stfem, ctx, Alpha, Beta, X, add_to=D0), _reference(name, False), rows, TOL, tag + " add", base=D0)
    plan_assert(ctx.last_tile_plan, tag + " add")
    return ctx, Alpha, Beta, X


@pytest.mark.parametrize("name,lz", FORCED, ids=[f"{n}-lz{z}" for n, z in FORCED])
def test_forced_layers(name, lz, stfem, oracle_mod, monkeypatch):
    blocks = CASES[name][8]
    ctx, Alpha, Beta, X = _all_checks(stfem, name, lz, monkeypatch, lambda plan, what: _assert_forced_plan(name, lz, plan, blocks, what))
    if name == "cart_q5_12":  # the launches of eight blocks are one cell wide: the leading 8 x 8 system alone shows their plan
        got = _run(stfem, ctx, Alpha[:8, :8], Beta[:8, :8], X[:8])
        plan = _assert_forced_plan(name, lz, ctx.last_tile_plan, 8, name + " leading 8 x 8")
        assert plan[0] >= 3, plan
        _check(got, _reference(name, False, 8), _constrained(name), TOL, f"{name} lz={lz} leading 8 x 8 vmult")


@pytest.mark.parametrize("name,lz", FP32, ids=[f"{n}-lz{z}" for n, z in FP32])
def test_forced_layers_fp32(name, lz, stfem, oracle_mod, monkeypatch):
    """the fp32 build has other waves-per-SIMD variants (and FE_Q(5) its own): vmult and add"""
    ctx, Alpha, Beta, X = _context(stfem, name, "float", lz, monkeypatch)
    rows, blocks = _constrained(name), CASES[name][8]
    X32 = X.astype(np.float32).astype(np.float64)  # what the device holds
    ref = _reference(name, False)
    got = _run(stfem, ctx, Alpha, Beta, X32)
    _assert_forced_plan(name, lz, ctx.last_tile_plan, blocks, f"{name} lz={lz} fp32")
    _check(got, ref, rows, TOL32, f"{name} lz={lz} fp32 vmult")
    D0 = _random_destination(ref, "float")
    got = _run(stfem, ctx, Alpha, Beta, X32, add_to=D0)
    _assert_forced_plan(name, lz, ctx.last_tile_plan, blocks, f"{name} lz={lz} fp32 add")
    _check(got, ref, rows, TOL32, f"{name} lz={lz} fp32 add", base=D0)


@pytest.mark.parametrize("name", list(NATURAL))
def test_planned_layers(name, stfem, oracle_mod, monkeypatch):
    """the chunking plan_chunks chooses on this device: several layers per chunk, chunks of unequal length"""
    p, nc = NATURAL[name][0], NATURAL[name][1]
    cw = TILE_WIDTH[(p, 2)]
    assert nc[0] % cw and nc[1] % ROWS

    def plan_assert(plan, what):
        ntx, nty, ntc, lz = plan
        print(f"{what}: plan (ntx, nty, ntc, lz) = {plan}, chunk lengths {sorted(set(_chunks(nc[2], ntc))) if ntc > 0 else ()}")
        assert ntx == -(-nc[0] // cw) >= 3 and nty == -(-nc[1] // ROWS) >= 2, plan
        assert lz >= 2 and lz == -(-nc[2] // ntc) and nc[2] % ntc != 0, plan

    _all_checks(stfem, name, 0, monkeypatch, plan_assert)
    _reference.cache_clear()  # (the two largest references of the file)


def test_no_tile_plan_after_a_pencil_launch(stfem):
    """an axis-aligned FE_Q(2) context runs the pencil sweep: it reports a sweep plan and no tile plan"""
    nc = (5, 4, 3)
    ctx = stfem.MatrixFreeOperator(2, nc, dirichlet_mask=63)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(stfem.CGP, 2, 0.02, 1)
    X = np.random.default_rng(1).uniform(-1, 1, (2, ctx.n_dofs))
    dst = stfem.BlockVector(ctx, 2)
    assert ctx.last_tile_plan == (0, 0, 0, 0)  # nothing launched yet
    stfem.SystemMatrix(ctx, Alpha, Beta).vmult(dst, stfem.BlockVector(ctx, 2).upload(X))
    assert ctx.last_kernel_name.startswith("st_sweep_pencil"), ctx.last_kernel_name
    assert ctx.last_sweep_plan[0] > 0 and ctx.last_tile_plan == (0, 0, 0, 0)
