"""The pencil sweep (csrc/stfem_pencil.hip: st_sweep_pencil) with more tiles than resident workgroups.  The kernel is persistent:
2 x n_cu workgroups (512 on MI355X) pull tiles from per-XCD counters until none is left.  The exact tests elsewhere have tens of
tiles, so a workgroup takes at most one; here every mesh has at least 1.5 x as many tiles as workgroups (asserted through
MatrixFreeOperator.last_sweep_plan, so a changed plan fails the test instead of emptying it), and the second and later passes of
the tile loop - mailbox and prod / cons reuse, the weight table written once before the loop, tiles taken from another XCD's
counter - run under an exact check against the CPU oracle: 1e-12 (fp64) / 1e-5 (fp32) rel-L2, the bounds of test_gpu_parity.py.

Meshes: the fewest cells that give 770 ... 1150 tiles for the instantiation; no extent divides evenly into pencils (cells per
wave - 1 in x), tile rows (4 or 8 or 16 cells in y) or z-chunks; anisotropic boxes, Dirichlet masks with open faces."""
import functools
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL, TOL32 = 1e-12, 1e-5
UPPER = (1.0, 0.7, 1.3)

# name: (degree, cells, time type, r, steps at once, Dirichlet mask, per-cell coefficients on K and M)
CASES = {
    "q4_1block":  (4, (111, 105, 10), "DG", 0, 1, 0b011011, False),   # 12 cells per wave: 11 x 14 x 5 = 770 tiles
    "q4_2blocks": (4, (56, 81, 14), "CGP", 2, 1, 0b100110, False),    # 12 x 11 x 6 = 792
    "q4_3blocks": (4, (37, 41, 30), "DG", 2, 1, 0b011011, False),     # one cell row per pencil: 13 x 11 x 8 = 1144
    "q3_4blocks": (3, (45, 49, 30), "CGP", 1, 4, 0b110110, False),    # streamed middle phase: 15 x 7 x 8 = 840
    "q2_6blocks": (2, (41, 47, 33), "DG", 1, 3, 0b011011, True),      # LDS weight table, coefficient tables: 21 x 6 x 8 = 1008
}


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _setup(stfem, name):
    p, nc, tt, r, ns, mask, coef = CASES[name]
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(stfem.CGP if tt == "CGP" else stfem.DG, r, 0.02, ns)
    verts = stfem.mesh_vertices(nc, (0, 0, 0), UPPER)
    rng = np.random.default_rng(17)
    ncells = int(np.prod(nc))
    cl, cm = (rng.uniform(0.5, 3.0, ncells), rng.uniform(0.5, 2.0, ncells)) if coef else (None, None)
    X = rng.uniform(-1, 1, (Alpha.shape[0], int(np.prod([p * c + 1 for c in nc]))))
    return p, nc, mask, Alpha, Beta, verts, cl, cm, X


@functools.lru_cache(maxsize=2)
def _reference(name, transpose):
    """the oracle's result, shared by the tests of a case (read-only)"""
    from oracle import oracle  # (built, and its thread count set, by the oracle_mod fixture the tests ask for)
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, mask, Alpha, Beta, verts, cl, cm, X = _setup(stfem, name)
    orc = oracle.Oracle(p, nc, verts, mask)
    if cl is not None:
        orc.set_coefficient(1, np.repeat(cl, (p + 1) ** 3))
        orc.set_coefficient(0, np.repeat(cm, (p + 1) ** 3))
    Y = orc.st_vmult(Alpha, Beta, X, transpose=transpose)
    Y.setflags(write=False)
    return Y


def _context(stfem, name, number):
    p, nc, mask, Alpha, Beta, verts, cl, cm, X = _setup(stfem, name)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, dirichlet_mask=mask, number=number)
    if cl is not None:
        ctx.evaluate_coefficient(cl, which=1)
        ctx.evaluate_coefficient(cm, which=0)
    return ctx, Alpha, Beta, X


def _assert_many_tiles(plan, what):
    tiles, workgroups = plan
    print(f"{what}: {tiles} tiles on {workgroups} workgroups")
    assert workgroups > 0 and tiles >= 1.5 * workgroups, plan


def _run(stfem, ctx, Alpha, Beta, X, transpose=False, add_to=None):
    n = Alpha.shape[0]
    src = stfem.BlockVector(ctx, n).upload(X)
    dst = stfem.BlockVector(ctx, n).upload(np.full(X.shape, np.nan) if add_to is None else add_to)  # overwritten unless add
    stfem.SystemMatrix(ctx, Alpha, Beta)._apply(dst, src, transpose, add_to is not None, None)
    if not os.environ.get("STFEM_VARIANT"):
        assert ctx.last_kernel_name.startswith("st_sweep_pencil"), ctx.last_kernel_name
    return dst.download()


@pytest.mark.parametrize("transpose", [False, True], ids=["vmult", "Tvmult"])
@pytest.mark.parametrize("name", list(CASES))
def test_several_tiles_per_workgroup(name, transpose, stfem, oracle_mod):
    ctx, Alpha, Beta, X = _context(stfem, name, "double")
    got = _run(stfem, ctx, Alpha, Beta, X, transpose)
    _assert_many_tiles(ctx.last_sweep_plan, name)
    err = rel(got, _reference(name, transpose))
    print(f"{name} {'Tvmult' if transpose else 'vmult'}: rel-L2 {err:.3e}")
    assert err < TOL
    again = _run(stfem, ctx, Alpha, Beta, X, transpose)  # the tile counters were reset; which workgroup takes a tile does not matter
    assert np.array_equal(again, got)


def test_add_with_cell_coefficients(stfem, oracle_mod):
    """dst += A src (ADD and COEF instantiation, six blocks)"""
    name = "q2_6blocks"
    ctx, Alpha, Beta, X = _context(stfem, name, "double")
    ref = _reference(name, False)
    D0 = np.random.default_rng(3).uniform(-1, 1, ref.shape)
    got = _run(stfem, ctx, Alpha, Beta, X, add_to=D0)
    _assert_many_tiles(ctx.last_sweep_plan, name + " add")
    err = rel(got - D0, ref)
    print(f"{name} add: rel-L2 of the increment {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("name", ["q2_6blocks", "q4_3blocks"])
def test_fp32_several_tiles_per_workgroup(name, stfem, oracle_mod):
    ctx, Alpha, Beta, X = _context(stfem, name, "float")
    got = _run(stfem, ctx, Alpha, Beta, X)
    _assert_many_tiles(ctx.last_sweep_plan, name + " fp32")
    err = rel(got, _reference(name, False))
    print(f"{name} fp32 vmult: rel-L2 {err:.3e}")
    assert err < TOL32


def test_stokes_gradient_sweep_several_tiles_per_workgroup(stfem, oracle_mod):
    """the GRAD instantiation (three FE_Q(2) components as blocks, - B^T p added to what the sweep stores): one source, one
    overwritten velocity destination, FE_Q(1) pressure on an axis-aligned mesh; 12 x 17 x 4 = 816 tiles; against
    oracle/stfem_oracle_stokes.c (1.4 s for its apply on eight threads)"""
    oracle = oracle_mod
    nc, upper, mask, nu = (67, 257, 5), (1.0, 2.0, 0.25), 0b111011, 0.7
    orc = oracle.StokesOracle(nc, stfem.mesh_vertices(nc, (0, 0, 0), upper), mask, nu)
    rng = np.random.default_rng(21)
    U, Pp = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, Pp)
    op = stfem.StokesMatrixFreeOperator(nc, upper=upper, dirichlet_mask=mask, viscosity=nu)
    u, p = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, Pp)
    ou, opr = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, np.nan)), op.initialize_dof_vector(1, np.full(op.n_pressure, np.nan))
    op.vmult(ou, opr, u, p)
    tiles, workgroups, grad_in_sweep = op.last_sweep_plan
    assert grad_in_sweep == 1  # the sweep added - B^T p itself (STFEM_STOKES_GRAD_KERNEL=1 would leave it to the gradient kernel)
    _assert_many_tiles((tiles, workgroups), "stokes gradient sweep")
    eu, ep = rel(ou.download(), ku), rel(opr.download(), kp)
    print(f"stokes: rel-L2 velocity {eu:.3e} pressure {ep:.3e}")
    assert eu < TOL and ep < TOL
