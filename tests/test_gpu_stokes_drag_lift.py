"""GPU parity of stfem_stokes_drag_lift (StokesMatrixFreeOperator::compute_drag_lift, reference include/operators.h:1344-1389) against
the numpy restatement tests/drag_lift_reference.py (dense tables at the nine face points, the normal from the cross product of the
face tangents; itself checked against closed forms by tests/test_drag_lift_reference_cpu.py).  Forces and per-item values within
1e-12 A, A = sum |tau_k| JxW over the contributing points and components: the project's parity bar for the Stokes kernels.
Meshes: 2 x 3 x 4 cells on a box with unequal extents (unequal counts expose swapped axes), a lone cell on all six faces, 3 x 2 x 2
perturbed by 0.15, and 9 x 2 x 2: 18 items on the x-y and x-z faces (more than one workgroup round of eight, not a multiple of eight)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drag_lift_reference as dref  # noqa: E402
import navier_reference as nref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
NU = 0.7
BOX = ((0.0, -0.5, 0.25), (1.0, 0.25, 2.25))
UNIT = ((0, 0, 0), (1, 1, 1))
MESHES = {"box": ((2, 3, 4), 0.0, BOX), "cell": ((1, 1, 1), 0.0, UNIT), "pert": ((3, 2, 2), 0.15, UNIT), "long": ((9, 2, 2), 0.0, UNIT)}
MASKS = [1, 2, 4, 8, 16, 32, 63, 0b100001]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _setup(stfem, mesh, dmask, dg=False, nu=NU):
    nc, distort, (lo, up) = MESHES[mesh]
    verts = nref.perturbed_vertices(nc, distort, 77, lo, up)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, lower=lo, upper=up, dirichlet_mask=dmask, viscosity=nu,
                                        dg_pressure=dg)
    return op, nc, verts


def _fields(op, seed, n=1):
    rng = np.random.default_rng(seed)
    U = [rng.uniform(-1, 1, 3 * op.n_velocity) for _ in range(n)]
    P = [rng.uniform(-1, 1, op.n_pressure) for _ in range(n)]
    return U, P, [op.initialize_dof_vector(0, u) for u in U], [op.initialize_dof_vector(1, p) for p in P]


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_parity_random_fields(mesh, dg, stfem):
    """each single face, all six and a mixed pair; the strong constraints of mask 0b011101 read as zero (the reference's rule)"""
    dmask = 0b011101
    op, nc, verts = _setup(stfem, mesh, dmask, dg)
    (u,), (p,), (du,), (dp,) = _fields(op, 21)
    worst = 0.0
    for mask in MASKS:
        force, items = op.drag_lift(du, dp, mask, scale=1.75, items=True)
        rf, ri, A = dref.drag_lift(u, p, nc, verts, NU, mask, dirichlet_mask=dmask, dg_pressure=dg, scale=1.75)
        assert op.drag_lift_n_items(mask) == dref.n_items(nc, mask) == len(ri)
        assert force.shape == (3,) and items.shape == ri.shape
        ratio = max(np.max(np.abs(force - rf)) / (1.75 * A), np.max(np.abs(items - ri)) / A)
        worst = max(worst, ratio)
        assert np.max(np.abs(rf)) > 1e-3 * A / max(len(ri), 1)  # (something is compared)
        assert ratio <= TOL, (mask, ratio)
        # faces as a set of ids, and the force alone, are the same numbers
        assert np.array_equal(op.drag_lift(du, dp, [f for f in range(6) if mask >> f & 1], scale=1.75), force)
    print(f"{mesh} dg={int(dg)}: largest |difference| / A = {worst:.3e}")


@pytest.mark.parametrize("dg", [False, True])
def test_reading_rule(dg, stfem):
    """with strong constraints on all faces the two rules differ and each matches the restatement with the same rule; without
    constraints they are bit-equal"""
    op, nc, verts = _setup(stfem, "pert", 63, dg)
    (u,), (p,), (du,), (dp,) = _fields(op, 22)
    got = {}
    for plain in (False, True):
        got[plain], items = op.drag_lift(du, dp, 63, plain=plain, items=True)
        rf, ri, A = dref.drag_lift(u, p, nc, verts, NU, 63, dirichlet_mask=63, plain=plain, dg_pressure=dg)
        assert np.max(np.abs(got[plain] - rf)) <= TOL * A and np.max(np.abs(items - ri)) <= TOL * A
    assert np.max(np.abs(got[True] - got[False])) > 1e-3 * A / len(ri)
    op0, _, _ = _setup(stfem, "pert", 0, dg)
    du0, dp0 = op0.initialize_dof_vector(0, u), op0.initialize_dof_vector(1, p)
    f0, i0 = op0.drag_lift(du0, dp0, 63, plain=False, items=True)
    f1, i1 = op0.drag_lift(du0, dp0, 63, plain=True, items=True)
    assert np.array_equal(f0, f1) and np.array_equal(i0, i1)
    assert np.array_equal(f1, got[True])  # (the plain read does not look at the mask)


@pytest.mark.parametrize("dmask,plain", [(12, False), (63, True)])
@pytest.mark.parametrize("dg", [False, True])
def test_poiseuille_closed_forms(dmask, plain, dg, stfem):
    """u = (y (1 - y), 0, 0), p = -2 nu x + c on [0, Lx] x [0, 1] x [0, Lz], 2 x 2 x 2 cells: every face and all six (0).  With the
    no-slip walls constrained (mask 12) the reference's read sees the whole field; with all faces constrained it takes the plain read"""
    nc, L, c0 = (2, 2, 2), (2.0, 1.0, 1.5), 1.3
    u, p, verts = dref.poiseuille(nc, L, NU, c0, dg)
    op = stfem.StokesMatrixFreeOperator(nc, lower=(0, 0, 0), upper=L, dirichlet_mask=dmask, viscosity=NU, dg_pressure=dg)
    du, dp = op.initialize_dof_vector(0, u), op.initialize_dof_vector(1, p)
    want = dref.poiseuille_forces(L, NU, c0)
    for f in range(6):
        _, _, A = dref.drag_lift(u, p, nc, verts, NU, 1 << f, plain=True, dg_pressure=dg)
        got = op.drag_lift(du, dp, [f], plain=plain)
        assert np.max(np.abs(got - np.array(want[f]))) <= TOL * A, (f, got, want[f])
    _, _, A = dref.drag_lift(u, p, nc, verts, NU, 63, plain=True, dg_pressure=dg)
    assert np.max(np.abs(op.drag_lift(du, dp, 63, plain=plain))) <= TOL * A


def test_closed_surface(stfem):
    """constant pressure, no flow, all six faces of the perturbed mesh: 0, though every item is not"""
    nc = MESHES["pert"][0]
    # (perturbed_vertices moves the interior vertices only: move the boundary ones too, so that the faces are truly trilinear)
    verts = nref.perturbed_vertices(nc, 0.15, 77) + 0.05 * np.random.default_rng(26).uniform(-1, 1, (36, 3))
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts, dirichlet_mask=0, viscosity=NU)
    p = np.full(op.n_pressure, 2.5)
    force, items = op.drag_lift(op.initialize_dof_vector(0), op.initialize_dof_vector(1, p), 63, items=True)
    _, ri, A = dref.drag_lift(np.zeros(3 * op.n_velocity), p, nc, verts, NU, 63)
    assert A > 1.0 and np.max(np.abs(ri)) > 0.1
    assert np.max(np.abs(items - ri)) <= TOL * A and np.max(np.abs(force)) <= TOL * A


@pytest.mark.parametrize("dg", [False, True])
def test_batched_calls_are_the_single_calls(dg, stfem):
    """n = 1, 3, 5 pairs in one call (5 crosses a group of four): every pair bit-equal to its own call, a repeated call bit-equal"""
    op, nc, verts = _setup(stfem, "long", 0b110011, dg)
    U, P, dU, dP = _fields(op, 23, 5)
    mask = 0b101110
    single = [op.drag_lift(dU[i], dP[i], mask, scale=0.5, items=True) for i in range(5)]
    rf, ri, A = dref.drag_lift(U[4], P[4], nc, verts, NU, mask, dirichlet_mask=0b110011, dg_pressure=dg, scale=0.5)
    assert np.max(np.abs(single[4][0] - rf)) <= TOL * A and np.max(np.abs(single[4][1] - ri)) <= TOL * A
    for n in (1, 3, 5):
        force, items = op.drag_lift(dU[:n], dP[:n], mask, scale=0.5, items=True)
        assert force.shape == (n, 3) and items.shape == (n, len(ri), 3)
        for i in range(n):
            assert np.array_equal(force[i], single[i][0]) and np.array_equal(items[i], single[i][1]), (n, i)
        again = op.drag_lift(dU[:n], dP[:n], mask, scale=0.5)
        assert np.array_equal(again, force)
    # the item array of ONE call of the library holds all five pairs ([i][item][3]) and nothing behind them
    nitems = op.drag_lift_n_items(mask)
    assert 5 * nitems * 3 < 3 * op.n_velocity
    sentinel = np.full(3 * op.n_velocity, -7.25)
    scratch = op.initialize_dof_vector(0, sentinel)
    out = np.zeros((5, 3))
    ptrs = lambda vs: (C.c_void_p * 5)(*[v.ptr for v in vs])  # noqa: E731
    assert stfem.lib().stfem_stokes_drag_lift(op._h, mask, 0.5, 0, 5, ptrs(dU), ptrs(dP), scratch.ptr, out.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    got = scratch.download()
    assert np.array_equal(got[:5 * nitems * 3].reshape(5, nitems, 3), np.stack([s[1] for s in single]))
    assert np.array_equal(got[5 * nitems * 3:], sentinel[5 * nitems * 3:])
    assert np.array_equal(out, np.stack([s[0] for s in single]))


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_z_slabs_add_up(world, dg, stfem):
    """a 3 x 2 x 6 mesh cut into z-slabs: a slab is a mesh of its own, the z faces are in its mask only where it meets the boundary,
    and the slabs' forces add up to the whole mesh's (the reference's MPI sum, operators.h:1387)"""
    nc, dmask = (3, 2, 6), 63 & ~1
    ndu, ndp = [2 * c + 1 for c in nc], [c + 1 for c in nc]
    whole = stfem.StokesMatrixFreeOperator(nc, dirichlet_mask=dmask, viscosity=NU, dg_pressure=dg)
    (u,), (p,), (du,), (dp,) = _fields(whole, 24)
    want = whole.drag_lift(du, dp, 63)
    _, _, A = dref.drag_lift(u, p, nc, nref.perturbed_vertices(nc, 0.0, 0), NU, 63, dirichlet_mask=dmask, dg_pressure=dg)
    bounds = [round(nc[2] * r / world) for r in range(world + 1)]
    total = np.zeros(3)
    for r in range(world):
        z0, z1 = bounds[r], bounds[r + 1]
        m, faces = dmask, 63
        if r > 0:
            m &= ~16; faces &= ~16
        if r < world - 1:
            m &= ~32; faces &= ~32
        op = stfem.StokesMatrixFreeOperator((nc[0], nc[1], z1 - z0), lower=(0, 0, z0 / nc[2]), upper=(1, 1, z1 / nc[2]), dirichlet_mask=m,
                                            viscosity=NU, dg_pressure=dg)
        su = u.reshape(3, ndu[2], ndu[0] * ndu[1])[:, 2 * z0:2 * z1 + 1].reshape(-1)
        sp = p.reshape(nc[2], -1)[z0:z1].reshape(-1) if dg else p.reshape(ndp[2], -1)[z0:z1 + 1].reshape(-1)
        total += op.drag_lift(op.initialize_dof_vector(0, su), op.initialize_dof_vector(1, sp), faces)
    print(f"{world} slabs dg={int(dg)}: |sum - whole| / A = {np.max(np.abs(total - want)) / A:.3e}")
    assert np.max(np.abs(want)) > 1e-3 * A / 72 and np.max(np.abs(total - want)) <= TOL * A


def test_refused_calls(stfem):
    """-1 (STFEM_ERR_INVALID_ARGUMENT) with the reason in the error record, `out` untouched"""
    op, nc, verts = _setup(stfem, "box", 63)
    _, _, dU, dP = _fields(op, 25, 2)
    lib = stfem.lib()
    out = np.full((2, 3), -7.25)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    U, P = (C.c_void_p * 2)(dU[0].ptr, dU[1].ptr), (C.c_void_p * 2)(dP[0].ptr, dP[1].ptr)
    holeU, holeP = (C.c_void_p * 2)(dU[0].ptr, None), (C.c_void_p * 2)(None, dP[1].ptr)
    call = lib.stfem_stokes_drag_lift
    refused = [("null context", lambda: call(None, 1, 1.0, 0, 2, U, P, None, po, None)),
               ("null u", lambda: call(op._h, 1, 1.0, 0, 2, None, P, None, po, None)),
               ("null p", lambda: call(op._h, 1, 1.0, 0, 2, U, None, None, po, None)),
               ("null out", lambda: call(op._h, 1, 1.0, 0, 2, U, P, None, None, None)),
               ("u[1]", lambda: call(op._h, 1, 1.0, 0, 2, holeU, P, None, po, None)),
               ("p[0]", lambda: call(op._h, 1, 1.0, 0, 2, U, holeP, None, po, None)),
               ("n = 0", lambda: call(op._h, 1, 1.0, 0, 0, U, P, None, po, None)),
               ("n = -1", lambda: call(op._h, 1, 1.0, 0, -1, U, P, None, po, None)),
               ("face_mask 0", lambda: call(op._h, 0, 1.0, 0, 2, U, P, None, po, None)),
               ("face_mask 64", lambda: call(op._h, 64, 1.0, 0, 2, U, P, None, po, None)),
               ("face_mask -1", lambda: call(op._h, -1, 1.0, 0, 2, U, P, None, po, None)),
               ("scale is not finite", lambda: call(op._h, 1, float("nan"), 0, 2, U, P, None, po, None)),
               ("scale is not finite", lambda: call(op._h, 1, float("inf"), 0, 2, U, P, None, po, None))]
    for reason, f in refused:
        assert f() == -1, reason
        assert reason in lib.stfem_last_error().decode(), (reason, lib.stfem_last_error())
        assert np.all(out == -7.25), reason
    assert lib.stfem_stokes_drag_lift_n_items(op._h, 0) == -1 and lib.stfem_stokes_drag_lift_n_items(op._h, 64) == -1
    assert lib.stfem_stokes_drag_lift_n_items(None, 1) == -1
    with pytest.raises(stfem.StfemError):
        op.drag_lift(dU[0], dP[0], 0)
    with pytest.raises(stfem.StfemError):
        op.drag_lift([], [], 1)
    with pytest.raises(ValueError):
        op.drag_lift(dU, dP[0], 1)
    # the same call with its arguments in place succeeds
    assert call(op._h, 1, 1.0, 0, 2, U, P, None, po, None) == 0 and np.all(out != -7.25)
    assert np.array_equal(out, op.drag_lift(dU, dP, [0]))
