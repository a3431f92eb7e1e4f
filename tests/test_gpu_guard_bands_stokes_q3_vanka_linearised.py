"""Guard-band test of the degree-3 Stokes Vanka smoother of the linearised operator (stfem_stokes_vanka_create_linearised_space,
stfem_stokes_vanka_update, _step): case pert222_dgp_cg2 (404 rows, time-major blocks, two states), jacobian, with the linearisation
states, sources and destinations all views packed by tests/guard_arena.py.  The scheme is that of
tests/test_gpu_guard_bands_stokes_q3_vanka.py: each call runs on arrays in allocations of their own and on views of one guarded arena;
the plain run agrees with tests/stokes_vanka_q3_linearised_reference.py within the 1e-10 of tests/test_gpu_stokes_vanka_q3_linearised.py,
the arena result equals the plain one bit for bit, and every guard and source byte of the arena - those of the states included - is
unchanged.  A velocity vector is one view of 3 Nu doubles with Nu = 343 odd: with the `packed` placement no component is 16-byte aligned
relative to the next."""
import importlib

import numpy as np
import pytest

import stokes_vanka_q3_linearised_reference as lq3
from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("STFEM_VANKA_SETUP_LAYERS", raising=False)


def within(ref, scale=None):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    scale = np.linalg.norm(ref) if scale is None else scale

    def check(got):
        err = np.linalg.norm(got - ref)
        print(f"|got - ref| = {err:.3e}, bound {TOL:.1e} x {scale:.3e}")
        assert scale > 0 and err <= TOL * scale, (err, TOL * scale)
    return check


@pytest.mark.parametrize("placement", ["aligned", "packed"])
def test_degree_3_linearised_vanka_on_packed_views(placement, stfem, oracle_mod):
    p, mode, lin, ref, _ = lq3.case("pert222_dgp_cg2")
    assert mode == lq3.JACOBIAN
    op = stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=p.dg)
    nb = p.nb
    lattice = tuple(3 * c + 1 for c in p.nc)
    shape = [lattice if v == 0 else None for v in p.var]  # (FE_DGP(2): ten per cell, no lattice)
    X = [np.random.default_rng(3 + j).uniform(-1, 1, p.sizes[j]) for j in range(nb)]
    D0 = [np.random.default_rng(20 + j).uniform(-1, 1, p.sizes[j]) for j in range(nb)]
    want = ref.vmult(X)
    src = [Spec(f"s{j}", X[j], "source", shape[j]) for j in range(nb)]
    states = [Spec(f"b{j}", lin[j], "source", lattice) for j in range(nb) if lin[j] is not None]
    assert len(states) == 2
    # the states the updated smoother is created about: others, in allocations of the library
    other = [None if b is None else op.initialize_dof_vector(0, b) for b in lq3.states(p, seed=12)]

    def dsts(seeded):
        return [Spec(f"d{j}", D0[j] if seeded else poison(p.sizes[j], np.float64), "destination", shape[j]) for j in range(nb)]

    def args(ptr):
        return [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)], [ptr.get(f"b{j}") for j in range(nb)]

    def create_and_step(ptr):  # the states read from the views at creation
        d, s, b = args(ptr)
        V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=b, mode=mode)
        V.step(d, 0.6, False, s)

    def update_and_step(ptr):  # ... and at update, into the storage of a smoother created about other states; onto seeded destinations
        d, s, b = args(ptr)
        V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=other, mode=mode)
        V.update(b)
        V.step(d, 0.6, True, s)

    guard_case(stfem, placement, src + states + dsts(False), create_and_step, {f"d{j}": within(0.6 * want[j]) for j in range(nb)})
    guard_case(stfem, placement, src + states + dsts(True), update_and_step,
               {f"d{j}": within(D0[j] + 0.6 * want[j], scale=0.6 * np.linalg.norm(want[j])) for j in range(nb)})
