"""Guard-band test of the degree-3 Stokes Vanka smoother (stfem_stokes_vanka_create_space): stfem_stokes_vanka_step and _vmult on
views packed by tests/guard_arena.py, case pert222_dgp_cg2 (404 rows, time-major blocks).  The scheme is that of
tests/test_gpu_guard_bands_stokes.py: each call runs on arrays in allocations of their own and on views of one guarded arena; the
plain run agrees with tests/stokes_vanka_q3_reference.py within the 1e-10 of tests/test_gpu_stokes_vanka_q3.py, the arena result equals
the plain one bit for bit, and every guard and source byte of the arena is unchanged.  A velocity vector is one view of 3 Nu doubles
with Nu = 343 odd: with the `packed` placement no component is 16-byte aligned relative to the next."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stokes_vanka_q3_reference as q3r
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
def test_degree_3_vanka_step_on_packed_views(placement, stfem, oracle_mod):
    p, ref = q3r.case("pert222_dgp_cg2")
    op = stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=p.dg)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    nb = p.nb
    shape = [tuple(3 * c + 1 for c in p.nc) if v == 0 else None for v in p.var]  # (FE_DGP(2): ten per cell, no lattice)
    X = [np.random.default_rng(3 + j).uniform(-1, 1, p.sizes[j]) for j in range(nb)]
    D0 = [np.random.default_rng(20 + j).uniform(-1, 1, p.sizes[j]) for j in range(nb)]
    want = ref.vmult(X)
    src = [Spec(f"s{j}", X[j], "source", shape[j]) for j in range(nb)]

    def dsts(seeded):
        return [Spec(f"d{j}", D0[j] if seeded else poison(p.sizes[j], np.float64), "destination", shape[j]) for j in range(nb)]

    def args(ptr):
        return [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)]

    def vmult(ptr):  # the entry point itself (the Python vmult goes through the step)
        d, s = ((C.c_void_p * nb)(*a) for a in args(ptr))
        stfem._check(stfem.lib().stfem_stokes_vanka_vmult(V._h, d, s, None), "stfem_stokes_vanka_vmult")

    guard_case(stfem, placement, src + dsts(False), vmult, {f"d{j}": within(want[j]) for j in range(nb)})
    guard_case(stfem, placement, src + dsts(False), lambda ptr: V.step(args(ptr)[0], 0.6, False, args(ptr)[1]),
               {f"d{j}": within(0.6 * want[j]) for j in range(nb)})
    guard_case(stfem, placement, src + dsts(True), lambda ptr: V.step(args(ptr)[0], 0.6, True, args(ptr)[1]),
               {f"d{j}": within(D0[j] + 0.6 * want[j], scale=0.6 * np.linalg.norm(want[j])) for j in range(nb)})
