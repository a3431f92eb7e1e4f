"""Guard-band tests of the weak faces at velocity degree 3 (include/stfem_stokes_boundary_space.h): stfem_stokes_nitsche_rhs_space and
the stfem_stokes_vmult of a context with weak faces on packed caller-owned views, both pressure spaces, on the perturbed 2 x 1 x 2
mesh of tests/stokes_q3_faces_reference.py (x and y faces weak, the y faces strongly constrained as well).

The scheme is that of tests/test_gpu_guard_bands_stokes_q3.py: each call runs on arrays in allocations of their own (`plain`) and on
views of one guarded arena (tests/guard_arena.py); plain agrees with the CPU oracle (pu = 3, with its weak mask) within the operator's
parity bound, the arena result equals plain bit for bit, and every guard and source byte of the arena is unchanged."""
import importlib

import numpy as np
import pytest

import stokes_q3_faces_reference as fr
from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
TOL = fr.TOL
CASE = "2x1x2_y_strong"
NC = fr.OPERATOR_CASES[CASE][0]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)
    monkeypatch.delenv("STFEM_STOKES_FACE_WORKGROUPS", raising=False)


def vec(name, data, variable=0, dg=False, role="source"):
    shape = tuple(3 * c + 1 for c in NC) if variable == 0 else (None if dg else tuple(2 * c + 1 for c in NC))
    return Spec(name, data, role, shape)


def within(ref, scale=None):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    scale = np.linalg.norm(ref) if scale is None else scale

    def check(got):
        err = np.linalg.norm(got - ref)
        print(f"|got - ref| = {err:.3e}, bound {TOL:.1e} x {scale:.3e}")
        assert scale > 0 and err <= TOL * scale, (err, TOL * scale)
    return check


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", fr.DGP, ids=fr.DGP_IDS)
def test_vmult_with_faces(dg, placement, stfem, oracle_mod):
    """stfem_stokes_vmult: the cell launches, then the eight boundary colour launches"""
    op, ref = fr.device_operator(stfem, CASE, dg), fr.operator_reference(CASE, dg)
    specs = [vec("u", ref["U"]), vec("p", ref["P"], 1, dg), vec("du", poison(ref["U"].size, np.float64), 0, dg, "destination"),
             vec("dp", poison(ref["P"].size, np.float64), 1, dg, "destination")]
    guard_case(stfem, placement, specs, lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"]),
               {"du": within(ref["ku"]), "dp": within(ref["kp"])}, check=lambda: op.last_face_plan())


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", fr.DGP, ids=fr.DGP_IDS)
def test_nitsche_rhs_space(dg, placement, stfem, oracle_mod):
    """stfem_stokes_nitsche_rhs_space onto seeded destinations (it accumulates); g is a host array"""
    op, orc = fr.device_operator(stfem, CASE, dg), fr.operator_oracle(CASE, dg)
    rng = np.random.default_rng(31)
    g = rng.uniform(-1, 1, (op.n_face_points_space(), 3))
    init_u, init_p = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ru, rp = orc.nitsche_rhs(g)
    specs = [vec("du", init_u, 0, dg, "destination"), vec("dp", init_p, 1, dg, "destination")]
    guard_case(stfem, placement, specs, lambda ptr: op.nitsche_rhs_space(g, ptr["du"], ptr["dp"]),
               {"du": within(init_u + ru.reshape(-1), scale=np.linalg.norm(ru)), "dp": within(init_p + rp, scale=np.linalg.norm(rp))})
