"""Guard-band tests of the CIP interior-face term at velocity degree 3 (include/stfem_stokes_cip_space.h): stfem_stokes_cip_add_space
and the integrated entries after stfem_stokes_set_cip_space - stfem_stokes_vmult, stfem_stokes_st_vmult (two sources) and
stfem_stokes_vmult_convection_space - on packed caller-owned views, on the perturbed 3 x 2 x 4 mesh of tests/cip_q3_reference.py
(st_vmult on its 4 x 3 x 2 box too: the CART several-source instantiation).

The scheme is that of tests/test_gpu_guard_bands_stokes_q3.py: each call runs on arrays in allocations of their own (`plain`) and on
views of one guarded arena (tests/guard_arena.py); plain agrees with the reference (the CPU oracle at pu = 3 plus the numpy
restatement of the term) within the operator's parity bound, the arena result equals plain bit for bit, and every guard and source
byte of the arena is unchanged."""
import importlib

import numpy as np
import pytest

import cip_q3_reference as c3
import navier_q3_reference as q3
from guard_arena import Spec, guard_case, poison
from test_gpu_stokes_q3_cip import ST_MASK, ST_MESH, cip_of, field, linear_reference, st_case, st_term

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
TOL = c3.TOL
NC = c3.MESHES[ST_MESH][0]
DELTA0 = c3.delta0_of(ST_MESH, ST_MASK)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("STFEM_STOKES_Q3_WORKGROUPS", "STFEM_STOKES_FACE_WORKGROUPS", "STFEM_STOKES_CIP_WORKGROUPS"):
        monkeypatch.delenv(name, raising=False)


def vec(name, data, variable=0, role="source", nc=NC):
    shape = tuple(3 * c + 1 for c in nc) if variable == 0 else tuple(2 * c + 1 for c in nc)
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
def test_cip_add_space(placement, stfem):
    """the term by itself onto a seeded destination (it accumulates), the weight velocity an array of its own"""
    op = c3.device_operator(stfem, ST_MESH, ST_MASK)
    f = c3.fields(ST_MESH)
    ref = DELTA0 * c3.term(ST_MESH, ST_MASK, 1, 0)
    specs = [vec("u", f[0]), vec("w", f[1]), vec("du", f[2], 0, "destination")]
    guard_case(stfem, placement, specs, lambda ptr: op.cip_add_space(ptr["du"], ptr["u"], ptr["w"], DELTA0),
               {"du": within(f[2] + ref, scale=np.linalg.norm(f[2]) + np.linalg.norm(ref))}, check=lambda: op.last_cip_plan())


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_vmult_with_cip(placement, stfem, oracle_mod):
    """stfem_stokes_vmult: the cell launches, then the eight CIP colour launches"""
    op, ref = c3.device_operator(stfem, ST_MESH, ST_MASK), linear_reference(ST_MESH, ST_MASK, False)
    op.set_cip_space(DELTA0)
    specs = [vec("u", ref["U"]), vec("p", ref["P"], 1), vec("du", poison(ref["U"].size, np.float64), 0, "destination"),
             vec("dp", poison(ref["P"].size, np.float64), 1, "destination")]
    guard_case(stfem, placement, specs, lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"]),
               {"du": within(ref["ku"] + DELTA0 * c3.term(ST_MESH, ST_MASK, 0, 0)), "dp": within(ref["kp"])}, check=lambda: op.last_cip_plan())


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_vmult_convection_space_with_cip(placement, stfem, oracle_mod):
    """stfem_stokes_vmult_convection_space in jacobian mode, the term weighted with the linearisation velocity"""
    op, ref = c3.device_operator(stfem, ST_MESH, ST_MASK), linear_reference(ST_MESH, ST_MASK, False)
    op.set_cip_space(DELTA0, stfem.CIP_WEIGHT_LINEARISATION)
    B = field(ST_MESH, ("f", 3))
    want = ref["ku"] + q3.convection(3, q3.JACOBIAN, B, ref["U"], NC, c3.mesh_vertices(ST_MESH), ST_MASK) + \
        DELTA0 * cip_of(ST_MESH, ST_MASK, ("f", 3), ("f", 0))
    specs = [vec("u", ref["U"]), vec("p", ref["P"], 1), vec("b", B), vec("du", poison(ref["U"].size, np.float64), 0, "destination"),
             vec("dp", poison(ref["P"].size, np.float64), 1, "destination")]
    guard_case(stfem, placement, specs, lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"], lin=ptr["b"], mode=q3.JACOBIAN),
               {"du": within(want), "dp": within(ref["kp"])}, check=lambda: op.last_cip_plan())


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mesh,mask", [(ST_MESH, ST_MASK), ("box", 0)], ids=["pert", "box"])
def test_st_vmult_with_cip(mesh, mask, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult with the two time dofs of cG(2): the several-source instantiations, general and CART"""
    nc = c3.MESHES[mesh][0]
    delta0 = c3.delta0_of(mesh, mask) if mesh == ST_MESH else c3.st_delta0_of(mesh, mask)
    Alpha, Beta, nt, var, keys, blocks, none = st_case(2, False, mesh, mask)
    op = c3.device_operator(stfem, mesh, mask)
    op.set_cip_space(delta0)
    add = st_term(Alpha, nt, keys, keys, mesh, mask)
    specs = [vec(f"s{j}", b, v, nc=nc) for j, (v, b) in enumerate(zip(var, blocks))]
    specs += [vec(f"d{j}", poison(b.size, np.float64), v, "destination", nc) for j, (v, b) in enumerate(zip(var, blocks))]
    refs = {f"d{j}": within(none[j] + (delta0 * add[j] if var[j] == 0 else 0.0)) for j in range(2 * nt)}
    guard_case(stfem, placement, specs,
               lambda ptr: op.st_vmult(Alpha, Beta, 1, nt, [ptr[f"d{j}"] for j in range(2 * nt)], [ptr[f"s{j}"] for j in range(2 * nt)], True),
               refs, check=lambda: op.last_cip_plan())
