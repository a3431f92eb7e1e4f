"""Guard-band tests of the convection modes of the degree-3 Stokes operator (include/stfem_stokes_convection_space.h):
stfem_stokes_vmult_convection_space, _st_vmult_convection_space (cG(2)) and _st_vmult_slice_add_convection_space on packed caller-owned
views, both pressure spaces and both modes, on a perturbed 2 x 3 x 2 mesh.

The scheme is that of tests/test_gpu_guard_bands_stokes_q3.py: each call runs on arrays in allocations of their own (`plain`) and on
views of one guarded arena (tests/guard_arena.py); plain agrees with the CPU oracle (pu = 3) plus the numpy restatement of the term
(tests/navier_q3_reference.py) within the operator's parity bound, the arena result equals plain bit for bit, and every guard and
source byte of the arena - the linearisation velocities are sources too - is unchanged."""
import functools
import importlib

import numpy as np
import pytest

import navier_q3_reference as q3
from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]
MODES = [q3.FORM, q3.JACOBIAN]
MODE_IDS = ["form", "jacobian"]
TOL = 1e-12
NC, DISTORT, SEED, MASK, NU, BSCALE = (2, 3, 2), 0.15, 77, 0b111011, 0.01, 8.0


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)


def vec(name, data, variable=0, dg=False, role="source"):
    shape = tuple(3 * c + 1 for c in NC) if variable == 0 else (None if dg else tuple(2 * c + 1 for c in NC))
    return Spec(name, data, role, shape)


def out(name, n, variable=0, dg=False, seeded=None):
    return vec(name, poison(n, np.float64) if seeded is None else seeded, variable, dg, "destination")


def within(ref, scale=None):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    scale = np.linalg.norm(ref) if scale is None else scale

    def check(got):
        err = np.linalg.norm(got - ref)
        print(f"|got - ref| = {err:.3e}, bound {TOL:.1e} x {scale:.3e}")
        assert scale > 0 and err <= TOL * scale, (err, TOL * scale)
    return check


@functools.lru_cache(maxsize=None)
def vertices():
    stfem = importlib.import_module("dealii-stfem_amd")
    v = stfem.mesh_vertices(NC, distort=DISTORT, seed=SEED)
    v.setflags(write=False)
    return v


def make(stfem, dg):
    return stfem.StokesMatrixFreeOperator.with_degree(3, NC, vertices=vertices(), dirichlet_mask=MASK, viscosity=NU, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def oracle_of(dg):
    from oracle import oracle
    return oracle.StokesOracle(NC, vertices(), MASK, NU, pu=3, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def space_reference(dg, mode):
    """one random (u, p, b) and the expected K_S (u, p) + C(b; u), M u: computed once and shared"""
    orc = oracle_of(dg)
    rng = np.random.default_rng(21)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), BSCALE * rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    conv = q3.convection(3, mode, B, U, NC, vertices(), MASK)
    res = dict(U=U, P=P, B=B, ku=ku.reshape(-1) + conv, kp=kp, mu=mu.reshape(-1))
    for v in res.values():
        v.setflags(write=False)
    return res


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_vmult_convection_space(dg, mode, placement, stfem, oracle_mod):
    """stfem_stokes_vmult_convection_space"""
    op, ref = make(stfem, dg), space_reference(dg, mode)
    specs = [vec("u", ref["U"]), vec("p", ref["P"], 1, dg), vec("b", ref["B"]), out("du", ref["U"].size), out("dp", ref["P"].size, 1, dg)]
    guard_case(stfem, placement, specs, lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"], lin=ptr["b"], mode=mode),
               {"du": within(ref["ku"]), "dp": within(ref["kp"])})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_st_vmult_convection_space(dg, mode, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult_convection_space, cG(2), one step: two sources in one set of launches, a linearisation velocity each"""
    op, orc = make(stfem, dg), oracle_of(dg)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    nt, nb = 2, 4
    var = [0, 0, 1, 1]
    rng = np.random.default_rng(201)
    blocks = [rng.uniform(-1, 1, 3 * orc.n_u if v == 0 else orc.n_p) for v in var]
    lin = [BSCALE * rng.uniform(-1, 1, 3 * orc.n_u) for _ in range(nt)]
    ref = orc.st_vmult(Alpha, Beta, 1, nt, blocks)
    add = q3.st_convection(3, mode, Alpha, 1, nt, blocks, lin + [None, None], lambda it, v, d: stfem.stokes_block_index(nt, it, v, d), NC,
                           vertices(), MASK)
    ref = [r if a is None else r + a for r, a in zip(ref, add)]
    specs = ([vec(f"s{j}", blocks[j], var[j], dg) for j in range(nb)] + [vec(f"b{j}", lin[j]) for j in range(nt)] +
             [out(f"d{j}", blocks[j].size, var[j], dg) for j in range(nb)])
    guard_case(stfem, placement, specs,
               lambda ptr: op.st_vmult(Alpha, Beta, 1, nt, [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)],
                                       lin=[ptr["b0"], ptr["b1"], None, None], mode=mode),
               {f"d{j}": within(ref[j]) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_st_vmult_slice_add_convection_space(dg, mode, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult_slice_add_convection_space onto seeded destinations, one Gamma entry zero"""
    op, ref = make(stfem, dg), space_reference(dg, mode)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 1, 0)] = 0.0
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    want = [init[j] + (Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"]) for j in range(nb)]
    specs = ([vec("u", ref["U"]), vec("p", ref["P"], 1, dg), vec("b", ref["B"])] +
             [out(f"d{j}", init[j].size, var[j], dg, seeded=init[j]) for j in range(nb)])
    guard_case(stfem, placement, specs,
               lambda ptr: op.st_vmult_slice_add(Gamma, Zeta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], ptr["u"], ptr["p"], lin=ptr["b"],
                                                 mode=mode),
               {f"d{j}": within(want[j]) for j in range(nb)})
