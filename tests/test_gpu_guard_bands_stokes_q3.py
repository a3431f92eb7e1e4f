"""Guard-band tests of the degree-3 Stokes operator (stfem_stokes_create_space with velocity degree 3): vmult, mass_vmult, st_vmult
(cG(2)) and st_vmult_slice_add on packed caller-owned views, both pressure spaces, on a perturbed 2 x 3 x 2 mesh.

The scheme is that of tests/test_gpu_guard_bands_stokes.py: each call runs on arrays in allocations of their own (`plain`) and on
views of one guarded arena (tests/guard_arena.py); plain agrees with the CPU oracle (pu = 3) within the operator's parity bound, the
arena result equals plain bit for bit, and every guard and source byte of the arena is unchanged.  A velocity vector is ONE view of
3 Nu doubles with Nu = 7 * 10 * 7 even here, a FE_Q(2) pressure vector has 5 * 7 * 5 = 175 doubles: with the `packed` placement the
views that follow it start at element alignment only."""
import functools
import importlib

import numpy as np
import pytest

from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]
TOL = 1e-12
NC, DISTORT, SEED, MASK, NU = (2, 3, 2), 0.15, 77, 0b111011, 0.7


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


def make(stfem, dg):
    return stfem.StokesMatrixFreeOperator.with_degree(3, NC, vertices=stfem.mesh_vertices(NC, distort=DISTORT, seed=SEED), dirichlet_mask=MASK,
                                                      viscosity=NU, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def oracle_of(dg):
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    return oracle.StokesOracle(NC, stfem.mesh_vertices(NC, distort=DISTORT, seed=SEED), MASK, NU, pu=3, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def space_reference(dg):
    orc = oracle_of(dg)
    rng = np.random.default_rng(21)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    res = dict(U=U, P=P, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1))
    for v in res.values():
        v.setflags(write=False)
    return res


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_vmult_and_mass_vmult(dg, placement, stfem, oracle_mod):
    """stfem_stokes_vmult, stfem_stokes_mass_vmult"""
    op, ref = make(stfem, dg), space_reference(dg)
    src = [vec("u", ref["U"]), vec("p", ref["P"], 1, dg)]
    guard_case(stfem, placement, src + [out("du", ref["U"].size), out("dp", ref["P"].size, 1, dg)],
               lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"]), {"du": within(ref["ku"]), "dp": within(ref["kp"])})
    guard_case(stfem, placement, src[:1] + [out("du", ref["U"].size)], lambda ptr: op.mass_vmult(ptr["du"], ptr["u"]), {"du": within(ref["mu"])})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_st_vmult(dg, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult, cG(2), one step: two sources in one set of launches"""
    op, orc = make(stfem, dg), oracle_of(dg)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    nt, nb = 2, 4
    var = [0, 0, 1, 1]
    rng = np.random.default_rng(201)
    blocks = [rng.uniform(-1, 1, 3 * orc.n_u if v == 0 else orc.n_p) for v in var]
    ref = orc.st_vmult(Alpha, Beta, 1, nt, blocks)
    specs = [vec(f"s{j}", blocks[j], var[j], dg) for j in range(nb)] + [out(f"d{j}", blocks[j].size, var[j], dg) for j in range(nb)]
    guard_case(stfem, placement, specs,
               lambda ptr: op.st_vmult(Alpha, Beta, 1, nt, [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)]),
               {f"d{j}": within(ref[j]) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", DGP, ids=DGP_IDS)
def test_st_vmult_slice_add(dg, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult_slice_add onto seeded destinations, one Gamma entry zero"""
    op, ref = make(stfem, dg), space_reference(dg)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 1, 0)] = 0.0
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    want = [init[j] + (Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"]) for j in range(nb)]
    specs = [vec("u", ref["U"]), vec("p", ref["P"], 1, dg)] + [out(f"d{j}", init[j].size, var[j], dg, seeded=init[j]) for j in range(nb)]
    guard_case(stfem, placement, specs, lambda ptr: op.st_vmult_slice_add(Gamma, Zeta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], ptr["u"], ptr["p"]),
               {f"d{j}": within(want[j]) for j in range(nb)})
