"""Guard-band tests of the Stokes side: every device entry point on packed caller-owned views (fp64, raw device pointers).

The scheme is that of tests/test_gpu_guard_bands.py: each call runs on arrays in allocations of their own (`plain`) and on views of one
guarded arena (tests/guard_arena.py); plain agrees with the CPU reference within the bound of the entry point's existing parity test,
the arena result equals plain bit for bit, and every guard and source byte of the arena is unchanged.  A velocity vector is ONE view
of 3 Nu doubles, so its components lie at base + c Nu with Nu odd: with the `packed` placement no component is 16-byte aligned
relative to the next.  Destinations start as a poison NaN where the call overwrites and as seeded values where it accumulates."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import cip_reference as cref
import cip_slab_reference as csr
import drag_lift_reference as dref
import navier_reference as nref
import navier_slab_reference as nsr
import stokes_slab_cases as ssc
import stokes_vanka_cip_reference as scr
import stokes_vanka_reference as svr
from guard_arena import BY_CALLER, Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
TOL = 1e-12       # the operator's parity bound (test_gpu_stokes.py, test_gpu_navier.py, test_gpu_stokes_cip.py)
TOL_VANKA = 1e-10  # inverted blocks (test_gpu_stokes_vanka.py, test_gpu_stokes_vanka_linearised.py)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for knob in ("STFEM_VARIANT", "STFEM_EXP", "STFEM_VANKA_COLOURS", "STFEM_VANKA_HOST_SETUP", "STFEM_VANKA_SETUP_LAYERS"):
        monkeypatch.delenv(knob, raising=False)


def vshape(nc):
    return tuple(2 * c + 1 for c in nc)


def pshape(nc, dg):
    return None if dg else tuple(c + 1 for c in nc)


def vec(name, data, nc, variable=0, dg=False, role="source"):
    return Spec(name, data, role, vshape(nc) if variable == 0 else pshape(nc, dg))


def out(name, n, nc, variable=0, dg=False, seeded=None):
    return vec(name, poison(n, np.float64) if seeded is None else seeded, nc, variable, dg, "destination")


def within(ref, tol=TOL, scale=None):
    """||got - ref|| <= tol * scale (the norm of ref, or of the term where the call accumulates), as the parity tests measure it"""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    scale = np.linalg.norm(ref) if scale is None else scale

    def check(got):
        err = np.linalg.norm(got - ref)
        print(f"|got - ref| = {err:.3e}, bound {tol:.1e} x {scale:.3e}")
        assert scale > 0 and err <= tol * scale, (err, tol * scale)
    return check


# ------------------------------------------------------------------------------------------ the operator

# name: (cells, distortion (0: a box without vertices: Kronecker path), seed, Dirichlet mask, weak faces, outflow faces, viscosity, FE_DGP)
CONFIGS = {
    "kron":  ((5, 4, 6), 0.0, 0, 0b111011, 0, 0, 0.7, False),   # FE_Q(1): 7 pressure planes, the z-march ends in a segment of 3
    "dgp":   ((5, 4, 6), 0.0, 0, 0b111011, 0, 0, 0.7, True),
    "cell":  ((5, 4, 6), 0.15, 77, 0b111011, 0, 0, 0.7, False),  # the cell kernel
    "weak":  ((4, 3, 5), 0.1, 41, 0b110000, 0b001011, 0b000100, 0.3, False),
    "sweep": ((3, 2, 6), 0.0, 0, 63 & ~1, 0, 0, 0.8, False),     # cG(1): the gradient rides in the sweep
}


def faces(mask):
    return [f for f in range(6) if mask >> f & 1]


def make(stfem, name, **kw):
    nc, distort, seed, mask, weak, outflow, nu, dg = CONFIGS[name]
    verts = stfem.mesh_vertices(nc, distort=distort, seed=seed) if distort else stfem.mesh_vertices(nc)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, dirichlet_mask=mask, viscosity=nu, weak_boundary_ids=faces(weak),
                                        outflow_boundary_ids=faces(outflow), dg_pressure=dg, **kw)
    return op, nc, verts, dg


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    nc, distort, seed, mask, weak, outflow, nu, dg = CONFIGS[name]
    verts = stfem.mesh_vertices(nc, distort=distort, seed=seed) if distort else stfem.mesh_vertices(nc)
    return oracle.StokesOracle(nc, verts, mask, nu, weak_mask=weak & ~outflow, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def space_reference(name):
    orc = oracle_of(name)
    rng = np.random.default_rng(21)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    res = dict(U=U, P=P, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1))
    for v in res.values():
        v.setflags(write=False)
    return res


SCHEMES = {"cg2": (2, 1), "cg1": (1, 1), "cg1x5": (1, 5)}  # (r, steps at once) of cG(r)


@functools.lru_cache(maxsize=None)
def st_reference(name, scheme, transpose=False):
    stfem = importlib.import_module("dealii-stfem_amd")
    orc = oracle_of(name)
    r, ns = SCHEMES[scheme]
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, r, 1.0 / 16, ns)
    nt, nb = r, 2 * r * ns
    var = [0] * nb
    rng = np.random.default_rng(100 * r + ns)
    blocks = [None] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[stfem.stokes_block_index(nt, it, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
            blocks[stfem.stokes_block_index(nt, it, 1, d)] = rng.uniform(-1, 1, orc.n_p)
            var[stfem.stokes_block_index(nt, it, 1, d)] = 1
    ref = (orc.st_Tvmult if transpose else orc.st_vmult)(Alpha, Beta, ns, nt, blocks)
    return Alpha, Beta, ns, nt, var, blocks, ref


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", ["kron", "dgp", "cell", "weak"])
def test_vmult_and_mass_vmult(name, placement, stfem, oracle_mod):
    """stfem_stokes_vmult, stfem_stokes_mass_vmult"""
    op, nc, verts, dg = make(stfem, name)
    ref = space_reference(name)
    src = [vec("u", ref["U"], nc), vec("p", ref["P"], nc, 1, dg)]
    guard_case(stfem, placement, src + [out("du", ref["U"].size, nc), out("dp", ref["P"].size, nc, 1, dg)],
               lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"]),
               {"du": within(ref["ku"]), "dp": within(ref["kp"], scale=np.linalg.norm(ref["kp"]) + 1e-14 / TOL)})
    guard_case(stfem, placement, src[:1] + [out("du", ref["U"].size, nc)], lambda ptr: op.mass_vmult(ptr["du"], ptr["u"]), {"du": within(ref["mu"])})


ST_CASES = [("kron", "cg2"), ("kron", "cg1x5"), ("sweep", "cg1"), ("dgp", "cg2"), ("cell", "cg2"), ("weak", "cg2")]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name,scheme", ST_CASES)
def test_st_vmult(name, scheme, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult: cG(2) fused with the gradient kernel; cG(1) with the gradient in the sweep; cG(1) x 5 steps, one launch set
    per source, destinations partly stored and partly added to"""
    op, nc, verts, dg = make(stfem, name)
    Alpha, Beta, ns, nt, var, blocks, ref = st_reference(name, scheme)
    nb = len(var)
    specs = [vec(f"s{j}", blocks[j], nc, var[j], dg) for j in range(nb)] + [out(f"d{j}", blocks[j].size, nc, var[j], dg) for j in range(nb)]

    def call(ptr):
        op.st_vmult(Alpha, Beta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)])

    def check():
        if name in ("kron", "sweep"):  # the Kronecker path's velocity sweep (a general mesh has no scalar context to ask)
            plan = op.last_sweep_plan
            assert plan[0] > 0 and plan[2] == (1 if scheme == "cg1" else 0), plan

    guard_case(stfem, placement, specs, call, {f"d{j}": within(ref[j], scale=np.linalg.norm(ref[j]) + 1e-14 / TOL) for j in range(nb)}, check=check)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", ["kron", "dgp", "cell", "weak"])
def test_st_Tvmult(name, placement, stfem, oracle_mod):
    """SystemMatrixStokes::Tvmult as the reference has it, run as one stfem_stokes_st_vmult with effective matrices; cG(2), two steps"""
    op, nc, verts, dg = make(stfem, name)
    orc = oracle_of(name)
    ns, r = 2, 2
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, r, 1.0 / 16, ns)
    nt, nb = r, 2 * r * ns
    rng = np.random.default_rng(6)
    var = [(j // nt) % 2 for j in range(nb)]
    blocks = [rng.uniform(-1, 1, 3 * orc.n_u if v == 0 else orc.n_p) for v in var]
    ref = orc.st_Tvmult(Alpha, Beta, ns, nt, blocks)
    assert any(np.linalg.norm(x) > 0 for x in ref)
    specs = [vec(f"s{j}", blocks[j], nc, var[j], dg) for j in range(nb)] + [out(f"d{j}", blocks[j].size, nc, var[j], dg) for j in range(nb)]
    guard_case(stfem, placement, specs,
               lambda ptr: op.st_Tvmult(Alpha, Beta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)]),
               {f"d{j}": within(ref[j], scale=max(np.linalg.norm(ref[j]), 1.0)) for j in range(nb)})  # test_stokes_reference_Tvmult


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", ["kron", "dgp", "cell", "weak"])
def test_st_vmult_slice_add(name, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult_slice_add onto seeded destinations, one Gamma entry zero"""
    op, nc, verts, dg = make(stfem, name)
    ref = space_reference(name)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 1, 0)] = 0.0
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    want = [init[j] + (Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"]) for j in range(nb)]
    specs = [vec("u", ref["U"], nc), vec("p", ref["P"], nc, 1, dg)] + [out(f"d{j}", init[j].size, nc, var[j], dg, seeded=init[j]) for j in range(nb)]
    guard_case(stfem, placement, specs, lambda ptr: op.st_vmult_slice_add(Gamma, Zeta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], ptr["u"], ptr["p"]),
               {f"d{j}": within(want[j]) for j in range(nb)})


# ------------------------------------------------------------------------------------------ convection modes

NAVIER = {"pert": ((3, 2, 4), 0.15), "cart": ((5, 4, 3), 0.0)}  # test_gpu_navier.py
NAVIER_NU, NAVIER_MASK = 0.3, 0b111011


def navier(stfem, mesh, dg=False, **kw):
    from oracle import oracle
    nc, distort = NAVIER[mesh]
    verts = stfem.mesh_vertices(nc, distort=distort, seed=77)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, dirichlet_mask=NAVIER_MASK, viscosity=NAVIER_NU, dg_pressure=dg, **kw)
    return op, oracle.StokesOracle(nc, verts, NAVIER_MASK, NAVIER_NU, dg_pressure=dg), nc, verts


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mode", [nref.FORM, nref.JACOBIAN], ids=["form", "jacobian"])
@pytest.mark.parametrize("mesh", list(NAVIER))
def test_convection_vmult_and_slice_add(mesh, mode, placement, stfem, oracle_mod):
    """stfem_stokes_vmult_convection, stfem_stokes_st_vmult_slice_add_convection: `lin` is a further source view"""
    op, orc, nc, verts = navier(stfem, mesh)
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = nref.vmult(orc, mode, B, U, P, nc, verts, NAVIER_MASK)
    src = [vec("u", U, nc), vec("p", P, nc, 1), vec("b", B, nc)]
    guard_case(stfem, placement, src + [out("du", U.size, nc), out("dp", P.size, nc, 1)],
               lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"], lin=ptr["b"], mode=mode),
               {"du": within(ku), "dp": within(kp, scale=np.linalg.norm(kp) + 1e-14 / TOL)})
    ns, nt = 2, 2
    nb = 2 * ns * nt
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 0, 0)] = 0.0
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, U.size if v == 0 else P.size) for v in var]
    want = [init[j] + (Gamma[j] * np.ravel(ku) + Zeta[j] * mu.reshape(-1) if var[j] == 0 else Gamma[j] * kp) for j in range(nb)]
    guard_case(stfem, placement, src + [out(f"d{j}", init[j].size, nc, var[j], seeded=init[j]) for j in range(nb)],
               lambda ptr: op.st_vmult_slice_add(Gamma, Zeta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], ptr["u"], ptr["p"], lin=ptr["b"], mode=mode),
               {f"d{j}": within(want[j]) for j in range(nb)})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mode", [nref.FORM, nref.JACOBIAN], ids=["form", "jacobian"])
@pytest.mark.parametrize("mesh", list(NAVIER))
def test_convection_st_vmult(mesh, mode, placement, stfem, oracle_mod):
    """stfem_stokes_st_vmult_convection, cG(2): a linearisation view per velocity block, null for the pressure blocks"""
    op, orc, nc, verts = navier(stfem, mesh, dg=(mesh == "cart"))
    dg = mesh == "cart"
    ns, nt = 1, 2
    nb = 2 * ns * nt
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d, True)  # noqa: E731
    rng = np.random.default_rng(9)
    blocks, lin, var = [None] * nb, [None] * nb, [0] * nb
    for d in range(nt):
        blocks[index(0, 0, d)], blocks[index(0, 1, d)] = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
        lin[index(0, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
        var[index(0, 1, d)] = 1
    ref = nref.st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, NAVIER_MASK, variable_major=True)
    specs = ([vec(f"s{j}", blocks[j], nc, var[j], dg) for j in range(nb)] + [vec(f"l{j}", lin[j], nc) for j in range(nb) if lin[j] is not None] +
             [out(f"d{j}", blocks[j].size, nc, var[j], dg) for j in range(nb)])

    def call(ptr):
        op.st_vmult(Alpha, Beta, ns, nt, [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)],
                    lin=[ptr.get(f"l{j}") for j in range(nb)], mode=mode)

    guard_case(stfem, placement, specs, call, {f"d{j}": within(ref[j], scale=np.linalg.norm(ref[j]) + 1e-14 / TOL) for j in range(nb)})


# ------------------------------------------------------------------------------------------ CIP

def cip_operator(stfem, mesh, mask, **kw):
    nc, lower, upper, distort = cref.MESHES[mesh]
    verts = cref.mesh_vertices(mesh)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, lower=lower, upper=upper, dirichlet_mask=mask, viscosity=cref.NU, **kw)
    return op, nc, verts


def field(nc, seed):
    return np.random.default_rng(seed).uniform(-1, 1, 3 * nref.n_velocity(nc))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_cip_add(mesh, placement, stfem):
    """stfem_stokes_cip_add onto a seeded destination, with a weight of its own and with the source as weight"""
    mask = 0b111011
    op, nc, verts = cip_operator(stfem, mesh, mask)
    delta0 = cref.delta0_of(mesh, mask)
    U, W, INIT = field(nc, cref.FIELD_SEED), field(nc, 6), field(nc, 7)
    ref = cref.cip(delta0, W, U, nc, verts, mask)
    assert np.linalg.norm(ref) > 0.1
    guard_case(stfem, placement, [vec("u", U, nc), vec("w", W, nc), out("d", U.size, nc, seeded=INIT)],
               lambda ptr: op.cip_add(ptr["d"], ptr["u"], ptr["w"], delta0), {"d": within(INIT + ref, scale=np.linalg.norm(ref))})
    ref = cref.cip(delta0, U, U, nc, verts, mask)
    guard_case(stfem, placement, [vec("u", U, nc), out("d", U.size, nc, seeded=INIT)],
               lambda ptr: op.cip_add(ptr["d"], ptr["u"], ptr["u"], delta0), {"d": within(INIT + ref, scale=np.linalg.norm(ref))})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("weight", [cref.SOURCE, cref.LINEARISATION], ids=["source", "linearisation"])
def test_vmult_with_cip(weight, placement, stfem, oracle_mod):
    """stfem_stokes_set_cip with both weights: the term inside stfem_stokes_vmult_convection (jacobian)"""
    from oracle import oracle
    mesh, mask, mode = "pert", 0b111011, nref.JACOBIAN
    delta0 = cref.delta0_of(mesh, mask)
    op, nc, verts = cip_operator(stfem, mesh, mask, delta0=delta0, cip_weight=weight)
    orc = oracle.StokesOracle(nc, verts, mask, cref.NU)
    rng = np.random.default_rng(cref.FIELD_SEED)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = cref.vmult(orc, delta0, weight, mode, B, U, P, nc, verts, mask)
    guard_case(stfem, placement, [vec("u", U, nc), vec("p", P, nc, 1), vec("b", B, nc), out("du", U.size, nc), out("dp", P.size, nc, 1)],
               lambda ptr: op.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"], lin=ptr["b"], mode=mode),
               {"du": within(ku), "dp": within(kp, scale=np.linalg.norm(kp) + 1e-14 / TOL)})


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_cip_on_a_slab(placement, stfem, oracle_mod):
    """A box slab of 3 x 2 x 4 cells with one neighbour above: stfem_stokes_cip_pack of the neighbour into an arena view,
    stfem_stokes_cip_add_slab reading it, stfem_stokes_cip_bind_ghosts + vmult with the term"""
    from oracle import oracle
    nc, delta0, nu = (3, 2, 4), 1.0, cref.NU
    whole = cref.box_vertices((3, 2, 8), (0, 0, 0), (1, 1, 1))
    strong_lo, strong_up = 63 & ~32, 63 & ~16
    v_lo, v_up = ssc.slab_vertices(whole, (3, 2, 8), 0, 4), ssc.slab_vertices(whole, (3, 2, 8), 4, 8)
    lo = stfem.StokesMatrixFreeOperator(nc, lower=(0, 0, 0), upper=(1, 1, 0.5), dirichlet_mask=strong_lo, viscosity=nu)
    up = stfem.StokesMatrixFreeOperator(nc, lower=(0, 0, 0.5), upper=(1, 1, 1), dirichlet_mask=strong_up, viscosity=nu)
    lo.set_cip_neighbours(csr.UPPER)
    up.set_cip_neighbours(csr.LOWER)
    n_ghost = lo.cip_ghost_size
    assert n_ghost == 6 * csr.plane_size(nc)
    U_lo, U_up, W, INIT = field(nc, 5), field(nc, 6), field(nc, 7), field(nc, 8)
    ghost = csr.pack(U_up, nc, strong_up, 0)
    # the neighbour packs its planes 1 and 2 into an arena view: bit for bit the numpy pack
    guard_case(stfem, placement, [vec("u", U_up, nc), Spec("ghost", poison(n_ghost, np.float64), "destination", (vshape(nc)[0], vshape(nc)[1], 6))],
               lambda ptr: up.cip_pack(ptr["u"], 0, ptr["ghost"]), {"ghost": lambda got: np.testing.assert_array_equal(got, ghost)})
    plane_beyond = np.asarray(whole).reshape(9, -1, 3)[5]
    term = csr.cip_slab(delta0, W, U_lo, nc, v_lo, strong_lo, mask=csr.UPPER, upper_ghost=ghost, upper_vertices=plane_beyond)
    inner = cref.cip(delta0, W, U_lo, nc, v_lo, strong_lo)
    assert np.linalg.norm(term - inner) > 1e-2 * np.linalg.norm(term)  # the interface faces are there
    gspec = Spec("ghost", ghost, "source", (vshape(nc)[0], vshape(nc)[1], 6))
    guard_case(stfem, placement, [vec("u", U_lo, nc), vec("w", W, nc), gspec, out("d", U_lo.size, nc, seeded=INIT)],
               lambda ptr: lo.cip_add_slab(ptr["d"], ptr["u"], ptr["w"], delta0, None, ptr["ghost"]),
               {"d": within(INIT + term, scale=np.linalg.norm(term))})
    # vmult with the term, the ghost planes bound to the source's pointer
    lo.set_cip(delta0, cref.SOURCE)
    orc = oracle.StokesOracle(nc, v_lo, strong_lo, nu)
    P = np.random.default_rng(9).uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U_lo, P)
    ku = ku.reshape(-1) + csr.cip_slab(delta0, U_lo, U_lo, nc, v_lo, strong_lo, mask=csr.UPPER, upper_ghost=ghost, upper_vertices=plane_beyond)

    def call(ptr):
        lo.cip_bind_ghosts(ptr["u"], None, ptr["ghost"])
        try:
            lo.vmult(ptr["du"], ptr["dp"], ptr["u"], ptr["p"])
        finally:
            lo.cip_bind_ghosts(ptr["u"], None, None)

    guard_case(stfem, placement, [vec("u", U_lo, nc), vec("p", P, nc, 1), gspec, out("du", U_lo.size, nc), out("dp", P.size, nc, 1)], call,
               {"du": within(ku), "dp": within(kp)})


# ------------------------------------------------------------------------------------------ functionals and helpers

@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mesh", ["box", "pert"])
def test_divergence(mesh, placement, stfem):
    """stfem_stokes_divergence with the per-cell output an arena view of n_cells doubles"""
    nc, distort, (lower, upper) = {"box": ((2, 3, 2), 0.0, ((0.0, -0.5, 0.25), (1.0, 0.25, 1.75))), "pert": ((3, 2, 2), 0.15, ((0, 0, 0), (1, 1, 1)))}[mesh]
    verts = stfem.mesh_vertices(nc, lower=lower, upper=upper, distort=distort, seed=77)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, lower=lower, upper=upper, dirichlet_mask=0b011101)
    u = np.random.default_rng(11).uniform(-1, 1, 3 * op.n_velocity)
    ref_cells, ref_total = nsr.divergence_cells(u, nc, verts)

    def returned(total):
        assert abs(total - ref_total) <= TOL * ref_total

    guard_case(stfem, placement, [vec("u", u, nc), Spec("cells", poison(op.n_cells, np.float64), "destination", nc)],
               lambda ptr: op.divergence(ptr["u"], cells=ptr["cells"]), {"cells": within(ref_cells)}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q1", "FE_DGP1"])
def test_drag_lift(dg, placement, stfem):
    """stfem_stokes_drag_lift: three (u, p) pairs in one call, the per-item output an arena view"""
    nc, nu, dmask, fmask, scale, npairs = (3, 2, 2), 0.7, 0b011101, 63, 1.75, 3
    verts = nref.perturbed_vertices(nc, 0.15, 77)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts, dirichlet_mask=dmask, viscosity=nu, dg_pressure=dg)
    rng = np.random.default_rng(21)
    U, P = [rng.uniform(-1, 1, 3 * op.n_velocity) for _ in range(npairs)], [rng.uniform(-1, 1, op.n_pressure) for _ in range(npairs)]
    want = [dref.drag_lift(u, p, nc, verts, nu, fmask, dirichlet_mask=dmask, dg_pressure=dg, scale=scale) for u, p in zip(U, P)]
    nitems, A = op.drag_lift_n_items(fmask), want[0][2]
    assert nitems == len(want[0][1])
    specs = ([vec(f"u{i}", U[i], nc) for i in range(npairs)] + [vec(f"p{i}", P[i], nc, 1, dg) for i in range(npairs)] +
             [Spec("items", poison(npairs * nitems * 3, np.float64), "destination")])

    def call(ptr):
        force = np.zeros((npairs, 3))
        stfem._check(stfem.lib().stfem_stokes_drag_lift(op._h, fmask, scale, 0, npairs, (C.c_void_p * npairs)(*[ptr[f"u{i}"] for i in range(npairs)]),
                                                        (C.c_void_p * npairs)(*[ptr[f"p{i}"] for i in range(npairs)]), ptr["items"], stfem._p(force), None),
                     "stfem_stokes_drag_lift")
        return force.ravel()

    def items(got):
        assert np.max(np.abs(got.reshape(npairs, nitems, 3) - np.stack([w[1] for w in want]))) <= TOL * A  # test_parity_random_fields

    def returned(force):
        assert np.max(np.abs(force.reshape(npairs, 3) - np.stack([w[0] for w in want]))) <= TOL * scale * A

    guard_case(stfem, placement, specs, call, {"items": items}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_nitsche_rhs(placement, stfem, oracle_mod):
    """stfem_stokes_nitsche_rhs accumulates into both destinations"""
    op, nc, verts, dg = make(stfem, "weak")
    orc = oracle_of("weak")
    pts = orc.face_points()
    assert np.abs(op.face_points() - pts).max() < 1e-13
    G = np.stack([np.sin(pts[:, 0] + 2 * pts[:, 1]), pts[:, 2] ** 2 - pts[:, 0], np.cos(pts[:, 1] * pts[:, 2])], axis=1)
    ru, rp = orc.nitsche_rhs(G)
    rng = np.random.default_rng(3)
    iu, ip = rng.uniform(-1, 1, ru.size) * np.abs(ru).max(), rng.uniform(-1, 1, rp.size) * np.abs(rp).max()
    guard_case(stfem, placement, [out("fu", iu.size, nc, seeded=iu), out("fp", ip.size, nc, 1, seeded=ip)],
               lambda ptr: op.nitsche_rhs(G, ptr["fu"], ptr["fp"]),
               {"fu": within(iu + ru.reshape(-1), scale=np.linalg.norm(ru)), "fp": within(ip + rp, scale=np.linalg.norm(rp))})


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q1", "FE_DGP1"])
def test_pressure_difference(dg, placement, stfem):
    from oracle import driver_oracle as D
    nc, lower, upper, nq = (4, 2, 6), (0.0, 0.0, 0.0), (1.0, 0.7, 1.3), 3  # test_pressure_helpers
    op = stfem.StokesMatrixFreeOperator(nc, lower=lower, upper=upper, dg_pressure=dg)
    rng = np.random.default_rng(4)
    coeffs, exact = rng.uniform(-1, 1, op.n_pressure), rng.uniform(-1, 1, (op.n_cells, nq ** 3))
    ref = D.pressure_difference(nc, D.box_vertices(nc, lower, upper), nq, coeffs, exact, dg)

    def returned(got):
        assert abs(got[0] - ref[0]) <= 1e-12 * ref[0] and abs(got[1] - ref[1]) <= 1e-13 * ref[1], (got, ref)

    guard_case(stfem, placement, [vec("p", coeffs, nc, 1, dg)], lambda ptr: op.pressure_difference(nq, ptr["p"], exact), {}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_load_vector_and_error_norms_on_component_blocks(placement, stfem):
    """stfem_integrate_rhs_product / stfem_integrate_difference_product on the three components of ONE velocity view, wrapped as the blocks
    of a scalar FE_Q(2) vector: block c starts at base + c Nu, Nu odd"""
    from oracle import driver_oracle as D
    nc, mask, nq, amplitude, frequency = (3, 2, 4), 0b100110, 3, -0.7, 1.0
    verts = D.box_vertices(nc, (0, 0, 0), (1, 1, 1))
    op = stfem.StokesMatrixFreeOperator(nc, dirichlet_mask=mask)
    ctx = stfem.MatrixFreeOperator(2, nc, dirichlet_mask=mask)
    nu_ = op.n_velocity
    assert ctx.n_dofs == nu_ and nu_ % 2 == 1
    w = 2.0 * np.pi * frequency
    pts = stfem.quadrature_points(ctx, nq)
    s, c = np.sin(w * pts), np.cos(w * pts)
    val = amplitude * s[..., 0] * s[..., 1] * s[..., 2]
    grad = amplitude * w * np.stack([c[..., 0] * s[..., 1] * s[..., 2], s[..., 0] * c[..., 1] * s[..., 2], s[..., 0] * s[..., 1] * c[..., 2]], axis=-1)
    U = np.random.default_rng(5).uniform(-1, 1, 3 * nu_)

    def components(ptr, name):
        return stfem.BlockVector(ctx, device_ptrs=[ptr[name] + 8 * nu_ * comp for comp in range(3)])

    want = U.copy()
    want[nu_:2 * nu_] = D.load_vector(2, nc, verts, nq, val, mask)
    guard_case(stfem, placement, [out("u", U.size, nc, seeded=U)], lambda ptr: stfem.integrate_rhs_product(ctx, nq, amplitude, frequency, components(ptr, "u"), block=1),
               {"u": within(want, scale=np.linalg.norm(want[nu_:2 * nu_]))})
    ref = D.difference(2, nc, verts, nq, U[2 * nu_:], val, grad)

    def returned(got):
        assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0]) and abs(got[1] - ref[1]) <= 1e-13 * abs(ref[1]) and abs(got[2] - ref[2]) <= 1e-12 * abs(ref[2]), (got, ref)

    guard_case(stfem, placement, [vec("u", U, nc)], lambda ptr: stfem.integrate_difference_product(ctx, nq, components(ptr, "u"), 2, amplitude, frequency), {},
               returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("add", [False, True], ids=["overwrite", "add"])
def test_dgp_transfers(add, placement, stfem):
    """stfem_stokes_dgp_prolongate / _restrict between 3 x 2 x 2 and 6 x 4 x 4 cells"""
    from oracle import driver_oracle as D
    nf, ncoarse = (6, 4, 4), (3, 2, 2)
    fine, coarse = stfem.StokesMatrixFreeOperator(nf, dg_pressure=True), stfem.StokesMatrixFreeOperator(ncoarse, dg_pressure=True)
    rng = np.random.default_rng(6)
    c, f = rng.uniform(-1, 1, coarse.n_pressure), rng.uniform(-1, 1, fine.n_pressure)
    yf, yc = rng.uniform(-1, 1, fine.n_pressure), rng.uniform(-1, 1, coarse.n_pressure)
    Pm = np.stack([D.dgp_prolongate(nf, e) for e in np.eye(coarse.n_pressure)], axis=1)  # the embedding, column by column
    Pc, Rf = Pm @ c, Pm.T @ f
    guard_case(stfem, placement, [vec("c", c, ncoarse, 1, True), out("f", f.size, nf, 1, True, seeded=yf if add else None)],
               lambda ptr: stfem.stokes_dgp_prolongate(fine, coarse, ptr["f"], ptr["c"], add=add), {"f": within(yf + Pc if add else Pc, scale=np.linalg.norm(Pc))})
    guard_case(stfem, placement, [vec("f", f, nf, 1, True), out("c", c.size, ncoarse, 1, True, seeded=yc if add else None)],
               lambda ptr: stfem.stokes_dgp_restrict(fine, coarse, ptr["c"], ptr["f"], add=add), {"c": within(yc + Rf if add else Rf, scale=np.linalg.norm(Rf))})


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_vector_upload_download_on_raw_pointers(placement, stfem):
    """stfem_stokes_vector_upload / _download take any device pointer of the variable's length"""
    op = stfem.StokesMatrixFreeOperator((3, 2, 2))
    nc, L, rng = (3, 2, 2), stfem.lib(), np.random.default_rng(7)
    U, P, X, Y = rng.uniform(-1, 1, 3 * op.n_velocity), rng.uniform(-1, 1, op.n_pressure), rng.uniform(-1, 1, 3 * op.n_velocity), rng.uniform(-1, 1, op.n_pressure)

    def call(ptr):
        gu, gp = np.zeros(U.size), np.zeros(P.size)
        stfem._check(L.stfem_stokes_vector_download(op._h, 0, ptr["u"], stfem._p(gu)), "stfem_stokes_vector_download")
        stfem._check(L.stfem_stokes_vector_download(op._h, 1, ptr["p"], stfem._p(gp)), "stfem_stokes_vector_download")
        stfem._check(L.stfem_stokes_vector_upload(op._h, 0, ptr["x"], stfem._p(X)), "stfem_stokes_vector_upload")
        stfem._check(L.stfem_stokes_vector_upload(op._h, 1, ptr["y"], stfem._p(Y)), "stfem_stokes_vector_upload")
        return np.concatenate([gu, gp])

    guard_case(stfem, placement, [vec("u", U, nc), vec("p", P, nc, 1), out("x", X.size, nc), out("y", Y.size, nc, 1)], call,
               {"x": lambda got: np.testing.assert_array_equal(got, X), "y": lambda got: np.testing.assert_array_equal(got, Y)},
               returned=lambda got: np.testing.assert_array_equal(got, np.concatenate([U, P])))


# ------------------------------------------------------------------------------------------ the Stokes Vanka smoother

def vanka_checks(stfem, placement, V, p_var, sizes, nc, dg, X, want, extra_sources=()):
    """vmult, an overwriting and an accumulating step on arena views in BlockSlice order"""
    nb = len(p_var)
    src = [vec(f"s{j}", X[j], nc, p_var[j], dg) for j in range(nb)] + list(extra_sources)
    D0 = [np.random.default_rng(20 + j).uniform(-1, 1, sizes[j]) for j in range(nb)]
    whole = np.linalg.norm(np.concatenate(want))

    def dsts(seeded):
        return [out(f"d{j}", sizes[j], nc, p_var[j], dg, seeded=D0[j] if seeded else None) for j in range(nb)]

    def args(ptr):
        return [ptr[f"d{j}"] for j in range(nb)], [ptr[f"s{j}"] for j in range(nb)]

    def overall(parts, factor, base):
        got = np.concatenate([parts[f"d{j}"] for j in range(nb)])
        ref = np.concatenate([(base[j] if base else 0.0) + factor * want[j] for j in range(nb)])
        assert np.linalg.norm(got - ref) <= TOL_VANKA * factor * whole

    # per block 1e-9 (test_stokes_vanka_vs_oracle) resp. 1e-10 (the per-cell files); overall 1e-10
    per_block = 1e-9 if V.setup_batches == 0 else TOL_VANKA

    def vmult(ptr):  # (the Python vmult goes through the step: the entry point itself)
        d, s = ((C.c_void_p * nb)(*a) for a in args(ptr))
        stfem._check(stfem.lib().stfem_stokes_vanka_vmult(V._h, d, s, None), "stfem_stokes_vanka_vmult")

    plain = guard_case(stfem, placement, src + dsts(False), vmult, {f"d{j}": within(want[j], per_block) for j in range(nb)})
    overall(plain, 1.0, None)
    plain = guard_case(stfem, placement, src + dsts(False), lambda ptr: V.step(args(ptr)[0], 0.6, False, args(ptr)[1]),
                       {f"d{j}": within(0.6 * want[j], per_block) for j in range(nb)})
    overall(plain, 0.6, None)
    plain = guard_case(stfem, placement, src + dsts(True), lambda ptr: V.step(args(ptr)[0], 0.6, True, args(ptr)[1]),
                       {f"d{j}": within(D0[j] + 0.6 * want[j], per_block, scale=0.6 * np.linalg.norm(want[j])) for j in range(nb)})
    overall(plain, 0.6, D0)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_stokes_vanka_class_blocks(placement, stfem, oracle_mod):
    """stfem_stokes_vanka_create / _vmult / _step: class blocks on a 3 x 2 x 3 box, cG(2)"""
    from oracle import vanka_oracle
    nc, mask, nu, nt = (3, 2, 3), 63, 0.7, 2
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 0.05, 1)
    var = [0, 0, 1, 1]
    op = stfem.StokesMatrixFreeOperator(nc, dirichlet_mask=mask, viscosity=nu)
    V = stfem.StokesPreconditionVanka(op, var, Alpha, Beta)
    assert V.n_classes == 18 and V.setup_batches == 0
    ref = vanka_oracle.StokesVankaOracle(nc, stfem.mesh_vertices(nc), mask, nu, var, Alpha, Beta)
    sizes = [3 * op.n_velocity if v == 0 else op.n_pressure for v in var]
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in sizes]
    vanka_checks(stfem, placement, V, var, sizes, nc, False, X, ref.vmult(X))


def stokes_problem_operator(stfem, p):
    return stfem.StokesMatrixFreeOperator(p.nc, vertices=p.verts if p.pert else None, dirichlet_mask=p.mask, viscosity=p.nu,
                                          weak_boundary_ids=faces(p.weak), dg_pressure=p.dg)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("delta0", [0.0, scr.DELTA0], ids=["plain", "cip"])
def test_stokes_vanka_per_cell_blocks(delta0, placement, stfem, oracle_mod):
    """stfem_stokes_vanka_create_linearised / _create_linearised_cip / _update on a perturbed 3 x 2 x 2 mesh (jacobian, cG(2),
    time-major blocks, weak x faces): the linearisation states are arena views the set-up reads; then vmult and step"""
    p, base, with_term = scr.case("pert322_jac_weak")
    ref = with_term if delta0 else base
    op = stokes_problem_operator(stfem, p)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    want = ref.vmult(X)
    states = [j for j in range(p.nb) if p.lin[j] is not None]
    lin_specs = [vec(f"l{j}", p.lin[j], p.nc) for j in states]
    specs = lin_specs + [vec(f"s{j}", X[j], p.nc, p.var[j], p.dg) for j in range(p.nb)] + [out(f"d{j}", p.sizes[j], p.nc, p.var[j], p.dg) for j in range(p.nb)]
    keep = {}

    def create_and_apply(ptr):
        V = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=[ptr.get(f"l{j}") for j in range(p.nb)], mode=p.mode, per_cell=True, delta0=delta0)
        assert V.n_classes == int(np.prod(p.nc)) and V.setup_batches >= 1
        V.vmult([ptr[f"d{j}"] for j in range(p.nb)], [ptr[f"s{j}"] for j in range(p.nb)])
        keep["V"] = V

    guard_case(stfem, placement, specs, create_and_apply, {f"d{j}": within(want[j], TOL_VANKA) for j in range(p.nb)})
    # (the blocks are the smoother's own storage: the states may go) vmult and step of the last smoother, all blocks in the arena
    vanka_checks(stfem, placement, keep["V"], p.var, p.sizes, p.nc, p.dg, X, want)
    # update with other states, again read from arena views
    other = scr.other_states("pert322_jac_weak")
    ref2 = svr.reference(p, lin=other)
    want2 = (scr.with_cip(ref2, p, delta0, other) if delta0 else ref2).vmult(X)
    specs2 = [vec(f"l{j}", other[j], p.nc) for j in states] + specs[len(lin_specs):]

    def update_and_apply(ptr):
        keep["V"].update([ptr.get(f"l{j}") for j in range(p.nb)])
        keep["V"].vmult([ptr[f"d{j}"] for j in range(p.nb)], [ptr[f"s{j}"] for j in range(p.nb)])

    guard_case(stfem, placement, specs2, update_and_apply, {f"d{j}": within(want2[j], TOL_VANKA) for j in range(p.nb)})


@pytest.mark.parametrize("placement", ["packed"])
def test_stokes_vanka_eight_blocks(placement, stfem, oracle_mod):
    """vmult and step on eight blocks in BlockSlice order (dG(1), two steps at once, FE_DGP(1) pressure, jacobian), packed"""
    p, ref = svr.case("box222_jac_dgp_2steps")
    assert p.nb == 8
    op = stokes_problem_operator(stfem, p)
    dlin = [op.initialize_dof_vector(0, x) if x is not None else None for x in p.lin]
    V = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=dlin, mode=p.mode, per_cell=True)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    vanka_checks(stfem, placement, V, p.var, p.sizes, p.nc, p.dg, X, ref.vmult(X))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_stokes_vanka_on_slabs(placement, stfem, oracle_mod):
    """stfem_stokes_vanka_create_linearised_partitioned: the two slabs of a perturbed 2 x 2 x 4 mesh cut at layer 2, each with its
    states on the extended context as arena views; the slabs' results sum to the whole-mesh smoother with the CIP term"""
    name, bounds = "pert224_jac", (0, 2, 4)
    p = svr.problem(csr.VANKA_SLAB_SPECS[name])
    ref = scr.with_cip(svr.reference(p), p, scr.DELTA0, p.lin)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    want = ref.vmult(X)
    parts = []
    for r in range(2):
        z0, z1 = bounds[r], bounds[r + 1]
        lo, hi = r > 0, r < 1
        e0, e1 = z0 - lo, z1 + hi
        neighbours = (16 if lo else 0) | (32 if hi else 0)
        beyond = (16 if lo and e0 > 0 else 0) | (32 if hi and e1 < p.nc[2] else 0)

        def operator(a, b):
            strong, weak, _ = ssc.slab_masks(p.mask, p.weak, 0, a > 0, b < p.nc[2])
            return stfem.StokesMatrixFreeOperator((p.nc[0], p.nc[1], b - a), vertices=ssc.slab_vertices(p.verts, p.nc, a, b), lower=(0, 0, a / p.nc[2]),
                                                  upper=(1, 1, b / p.nc[2]), dirichlet_mask=strong, viscosity=p.nu, weak_boundary_ids=ssc.faces_of(weak),
                                                  dg_pressure=p.dg)

        op, ext = operator(z0, z1), operator(e0, e1)
        snc, enc = (p.nc[0], p.nc[1], z1 - z0), (p.nc[0], p.nc[1], e1 - e0)
        lin = [None if x is None else ssc.cut(x, v, p.dg, p.nc, e0, e1) for x, v in zip(p.lin, p.var)]
        Xs = [ssc.cut(x, v, p.dg, p.nc, z0, z1) for x, v in zip(X, p.var)]
        specs = ([vec(f"l{j}", lin[j], enc) for j in range(p.nb) if lin[j] is not None] + [vec(f"s{j}", Xs[j], snc, p.var[j], p.dg) for j in range(p.nb)] +
                 [out(f"d{j}", Xs[j].size, snc, p.var[j], p.dg) for j in range(p.nb)])

        def call(ptr):
            V = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=[ptr.get(f"l{j}") for j in range(p.nb)], mode=p.mode, delta0=scr.DELTA0,
                                              partition=(ext, neighbours, beyond))
            assert V.n_classes == p.nc[0] * p.nc[1] * (z1 - z0) and V.setup_batches == 1
            V.vmult([ptr[f"d{j}"] for j in range(p.nb)], [ptr[f"s{j}"] for j in range(p.nb)])

        # (a slab by itself has no reference: its destinations are collected and summed with the other slab's below)
        plain = guard_case(stfem, placement, specs, call, {f"d{j}": BY_CALLER for j in range(p.nb)})
        parts.append([plain[f"d{j}"].copy() for j in range(p.nb)])
    Y = [ssc.assemble([q[b] for q in parts], v, p.dg, p.nc, bounds) for b, v in enumerate(p.var)]
    assert ssc.rel(np.concatenate(Y), np.concatenate(want)) <= TOL_VANKA
    assert max(ssc.rel(Y[b], want[b]) for b in range(p.nb)) <= TOL_VANKA
