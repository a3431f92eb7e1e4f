"""GPU parity of the Stokes two-field operator at velocity degree 3, FE_Q(3)^3 x FE_Q(2) / FE_DGP(2) with QGauss(4)
(stfem_stokes_create_space, csrc/stfem_stokes_cell.hip at DEG = 3): against the dense numpy fixtures tests/golden/stokes_q3_*.npz and
against the CPU oracle at pu = 3.  Tolerance rel-L2 <= 1e-12 per block (fp64).  The largest mesh has 6^3 cells."""
import ctypes as C
import functools
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-12
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["stokes_q3_cart_2x2x2", "stokes_q3_pert_2x3x2", "stokes_q3_free_3x2x2"]
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)


def vertices_of(stfem, nc, distort, seed):
    return stfem.mesh_vertices(nc, distort=distort, seed=seed) if distort else stfem.mesh_vertices(nc)


@functools.lru_cache(maxsize=None)
def oracle_of(nc, distort, seed, mask, nu, dgp):
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    return oracle.StokesOracle(nc, vertices_of(stfem, nc, distort, seed), mask, nu, pu=3, dg_pressure=dgp)


@functools.lru_cache(maxsize=None)
def space_reference(nc, distort, seed, mask, nu, dgp):
    """one random (u, p) and the oracle's K_S (u, p) and M u, computed once and shared"""
    orc = oracle_of(nc, distort, seed, mask, nu, dgp)
    rng = np.random.default_rng(21)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    res = dict(U=U, P=P, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1))
    for v in res.values():
        v.setflags(write=False)
    return res


def operator(stfem, nc, distort, seed, mask, nu, dgp, box=False):
    verts = None if box else vertices_of(stfem, nc, distort, seed)
    return stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=verts, dirichlet_mask=mask, viscosity=nu, dg_pressure=dgp)


def time_blocks(stfem, orc, Alpha_vm, Beta_vm, ns, nt, variable_major, seed):
    """Alpha, Beta in the requested BlockSlice ordering and random source blocks"""
    nb = 2 * nt * ns
    perm = np.zeros(nb, dtype=int)
    for it in range(ns):
        for v in range(2):
            for d in range(nt):
                perm[stfem.stokes_block_index(nt, it, v, d, variable_major)] = stfem.stokes_block_index(nt, it, v, d, True)
    Alpha, Beta = Alpha_vm[np.ix_(perm, perm)], Beta_vm[np.ix_(perm, perm)]
    rng = np.random.default_rng(seed)
    blocks, var = [None] * nb, [0] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[stfem.stokes_block_index(nt, it, 0, d, variable_major)] = rng.uniform(-1, 1, 3 * orc.n_u)
            blocks[stfem.stokes_block_index(nt, it, 1, d, variable_major)] = rng.uniform(-1, 1, orc.n_p)
            var[stfem.stokes_block_index(nt, it, 1, d, variable_major)] = 1
    return Alpha, Beta, blocks, var


def run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var, variable_major=True, transpose=False):
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]  # st_vmult overwrites
    (op.st_Tvmult if transpose else op.st_vmult)(Alpha, Beta, ns, nt, dst, src, variable_major)
    return [d.download() for d in dst]


# ---- 1. the dense numpy fixtures
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixture(name, dgp, stfem):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sfx = "_dgp" if dgp else ""
    op = stfem.StokesMatrixFreeOperator.with_degree(3, tuple(int(v) for v in g["ncell"]), vertices=g["vertices"], dirichlet_mask=int(g["mask"]),
                                                    viscosity=float(g["nu"]), dg_pressure=dgp)
    nt = int(g["nt"])
    assert op.velocity_degree == 3 and op.n_velocity == g["U"].shape[2] and op.n_pressure == g["P" + sfx].shape[1]
    for i in range(nt):
        u, p = op.initialize_dof_vector(0, g["U"][i]), op.initialize_dof_vector(1, g["P" + sfx][i])
        ou = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, 7.0))   # vmult overwrites
        opr = op.initialize_dof_vector(1, np.full(op.n_pressure, -3.0))
        op.vmult(ou, opr, u, p)
        mu = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, 5.0))
        op.mass_vmult(mu, u)
        errs = rel(ou.download(), g["SU" + sfx][i]), rel(opr.download(), g["SP" + sfx][i]), rel(mu.download(), g["MU"][i])
        print(name, sfx, i, "vmult u %.2e p %.2e mass %.2e" % errs)
        assert max(errs) < TOL
    blocks = [g["U"][d].reshape(-1) for d in range(nt)] + [g["P" + sfx][d] for d in range(nt)]
    got = run_st_vmult(op, g["Alpha"], g["Beta"], 1, nt, blocks, [0] * nt + [1] * nt)
    for d in range(nt):
        errs = rel(got[d], g["DU" + sfx][d]), rel(got[nt + d], g["DP" + sfx][d])
        print(name, sfx, d, "st_vmult u %.2e p %.2e" % errs)
        assert max(errs) < TOL


# ---- 2. the oracle on shapes where the kernel can go wrong
SHAPES = [
    # cells, distortion, seed, mask, viscosity, box (created without vertices)
    ((5, 4, 6), 0.15, 77, 0b111011, 0.3, False),  # colour populations 18, 12, ...: none a multiple of the four cells of a workgroup
    ((1, 3, 2), 0.1, 5, 0, 0.7, False),           # empty colours, a one-cell direction, nothing constrained
    ((4, 1, 1), 0.0, 0, 63, 0.7, True),           # a box: the constant diagonal Jacobian
]


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("nc,distort,seed,mask,nu,box", SHAPES, ids=["5x4x6", "1x3x2", "4x1x1box"])
def test_vs_oracle(nc, distort, seed, mask, nu, box, dgp, stfem, oracle_mod):
    orc = oracle_of(nc, distort, seed, mask, nu, dgp)
    ref = space_reference(nc, distort, seed, mask, nu, dgp)
    op = operator(stfem, nc, distort, seed, mask, nu, dgp, box)
    assert (op.n_velocity, op.n_pressure) == (orc.n_u, orc.n_p)
    u, p = op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"])
    ou, opr = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, 7.0)), op.initialize_dof_vector(1, np.full(op.n_pressure, -3.0))
    op.vmult(ou, opr, u, p)
    m = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, 5.0))
    op.mass_vmult(m, u)
    errs = rel(ou.download(), ref["ku"]), rel(opr.download(), ref["kp"]), rel(m.download(), ref["mu"])
    print(nc, dgp, "vmult u %.2e p %.2e mass %.2e" % errs)
    assert max(errs) < TOL
    Alpha_vm, Beta_vm, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    Alpha, Beta, blocks, var = time_blocks(stfem, orc, Alpha_vm, Beta_vm, 1, 2, True, 8)
    want = orc.st_vmult(Alpha, Beta, 1, 2, blocks, True)
    got = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    for j in range(4):
        print(nc, dgp, j, "st_vmult %.2e" % rel(got[j], want[j]))
        assert np.linalg.norm(want[j]) > 0 and rel(got[j], want[j]) < TOL, j


# ---- 3. every launch shape of the launch description
LAUNCH = ((3, 4, 2), 0.1, 3, 63, 1.7)
SCHEMES = {"cg2x1": ("CGP", 2, 1), "dg2x1": ("DG", 2, 1), "cg2x2": ("CGP", 2, 2), "cg2x3": ("CGP", 2, 3)}


@functools.lru_cache(maxsize=None)
def launch_reference(scheme, variable_major, dgp):
    stfem = importlib.import_module("dealii-stfem_amd")
    kind, r, ns = SCHEMES[scheme]
    orc = oracle_of(*LAUNCH, dgp)
    Alpha_vm, Beta_vm, _, _ = stfem.get_fe_time_weights_stokes(getattr(stfem, kind), r, 1.0 / 16, ns)
    nt = Alpha_vm.shape[0] // (2 * ns)
    Alpha, Beta, blocks, var = time_blocks(stfem, orc, Alpha_vm, Beta_vm, ns, nt, variable_major, 100 * r + ns)
    return Alpha, Beta, ns, nt, blocks, var, orc.st_vmult(Alpha, Beta, ns, nt, blocks, variable_major)


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("variable_major", [True, False])
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_st_vmult_launch_shapes(scheme, variable_major, dgp, stfem, oracle_mod):
    """cG(2) x 1 step: 2 sources in one set; dG(2) x 1: 3 sources; cG(2) x 2: 4 sources, as many as one set takes; cG(2) x 3: 6 sources,
    one set per source whose destinations are partly overwritten and partly accumulated into.  Both BlockSlice orderings.
    (STFEM_STOKES_FUSED is read once per process, not per call: the unfused run of the short schemes is left out.)"""
    Alpha, Beta, ns, nt, blocks, var, want = launch_reference(scheme, variable_major, dgp)
    assert ns * nt == {"cg2x1": 2, "dg2x1": 3, "cg2x2": 4, "cg2x3": 6}[scheme]
    op = operator(stfem, *LAUNCH, dgp)
    got = run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var, variable_major)
    for j in range(len(blocks)):
        print(scheme, variable_major, dgp, j, "%.2e" % rel(got[j], want[j]))
        assert np.linalg.norm(want[j]) > 0 and rel(got[j], want[j]) < TOL, j


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_st_vmult_slice_add(dgp, stfem, oracle_mod):
    """random Gamma / Zeta with one exact zero, onto non-zero destinations"""
    ref = space_reference(*LAUNCH, dgp)
    op = operator(stfem, *LAUNCH, dgp)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 1, 0)] = 0.0  # a skipped entry
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    dst = [op.initialize_dof_vector(v, x) for v, x in zip(var, init)]
    op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"]))
    for j in range(nb):
        want = init[j] + (Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"])
        assert rel(dst[j].download(), want) < TOL, j
    assert np.array_equal(dst[stfem.stokes_block_index(nt, 1, 1, 0)].download(), init[stfem.stokes_block_index(nt, 1, 1, 0)])


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_reference_Tvmult(dgp, stfem, oracle_mod):
    """SystemMatrixStokes::Tvmult as the reference has it, through st_vmult with effective matrices"""
    orc = oracle_of(*LAUNCH, dgp)
    op = operator(stfem, *LAUNCH, dgp)
    ns, nt = 2, 2
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    _, _, blocks, var = time_blocks(stfem, orc, Alpha, Beta, ns, nt, True, 6)
    want = orc.st_Tvmult(Alpha, Beta, ns, nt, blocks)
    got = run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var, transpose=True)
    assert any(np.linalg.norm(w) > 0 for w in want)
    for j in range(len(blocks)):
        assert np.linalg.norm(got[j] - want[j]) <= TOL * max(np.linalg.norm(want[j]), 1.0), j  # (the bound of test_stokes_reference_Tvmult)


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_alpha_with_a_zero_pressure_row(dgp, stfem, oracle_mod):
    """a pressure destination none of whose weights is non-zero is not part of the launch (its pointer is null there) and is zeroed"""
    orc = oracle_of(*LAUNCH, dgp)
    op = operator(stfem, *LAUNCH, dgp)
    ns, nt = 1, 2
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    Alpha = Alpha.copy()
    Alpha[stfem.stokes_block_index(nt, 0, 1, 1), :] = 0.0
    _, _, blocks, var = time_blocks(stfem, orc, Alpha, Beta, ns, nt, True, 9)
    want = orc.st_vmult(Alpha, Beta, ns, nt, blocks, True)
    got = run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var)
    for j in range(len(blocks)):
        if j == stfem.stokes_block_index(nt, 0, 1, 1):
            assert np.all(got[j] == 0.0) and np.all(want[j] == 0.0)
        else:
            assert rel(got[j], want[j]) < TOL, j


# ---- 4. several cells per wave, 5. reproducibility
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_several_cells_per_wave_and_reproducible(dgp, stfem, oracle_mod, monkeypatch):
    """6^3 cells with the colour launches capped at one workgroup: colour 0 has 27 cells on 4 waves.  The result equals the uncapped
    run bit for bit (the cell -> wave assignment changes no sum), a repeated run equals the first bit for bit, and it is the oracle's."""
    case = ((6, 6, 6), 0.12, 9, 0b011110, 0.9)
    orc = oracle_of(*case, dgp)
    op = operator(stfem, *case, dgp)
    Alpha_vm, Beta_vm, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    Alpha, Beta, blocks, var = time_blocks(stfem, orc, Alpha_vm, Beta_vm, 1, 2, True, 4)
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2)).last_cell_plan()  # a context that has not launched the kernel
    assert e.value.status == -2
    free = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    plan = op.last_cell_plan()
    assert plan == (7, 1), plan  # colour 7: 27 cells, one per wave
    again = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")
    capped = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    plan = op.last_cell_plan()
    assert plan[0] == 1 and plan[1] >= 2, plan
    want = orc.st_vmult(Alpha, Beta, 1, 2, blocks, True)
    for j in range(4):
        assert np.array_equal(again[j], free[j]), j
        assert np.array_equal(capped[j], free[j]), j
        assert rel(free[j], want[j]) < TOL, j


# ---- 6. the two constructors at degree 2
@pytest.mark.parametrize("dgp", DGP, ids=["FE_Q1", "FE_DGP1"])
@pytest.mark.parametrize("box", [True, False], ids=["box", "perturbed"])
def test_degree_2_equals_the_old_constructor(box, dgp, stfem):
    nc, mask, nu = (3, 4, 2), 0b111011, 0.6
    kw = dict(vertices=None if box else stfem.mesh_vertices(nc, distort=0.1, seed=3), dirichlet_mask=mask, viscosity=nu, dg_pressure=dgp)
    old, new = stfem.StokesMatrixFreeOperator(nc, **kw), stfem.StokesMatrixFreeOperator.with_degree(2, nc, **kw)
    assert (old.n_velocity, old.n_pressure) == (new.n_velocity, new.n_pressure) and new.velocity_degree == 2
    rng = np.random.default_rng(2)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    blocks = [rng.uniform(-1, 1, 3 * old.n_velocity) for _ in range(2)] + [rng.uniform(-1, 1, old.n_pressure) for _ in range(2)]
    var = [0, 0, 1, 1]
    res = []
    for op in (old, new):
        ou, opr = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
        op.vmult(ou, opr, op.initialize_dof_vector(0, blocks[0]), op.initialize_dof_vector(1, blocks[2]))
        res.append([ou.download(), opr.download()] + run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var))
    assert np.linalg.norm(res[0][0]) > 0
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 7. refusals
SENTINEL = -123.25


def test_constructor_refusals(stfem):
    for degree in (1, 4):
        with pytest.raises(stfem.StfemError) as e:
            stfem.StokesMatrixFreeOperator.with_degree(degree, (2, 2, 2))
        assert e.value.status == -2 and stfem.lib().stfem_last_error()
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2), reserved=(0, 0, 1, 0))
    assert e.value.status in (-1, -2) and b"reserved" in stfem.lib().stfem_last_error()
    for kw in (dict(weak_boundary_ids=[0]), dict(outflow_boundary_ids=[3]), dict(delta0=0.1)):
        with pytest.raises(stfem.StfemError) as e:
            stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2), **kw)
        assert e.value.status == -2 and b"velocity degree 2 only" in stfem.lib().stfem_last_error()
    op = stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2))
    u, p = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
    with pytest.raises(stfem.StfemError) as e:
        op.vmult(u, p, u, p)
    assert e.value.status == -6  # STFEM_ERR_ALIAS as before


def test_every_other_entry_point_refuses(stfem):
    """On a degree-3 context every entry point outside the linear cell operator returns STFEM_ERR_UNSUPPORTED with a reason and
    leaves a sentinel-filled destination untouched"""
    L = stfem.lib()
    nc = (2, 2, 2)
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, dg_pressure=True)
    other = stfem.StokesMatrixFreeOperator.with_degree(3, (1, 1, 1), dg_pressure=True)
    q2 = stfem.StokesMatrixFreeOperator((2, 2, 2), dg_pressure=True)
    h = op._h
    rng = np.random.default_rng(1)
    u, p = op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)), op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure))
    du = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, SENTINEL))
    dp = op.initialize_dof_vector(1, np.full(op.n_pressure, SENTINEL))
    host = np.full(4096, SENTINEL)
    hp = stfem._p(host)
    one, two = (C.c_void_p * 1), (C.c_void_p * 2)
    A = np.eye(2)
    var = (C.c_int32 * 2)(0, 1)
    out = C.c_void_p()
    calls = {
        "stfem_stokes_set_weak_boundaries": lambda: L.stfem_stokes_set_weak_boundaries(h, 1, 0, 20.0, 10.0),
        "stfem_stokes_vmult_convection": lambda: L.stfem_stokes_vmult_convection(h, 1, du.ptr, dp.ptr, u.ptr, p.ptr, u.ptr, None),
        "stfem_stokes_st_vmult_convection": lambda: L.stfem_stokes_st_vmult_convection(h, 2, 1, 1, 1, stfem._p(A), stfem._p(A), two(du.ptr, dp.ptr),
                                                                                       two(u.ptr, p.ptr), two(u.ptr, None), None),
        "stfem_stokes_st_vmult_slice_add_convection": lambda: L.stfem_stokes_st_vmult_slice_add_convection(
            h, 1, 1, 1, 1, stfem._p(np.ones(2)), stfem._p(np.ones(2)), two(du.ptr, dp.ptr), u.ptr, p.ptr, u.ptr, None),
        "stfem_stokes_set_cip": lambda: L.stfem_stokes_set_cip(h, 0.5, 0),
        "stfem_stokes_cip_add": lambda: L.stfem_stokes_cip_add(h, du.ptr, u.ptr, u.ptr, 0.5, None),
        "stfem_stokes_set_cip_neighbours": lambda: L.stfem_stokes_set_cip_neighbours(h, 16, None, None),
        "stfem_stokes_cip_ghost_size": lambda: L.stfem_stokes_cip_ghost_size(h),
        "stfem_stokes_cip_ghost_create": lambda: L.stfem_stokes_cip_ghost_create(h, C.byref(out)),
        "stfem_stokes_cip_pack": lambda: L.stfem_stokes_cip_pack(h, u.ptr, 0, du.ptr, None),
        "stfem_stokes_cip_add_slab": lambda: L.stfem_stokes_cip_add_slab(h, du.ptr, u.ptr, u.ptr, 0.5, None, None, None),
        "stfem_stokes_cip_bind_ghosts": lambda: L.stfem_stokes_cip_bind_ghosts(h, u.ptr, None, None),
        "stfem_stokes_divergence": lambda: L.stfem_stokes_divergence(h, u.ptr, du.ptr, hp, None),
        "stfem_stokes_drag_lift_n_items": lambda: L.stfem_stokes_drag_lift_n_items(h, 63),
        "stfem_stokes_drag_lift": lambda: L.stfem_stokes_drag_lift(h, 63, 1.0, 0, 1, one(u.ptr), one(p.ptr), du.ptr, hp, None),
        "stfem_stokes_n_face_points": lambda: L.stfem_stokes_n_face_points(h),
        "stfem_stokes_face_points": lambda: L.stfem_stokes_face_points(h, hp),
        "stfem_stokes_nitsche_rhs": lambda: L.stfem_stokes_nitsche_rhs(h, hp, du.ptr, dp.ptr, None),
        "stfem_stokes_pressure_ctx": lambda: L.stfem_stokes_pressure_ctx(h, C.byref(out)),
        "stfem_stokes_pressure_mean_vectors": lambda: L.stfem_stokes_pressure_mean_vectors(h, hp, hp, hp),
        "stfem_stokes_pressure_quadrature_points": lambda: L.stfem_stokes_pressure_quadrature_points(h, 1, hp),
        "stfem_stokes_pressure_difference": lambda: L.stfem_stokes_pressure_difference(h, 1, p.ptr, hp, hp, None),
        "stfem_stokes_dgp_prolongate": lambda: L.stfem_stokes_dgp_prolongate(h, other._h, dp.ptr, p.ptr, 0, None),
        "stfem_stokes_dgp_prolongate (coarse)": lambda: L.stfem_stokes_dgp_prolongate(q2._h, other._h, dp.ptr, p.ptr, 0, None),
        "stfem_stokes_dgp_restrict": lambda: L.stfem_stokes_dgp_restrict(h, other._h, dp.ptr, p.ptr, 0, None),
        "stfem_stokes_vanka_create": lambda: L.stfem_stokes_vanka_create(h, 2, var, stfem._p(A), stfem._p(A), C.byref(out)),
        "stfem_stokes_vanka_create_linearised": lambda: L.stfem_stokes_vanka_create_linearised(h, 2, var, stfem._p(A), stfem._p(A), 0, None, C.byref(out)),
        "stfem_stokes_vanka_create_linearised_cip": lambda: L.stfem_stokes_vanka_create_linearised_cip(h, 2, var, stfem._p(A), stfem._p(A), 0, None, 0.0,
                                                                                                       C.byref(out)),
        "stfem_stokes_vanka_create_linearised_partitioned": lambda: L.stfem_stokes_vanka_create_linearised_partitioned(
            h, h, 2, var, stfem._p(A), stfem._p(A), 0, None, 0.0, 0, 0, C.byref(out)),
        "stfem_stokes_vanka_create_linearised_partitioned (extended)": lambda: L.stfem_stokes_vanka_create_linearised_partitioned(
            q2._h, h, 2, var, stfem._p(A), stfem._p(A), 0, None, 0.0, 0, 0, C.byref(out)),
    }
    for name, call in calls.items():
        L.stfem_stokes_set_weak_boundaries(q2._h, 0, 0, 20.0, 10.0)  # (a successful call in between: the reason below is this call's)
        status = call()
        why = L.stfem_last_error().decode()
        assert status == -2, (name, status, why)
        assert name.split(" ")[0] in why and "velocity degree 2 only" in why, (name, why)
        assert not out.value, name
    assert np.all(du.download() == SENTINEL) and np.all(dp.download() == SENTINEL) and np.all(host == SENTINEL)
    # the Python wrappers raise the same status
    for call in (op.face_points, lambda: op.divergence(u), lambda: op.drag_lift_n_items(63), lambda: op.set_cip(0.5),
                 lambda: stfem.StokesPreconditionVanka(op, [0, 1], A, A)):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == -2
    # and the operator itself still runs
    op.vmult(du, dp, u, p)
    assert np.all(du.download() != SENTINEL)
