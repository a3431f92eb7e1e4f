"""GPU parity of the Navier-Stokes modes (form / jacobian) of the Stokes operator at velocity degree 3, FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)
with QGauss(4): stokes_convection_kernel<3, ...> of csrc/stfem_stokes_convection.hip through the _space entries of include/stfem_stokes_convection_space.h.

Expected value: the linear part from the CPU oracle at pu = 3 (as tests/test_gpu_stokes_q3.py) plus the dense numpy restatement of the
term (tests/navier_q3_reference.py).  Two bars, per block:
  the full result      rel-L2 <= 1e-12, the project's GPU parity bar;
  the term alone       |(y_mode - y_none) - conv_ref| <= 1e-12 (|y_none_ref| + |y_mode_ref|): the difference of two results that each
                       carry a rounding error of their own size.
The second bar has teeth only where the term is not small beside the result, so every case asserts on the REFERENCE values
|conv_ref| >= 0.1 |y_mode_ref|.  With uniform(-1, 1) sources that holds for the viscosity NU = 0.01 and linearisation velocities
b = BSCALE * uniform(-1, 1), BSCALE = 8: on the CPU the ratio is 0.80 ... 1.00 over the vmult cases and 0.23 at the lowest over the
velocity blocks of the space-time cases, where the mass term of a time step 1 / 16 stands beside it (with viscosity 1 and BSCALE 1 it
is 0.02; with viscosity 0.01 and BSCALE 2 the lowest space-time block has 0.06).

Several cells per wave: no colour of the 3 x 2 x 2 mesh has more than two cells, so one workgroup (four waves) walks runs of one
cell there whatever the cap - the capped run on that mesh is compared bit for bit and its plan must name one workgroup; the run > 1
is asserted on a 6 x 6 x 6 mesh (colour 7: 27 cells on four waves, runs of 7), with the same comparisons."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import navier_q3_reference as q3
from test_gpu_stokes_q3 import SCHEMES, oracle_of, rel, time_blocks, vertices_of

pytestmark = pytest.mark.gpu
TOL = 1e-12
NU, BSCALE = 0.01, 8.0
TEETH = 0.1
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]
MODES = [q3.FORM, q3.JACOBIAN]
MODE_IDS = ["form", "jacobian"]
SENTINEL = -123.25
UNSUPPORTED, INVALID, ALIAS = -2, -1, -6
# cells, distortion, seed, mask, box (created without vertices)
MESHES = {
    "3x2x2pert": ((3, 2, 2), 0.1, 3, 63, False),           # every colour, an odd count
    "2x3x2box": ((2, 3, 2), 0.0, 0, 63, True),             # the constant diagonal Jacobian
    "1x3x2partial": ((1, 3, 2), 0.1, 5, 0b010110, False),  # a one-cell direction, empty colours, free faces
}
LONG = ((6, 6, 6), 0.12, 9, 0b011110, False)              # runs of several cells per wave under the cap
ST_MESH = MESHES["3x2x2pert"]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)


def ref_vertices(stfem, nc, distort, seed):
    """what the restatement and the oracle see: the vertex grid, of a box too"""
    return vertices_of(stfem, nc, distort, seed)


def operator(stfem, mesh, dgp, degree=3, **kw):
    nc, distort, seed, mask, box = mesh
    verts = None if box else vertices_of(stfem, nc, distort, seed)
    return stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=verts, dirichlet_mask=mask, viscosity=NU, dg_pressure=dgp, **kw)


@functools.lru_cache(maxsize=None)
def space_reference(mesh, dgp):
    """one random (u, p, b), the oracle's K_S (u, p) and the restatement's term for both modes: computed once and shared"""
    stfem = importlib.import_module("dealii-stfem_amd")
    nc, distort, seed, mask, _ = mesh
    orc = oracle_of(nc, distort, seed, mask, NU, dgp)
    rng = np.random.default_rng(21)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), BSCALE * rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    res = dict(U=U, P=P, B=B, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1), con=np.tile(q3.constrained(3, nc, mask), 3))
    for mode in MODES:
        res[mode] = q3.convection(3, mode, B, U, nc, ref_vertices(stfem, nc, distort, seed), mask)
    for v in res.values():
        v.setflags(write=False)
    return res


def check_block(what, got_mode, got_none, none_ref, conv_ref, teeth=True):
    """the two bars on one velocity block"""
    mode_ref = none_ref + conv_ref
    n_none, n_mode, n_conv = np.linalg.norm(none_ref), np.linalg.norm(mode_ref), np.linalg.norm(conv_ref)
    full = rel(got_mode, mode_ref)
    term = np.linalg.norm((got_mode - got_none) - conv_ref)
    print(what, "full %.2e  term %.2e of bound %.2e  |conv| / |y_mode| = %.3f" % (full, term, TOL * (n_none + n_mode), n_conv / n_mode))
    if teeth:
        assert n_conv >= TEETH * n_mode, (what, n_conv, n_mode)
    assert full <= TOL, (what, full)
    assert term <= TOL * (n_none + n_mode), (what, term, TOL * (n_none + n_mode))


def run_vmult(op, ref, mode, U=None, B=None):
    u, p = op.initialize_dof_vector(0, ref["U"] if U is None else U), op.initialize_dof_vector(1, ref["P"])
    b = op.initialize_dof_vector(0, ref["B"] if B is None else B)
    ou, opr = op.initialize_dof_vector(0, np.full(ref["U"].size, 7.0)), op.initialize_dof_vector(1, np.full(ref["P"].size, -3.0))  # overwritten
    if mode:
        op.vmult(ou, opr, u, p, lin=b, mode=mode)
    else:
        op.vmult(ou, opr, u, p)
    return ou.download(), opr.download()


# ---- 1. vmult on the three meshes, both pressure spaces, both modes; the exact rows
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_vmult(mesh, dgp, mode, stfem, oracle_mod):
    ref = space_reference(MESHES[mesh], dgp)
    op = operator(stfem, MESHES[mesh], dgp)
    assert op.velocity_degree == 3 and 3 * op.n_velocity == ref["U"].size
    nu_, np_ = run_vmult(op, ref, 0)
    mu_, mp_ = run_vmult(op, ref, mode)
    assert rel(nu_, ref["ku"]) <= TOL and rel(np_, ref["kp"]) <= TOL
    check_block((mesh, dgp, mode), mu_, nu_, ref["ku"], ref[mode])
    # the pressure destination and the constrained velocity rows are those of mode 0, bit for bit
    con = ref["con"]
    assert np.array_equal(mp_, np_) and rel(mp_, ref["kp"]) <= TOL
    assert np.array_equal(mu_[con], nu_[con]) and np.all(mu_[con] == 0.0)
    assert np.all(ref[mode][~con] != 0.0)  # (the free rows all receive the term)
    # entries of u and b on constrained DoFs are not read
    U2, B2 = ref["U"].copy(), ref["B"].copy()
    U2[con] = 1e30
    B2[con] = 1e30
    pu_, pp_ = run_vmult(op, ref, mode, U2, B2)
    assert np.array_equal(pu_, mu_) and np.array_equal(pp_, mp_)
    assert op.last_convection_plan()[0] >= 1


# ---- 2. st_vmult: every launch shape, both block orderings, a different b per time dof
@functools.lru_cache(maxsize=None)
def st_reference(scheme, variable_major, dgp, mode):
    stfem = importlib.import_module("dealii-stfem_amd")
    nc, distort, seed, mask, _ = ST_MESH
    kind, r, ns = SCHEMES[scheme]
    orc = oracle_of(nc, distort, seed, mask, NU, dgp)
    Alpha_vm, Beta_vm, _, _ = stfem.get_fe_time_weights_stokes(getattr(stfem, kind), r, 1.0 / 16, ns)
    nt = Alpha_vm.shape[0] // (2 * ns)
    Alpha, Beta, blocks, var = time_blocks(stfem, orc, Alpha_vm, Beta_vm, ns, nt, variable_major, 100 * r + ns)
    rng = np.random.default_rng(17 + ns)
    lin = [BSCALE * rng.uniform(-1, 1, 3 * orc.n_u) if v == 0 else None for v in var]
    none = orc.st_vmult(Alpha, Beta, ns, nt, blocks, variable_major)
    add = q3.st_convection(3, mode, Alpha, ns, nt, blocks, lin, lambda it, v, d: stfem.stokes_block_index(nt, it, v, d, variable_major), nc,
                           ref_vertices(stfem, nc, distort, seed), mask)
    return Alpha, Beta, ns, nt, blocks, var, lin, none, add


def run_st(op, Alpha, Beta, ns, nt, blocks, var, lin, mode, variable_major):
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]  # st_vmult overwrites
    lv = [None if b is None else op.initialize_dof_vector(0, b) for b in lin]
    if mode:
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major, lin=lv, mode=mode)
    else:
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major)
    return [d.download() for d in dst]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("variable_major", [True, False])
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_st_vmult(scheme, variable_major, dgp, mode, stfem, oracle_mod):
    """cG(2) x 1 step: 2 sources in one set; dG(2) x 1: 3; cG(2) x 2: 4 = MAXSRC, one fused set; cG(2) x 3: 6, one set per source, the
    later sets accumulating onto what the earlier ones wrote"""
    Alpha, Beta, ns, nt, blocks, var, lin, none, add = st_reference(scheme, variable_major, dgp, mode)
    assert ns * nt == {"cg2x1": 2, "dg2x1": 3, "cg2x2": 4, "cg2x3": 6}[scheme]
    op = operator(stfem, ST_MESH, dgp)
    got_none = run_st(op, Alpha, Beta, ns, nt, blocks, var, lin, 0, variable_major)
    got = run_st(op, Alpha, Beta, ns, nt, blocks, var, lin, mode, variable_major)
    assert sum(a is not None for a in add) == ns * nt
    for j in range(len(blocks)):
        if var[j] == 0:
            check_block((scheme, variable_major, dgp, mode, j), got[j], got_none[j], none[j], add[j])
        else:
            assert add[j] is None and np.array_equal(got[j], got_none[j]) and rel(got[j], none[j]) <= TOL, j


# ---- 3. st_vmult_slice_add with a mode into non-zero destinations
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_st_vmult_slice_add(dgp, mode, stfem, oracle_mod):
    """random Gamma / Zeta with one exact zero, onto non-zero destinations: the term rides with Gamma"""
    ref = space_reference(ST_MESH, dgp)
    op = operator(stfem, ST_MESH, dgp)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    skipped = stfem.stokes_block_index(nt, 1, 0, 0)
    Gamma[skipped] = 0.0  # a velocity destination that receives the mass term alone
    var = [(j // nt) % 2 for j in range(nb)]
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    u, p, b = op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"]), op.initialize_dof_vector(0, ref["B"])
    res = []
    for m in (0, mode):
        dst = [op.initialize_dof_vector(v, x) for v, x in zip(var, init)]
        if m:
            op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, u, p, lin=b, mode=m)
        else:
            op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, u, p)
        res.append([d.download() for d in dst])
    for j in range(nb):
        if var[j] == 1 or j == skipped:
            want = init[j] + (Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"])
            assert np.array_equal(res[1][j], res[0][j]) and rel(res[1][j], want) <= TOL, j
        else:
            # (the bars on what was added: the initial values are the same bits in both results and in the reference)
            none_ref = init[j] + Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"]
            check_block(("slice_add", dgp, mode, j), res[1][j], res[0][j], none_ref, Gamma[j] * ref[mode], teeth=False)


# ---- 4. several cells per wave, 5. reproducibility
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("mesh", [ST_MESH, LONG], ids=["3x2x2", "6x6x6"])
def test_capped_workgroups_and_reproducible(mesh, dgp, stfem, oracle_mod, monkeypatch):
    """STFEM_STOKES_Q3_WORKGROUPS=1: the same bits as uncapped, one workgroup in the plan, on 6 x 6 x 6 runs of several cells per wave;
    a second call gives the same bits; cG(2) in jacobian mode (two sources, the sums in registers) and vmult in form mode"""
    nc, distort, seed, mask, _ = mesh
    orc = oracle_of(nc, distort, seed, mask, NU, dgp)
    op = operator(stfem, mesh, dgp)
    with pytest.raises(stfem.StfemError) as e:
        op.last_convection_plan()  # no convection launch yet
    assert e.value.status == UNSUPPORTED and b"stfem_stokes_last_convection_plan" in stfem.lib().stfem_last_error()
    Alpha_vm, Beta_vm, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    Alpha, Beta, blocks, var = time_blocks(stfem, orc, Alpha_vm, Beta_vm, 1, 2, True, 4)
    rng = np.random.default_rng(5)
    lin = [BSCALE * rng.uniform(-1, 1, 3 * orc.n_u), BSCALE * rng.uniform(-1, 1, 3 * orc.n_u), None, None]
    ref = dict(U=blocks[0], P=blocks[2], B=lin[0])

    def both():
        return run_st(op, Alpha, Beta, 1, 2, blocks, var, lin, q3.JACOBIAN, True) + list(run_vmult(op, ref, q3.FORM))

    free = both()
    plan = op.last_convection_plan()
    ncol7 = (nc[0] // 2) * (nc[1] // 2) * (nc[2] // 2)
    assert plan == ((ncol7 + 3) // 4, 1), plan  # colour 7, one cell per wave
    again = both()
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")
    capped = both()
    plan = op.last_convection_plan()
    assert plan == (1, (ncol7 + 3) // 4), plan
    if mesh is LONG:
        assert plan[1] > 1
    for j in range(len(free)):
        assert np.array_equal(again[j], free[j]), j
        assert np.array_equal(capped[j], free[j]), j
    # and it is the expected result (the linear part from the oracle, the term from the restatement)
    verts = ref_vertices(stfem, nc, distort, seed)
    want = orc.apply(ref["U"], ref["P"])[0].reshape(-1) + q3.convection(3, q3.FORM, ref["B"], ref["U"], nc, verts, mask)
    assert rel(free[4], want) <= TOL
    none = orc.st_vmult(Alpha, Beta, 1, 2, blocks, True)
    add = q3.st_convection(3, q3.JACOBIAN, Alpha, 1, 2, blocks, lin, lambda it, v, d: stfem.stokes_block_index(2, it, v, d), nc, verts, mask)
    for j in range(2):
        assert rel(free[j], none[j] + add[j]) <= TOL, j


# ---- 6. equivalences: the raw entries by name on one context
def raw_calls(stfem, op, suffix):
    """the three entries with (`_space`) or without the suffix on the handle of `op`, statuses returned"""
    L = stfem.lib()
    ptr = lambda v: getattr(v, "ptr", v)  # noqa: E731

    def vmult(mode, du, dp, u, p, lin):
        return getattr(L, "stfem_stokes_vmult_convection" + suffix)(op._h, mode, ptr(du), ptr(dp), ptr(u), ptr(p), ptr(lin), None)

    def st(mode, ns, nt, Alpha, Beta, dst, src, lin):
        nb = len(dst)
        arr = lambda vs: (C.c_void_p * nb)(*[ptr(v) for v in vs])  # noqa: E731
        A, B = np.ascontiguousarray(Alpha, dtype=np.float64), np.ascontiguousarray(Beta, dtype=np.float64)
        return getattr(L, "stfem_stokes_st_vmult_convection" + suffix)(op._h, mode, ns, nt, 1, stfem._p(A), stfem._p(B), arr(dst), arr(src),
                                                                      None if lin is None else arr(lin), None)

    def slice_add(mode, ns, nt, Gamma, Zeta, dst, u, p, lin):
        nb = len(dst)
        g, z = np.ascontiguousarray(Gamma, dtype=np.float64), np.ascontiguousarray(Zeta, dtype=np.float64)
        return getattr(L, "stfem_stokes_st_vmult_slice_add_convection" + suffix)(op._h, mode, ns, nt, 1, stfem._p(g), stfem._p(z),
                                                                                (C.c_void_p * nb)(*[ptr(v) for v in dst]), ptr(u), ptr(p), ptr(lin), None)

    return vmult, st, slice_add


def all_three(stfem, op, suffix, mode, seed=31):
    """vmult, cG(2) st_vmult and slice_add (onto seeded destinations) through the entries with the given suffix: ten result arrays"""
    vmult, st, slice_add = raw_calls(stfem, op, suffix)
    rng = np.random.default_rng(seed)
    nu_, np_ = 3 * op.n_velocity, op.n_pressure
    var = [0, 0, 1, 1]
    blocks = [rng.uniform(-1, 1, nu_ if v == 0 else np_) for v in var]
    lin_h = [BSCALE * rng.uniform(-1, 1, nu_) for _ in range(2)]
    init = [rng.uniform(-1, 1, b.size) for b in blocks]
    Alpha, Beta, Gamma, Zeta = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    lin = [op.initialize_dof_vector(0, b) for b in lin_h]
    res = []
    du, dp = op.initialize_dof_vector(0, np.full(nu_, 7.0)), op.initialize_dof_vector(1, np.full(np_, -3.0))
    assert vmult(mode, du, dp, src[0], src[2], lin[0] if mode else None) == 0
    res += [du.download(), dp.download()]
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]
    assert st(mode, 1, 2, Alpha, Beta, dst, src, lin + [None, None] if mode else None) == 0
    res += [d.download() for d in dst]
    dst = [op.initialize_dof_vector(v, x) for v, x in zip(var, init)]
    assert slice_add(mode, 1, 2, Gamma.reshape(-1), Zeta.reshape(-1), dst, src[1], src[3], lin[1] if mode else None) == 0
    res += [d.download() for d in dst]
    assert all(np.linalg.norm(r) > 0 for r in res)
    return res


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_mode_0_through_the_space_entries_at_degree_3(dgp, stfem):
    op = operator(stfem, ST_MESH, dgp)
    for a, b in zip(all_three(stfem, op, "", 0), all_three(stfem, op, "_space", 0)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("box", [True, False], ids=["box", "perturbed"])
def test_degree_2_space_entries_equal_the_old_ones(box, mode, stfem):
    """a weak face (the inflow launches are reached) and a strongly constrained rest; the Kronecker path on the box"""
    mesh = ((3, 4, 2), 0.0 if box else 0.1, 3, 0b111110, box)
    op = operator(stfem, mesh, False, degree=2, weak_boundary_ids=[0])
    assert op.velocity_degree == 2 and op.weak_mask == 1
    old, new = all_three(stfem, op, "", mode), all_three(stfem, op, "_space", mode)
    for a, b in zip(old, new):
        assert np.array_equal(a, b)
    plain = all_three(stfem, op, "_space", 0)
    assert not np.array_equal(plain[0], new[0])  # (the mode is not ignored)
    assert op.last_convection_plan()[0] >= 1


# ---- 7. refusals
def test_refusals(stfem):
    L = stfem.lib()
    op = operator(stfem, MESHES["2x3x2box"], True)
    fresh = operator(stfem, MESHES["2x3x2box"], True)
    rng = np.random.default_rng(1)
    nu_, np_ = 3 * op.n_velocity, op.n_pressure
    u, p, b = (op.initialize_dof_vector(0, rng.uniform(-1, 1, nu_)), op.initialize_dof_vector(1, rng.uniform(-1, 1, np_)),
               op.initialize_dof_vector(0, rng.uniform(-1, 1, nu_)))
    du, dp = op.initialize_dof_vector(0, np.full(nu_, SENTINEL)), op.initialize_dof_vector(1, np.full(np_, SENTINEL))
    A, ones = np.eye(2), np.ones(2)
    # the entries of stfem.h still refuse a mode at degree 3, with their reason
    vmult, st, slice_add = raw_calls(stfem, op, "")
    for name, call in (("stfem_stokes_vmult_convection", lambda: vmult(1, du, dp, u, p, b)),
                       ("stfem_stokes_st_vmult_convection", lambda: st(2, 1, 1, A, A, [du, dp], [u, p], [b, None])),
                       ("stfem_stokes_st_vmult_slice_add_convection", lambda: slice_add(1, 1, 1, ones, ones, [du, dp], u, p, b))):
        assert call() == UNSUPPORTED, name
        why = L.stfem_last_error().decode()
        assert name in why and "velocity degree 2 only" in why, why
    # the _space entries: the argument refusals of the entries without the suffix, status for status
    for suffix in ("", "_space"):
        vmult, st, slice_add = raw_calls(stfem, op, suffix)
        for mode in (-1, 3):
            assert vmult(mode, du, dp, u, p, b) == INVALID
            assert st(mode, 1, 1, A, A, [du, dp], [u, p], [b, None]) == INVALID
            assert slice_add(mode, 1, 1, ones, ones, [du, dp], u, p, b) == INVALID
        for mode in (1, 2):
            assert vmult(mode, du, dp, u, p, None) == INVALID
            assert st(mode, 1, 1, A, A, [du, dp], [u, p], None) == INVALID
            assert st(mode, 1, 1, A, A, [du, dp], [u, p], [None, None]) == INVALID
            assert slice_add(mode, 1, 1, ones, ones, [du, dp], u, p, None) == INVALID
            assert vmult(mode, du, dp, u, p, du) == ALIAS
            assert st(mode, 1, 1, A, A, [du, dp], [u, p], [du, None]) == ALIAS
            assert slice_add(mode, 1, 1, ones, ones, [du, dp], u, p, du) == ALIAS
    assert np.all(du.download() == SENTINEL) and np.all(dp.download() == SENTINEL)
    # the diagnostic before any convection launch of the context (`op` has launched none either: every call above was refused)
    out = (C.c_int32 * 2)(-5, -5)
    for o in (op, fresh):
        assert L.stfem_stokes_last_convection_plan(o._h, out) == UNSUPPORTED and b"has not launched" in L.stfem_last_error()
    assert tuple(out) == (-5, -5)
    # and the entries run
    vmult, _, _ = raw_calls(stfem, op, "_space")
    assert vmult(1, du, dp, u, p, b) == 0 and np.all(du.download() != SENTINEL)
    assert L.stfem_stokes_last_convection_plan(op._h, out) == 0 and out[0] >= 1 and out[1] >= 1
