"""GPU parity of the CIP interior-face term of the Stokes operator at velocity degree 3 (include/stfem_stokes_cip_space.h,
stokes_cip_q3_kernel of csrc/stfem_stokes_cip.hip) against the numpy restatement tests/cip_q3_reference.py; the linear part from the CPU
oracle at pu = 3, the convection term from tests/navier_q3_reference.py.  Tolerance rel-L2 <= 1e-12 (cip_q3_reference.TOL, the
tolerance of the other degree-3 operator tests).  Two bars where the term rides on another result:
  the full result   rel-L2 <= 1e-12;
  the term alone    |(y_with - y_without) - term_ref| <= 1e-12 (|y_without_ref| + |y_with_ref|): the difference of two results that each
                    carry a rounding error of their own size.
tests/test_cip_q3_reference_cpu.py::test_gpu_cases_are_not_hollow keeps the term at a tenth of the linear result or more for every
(mesh, mask, delta0) used here, and check_term asserts the same share, on the reference values, of every block it compares - the
results with weak faces, a convection mode or the mass part of a time step beside the term.  The meshes: 2 x 1 x 1 (one face), 1 x 1 x 3 (a cell with both z faces), 2 x 2 x 2 (every colour),
4 x 3 x 2 (a box with three edge lengths: the CART path), 3 x 2 x 4 perturbed (the general path)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import cip_q3_reference as c3
import navier_q3_reference as q3

pytestmark = pytest.mark.gpu
TOL = c3.TOL
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]
SENTINEL = -123.25
UNSUPPORTED = -2
EPS10 = q3.EPS10
ST_MESH, ST_MASK = "pert", 0b111011
TEETH = 0.1
CART_MESHES = ["box", "cube"]  # the several-source cases of the CART instantiation


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    for name in ("STFEM_STOKES_Q3_WORKGROUPS", "STFEM_STOKES_FACE_WORKGROUPS", "STFEM_STOKES_CIP_WORKGROUPS"):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def oracle_of(mesh, mask, dgp, weak=0):
    from oracle import oracle
    return oracle.StokesOracle(c3.MESHES[mesh][0], c3.mesh_vertices(mesh), mask, c3.NU, pu=3, weak_mask=weak, dg_pressure=dgp)


@functools.lru_cache(maxsize=None)
def linear_reference(mesh, mask, dgp, weak=0):
    """the oracle's K_S (u, p) and M u for u = fields(mesh)[0] and one random p: computed once and shared"""
    orc = oracle_of(mesh, mask, dgp, weak)
    U = c3.fields(mesh)[0]
    P = np.random.default_rng(c3.FIELD_SEED + 1).uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    res = dict(U=U, P=P, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1), con=np.tile(q3.constrained(3, c3.MESHES[mesh][0], mask), 3))
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def cip_of(mesh, mask, w_key, u_key):
    """C(w; u) with delta0 = 1 for fields named by hashable keys: ("f", i) = fields(mesh)[i], ("r", seed) = a seeded field"""
    nc = c3.MESHES[mesh][0]
    c = c3.cip(3, 1.0, field(mesh, w_key), field(mesh, u_key), nc, c3.mesh_vertices(mesh), mask)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def field(mesh, key):
    if key[0] == "f":
        return c3.fields(mesh)[key[1]]
    v = np.random.default_rng(key[1]).uniform(-1, 1, 3 * q3.n_velocity(3, c3.MESHES[mesh][0]))
    v.setflags(write=False)
    return v


def check_term(what, got_with, got_without, without_ref, term_ref, base=0.0):
    """the two bars on one velocity block.  Not hollow: on the REFERENCE values the term is at least a tenth (TEETH, the threshold of
    tests/test_cip_q3_reference_cpu.py) of what the call computed - the compared result less `base`, the initial content of a
    destination that is accumulated into"""
    with_ref = without_ref + term_ref
    n0, n1 = np.linalg.norm(without_ref), np.linalg.norm(with_ref)
    full = rel(got_with, with_ref)
    term = np.linalg.norm((got_with - got_without) - term_ref)
    share = np.linalg.norm(term_ref) / np.linalg.norm(with_ref - base)
    print(what, "full %.2e  term %.2e of bound %.2e  |term| / |y| = %.3f" % (full, term, TOL * (n0 + n1), share))
    assert share >= TEETH, (what, share)
    assert full <= TOL, (what, full)
    assert term <= TOL * (n0 + n1), (what, term)


def vmult(op, U, P, lin=None, mode=0):
    u, p = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))  # vmult overwrites
    if mode:
        op.vmult(ou, opr, u, p, lin=op.initialize_dof_vector(0, lin), mode=mode)
    else:
        op.vmult(ou, opr, u, p)
    return ou.download(), opr.download()


# ---- 1. the term by itself: weight = source and a weight velocity of its own, on every mesh and mask
@pytest.mark.parametrize("mask", c3.MASKS)
@pytest.mark.parametrize("mesh", list(c3.MESHES))
def test_cip_add_space(mesh, mask, stfem):
    op = c3.device_operator(stfem, mesh, mask)
    assert op.velocity_degree == 3
    delta0 = c3.delta0_of(mesh, mask)
    f = c3.fields(mesh)
    con = np.tile(q3.constrained(3, c3.MESHES[mesh][0], mask), 3)
    u, w = op.initialize_dof_vector(0, f[0]), op.initialize_dof_vector(0, f[1])
    for what, wv, ref in (("w = u", u, c3.term(mesh, mask, 0, 0)), ("w of its own", w, c3.term(mesh, mask, 1, 0))):
        dst = op.initialize_dof_vector(0, np.zeros(f[0].size))
        op.cip_add_space(dst, u, wv, delta0)
        got = dst.download()
        print(mesh, mask, what, "%.2e" % rel(got, delta0 * ref), "|C| = %.3e" % np.linalg.norm(delta0 * ref))
        assert np.linalg.norm(ref) > 0 and rel(got, delta0 * ref) <= TOL
        assert np.all(got[con] == 0.0)  # constrained rows receive nothing
        init = f[2]
        dst = op.initialize_dof_vector(0, init)  # it accumulates
        op.cip_add_space(dst, u, wv, delta0)
        assert np.linalg.norm(dst.download() - init - delta0 * ref) <= TOL * (np.linalg.norm(init) + np.linalg.norm(delta0 * ref))
        assert np.array_equal(dst.download()[con], init[con])
    # entries of u and w on constrained DoFs are not read
    if con.any():
        U2, W2 = f[0].copy(), f[1].copy()
        U2[con], W2[con] = 1e30, -1e30
        a, b = op.initialize_dof_vector(0, np.zeros(U2.size)), op.initialize_dof_vector(0, np.zeros(U2.size))
        op.cip_add_space(a, u, w, delta0)
        op.cip_add_space(b, op.initialize_dof_vector(0, U2), op.initialize_dof_vector(0, W2), delta0)
        assert np.array_equal(a.download(), b.download())
    assert op.last_cip_plan()[1] == 1


# ---- 2. vmult after set_cip_space = the result without CIP plus the term; mass_vmult never gets it
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("mask", c3.MASKS)
@pytest.mark.parametrize("mesh", list(c3.MESHES))
def test_vmult_adds_the_term_last(mesh, mask, dgp, stfem, oracle_mod):
    ref = linear_reference(mesh, mask, dgp)
    delta0 = c3.delta0_of(mesh, mask)
    op = c3.device_operator(stfem, mesh, mask, dgp)
    none_u, none_p = vmult(op, ref["U"], ref["P"])
    m0 = op.initialize_dof_vector(0, np.full(ref["U"].size, 5.0))
    op.mass_vmult(m0, op.initialize_dof_vector(0, ref["U"]))
    op.set_cip_space(delta0)
    assert (op.delta0, op.cip_weight) == (delta0, stfem.CIP_WEIGHT_SOURCE)
    got_u, got_p = vmult(op, ref["U"], ref["P"])
    assert rel(none_u, ref["ku"]) <= TOL and rel(none_p, ref["kp"]) <= TOL
    check_term((mesh, mask, dgp), got_u, none_u, ref["ku"], delta0 * c3.term(mesh, mask, 0, 0))
    assert np.array_equal(got_p, none_p)  # the pressure rows receive nothing
    assert np.array_equal(got_u[ref["con"]], none_u[ref["con"]])
    m1 = op.initialize_dof_vector(0, np.full(ref["U"].size, 5.0))
    op.mass_vmult(m1, op.initialize_dof_vector(0, ref["U"]))
    assert np.array_equal(m1.download(), m0.download()) and rel(m1.download(), ref["mu"]) <= TOL
    op.set_cip_space(delta0, stfem.CIP_WEIGHT_LINEARISATION)  # without a mode the weight stays the source: the same bits
    again_u, again_p = vmult(op, ref["U"], ref["P"])
    assert np.array_equal(again_u, got_u) and np.array_equal(again_p, got_p)


# ---- 3. several sources per launch (MULTI): st_vmult with two and three blocks, each source with its own weight; slice_add
@functools.lru_cache(maxsize=None)
def st_case(nsrc, dgp, mesh=ST_MESH, mask=ST_MASK):
    """cG(2) x 1 step: two sources, dG(2) x 1 step: three; random blocks in variable-major order"""
    stfem = importlib.import_module("dealii-stfem_amd")
    orc = oracle_of(mesh, mask, dgp)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP if nsrc == 2 else stfem.DG, 2, 1.0 / 16, 1)
    nt = Alpha.shape[0] // 2
    assert nt == nsrc
    var = [0] * nt + [1] * nt
    keys = [("r", 100 + 10 * nsrc + j) for j in range(nt)]
    rng = np.random.default_rng(40 + nsrc)
    blocks = [field(mesh, keys[j]) if v == 0 else rng.uniform(-1, 1, orc.n_p) for j, v in enumerate(var)]
    none = [np.ravel(x) for x in orc.st_vmult(Alpha, Beta, 1, nt, blocks)]
    return Alpha, Beta, nt, var, keys, blocks, none


def st_term(Alpha, nt, keys, wkeys, mesh=ST_MESH, mask=ST_MASK):
    """per velocity destination the sum over the sources of Alpha(j, i) C(w_i; u_i), the 10-eps skip rule"""
    add = []
    for j in range(nt):
        a = 0.0
        for i in range(nt):
            if abs(Alpha[j, i]) > EPS10:
                a = a + Alpha[j, i] * cip_of(mesh, mask, wkeys[i], keys[i])
        add.append(a)
    return add


def run_st(op, Alpha, Beta, nt, var, blocks, lin=None, mode=0):
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]  # st_vmult overwrites
    if mode:
        lv = [op.initialize_dof_vector(0, b) if b is not None else None for b in lin]
        op.st_vmult(Alpha, Beta, 1, nt, dst, src, True, lin=lv, mode=mode)
    else:
        op.st_vmult(Alpha, Beta, 1, nt, dst, src, True)
    return [d.download() for d in dst]


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("nsrc", [2, 3])
def test_st_vmult_each_source_its_own_weight(nsrc, dgp, stfem, oracle_mod):
    Alpha, Beta, nt, var, keys, blocks, none = st_case(nsrc, dgp)
    delta0 = c3.delta0_of(ST_MESH, ST_MASK)
    op = c3.device_operator(stfem, ST_MESH, ST_MASK, dgp)
    got_none = run_st(op, Alpha, Beta, nt, var, blocks)
    op.set_cip_space(delta0)
    got = run_st(op, Alpha, Beta, nt, var, blocks)
    add = st_term(Alpha, nt, keys, keys)  # weight = the source of each block
    for j in range(2 * nt):
        if var[j] == 0:
            check_term(("st_vmult", nsrc, dgp, j), got[j], got_none[j], none[j], delta0 * add[j])
        else:
            assert np.array_equal(got[j], got_none[j]) and rel(got[j], none[j]) <= TOL, j
    # a weight shared by all sources would give another result: the check can tell
    shared = st_term(Alpha, nt, keys, [keys[0]] * nt)
    assert max(rel(shared[j], add[j]) for j in range(nt)) > 1e-3


@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("mask", c3.MASKS)
@pytest.mark.parametrize("mesh", CART_MESHES)
def test_st_vmult_on_boxes(mesh, mask, nsrc, stfem, oracle_mod):
    """several sources on the meshes created without vertices - the CART several-source instantiation, with its six neighbours
    fetched up front per source: the linear st_vmult with each source its own weight, then in jacobian mode with the term weighted by
    each block's linearisation velocity; FE_DGP(2) with three sources, FE_Q(2) with two"""
    dgp = nsrc == 3
    nc, verts = c3.MESHES[mesh][0], c3.mesh_vertices(mesh)
    Alpha, Beta, nt, var, keys, blocks, none = st_case(nsrc, dgp, mesh, mask)
    delta0 = c3.st_delta0_of(mesh, mask)
    op0, op = c3.device_operator(stfem, mesh, mask, dgp), c3.device_operator(stfem, mesh, mask, dgp)
    op.set_cip_space(delta0, stfem.CIP_WEIGHT_LINEARISATION)
    got_none, got = run_st(op0, Alpha, Beta, nt, var, blocks), run_st(op, Alpha, Beta, nt, var, blocks)
    add = st_term(Alpha, nt, keys, keys, mesh, mask)  # no mode: the weight is the source of each block
    for j in range(2 * nt):
        if var[j] == 0:
            check_term(("st_vmult", mesh, mask, nsrc, j), got[j], got_none[j], none[j], delta0 * add[j])
        else:
            assert np.array_equal(got[j], got_none[j]) and rel(got[j], none[j]) <= TOL, j
    assert op.last_cip_plan()[0] >= 1
    lkeys = [("r", 500 + j) for j in range(nt)]
    lin = [field(mesh, k) for k in lkeys] + [None] * nt
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d)  # noqa: E731
    cadd = q3.st_convection(3, q3.JACOBIAN, Alpha, 1, nt, blocks, lin, index, nc, verts, mask)
    add = st_term(Alpha, nt, keys, lkeys, mesh, mask)
    got_none, got = run_st(op0, Alpha, Beta, nt, var, blocks, lin, q3.JACOBIAN), run_st(op, Alpha, Beta, nt, var, blocks, lin, q3.JACOBIAN)
    for j in range(2 * nt):
        if var[j] == 0:
            check_term(("st_vmult jacobian", mesh, mask, nsrc, j), got[j], got_none[j], none[j] + cadd[j], delta0 * add[j])
        else:
            assert np.array_equal(got[j], got_none[j]), j


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_st_vmult_slice_add_and_zero_weight_destination(dgp, stfem, oracle_mod):
    """onto non-zero destinations, two time dofs; one Gamma entry zero: that destination gets the mass part alone, bit for bit what it
    gets without CIP"""
    ref = linear_reference(ST_MESH, ST_MASK, dgp)
    delta0, nt = c3.delta0_of(ST_MESH, ST_MASK), 3
    nb = 2 * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    skipped = stfem.stokes_block_index(nt, 0, 0, 1)
    Gamma[skipped] = 0.0
    var = [0] * nt + [1] * nt
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    res = []
    for d0 in (0.0, delta0):
        op = c3.device_operator(stfem, ST_MESH, ST_MASK, dgp)
        op.set_cip_space(d0)
        dst = [op.initialize_dof_vector(v, x) for v, x in zip(var, init)]
        op.st_vmult_slice_add(Gamma, Zeta, 1, nt, dst, op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"]))
        res.append([d.download() for d in dst])
    term = c3.term(ST_MESH, ST_MASK, 0, 0)
    for j in range(nb):
        if var[j] == 1 or j == skipped:
            want = init[j] + (Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"])
            assert np.array_equal(res[1][j], res[0][j]) and rel(res[1][j], want) <= TOL, j
        else:
            check_term(("slice_add", dgp, j), res[1][j], res[0][j], init[j] + Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"], Gamma[j] * delta0 * term,
                       base=init[j])


# ---- 4. the _convection_space entries: both modes, both weights
@pytest.mark.parametrize("weight", [c3.SOURCE, c3.LINEARISATION], ids=["source", "linearisation"])
@pytest.mark.parametrize("mode", [q3.FORM, q3.JACOBIAN], ids=["form", "jacobian"])
def test_convection_space_entries(mode, weight, stfem, oracle_mod):
    dgp, delta0 = False, c3.delta0_of(ST_MESH, ST_MASK)
    nc, verts = c3.MESHES[ST_MESH][0], c3.mesh_vertices(ST_MESH)
    ref = linear_reference(ST_MESH, ST_MASK, dgp)
    bkey = ("f", 3)
    B = field(ST_MESH, bkey)
    op0, op = c3.device_operator(stfem, ST_MESH, ST_MASK, dgp), c3.device_operator(stfem, ST_MESH, ST_MASK, dgp)
    op.set_cip_space(delta0, weight)
    # vmult: one source
    conv = q3.convection(3, mode, B, ref["U"], nc, verts, ST_MASK)
    wkey = bkey if weight == c3.LINEARISATION else ("f", 0)
    none_u, none_p = vmult(op0, ref["U"], ref["P"], B, mode)
    got_u, got_p = vmult(op, ref["U"], ref["P"], B, mode)
    check_term(("vmult", mode, weight), got_u, none_u, ref["ku"] + conv, delta0 * cip_of(ST_MESH, ST_MASK, wkey, ("f", 0)))
    assert np.array_equal(got_p, none_p)
    if weight == c3.LINEARISATION:
        assert rel(cip_of(ST_MESH, ST_MASK, bkey, ("f", 0)), c3.term(ST_MESH, ST_MASK, 0, 0)) > 1e-3  # (the two weights differ)
    # st_vmult: two sources, each linearised about its own velocity
    Alpha, Beta, nt, var, keys, blocks, none = st_case(2, dgp)
    lkeys = [("r", 300), ("r", 301)]
    lin = [field(ST_MESH, k) for k in lkeys] + [None, None]
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d)  # noqa: E731
    cadd = q3.st_convection(3, mode, Alpha, 1, nt, blocks, lin, index, nc, verts, ST_MASK)
    add = st_term(Alpha, nt, keys, lkeys if weight == c3.LINEARISATION else keys)
    got_none, got = run_st(op0, Alpha, Beta, nt, var, blocks, lin, mode), run_st(op, Alpha, Beta, nt, var, blocks, lin, mode)
    for j in range(2 * nt):
        if var[j] == 0:
            check_term(("st_vmult", mode, weight, j), got[j], got_none[j], none[j] + cadd[j], delta0 * add[j])
        else:
            assert np.array_equal(got[j], got_none[j]), j
    # st_vmult_slice_add with the mode
    Gamma, Zeta = np.array([0.7, -1.3, 0.4, 0.9]), np.array([0.2, 0.5, 0.0, 0.0])
    init = [field(ST_MESH, ("r", 400 + j)) if v == 0 else np.zeros(ref["P"].size) for j, v in enumerate(var)]
    res = []
    for o in (op0, op):
        dst = [o.initialize_dof_vector(v, x) for v, x in zip(var, init)]
        o.st_vmult_slice_add(Gamma, Zeta, 1, nt, dst, o.initialize_dof_vector(0, ref["U"]), o.initialize_dof_vector(1, ref["P"]),
                             lin=o.initialize_dof_vector(0, B), mode=mode)
        res.append([d.download() for d in dst])
    for j in range(nt):
        check_term(("slice_add", mode, weight, j), res[1][j], res[0][j], init[j] + Gamma[j] * (ref["ku"] + conv) + Zeta[j] * ref["mu"],
                   Gamma[j] * delta0 * cip_of(ST_MESH, ST_MASK, wkey, ("f", 0)), base=init[j])


# ---- 5. CIP together with weak faces in the linear vmult: cell, boundary, CIP
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_with_weak_faces(dgp, stfem, oracle_mod):
    mesh, mask, weak, delta0 = "pert", 0, 0b000111, c3.delta0_of("pert", 0)
    ref = linear_reference(mesh, mask, dgp, weak)
    faceless = linear_reference(mesh, mask, dgp)
    assert rel(ref["ku"], faceless["ku"]) > 1e-3  # (the faces are in the reference)
    op = c3.device_operator(stfem, mesh, mask, dgp)
    op.set_weak_boundaries_space([0, 1, 2])
    none_u, none_p = vmult(op, ref["U"], ref["P"])
    op.set_cip_space(delta0)
    got_u, got_p = vmult(op, ref["U"], ref["P"])
    assert rel(none_p, ref["kp"]) <= TOL and np.array_equal(got_p, none_p)
    check_term(("weak faces", dgp), got_u, none_u, ref["ku"], delta0 * cip_of(mesh, mask, ("f", 0), ("f", 0)))
    assert op.last_face_plan()[0] >= 1 and op.last_cip_plan()[0] >= 1
    # a mode stays refused before the device is touched, with CIP set or not
    du = op.initialize_dof_vector(0, np.full(ref["U"].size, SENTINEL))
    dp = op.initialize_dof_vector(1, np.full(ref["P"].size, SENTINEL))
    u, p = op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"])
    for d0 in (delta0, 0.0):
        op.set_cip_space(d0)
        with pytest.raises(stfem.StfemError) as e:
            op.vmult(du, dp, u, p, lin=u, mode=1)
        assert e.value.status == UNSUPPORTED and b"inflow term" in stfem.lib().stfem_last_error()
    assert np.all(du.download() == SENTINEL) and np.all(dp.download() == SENTINEL)


# ---- 6. delta0 = 0 launches nothing
def test_delta0_zero_launches_nothing(stfem):
    ref = linear_reference(ST_MESH, ST_MASK, False)
    never, op = c3.device_operator(stfem, ST_MESH, ST_MASK), c3.device_operator(stfem, ST_MESH, ST_MASK)
    op.set_cip_space(0.0, stfem.CIP_WEIGHT_LINEARISATION)
    a, b = vmult(never, ref["U"], ref["P"]), vmult(op, ref["U"], ref["P"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    init = c3.fields(ST_MESH)[2]
    dst = op.initialize_dof_vector(0, init)
    op.cip_add_space(dst, op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(0, ref["U"]), 0.0)
    assert np.array_equal(dst.download(), init)
    lone = stfem.StokesMatrixFreeOperator.with_degree(3, (1, 1, 1), dirichlet_mask=0)  # a lone cell has no face
    z = lone.initialize_dof_vector(0, np.zeros(192))
    lone.cip_add_space(z, lone.initialize_dof_vector(0, np.ones(192)), lone.initialize_dof_vector(0, np.ones(192)), 1.0)
    assert np.all(z.download() == 0.0)
    for o in (op, never, lone):
        with pytest.raises(stfem.StfemError) as e:
            o.last_cip_plan()
        assert e.value.status == UNSUPPORTED and b"stfem_stokes_last_cip_plan" in stfem.lib().stfem_last_error()


# ---- 7. two runs give identical bits; capped at one workgroup the same bits, in more than one pass
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_capped_and_reproducible(dgp, stfem, oracle_mod, monkeypatch):
    """3 x 2 x 4 cells: colour 7 has 1 x 1 x 2 cells.  Uncapped they take two workgroups of one wave, one pass; one workgroup walks
    them in two passes.  The cell -> wave assignment changes no sum"""
    Alpha, Beta, nt, var, keys, blocks, none = st_case(2, dgp)
    ref = linear_reference(ST_MESH, ST_MASK, dgp)
    op = c3.device_operator(stfem, ST_MESH, ST_MASK, dgp)
    op.set_cip_space(c3.delta0_of(ST_MESH, ST_MASK))

    def both():
        return run_st(op, Alpha, Beta, nt, var, blocks) + list(vmult(op, ref["U"], ref["P"]))

    free = both()
    assert op.last_cip_plan() == (2, 1)
    again = both()
    monkeypatch.setenv("STFEM_STOKES_CIP_WORKGROUPS", "1")
    capped = both()
    plan = op.last_cip_plan()
    assert plan[0] == 1 and plan[1] > 1, plan
    capped_again = both()
    for j in range(len(free)):
        assert np.array_equal(again[j], free[j]) and np.array_equal(capped[j], free[j]) and np.array_equal(capped_again[j], free[j]), j
    assert rel(free[-2], ref["ku"] + c3.delta0_of(ST_MESH, ST_MASK) * c3.term(ST_MESH, ST_MASK, 0, 0)) <= TOL


# ---- 8. degree 2: the _space forms are the entries without the suffix
@pytest.mark.parametrize("box", [False, True], ids=["pert", "box"])
def test_degree_2_space_forms_equal_the_entries_bitwise(box, stfem):
    nc, mask, nu = (3, 2, 4), 0b111011, 0.6
    kw = dict(vertices=None if box else stfem.mesh_vertices(nc, distort=0.15, seed=77), dirichlet_mask=mask, viscosity=nu)
    old, new = stfem.StokesMatrixFreeOperator(nc, **kw), stfem.StokesMatrixFreeOperator.with_degree(2, nc, **kw)
    rng = np.random.default_rng(2)
    U, W, P = rng.uniform(-1, 1, 3 * old.n_velocity), rng.uniform(-1, 1, 3 * old.n_velocity), rng.uniform(-1, 1, old.n_pressure)
    res = []
    for op, add, setter in ((old, old.cip_add, old.set_cip), (new, new.cip_add_space, new.set_cip_space)):
        dst = op.initialize_dof_vector(0, W)
        add(dst, op.initialize_dof_vector(0, U), op.initialize_dof_vector(0, W), 0.8)
        setter(1.3, stfem.CIP_WEIGHT_LINEARISATION)
        res.append([dst.download(), *vmult(op, U, P), *vmult(op, U, P, W, 2)])
        assert op.last_cip_plan()[1] == 1
    assert np.linalg.norm(res[0][0] - W) > 0
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 9. what a degree-3 context still refuses
def test_refusals(stfem):
    L = stfem.lib()
    op = c3.device_operator(stfem, "cube", 0, True)
    h = op._h
    rng = np.random.default_rng(1)
    u, p = op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)), op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure))
    du = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, SENTINEL))
    dp = op.initialize_dof_vector(1, np.full(op.n_pressure, SENTINEL))
    host = np.full(4096, SENTINEL)
    hp = stfem._p(host)
    two = (C.c_void_p * 2)
    A = np.eye(2)
    var = (C.c_int32 * 2)(0, 1)
    out = C.c_void_p()
    calls = {
        "stfem_stokes_set_cip": lambda: L.stfem_stokes_set_cip(h, 1.0, 0),
        "stfem_stokes_cip_add": lambda: L.stfem_stokes_cip_add(h, du.ptr, u.ptr, u.ptr, 1.0, None),
        "stfem_stokes_set_cip_neighbours": lambda: L.stfem_stokes_set_cip_neighbours(h, 16, hp, None),
        "stfem_stokes_cip_ghost_size": lambda: L.stfem_stokes_cip_ghost_size(h),
        "stfem_stokes_cip_ghost_create": lambda: L.stfem_stokes_cip_ghost_create(h, C.byref(out)),
        "stfem_stokes_cip_pack": lambda: L.stfem_stokes_cip_pack(h, u.ptr, 0, du.ptr, None),
        "stfem_stokes_cip_add_slab": lambda: L.stfem_stokes_cip_add_slab(h, du.ptr, u.ptr, u.ptr, 1.0, None, None, None),
        "stfem_stokes_cip_bind_ghosts": lambda: L.stfem_stokes_cip_bind_ghosts(h, u.ptr, du.ptr, None),
        "stfem_stokes_vanka_create_linearised_cip": lambda: L.stfem_stokes_vanka_create_linearised_cip(
            h, 2, var, stfem._p(A), stfem._p(A), 0, two(u.ptr, None), 1.0, C.byref(out)),
    }
    q2 = stfem.StokesMatrixFreeOperator((2, 2, 2))
    for name, call in calls.items():
        L.stfem_stokes_set_cip(q2._h, 0.0, 0)  # (a successful call in between: the reason below is this call's)
        status = call()
        why = L.stfem_last_error().decode()
        assert status == UNSUPPORTED, (name, status, why)
        assert name in why and "velocity degree 2 only" in why, (name, why)
        assert not out.value, name
    assert np.all(du.download() == SENTINEL) and np.all(dp.download() == SENTINEL) and np.all(host == SENTINEL)
    # the Python wrappers raise the same status: the keyword of the constructor, set_cip, the Vanka blocks with a delta0
    for call in (lambda: stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2), delta0=1.0), lambda: op.set_cip(1.0),
                 lambda: op.cip_add(du, u, u, 1.0),
                 lambda: stfem.StokesPreconditionVanka(op, [0, 1], A, A, lin=[u, None], mode=0, delta0=1.0)):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert op.delta0 == 0.0
    with pytest.raises(stfem.StfemError):
        op.last_cip_plan()  # no refused call launched the kernel
    # the _space entries run on the same context
    op.set_cip_space(2.0)
    op.vmult(du, dp, u, p)
    assert np.all(du.download() != SENTINEL) and op.last_cip_plan()[0] >= 1
