"""GPU parity of the convection modes (form / jacobian) of the Stokes operator through stfem_stokes_*_convection: against the existing
linear oracle plus the numpy restatement of the convection term (tests/navier_reference.py).  Tolerance rel-L2 <= 1e-12, the
project's fp64 parity tolerance; random fields in [-1, 1].  Meshes: a lone cell (idle half-waves), 3 x 2 x 4 perturbed and
5 x 4 x 3 Cartesian (unequal extents, all eight colours, cells with neighbours on both sides, cell counts no multiple of 8)."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
MESHES = {"cell": ((1, 1, 1), 0.0), "pert": ((3, 2, 4), 0.15), "cart": ((5, 4, 3), 0.0)}
MASKS = [63, 0b111011, 0]
MODES = [nref.FORM, nref.JACOBIAN]
NU = 0.3


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@functools.lru_cache(maxsize=None)
def _vertices(mesh):
    stfem = importlib.import_module("dealii-stfem_amd")
    nc, distort = MESHES[mesh]
    return stfem.mesh_vertices(nc, distort=distort, seed=77)


def _operator(stfem, mesh, mask, dg, weak=(), outflow=()):
    """the operator (general meshes get their vertices: the cell kernel; the Cartesian one none: Kronecker path + CART kernels) and
    the linear oracle of the same problem"""
    from oracle import oracle
    nc, distort = MESHES[mesh]
    verts = _vertices(mesh)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if mesh != "cart" else None, dirichlet_mask=mask, viscosity=NU,
                                        dg_pressure=dg, weak_boundary_ids=weak, outflow_boundary_ids=outflow)
    wm = sum(1 << f for f in weak) & ~sum(1 << f for f in outflow)
    orc = oracle.StokesOracle(nc, verts, mask, NU, weak_mask=wm, dg_pressure=dg)
    assert (op.n_velocity, op.n_pressure) == (orc.n_u, orc.n_p)
    return op, orc, nc, verts, wm


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_vmult(mesh, mask, mode, dg, stfem):
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, dg)
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = nref.vmult(orc, mode, B, U, P, nc, verts, mask)
    u, p, b = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P), op.initialize_dof_vector(0, B)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))  # overwritten
    op.vmult(ou, opr, u, p, lin=b, mode=mode)
    got = ou.download()
    lin_u, _ = orc.apply(U, P)
    if mask != 63 or mesh != "cell":
        assert rel(got, lin_u) > 1e-3  # the term is there
    assert np.linalg.norm(got - ku) <= TOL * np.linalg.norm(ku), rel(got, ku)
    assert np.linalg.norm(opr.download() - kp) <= TOL * np.linalg.norm(kp) + 1e-14
    con = np.tile(nref.constrained(nc, mask), 3)
    assert np.all(got[con] == 0.0)  # constrained velocity rows receive nothing
    # Picard: the linearisation may be the source itself
    op.vmult(ou, opr, u, p, lin=u, mode=mode)
    ku2, _ = nref.vmult(orc, mode, U, U, P, nc, verts, mask)
    assert np.linalg.norm(ou.download() - ku2) <= TOL * np.linalg.norm(ku2)


def _weights(stfem, scheme, variable_major):
    """(Alpha, Beta, ns, nt, index): cG(2), one step - four blocks, two sources, the fused path; dG(2), two steps - six sources, more
    than the fused path takes, one set of launches per source"""
    if scheme == "cg2":
        ns, nt = 1, 2
        A, B, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    else:
        ns, nt = 2, 3
        A, B, _, _ = stfem.get_fe_time_weights_stokes(stfem.DG, 2, 1.0 / 16, ns)
    nb = 2 * nt * ns
    assert A.shape == (nb, nb)
    perm = np.zeros(nb, dtype=int)
    for it in range(ns):
        for v in range(2):
            for d in range(nt):
                perm[stfem.stokes_block_index(nt, it, v, d, variable_major)] = stfem.stokes_block_index(nt, it, v, d, True)
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d, variable_major)  # noqa: E731
    return A[np.ix_(perm, perm)], B[np.ix_(perm, perm)], ns, nt, index


def _st_problem(stfem, op, orc, scheme, variable_major, seed=9):
    Alpha, Beta, ns, nt, index = _weights(stfem, scheme, variable_major)
    nb = 2 * ns * nt
    rng = np.random.default_rng(seed)
    blocks, lin, var = [None] * nb, [None] * nb, [0] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[index(it, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
            blocks[index(it, 1, d)] = rng.uniform(-1, 1, orc.n_p)
            lin[index(it, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)  # not the source
            var[index(it, 1, d)] = 1
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    dlin = [op.initialize_dof_vector(0, b) if b is not None else None for b in lin]  # pressure entries: null
    return Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variable_major", [True, False])
@pytest.mark.parametrize("scheme", ["cg2", "dg2x2"])
@pytest.mark.parametrize("mesh", ["pert", "cart"])
def test_st_vmult(mesh, scheme, variable_major, mode, stfem):
    mask, dg = 0b111011, mesh == "cart"
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, dg)
    Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, op, orc, scheme, variable_major)
    ref = nref.st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, mask, variable_major=variable_major)
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]
    op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major, lin=dlin, mode=mode)
    for j in range(len(blocks)):
        assert np.linalg.norm(ref[j]) > 0
        assert np.linalg.norm(dst[j].download() - ref[j]) <= TOL * np.linalg.norm(ref[j]) + 1e-14, (j, rel(dst[j].download(), ref[j]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mesh", ["pert", "cart"])
def test_st_vmult_slice_add(mesh, mode, stfem):
    """onto non-zero destinations, one Gamma entry zero (that destination gets the mass part alone)"""
    mask = 63
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, False)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 0, 0)] = 0.0
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = nref.vmult(orc, mode, B, U, P, nc, verts, mask)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    init = [rng.uniform(-1, 1, 3 * orc.n_u if (j // nt) % 2 == 0 else orc.n_p) for j in range(nb)]
    dst = [op.initialize_dof_vector((j // nt) % 2, init[j]) for j in range(nb)]
    op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P),
                          lin=op.initialize_dof_vector(0, B), mode=mode)
    for it in range(ns):
        for d in range(nt):
            ju, jp = stfem.stokes_block_index(nt, it, 0, d), stfem.stokes_block_index(nt, it, 1, d)
            assert rel(dst[ju].download(), init[ju] + Gamma[ju] * ku + Zeta[ju] * mu.reshape(-1)) < TOL
            assert rel(dst[jp].download(), init[jp] + Gamma[jp] * kp) < TOL


WEAK, OUTFLOW, WEAK_DIRICHLET = (0, 1, 5), (3,), 0b010100  # faces 2 and 4 stay strong


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_weak_faces(mesh, mode, dg, stfem):
    """the inflow term - min(b.n, 0) u on the weak faces 0, 1, 5, nothing on the outflow face 3: a random b points in on some face
    points and out on others; vmult (one source) and the fused space-time vmult (several sources, each with its own b)"""
    op, orc, nc, verts, wm = _operator(stfem, mesh, WEAK_DIRICHLET, dg, WEAK, OUTFLOW)
    assert wm == 0b100011
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    faces = nref.convection_faces(B, U, nc, verts, WEAK_DIRICHLET, wm)
    cells = nref.convection_cells(mode, B, U, nc, verts, WEAK_DIRICHLET)
    assert np.linalg.norm(faces) > 1e-3 * np.linalg.norm(cells)  # some inflow
    assert np.linalg.norm(nref.convection_faces(-B, U, nc, verts, WEAK_DIRICHLET, wm)) > 1e-3 * np.linalg.norm(cells)  # and some outflow
    ku, kp = nref.vmult(orc, mode, B, U, P, nc, verts, WEAK_DIRICHLET, wm)
    u, p, b = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P), op.initialize_dof_vector(0, B)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))
    op.vmult(ou, opr, u, p, lin=b, mode=mode)
    assert np.linalg.norm(ou.download() - ku) <= TOL * np.linalg.norm(ku), rel(ou.download(), ku)
    assert np.linalg.norm(opr.download() - kp) <= TOL * np.linalg.norm(kp) + 1e-14
    Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, op, orc, "cg2", True)
    ref = nref.st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, WEAK_DIRICHLET, wm)
    dst = [op.initialize_dof_vector(v, np.full(b_.size, 11.0)) for v, b_ in zip(var, blocks)]
    op.st_vmult(Alpha, Beta, ns, nt, dst, src, True, lin=dlin, mode=mode)
    for j in range(len(blocks)):
        assert np.linalg.norm(dst[j].download() - ref[j]) <= TOL * np.linalg.norm(ref[j]) + 1e-14, (j, rel(dst[j].download(), ref[j]))


@pytest.mark.parametrize("mesh", ["pert", "cart"])
def test_mode_none_is_the_linear_operator_bitwise(mesh, stfem):
    """mode 0 through the new entry points = the old entry points, bit for bit; the pressure destinations of modes 1 and 2 = those
    of mode 0, bit for bit"""
    mask = 0b111010
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, mesh == "cart", (0,), ())
    L = stfem.lib()
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    u, p, b = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P), op.initialize_dof_vector(0, B)

    def run(call):
        ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))
        call(ou, opr)
        return ou.download(), opr.download()

    old = run(lambda ou, opr: op.vmult(ou, opr, u, p))
    for lin in (None, b.ptr):  # mode 0 ignores lin
        new = run(lambda ou, opr: stfem._check(L.stfem_stokes_vmult_convection(op._h, 0, ou.ptr, opr.ptr, u.ptr, p.ptr, lin, None), "vmult"))
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
    for mode in MODES:
        got = run(lambda ou, opr: op.vmult(ou, opr, u, p, lin=b, mode=mode))
        assert np.array_equal(old[1], got[1]) and not np.array_equal(old[0], got[0])
    # space-time, both paths
    for scheme in ("cg2", "dg2x2"):
        Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, op, orc, scheme, True)

        def st(mode, use_lin):
            dst = [op.initialize_dof_vector(v, np.full(b_.size, 11.0)) for v, b_ in zip(var, blocks)]
            if mode == 0 and not use_lin:
                op.st_vmult(Alpha, Beta, ns, nt, dst, src, True)
            else:
                op.st_vmult(Alpha, Beta, ns, nt, dst, src, True, lin=dlin, mode=mode)
            return [d.download() for d in dst]

        old_st, new_st = st(0, False), st(0, True)
        assert all(np.array_equal(x, y) for x, y in zip(old_st, new_st))
        for mode in MODES:
            got = st(mode, True)
            for j in range(len(blocks)):
                assert np.array_equal(old_st[j], got[j]) == (var[j] == 1), j
    # slice_add
    nb = 4
    G, Z = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    init = [rng.uniform(-1, 1, 3 * orc.n_u if v == 0 else orc.n_p) for v in (0, 0, 1, 1)]

    def sl(mode, use_lin):
        dst = [op.initialize_dof_vector(v, i) for v, i in zip((0, 0, 1, 1), init)]
        if use_lin:
            op.st_vmult_slice_add(G, Z, 1, 2, dst, u, p, lin=b, mode=mode)
        else:
            op.st_vmult_slice_add(G, Z, 1, 2, dst, u, p)
        return [d.download() for d in dst]

    old_sl = sl(0, False)
    assert all(np.array_equal(x, y) for x, y in zip(old_sl, sl(0, True)))
    for mode in MODES:
        got = sl(mode, True)
        assert np.array_equal(old_sl[2], got[2]) and np.array_equal(old_sl[3], got[3]) and not np.array_equal(old_sl[0], got[0])


@pytest.mark.parametrize("mesh", ["pert", "cart"])
def test_newton_identity_on_the_device(mesh, stfem):
    """F(u + d) = F(u) + J(u) d + C_form(d, d), F(w) = L w + C_form(w, w), every term a device vmult; C_form(d, d) as the
    difference of the form mode and the linear operator applied to d"""
    mask = 0b111011
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, mesh == "pert")
    rng = np.random.default_rng(13)
    U, D = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, 3 * orc.n_u)
    P, DP = rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, orc.n_p)

    def apply(mode, lin, src_u, src_p):
        u, p = op.initialize_dof_vector(0, src_u), op.initialize_dof_vector(1, src_p)
        b = op.initialize_dof_vector(0, lin)
        ou, opr = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
        op.vmult(ou, opr, u, p, lin=b, mode=mode)
        return ou.download(), opr.download()

    fu, fp = apply(nref.FORM, U + D, U + D, P + DP)
    gu, gp = apply(nref.FORM, U, U, P)
    ju, jp = apply(nref.JACOBIAN, U, D, DP)
    cdd = apply(nref.FORM, D, D, DP)[0] - apply(0, D, D, DP)[0]
    assert np.linalg.norm(cdd) > 1e-3 * np.linalg.norm(fu)
    assert np.linalg.norm(fu - (gu + ju + cdd)) <= TOL * np.linalg.norm(fu)
    assert np.linalg.norm(fp - (gp + jp)) <= TOL * np.linalg.norm(fp)


@pytest.mark.parametrize("scheme", ["cg2", "dg2x2"])
def test_replays_are_bitwise_equal(scheme, stfem):
    op, orc, nc, verts, _ = _operator(stfem, "pert", 0b111000, False, (0, 1), ())
    Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, op, orc, scheme, True)
    runs = []
    for _ in range(2):
        dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, True, lin=dlin, mode=nref.JACOBIAN)
        runs.append([d.download() for d in dst])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


# ---- the convection kernel's walk over several cells per half-wave (STFEM_STOKES_Q3_WORKGROUPS caps the workgroups of its colour
# launches as it caps those of the linear cell kernel; last_convection_plan reports the last colour launch)
LONG_NC, LONG_DISTORT, LONG_SEED, LONG_MASK = (6, 6, 6), 0.12, 9, 0b011110  # the perturbed mesh of SEVERAL_CELLS in test_gpu_stokes.py


@functools.lru_cache(maxsize=None)
def _long_reference():
    """one (u, p, b) with the expected vmult in form mode, and a cG(2) step (two sources, each with its own b, four destination blocks)
    with the expected st_vmult in jacobian mode: computed once for both walks"""
    from oracle import oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    verts = stfem.mesh_vertices(LONG_NC, distort=LONG_DISTORT, seed=LONG_SEED)
    orc = oracle.StokesOracle(LONG_NC, verts, LONG_MASK, NU, weak_mask=0, dg_pressure=False)
    rng = np.random.default_rng(17)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, _ = nref.vmult(orc, nref.FORM, B, U, P, LONG_NC, verts, LONG_MASK)
    Alpha, Beta, ns, nt, index = _weights(stfem, "cg2", True)
    blocks, lin, var = [None] * 4, [None] * 4, [0] * 4
    for d in range(nt):
        blocks[index(0, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
        blocks[index(0, 1, d)] = rng.uniform(-1, 1, orc.n_p)
        lin[index(0, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
        var[index(0, 1, d)] = 1
    want = nref.st_vmult(orc, nref.JACOBIAN, Alpha, Beta, ns, nt, blocks, lin, index, LONG_NC, verts, LONG_MASK)
    for x in [U, P, B, ku] + blocks + [b for b in lin if b is not None] + list(want):
        x.setflags(write=False)
    return verts, (U, P, B, ku), (Alpha, Beta, blocks, lin, var, want)


@pytest.mark.parametrize("interleave", ["0", "1"])
def test_convection_kernel_several_cells_per_half_wave(interleave, stfem, monkeypatch):
    """6^3 perturbed cells, both cell -> half-wave assignments.  Every colour has 3^3 = 27 cells, 8 per workgroup.  Uncapped:
    ceil(27 / 8) = 4 workgroups, runs of one cell - the plan of the last convection launch (colour 7) is (4, 1).  Capped at one
    workgroup: 27 cells on 8 half-waves, runs of ceil(27 / 8) = 4 - the plan is (1, 4).  vmult in form mode and a cG(2) st_vmult in
    jacobian mode (the sums over the sources in registers): the capped and a repeated run equal the uncapped one bit for bit, and it is
    the restatement's result."""
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)
    monkeypatch.setenv("STFEM_STOKES_INTERLEAVE", interleave)  # (read when the context is created)
    verts, (U, P, B, ku), (Alpha, Beta, blocks, lin, var, want) = _long_reference()
    op = stfem.StokesMatrixFreeOperator(LONG_NC, vertices=verts, dirichlet_mask=LONG_MASK, viscosity=NU)
    u, p, b = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P), op.initialize_dof_vector(0, B)
    src = [op.initialize_dof_vector(v, x) for v, x in zip(var, blocks)]
    dlin = [op.initialize_dof_vector(0, x) if x is not None else None for x in lin]

    def both():
        dst = [op.initialize_dof_vector(v, np.full(x.size, 11.0)) for v, x in zip(var, blocks)]  # overwritten
        op.st_vmult(Alpha, Beta, 1, 2, dst, src, True, lin=dlin, mode=nref.JACOBIAN)
        ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))
        op.vmult(ou, opr, u, p, lin=b, mode=nref.FORM)
        return [d.download() for d in dst] + [ou.download()]

    free = both()
    plan = op.last_convection_plan()
    assert plan == (4, 1), plan
    again = both()
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")
    capped = both()
    plan = op.last_convection_plan()
    assert plan == (1, 4), plan
    for j, ref in enumerate(list(want) + [ku]):
        assert np.array_equal(again[j], free[j]), j
        assert np.array_equal(capped[j], free[j]), j
        print(interleave, j, "%.2e" % rel(free[j], ref))
        assert np.linalg.norm(ref) > 0 and np.linalg.norm(free[j] - ref) <= TOL * np.linalg.norm(ref), (j, rel(free[j], ref))


def test_refusals_leave_the_destinations_alone(stfem):
    op, orc, nc, verts, _ = _operator(stfem, "pert", 63, False)
    rng = np.random.default_rng(5)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    u, p = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P)
    IU, IP = np.full(U.size, 7.0), np.full(P.size, -3.0)
    ou, opr = op.initialize_dof_vector(0, IU), op.initialize_dof_vector(1, IP)

    def refused(status, call):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == status
        assert np.array_equal(ou.download(), IU) and np.array_equal(opr.download(), IP)

    refused(-6, lambda: op.vmult(ou, opr, u, p, lin=ou, mode=1))      # the linearisation is a destination: STFEM_ERR_ALIAS
    refused(-1, lambda: op.vmult(ou, opr, u, p, lin=u, mode=3))       # no such mode: STFEM_ERR_INVALID_ARGUMENT
    refused(-1, lambda: op.vmult(ou, opr, u, p, lin=u, mode=-1))
    refused(-1, lambda: op.vmult(ou, opr, u, p, lin=None, mode=2))    # no linearisation state
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 1.0 / 16, 1)
    refused(-6, lambda: op.st_vmult(Alpha, Beta, 1, 1, [ou, opr], [u, p], lin=[ou, None], mode=2))
    refused(-1, lambda: op.st_vmult(Alpha, Beta, 1, 1, [ou, opr], [u, p], lin=[u, None], mode=5))
    refused(-1, lambda: op.st_vmult(Alpha, Beta, 1, 1, [ou, opr], [u, p], lin=[None, None], mode=1))
    refused(-6, lambda: op.st_vmult_slice_add([1.0, 1.0], [1.0, 0.0], 1, 1, [ou, opr], u, p, lin=ou, mode=1))
    refused(-1, lambda: op.st_vmult_slice_add([1.0, 1.0], [1.0, 0.0], 1, 1, [ou, opr], u, p, lin=u, mode=4))
