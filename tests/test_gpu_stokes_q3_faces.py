"""GPU parity of the weak (Nitsche) faces of the Stokes operator at velocity degree 3 (include/stfem_stokes_boundary_space.h,
csrc/stfem_stokes_boundary.hip at DEG = 3) against the CPU oracle at pu = 3 with its weak mask.  Tolerance rel-L2 <= 1e-12 per block
(fp64), as in tests/test_gpu_stokes_q3.py; both pressure spaces.  The largest mesh has 5 x 4 x 3 cells."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stokes_q3_faces_reference as fr

pytestmark = pytest.mark.gpu
TOL = fr.TOL
DGP, DGP_IDS = fr.DGP, fr.DGP_IDS
SENTINEL = -123.25
UNSUPPORTED = -2


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
    monkeypatch.delenv("STFEM_STOKES_FACE_WORKGROUPS", raising=False)


def vmult(op, U, P):
    u, p = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))  # vmult overwrites
    op.vmult(ou, opr, u, p)
    return ou.download(), opr.download()


def time_blocks(stfem, orc, ns, nt, seed):
    """random source blocks in variable-major BlockSlice order and which variable each is"""
    rng = np.random.default_rng(seed)
    nb = 2 * nt * ns
    blocks, var = [None] * nb, [0] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[stfem.stokes_block_index(nt, it, 0, d)] = rng.uniform(-1, 1, 3 * orc.n_u)
            blocks[stfem.stokes_block_index(nt, it, 1, d)] = rng.uniform(-1, 1, orc.n_p)
            var[stfem.stokes_block_index(nt, it, 1, d)] = 1
    return blocks, var


def run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var, transpose=False):
    src = [op.initialize_dof_vector(v, b) for v, b in zip(var, blocks)]
    dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]  # st_vmult overwrites
    (op.st_Tvmult if transpose else op.st_vmult)(Alpha, Beta, ns, nt, dst, src)
    return [d.download() for d in dst]


# ---- 1. vmult on the four meshes
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("name", list(fr.OPERATOR_CASES))
def test_vmult_vs_oracle(name, dgp, stfem, oracle_mod):
    orc, ref = fr.operator_oracle(name, dgp), fr.operator_reference(name, dgp)
    op = fr.device_operator(stfem, name, dgp)
    assert (op.n_velocity, op.n_pressure) == (orc.n_u, orc.n_p)
    gu, gp = vmult(op, ref["U"], ref["P"])
    errs = rel(gu, ref["ku"]), rel(gp, ref["kp"])
    share = np.linalg.norm(ref["ku"] - ref["cell_u"]) / np.linalg.norm(ref["cell_u"])
    print(name, dgp, "vmult u %.2e p %.2e, the faces are %.2f of the cell part" % (*errs, share))
    assert share > 100 * TOL and rel(ref["kp"], ref["cell_p"]) > 100 * TOL  # a result without the faces cannot pass
    assert max(errs) < TOL
    m = op.initialize_dof_vector(0, np.full(3 * op.n_velocity, 5.0))
    op.mass_vmult(m, op.initialize_dof_vector(0, ref["U"]))  # the mass operator has no face term
    assert rel(m.download(), ref["mu"]) < TOL


# ---- 2. several sources per launch: the MULTI instantiation
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_st_vmult_Tvmult_and_slice_add(dgp, stfem, oracle_mod):
    name = "2x1x2_y_strong"
    orc, ref = fr.operator_oracle(name, dgp), fr.operator_reference(name, dgp)
    op = fr.device_operator(stfem, name, dgp)
    ns, nt = 1, 2
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    blocks, var = time_blocks(stfem, orc, ns, nt, 8)
    for transpose, oracle_call in ((False, orc.st_vmult), (True, orc.st_Tvmult)):
        want = oracle_call(Alpha, Beta, ns, nt, blocks)
        got = run_st_vmult(op, Alpha, Beta, ns, nt, blocks, var, transpose)
        for j in range(len(blocks)):
            print(dgp, "Tvmult" if transpose else "st_vmult", j, "%.2e" % rel(got[j], want[j]))
            if transpose:  # (blocks the reference's Tvmult leaves zero: the bound of test_reference_Tvmult in tests/test_gpu_stokes_q3.py)
                assert np.linalg.norm(got[j] - want[j]) <= TOL * max(np.linalg.norm(want[j]), 1.0), j
            else:
                assert np.linalg.norm(want[j]) > 0 and rel(got[j], want[j]) < TOL, j
        assert any(np.linalg.norm(w) > 0 for w in want)
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    init = [rng.uniform(-1, 1, ref["U"].size if v == 0 else ref["P"].size) for v in var]
    dst = [op.initialize_dof_vector(v, x) for v, x in zip(var, init)]
    op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, op.initialize_dof_vector(0, ref["U"]), op.initialize_dof_vector(1, ref["P"]))
    for j in range(nb):
        add = Gamma[j] * ref["ku"] + Zeta[j] * ref["mu"] if var[j] == 0 else Gamma[j] * ref["kp"]
        assert np.linalg.norm(dst[j].download() - init[j] - add) < TOL * np.linalg.norm(add), j


# ---- 3. the face points and the functional of the Dirichlet data
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
@pytest.mark.parametrize("name", ["5x4x3", "1x1x1_six_faces", "3x2x2_box"])
def test_face_points_and_nitsche_rhs(name, dgp, stfem, oracle_mod):
    nc, _, _, _, weak, _, _ = fr.OPERATOR_CASES[name]
    orc = fr.operator_oracle(name, dgp)
    op = fr.device_operator(stfem, name, dgp)
    face_cells = sum(nc[1 if f // 2 == 0 else 0] * nc[1 if f // 2 == 2 else 2] for f in range(6) if weak >> f & 1)
    assert op.n_face_points_space() == 16 * face_cells
    pts, want_pts = op.face_points_space(), orc.face_points()
    assert pts.shape == want_pts.shape and np.abs(pts - want_pts).max() <= 1e-14
    g = np.random.default_rng(3).uniform(-1, 1, pts.shape)
    init_u, init_p = np.random.default_rng(4).uniform(-1, 1, 3 * orc.n_u), np.random.default_rng(5).uniform(-1, 1, orc.n_p)
    du, dp = op.initialize_dof_vector(0, init_u), op.initialize_dof_vector(1, init_p)  # accumulated into
    op.nitsche_rhs_space(g, du, dp)
    ru, rp = orc.nitsche_rhs(g)
    errs = np.linalg.norm(du.download() - init_u - ru.reshape(-1)) / np.linalg.norm(ru), np.linalg.norm(dp.download() - init_p - rp) / np.linalg.norm(rp)
    print(name, dgp, "nitsche_rhs u %.2e p %.2e" % errs)
    assert max(errs) < TOL


@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_consistency_identity_on_the_device(dgp, stfem, oracle_mod):
    """vmult(u, p) - nitsche_rhs(g = u) = M (- nu Laplace u + grad p), zero pressure rows, for quadratic u and p on the sheared mesh"""
    op = stfem.StokesMatrixFreeOperator.with_degree(3, fr.IDENTITY_NC, vertices=fr.identity_vertices(), dirichlet_mask=0, viscosity=fr.IDENTITY_NU,
                                                    dg_pressure=dgp)
    op.set_weak_boundaries_space(range(6))
    U, P, F, g = fr.identity_fields(dgp)
    ku, kp = vmult(op, U, P)
    ru, rp = op.initialize_dof_vector(0, np.zeros(U.size)), op.initialize_dof_vector(1, np.zeros(P.size))
    op.nitsche_rhs_space(g(op.face_points_space()), ru, rp)
    mf = op.initialize_dof_vector(0, np.full(U.size, 5.0))
    op.mass_vmult(mf, op.initialize_dof_vector(0, F))
    scale = max(np.abs(ku).max(), np.abs(kp).max())
    dev_u, dev_p = np.abs(ku - ru.download() - mf.download()).max(), np.abs(kp - rp.download()).max()
    print(dgp, "max|vmult| %.3f deviation u %.2e p %.2e" % (scale, dev_u, dev_p))
    assert scale > 1.0 and max(dev_u, dev_p) <= 1e-12 * scale


# ---- 4. states that add no face term equal a context that never had faces, bit for bit
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_outflow_wins_and_mask_zero(dgp, stfem):
    name = "2x1x2_y_strong"
    nc, distort, seed, mask, weak, nu, _ = fr.OPERATOR_CASES[name]
    ref = fr.operator_reference(name, dgp)
    make = lambda: stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=fr.vertices_of(nc, distort, seed), dirichlet_mask=mask,  # noqa: E731
                                                              viscosity=nu, dg_pressure=dgp)
    never = vmult(make(), ref["U"], ref["P"])
    both = make()
    both.set_weak_boundaries_space([0, 3], outflow_boundary_ids=[0, 3, 5])  # every weak face is an outflow face too
    assert both.n_face_points_space() == 0
    cleared = fr.device_operator(stfem, name, dgp)
    cleared.set_weak_boundaries_space([])
    for op in (both, cleared):
        got = vmult(op, ref["U"], ref["P"])
        assert np.array_equal(got[0], never[0]) and np.array_equal(got[1], never[1])
        with pytest.raises(stfem.StfemError) as e:
            op.last_face_plan()  # nothing was launched
        assert e.value.status == UNSUPPORTED
    assert rel(never[0], ref["cell_u"]) < TOL


# ---- 5. several boundary cells per wave, reproducibility
@pytest.mark.parametrize("dgp", DGP, ids=DGP_IDS)
def test_capped_launches_and_reproducible(dgp, stfem, oracle_mod, monkeypatch):
    """5 x 4 x 3 cells, weak faces 0, 2, 5: 47 boundary cells.  One workgroup walks them in 12 rounds of its four waves; the result equals
    the uncapped run bit for bit (the cell -> wave assignment changes no sum), and a repeated run equals the first bit for bit"""
    orc = fr.operator_oracle(fr.CAPPED, dgp)
    op = fr.device_operator(stfem, fr.CAPPED, dgp)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    blocks, var = time_blocks(stfem, orc, 1, 2, 4)
    free = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    assert op.last_face_plan() == (12, 1)
    again = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    monkeypatch.setenv("STFEM_STOKES_FACE_WORKGROUPS", "1")
    capped = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    plan = op.last_face_plan()
    assert plan[0] == 1 and plan[1] > 1, plan
    capped_again = run_st_vmult(op, Alpha, Beta, 1, 2, blocks, var)
    want = orc.st_vmult(Alpha, Beta, 1, 2, blocks)
    for j in range(4):
        assert np.array_equal(again[j], free[j]) and np.array_equal(capped[j], free[j]) and np.array_equal(capped_again[j], free[j]), j
        assert rel(free[j], want[j]) < TOL, j
    ref = fr.operator_reference(fr.CAPPED, dgp)
    single = vmult(op, ref["U"], ref["P"])  # one source, still capped
    monkeypatch.delenv("STFEM_STOKES_FACE_WORKGROUPS")
    assert all(np.array_equal(a, b) for a, b in zip(single, vmult(op, ref["U"], ref["P"])))


# ---- 6. refusals
def test_refusals(stfem):
    L = stfem.lib()
    op = fr.device_operator(stfem, "3x2x2_box", True)
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
    lin_desc = stfem._StokesVankaLinearisedSpaceDesc()
    lin_desc.n_blocks, lin_desc.block_variable, lin_desc.Alpha, lin_desc.Beta = 2, var, stfem._p(A), stfem._p(A)
    lin_desc.mode, lin_desc.lin_blocks = 1, two(u.ptr, None)
    calls = {
        # the entries of stfem.h keep refusing a degree-3 context
        "stfem_stokes_set_weak_boundaries": (lambda: L.stfem_stokes_set_weak_boundaries(h, 1, 0, 20.0, 10.0), "velocity degree 2 only"),
        "stfem_stokes_n_face_points": (lambda: L.stfem_stokes_n_face_points(h), "velocity degree 2 only"),
        "stfem_stokes_face_points": (lambda: L.stfem_stokes_face_points(h, hp), "velocity degree 2 only"),
        "stfem_stokes_nitsche_rhs": (lambda: L.stfem_stokes_nitsche_rhs(h, hp, du.ptr, dp.ptr, None), "velocity degree 2 only"),
        # a convection mode on a degree-3 context with weak faces
        "stfem_stokes_vmult_convection_space": (lambda: L.stfem_stokes_vmult_convection_space(h, 1, du.ptr, dp.ptr, u.ptr, p.ptr, u.ptr, None),
                                                "inflow term"),
        "stfem_stokes_st_vmult_convection_space": (lambda: L.stfem_stokes_st_vmult_convection_space(
            h, 2, 1, 1, 1, stfem._p(A), stfem._p(A), two(du.ptr, dp.ptr), two(u.ptr, p.ptr), two(u.ptr, None), None), "inflow term"),
        "stfem_stokes_st_vmult_slice_add_convection_space": (lambda: L.stfem_stokes_st_vmult_slice_add_convection_space(
            h, 1, 1, 1, 1, stfem._p(np.ones(2)), stfem._p(np.ones(2)), two(du.ptr, dp.ptr), u.ptr, p.ptr, u.ptr, None), "inflow term"),
        "stfem_stokes_vanka_create_linearised_space": (lambda: L.stfem_stokes_vanka_create_linearised_space(h, C.byref(lin_desc), C.byref(out)),
                                                       "inflow term"),
    }
    q2 = stfem.StokesMatrixFreeOperator((2, 2, 2), dg_pressure=True)
    for name, (call, reason) in calls.items():
        L.stfem_stokes_set_weak_boundaries(q2._h, 0, 0, 20.0, 10.0)  # (a successful call in between: the reason below is this call's)
        status = call()
        why = L.stfem_last_error().decode()
        assert status == UNSUPPORTED, (name, status, why)
        assert name in why and reason in why, (name, why)
        assert not out.value, name
    assert np.all(du.download() == SENTINEL) and np.all(dp.download() == SENTINEL) and np.all(host == SENTINEL)
    # the Python wrappers raise the same status, the keyword of the constructor too; the linear operator and its blocks still run
    for call in (op.face_points, lambda: op.vmult(du, dp, u, p, lin=u, mode=1),
                 lambda: stfem.StokesPreconditionVanka.for_space(op, [0, 1], A, A, lin=[u, None], mode=1),
                 lambda: stfem.StokesMatrixFreeOperator.with_degree(3, (2, 2, 2), weak_boundary_ids=[0])):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert op.weak_mask == 0b000011 and op.n_face_points_space() == 16 * 2 * 2 * 2  # no refused call changed the faces
    op.vmult(du, dp, u, p)
    assert np.all(du.download() != SENTINEL)


# ---- 7. degree 2: the _space forms are the entries without the suffix
@pytest.mark.parametrize("dgp", DGP, ids=["FE_Q1", "FE_DGP1"])
def test_degree_2_space_forms_equal_the_entries_bitwise(dgp, stfem):
    nc, mask, weak, nu = (3, 2, 2), 0b110000, [0, 1, 2], 0.6
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=3)
    old = stfem.StokesMatrixFreeOperator(nc, vertices=verts, dirichlet_mask=mask, viscosity=nu, dg_pressure=dgp, weak_boundary_ids=weak,
                                         penalty1=15.0, penalty2=7.0)
    new = stfem.StokesMatrixFreeOperator.with_degree(2, nc, vertices=verts, dirichlet_mask=mask, viscosity=nu, dg_pressure=dgp)
    new.set_weak_boundaries_space(weak, penalty1=15.0, penalty2=7.0)
    assert new.n_face_points_space() == stfem.lib().stfem_stokes_n_face_points(old._h) == 9 * (2 * 2 + 2 * 2 + 3 * 2)
    assert np.array_equal(new.face_points_space(), old.face_points())
    rng = np.random.default_rng(2)
    U, P = rng.uniform(-1, 1, 3 * old.n_velocity), rng.uniform(-1, 1, old.n_pressure)
    g = rng.uniform(-1, 1, (new.n_face_points_space(), 3))
    res = []
    for op, rhs in ((old, old.nitsche_rhs), (new, new.nitsche_rhs_space)):
        ku, kp = vmult(op, U, P)
        ru, rp = op.initialize_dof_vector(0, np.zeros(U.size)), op.initialize_dof_vector(1, np.zeros(P.size))
        rhs(g, ru, rp)
        res.append([ku, kp, ru.download(), rp.download()])
        assert op.last_face_plan()[1] == 1
    assert all(np.linalg.norm(a) > 0 for a in res[0])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
