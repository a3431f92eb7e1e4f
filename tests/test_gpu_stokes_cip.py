"""GPU parity of the CIP interior-face term of the Stokes operator (stfem_stokes_set_cip, stfem_stokes_cip_add) against the numpy
restatement tests/cip_reference.py on top of the linear oracle and the convection restatement.  Tolerance rel-L2 <= 1e-12, the
project's fp64 parity tolerance; random fields in [-1, 1]; tests/test_cip_reference_cpu.py::test_gpu_cases_are_not_hollow keeps the
term at least a tenth of the linear result on every mesh and mask used here.  Meshes (cip_reference.MESHES): a lone cell (no face, no
launch), 2 x 1 x 1 (the closed form), 1 x 1 x 3 (one direction only), 2 x 2 x 2, 3 x 2 x 4 perturbed, and 4 x 3 x 2 on a box with three
different edge lengths (all colours, cells with neighbours on both sides, h_F different per direction, cell counts no multiple of
8).  Cartesian meshes run without vertices (Kronecker path + CART kernel), the perturbed one with."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import navier_reference as nref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
NU = cref.NU
SOURCE, LIN = cref.SOURCE, cref.LINEARISATION


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@functools.lru_cache(maxsize=None)
def _vertices(mesh):
    return cref.mesh_vertices(mesh)


@functools.lru_cache(maxsize=None)
def _cip(mesh, mask, delta0, wseed, useed):
    """C(w; u) of the restatement for fields drawn from the two seeds (computed once, shared, never modified)"""
    nc = cref.MESHES[mesh][0]
    r = cref.cip(delta0, _field(nc, wseed), _field(nc, useed), nc, _vertices(mesh), mask)
    r.setflags(write=False)
    return r


def _field(nc, seed):
    return np.random.default_rng(seed).uniform(-1, 1, 3 * nref.n_velocity(nc))


def _operator(stfem, mesh, mask, dg=False, weak=(), outflow=(), delta0=0.0, weight=SOURCE):
    from oracle import oracle
    nc, lower, upper, distort = cref.MESHES[mesh]
    verts = _vertices(mesh)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, lower=lower, upper=upper, dirichlet_mask=mask,
                                        viscosity=NU, dg_pressure=dg, weak_boundary_ids=weak, outflow_boundary_ids=outflow,
                                        delta0=delta0, cip_weight=weight)
    wm = sum(1 << f for f in weak) & ~sum(1 << f for f in outflow)
    orc = oracle.StokesOracle(nc, verts, mask, NU, weak_mask=wm, dg_pressure=dg)
    assert (op.n_velocity, op.n_pressure) == (orc.n_u, orc.n_p)
    return op, orc, nc, verts, wm


@pytest.mark.parametrize("mask", cref.MASKS)
@pytest.mark.parametrize("mesh", list(cref.MESHES))
def test_cip_add(mesh, mask, stfem):
    """the primitive by itself, w != u and w = u: added to a prefilled destination, constrained rows untouched, two calls equal"""
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask)
    delta0 = cref.delta0_of(mesh, mask)
    U, W, INIT = _field(nc, cref.FIELD_SEED), _field(nc, 6), _field(nc, 7)
    u, w = op.initialize_dof_vector(0, U), op.initialize_dof_vector(0, W)
    con = np.tile(nref.constrained(nc, mask), 3)
    for wdev, wseed in ((w, 6), (u, cref.FIELD_SEED)):
        ref = _cip(mesh, mask, delta0, wseed, cref.FIELD_SEED)
        runs = []
        for _ in range(2):
            dst = op.initialize_dof_vector(0, INIT)
            op.cip_add(dst, u, wdev, delta0)
            runs.append(dst.download())
        got = runs[0]
        assert np.array_equal(runs[0], runs[1])
        assert np.array_equal(got[con], INIT[con])
        if mesh == "cell":
            assert not ref.any() and np.array_equal(got, INIT)  # no face: nothing is launched
            continue
        assert np.linalg.norm(ref) > 0.1
        err = np.linalg.norm(got - (INIT + ref)) / np.linalg.norm(ref)
        print(f"{mesh} mask {mask} w {'= u' if wdev is u else '!= u'}: rel-L2 {err:.2e}")
        assert err <= TOL
    # delta0 scales the term; 0 launches nothing
    dst = op.initialize_dof_vector(0, INIT)
    op.cip_add(dst, u, w, 0.0)
    assert np.array_equal(dst.download(), INIT)


def test_closed_form(stfem):
    """[0, 2] x [0, 1]^2, 2 x 1 x 1 cells, u = (|x - 1|, 0, 0), w = (0.7, 0, 0), delta0 = 3: u . C(w; u) = 3 / 2^3.5 * 0.49 * 4"""
    op, orc, nc, verts, _ = _operator(stfem, "pair", 0)
    X = cref.dof_points(nc, verts)
    z = np.zeros(len(X))
    U, W = np.concatenate([np.abs(X[:, 0] - 1.0), z, z]), np.concatenate([np.full(len(X), 0.7), z, z])
    dst = op.initialize_dof_vector(0)
    op.cip_add(dst, op.initialize_dof_vector(0, U), op.initialize_dof_vector(0, W), 3.0)
    val, exact = U @ dst.download(), 3.0 / 2 ** 3.5 * 0.49 * 4.0
    print(f"closed form: {val!r} against {exact!r}")
    assert abs(val - exact) <= TOL * exact


def test_cip_add_refusals_leave_the_destination_alone(stfem):
    op, orc, nc, verts, _ = _operator(stfem, "cube", 63)
    U, INIT = _field(nc, 5), _field(nc, 7)
    u, w, dst = op.initialize_dof_vector(0, U), op.initialize_dof_vector(0, U), op.initialize_dof_vector(0, INIT)

    def refused(status, call):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == status
        assert np.array_equal(dst.download(), INIT)

    refused(-6, lambda: op.cip_add(dst, dst, w, 1.0))   # STFEM_ERR_ALIAS
    refused(-6, lambda: op.cip_add(dst, u, dst, 1.0))
    refused(-1, lambda: op.cip_add(None, u, w, 1.0))    # STFEM_ERR_INVALID_ARGUMENT
    refused(-1, lambda: op.cip_add(dst, None, w, 1.0))
    refused(-1, lambda: op.cip_add(dst, u, None, 1.0))
    refused(-1, lambda: op.cip_add(dst, u, w, float("nan")))
    refused(-1, lambda: op.set_cip(float("inf")))
    refused(-1, lambda: op.set_cip(1.0, 2))
    refused(-1, lambda: op.set_cip(1.0, -1))
    assert (op.delta0, op.cip_weight) == (0.0, SOURCE)
    op.cip_add(dst, u, u, 1.0)  # weight_u may be src_u
    assert not np.array_equal(dst.download(), INIT)


@pytest.mark.parametrize("weight", [SOURCE, LIN])
@pytest.mark.parametrize("mode", [0, nref.FORM, nref.JACOBIAN])
@pytest.mark.parametrize("mask,dg", [(63, False), (0b111011, True), (0, False), (0, True)])
@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_vmult(mesh, mask, dg, mode, weight, stfem):
    """vmult after set_cip in the three modes with both weight choices and both pressure spaces; dst_p is bit for bit that of a context
    without the term; with choice 1 and a mode the weight is lin, and that result is another one"""
    delta0 = cref.delta0_of(mesh, mask)
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, dg, delta0=delta0, weight=weight)
    plain, _, _, _, _ = _operator(stfem, mesh, mask, dg)
    rng = np.random.default_rng(cref.FIELD_SEED)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    assert np.array_equal(U, _field(nc, cref.FIELD_SEED))
    ku, kp = cref.vmult(orc, delta0, weight, mode, B, U, P, nc, verts, mask)
    results = []
    for o in (op, plain):
        u, p, b = o.initialize_dof_vector(0, U), o.initialize_dof_vector(1, P), o.initialize_dof_vector(0, B)
        ou, opr = o.initialize_dof_vector(0, np.full(U.size, 7.0)), o.initialize_dof_vector(1, np.full(P.size, -3.0))  # overwritten
        if mode:
            o.vmult(ou, opr, u, p, lin=b, mode=mode)
        else:
            o.vmult(ou, opr, u, p)
        results.append((ou.download(), opr.download()))
    (got, gotp), (got0, gotp0) = results
    err = rel(got, ku)
    print(f"{mesh} mask {mask} dg {dg} mode {mode} weight {weight}: rel-L2 {err:.2e}")
    assert np.linalg.norm(got - ku) <= TOL * np.linalg.norm(ku), err
    assert np.array_equal(gotp, gotp0)
    assert np.linalg.norm(gotp - kp) <= TOL * np.linalg.norm(kp) + 1e-14
    assert rel(got, got0) > 1e-2  # the term is there
    con = np.tile(nref.constrained(nc, mask), 3)
    assert np.all(got[con] == 0.0)
    other, _ = cref.vmult(orc, delta0, 1 - weight, mode, B, U, P, nc, verts, mask)
    if mode:
        assert rel(other, ku) > 1e-3 and rel(got, other) > 1e-3  # the two weight choices are two operators
    else:
        assert np.array_equal(other, ku)  # mode 0: choice 1 falls back to the source


WEAK, OUTFLOW, WEAK_DIRICHLET = (0, 1, 5), (3,), 0b010100  # faces 2 and 4 stay strong


@pytest.mark.parametrize("mode,weight", [(nref.FORM, SOURCE), (nref.JACOBIAN, LIN)])
@pytest.mark.parametrize("outflow", [(), OUTFLOW])
@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_weak_and_outflow_faces(mesh, outflow, mode, weight, stfem):
    """after the Nitsche and inflow launches of the weak faces 0, 1, 5, with and without the outflow face 3"""
    op, orc, nc, verts, wm = _operator(stfem, mesh, WEAK_DIRICHLET, mesh == "box", WEAK, outflow, delta0=1.0, weight=weight)
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = cref.vmult(orc, 1.0, weight, mode, B, U, P, nc, verts, WEAK_DIRICHLET, wm)
    u, p, b = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P), op.initialize_dof_vector(0, B)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))
    op.vmult(ou, opr, u, p, lin=b, mode=mode)
    assert np.linalg.norm(ou.download() - ku) <= TOL * np.linalg.norm(ku), rel(ou.download(), ku)
    assert np.linalg.norm(opr.download() - kp) <= TOL * np.linalg.norm(kp) + 1e-14


def _weights(stfem, scheme, variable_major):
    """(Alpha, Beta, ns, nt, index): cG(2), one step - four blocks, two sources, the fused launch set; dG(2), two steps - six sources,
    one set of launches per source"""
    if scheme == "cg2":
        ns, nt = 1, 2
        A, B, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, ns)
    else:
        ns, nt = 2, 3
        A, B, _, _ = stfem.get_fe_time_weights_stokes(stfem.DG, 2, 1.0 / 16, ns)
    nb = 2 * nt * ns
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


@pytest.mark.parametrize("mode,weight", [(0, SOURCE), (nref.JACOBIAN, SOURCE), (nref.JACOBIAN, LIN), (nref.FORM, LIN)])
@pytest.mark.parametrize("scheme,variable_major", [("cg2", True), ("cg2", False), ("dg2x2", True)])
@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_st_vmult(mesh, scheme, variable_major, mode, weight, stfem):
    """cG(2) x 1 step: two sources in the fused launch set (MULTI), both block orderings; dG(2) x 2 steps: six sources, one set each"""
    mask, dg = 0b111011, mesh == "box"
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, dg, delta0=1.0, weight=weight)
    Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, op, orc, scheme, variable_major)
    ref = cref.st_vmult(orc, 1.0, weight, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, mask, variable_major=variable_major)
    base = nref.st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, mask, variable_major=variable_major)
    runs = []
    for _ in range(2):
        dst = [op.initialize_dof_vector(v, np.full(b.size, 11.0)) for v, b in zip(var, blocks)]
        if mode:
            op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major, lin=dlin, mode=mode)
        else:
            op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major)
        runs.append([d.download() for d in dst])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
    for j in range(len(blocks)):
        assert np.linalg.norm(ref[j]) > 0
        if var[j] == 0:
            assert rel(ref[j], base[j]) > 1e-2  # the term is there
        assert np.linalg.norm(runs[0][j] - ref[j]) <= TOL * np.linalg.norm(ref[j]) + 1e-14, (j, rel(runs[0][j], ref[j]))


@pytest.mark.parametrize("mode,weight", [(0, SOURCE), (nref.FORM, SOURCE), (nref.FORM, LIN)])
@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_st_vmult_slice_add(mesh, mode, weight, stfem):
    """onto non-zero destinations, one Gamma entry zero (that destination gets the mass part alone, and no CIP term)"""
    mask = 63
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, False, delta0=1.0, weight=weight)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[stfem.stokes_block_index(nt, 1, 0, 0)] = 0.0
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)
    ku, kp = cref.vmult(orc, 1.0, weight, mode, B, U, P, nc, verts, mask)
    ku0, _ = nref.vmult(orc, mode, B, U, P, nc, verts, mask)
    assert rel(ku, ku0) > 1e-2
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    init = [rng.uniform(-1, 1, 3 * orc.n_u if (j // nt) % 2 == 0 else orc.n_p) for j in range(nb)]
    dst = [op.initialize_dof_vector((j // nt) % 2, init[j]) for j in range(nb)]
    if mode:
        op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P),
                              lin=op.initialize_dof_vector(0, B), mode=mode)
    else:
        op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P))
    for it in range(ns):
        for d in range(nt):
            ju, jp = stfem.stokes_block_index(nt, it, 0, d), stfem.stokes_block_index(nt, it, 1, d)
            assert rel(dst[ju].download(), init[ju] + Gamma[ju] * ku + Zeta[ju] * mu.reshape(-1)) < TOL
            assert rel(dst[jp].download(), init[jp] + Gamma[jp] * kp) < TOL


@pytest.mark.parametrize("mesh", ["pert", "box"])
def test_delta0_zero_again_is_a_fresh_context_bitwise(mesh, stfem):
    """set_cip(0.0, .) after a non-zero value: vmult, st_vmult and mass_vmult as on a context that never had the term"""
    mask = 0b111010
    op, orc, nc, verts, _ = _operator(stfem, mesh, mask, mesh == "box", (0,), (), delta0=2.0, weight=LIN)
    fresh, _, _, _, _ = _operator(stfem, mesh, mask, mesh == "box", (0,), ())
    rng = np.random.default_rng(5)
    U, P, B = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, 3 * orc.n_u)

    def run(o):
        out = []
        u, p, b = o.initialize_dof_vector(0, U), o.initialize_dof_vector(1, P), o.initialize_dof_vector(0, B)
        for mode in (0, nref.JACOBIAN):
            ou, opr = o.initialize_dof_vector(0, np.full(U.size, 7.0)), o.initialize_dof_vector(1, np.full(P.size, -3.0))
            o.vmult(ou, opr, u, p, lin=b if mode else None, mode=mode)
            out += [ou.download(), opr.download()]
        Alpha, Beta, ns, nt, index, blocks, lin, var, src, dlin = _st_problem(stfem, o, orc, "cg2", True)
        dst = [o.initialize_dof_vector(v, np.full(b_.size, 11.0)) for v, b_ in zip(var, blocks)]
        o.st_vmult(Alpha, Beta, ns, nt, dst, src, True, lin=dlin, mode=nref.FORM)
        out += [d.download() for d in dst]
        ou = o.initialize_dof_vector(0, np.full(U.size, 7.0))
        o.mass_vmult(ou, u)
        out.append(ou.download())
        return out

    with_term, ref = run(op), run(fresh)
    assert not np.array_equal(with_term[0], ref[0]) and not np.array_equal(with_term[2], ref[2])
    assert np.array_equal(with_term[-1], ref[-1])  # mass_vmult never gets the term
    op.set_cip(0.0, LIN)
    assert all(np.array_equal(x, y) for x, y in zip(run(op), ref))
    op.set_cip(2.0, LIN)
    assert all(np.array_equal(x, y) for x, y in zip(run(op), with_term))


@pytest.mark.parametrize("mesh,per_cell", [("box", False), ("box", True), ("pert", True)])
def test_vanka_blocks_are_built_without_the_term(mesh, per_cell, stfem):
    """StokesPreconditionVanka (class blocks on a box; per cell, with update) created on a context with delta0 = 1 applies bit for bit
    like one created on a context without: the smoother is that of the operator without the stabilisation"""
    mask = 0b111011
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 1.0 / 16, 1)
    outs = []
    for delta0 in (1.0, 0.0):
        op, orc, nc, verts, _ = _operator(stfem, mesh, mask, False, delta0=delta0, weight=LIN)
        rng = np.random.default_rng(21)
        R = [rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)]
        B = rng.uniform(-1, 1, 3 * orc.n_u)
        src = [op.initialize_dof_vector(v, r) for v, r in enumerate(R)]
        lin = [op.initialize_dof_vector(0, B), None]
        if per_cell:
            vk = stfem.StokesPreconditionVanka(op, [0, 1], Alpha, Beta, lin=[op.initialize_dof_vector(0, 0.5 * B), None],
                                               mode=nref.JACOBIAN)
            vk.update(lin)
        else:
            vk = stfem.StokesPreconditionVanka(op, [0, 1], Alpha, Beta)
        dst = [op.initialize_dof_vector(v) for v in (0, 1)]
        vk.vmult(dst, src)
        outs.append([d.download() for d in dst])
        assert np.linalg.norm(outs[-1][0]) > 0
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
