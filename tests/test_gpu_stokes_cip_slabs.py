"""The CIP interior-face term of the Stokes operator on z-slabs (stfem_stokes_set_cip_neighbours, _cip_pack, _cip_add_slab,
_cip_bind_ghosts): every slab of a cut treats its interface faces as interior, reads the neighbour through the ghost planes that the
neighbour's own cip_pack made on the device and through one ghost vertex plane, and leaves partial sums in its interface planes; the
slabs' results, summed on the host (stokes_slab_cases.assemble), are compared with the WHOLE-MESH numpy term of tests/cip_reference.py
(tests/test_cip_slab_contract_cpu.py shows the same for the numpy slab rule).  Bound: rel-L2 <= 1e-12 per velocity block, the bound of
tests/test_gpu_stokes_cip.py and tests/test_gpu_stokes_slabs.py.  Slabs, masks and cuts are those of tests/stokes_slab_cases.py."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import cip_slab_reference as csr  # noqa: E402
import navier_reference as nref  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
DELTA0 = 1.0
SOURCE, LIN = cref.SOURCE, cref.LINEARISATION
INVALID, ALIAS = -1, -6


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _operator(stfem, case, s, box=None, **kw):
    box = ssc.is_box(case) if box is None else box
    return stfem.StokesMatrixFreeOperator(s.ncell, vertices=None if box else s.vertices, lower=s.lower, upper=s.upper,
                                          dirichlet_mask=s.strong, viscosity=ssc.NU, weak_boundary_ids=ssc.faces_of(s.weak),
                                          outflow_boundary_ids=ssc.faces_of(s.outflow), penalty1=ssc.PENALTY1, penalty2=ssc.PENALTY2,
                                          dg_pressure=case.dg, **kw)


def _set_neighbours(op, verts, nc, s, box):
    lv, uv = (None, None) if box else csr.ghost_vertex_planes(verts, nc, s)
    op.set_cip_neighbours(csr.neighbour_mask(s), lv, uv)


def _slab_operators(stfem, case, verts=None, slabs=None, box=None, **kw):
    """the operators of all slabs of a cut, each told of its neighbours"""
    box = ssc.is_box(case) if box is None else box
    verts = ssc.vertices(case.mesh) if verts is None else verts
    slabs = ssc.slabs(case) if slabs is None else slabs
    nc = (slabs[0].ncell[0], slabs[0].ncell[1], slabs[-1].z1)
    ops = [_operator(stfem, case, s, box, **kw) for s in slabs]
    for op, s in zip(ops, slabs):
        _set_neighbours(op, verts, nc, s, box)
    return slabs, ops, nc


def _pack_ghosts(ops, slabs, srcs, hosts):
    """per slab (lower, upper): the device buffers its neighbours packed from their own source (one GPU: the buffer is handed over as
    it is); every packed buffer bit for bit the numpy pack"""
    def packed(r, side):
        buf = ops[r].initialize_dof_vector(0)  # (3 n_u >= 9 planes: room for the six)
        ops[r].cip_pack(srcs[r], side, buf)
        n = ops[r].cip_ghost_size
        assert n == 6 * csr.plane_size(slabs[r].ncell)
        assert np.array_equal(buf.download()[:n], csr.pack(hosts[r], slabs[r].ncell, slabs[r].strong, side))
        return buf
    return [(packed(r - 1, 1) if s.has_lower else None, packed(r + 1, 0) if s.has_upper else None) for r, s in enumerate(slabs)]


@functools.lru_cache(maxsize=None)
def _whole_cip(mesh, masks):
    case = ssc.Case(mesh, ssc.BOUNDS[mesh][0], masks, False, 0, None, True)
    U, _, W = ssc.fields(case)
    r = cref.cip(DELTA0, W, U, ssc.ncell(case), ssc.vertices(mesh), ssc.global_masks(case)[0])
    r.setflags(write=False)
    return r


ADD_CASES = [(mesh, bounds, masks) for mesh in ("pert", "box54", "box43") for bounds in ssc.BOUNDS[mesh] for masks in ("strong", "allweak")]


@pytest.mark.parametrize("mesh,bounds,masks", ADD_CASES, ids=["-".join([m, "".join(map(str, b)), k]) for m, b, k in ADD_CASES])
def test_cip_add_slab(mesh, bounds, masks, stfem):
    """the term by itself on every slab, w != u, added to a prefilled destination; constrained rows untouched; two runs bit for bit;
    without the neighbours (cip_add) the sum lacks the interface faces"""
    case = ssc.Case(mesh, bounds, masks, False, 0, None, True)
    slabs, ops, nc = _slab_operators(stfem, case)
    U, _, W = ssc.fields(case)
    hosts = [ssc.cut_velocity(U, nc, s.z0, s.z1) for s in slabs]
    srcs = [op.initialize_dof_vector(0, h) for op, h in zip(ops, hosts)]
    ghosts = _pack_ghosts(ops, slabs, srcs, hosts)
    parts, inner = [], []
    for op, s, u, (lo, up) in zip(ops, slabs, srcs, ghosts):
        w = op.initialize_dof_vector(0, ssc.cut_velocity(W, nc, s.z0, s.z1))
        init = np.random.default_rng(7).uniform(-1, 1, u.size)
        runs = []
        for _ in range(2):
            dst = op.initialize_dof_vector(0, init)
            op.cip_add_slab(dst, u, w, DELTA0, lo, up)
            runs.append(dst.download())
        assert np.array_equal(runs[0], runs[1])
        con = ssc.constrained3(s.ncell, s.strong)
        assert np.array_equal(runs[0][con], init[con])
        dst = op.initialize_dof_vector(0)
        op.cip_add_slab(dst, u, w, DELTA0, lo, up)
        parts.append(dst.download())
        assert np.allclose(runs[0] - init, parts[-1], rtol=0, atol=1e-13)  # added, not stored
        dst = op.initialize_dof_vector(0)
        op.cip_add(dst, u, w, DELTA0)
        inner.append(dst.download())
    whole = _whole_cip(mesh, masks)
    got = ssc.assemble(parts, 0, False, nc, bounds)
    err = ssc.rel(got, whole)
    planes = ssc.rel(ssc.interface_planes(got, 0, False, nc, bounds), ssc.interface_planes(whole, 0, False, nc, bounds))
    print(f"{mesh} {bounds} {masks}: rel-L2 {err:.2e}, interface planes {planes:.2e}")
    assert err <= TOL and planes <= TOL
    assert ssc.rel(ssc.assemble(inner, 0, False, nc, bounds), whole) > 1e-2


def _box_column():
    """1 x 1 x 3 cells on the unit cube cut into three one-cell slabs"""
    nc, upper = (1, 1, 3), (1.0, 1.0, 1.0)
    verts = cref.box_vertices(nc, (0, 0, 0), upper)
    return nc, upper, verts


@pytest.mark.parametrize("strong", [0, 63])
def test_one_cell_slab_between_two_neighbours(strong, stfem):
    """a 1 x 1 x 1 slab has no face of its own: with neighbours the launch must not return early"""
    nc, upper, verts = _box_column()
    case = ssc.Case("column", (0, 1, 2, 3), "none", False, 0, None, True)
    slabs = []
    for r in range(3):
        lo, hi = r > 0, r < 2
        s, _, _ = ssc.slab_masks(strong, 0, 0, lo, hi)
        slabs.append(ssc.Slab(r, r + 1, (1, 1, 1), ssc.slab_vertices(verts, nc, r, r + 1), (0.0, 0.0, r / 3), (1.0, 1.0, (r + 1) / 3), s, 0, 0,
                              lo, hi))
    _, ops, _ = _slab_operators(stfem, case, verts, slabs, box=True)
    rng = np.random.default_rng(5)
    U, W = rng.uniform(-1, 1, 3 * nref.n_velocity(nc)), rng.uniform(-1, 1, 3 * nref.n_velocity(nc))
    hosts = [ssc.cut_velocity(U, nc, s.z0, s.z1) for s in slabs]
    srcs = [op.initialize_dof_vector(0, h) for op, h in zip(ops, hosts)]
    ghosts = _pack_ghosts(ops, slabs, srcs, hosts)
    parts = []
    for op, s, u, (lo, up) in zip(ops, slabs, srcs, ghosts):
        dst = op.initialize_dof_vector(0)
        op.cip_add_slab(dst, u, op.initialize_dof_vector(0, ssc.cut_velocity(W, nc, s.z0, s.z1)), DELTA0, lo, up)
        parts.append(dst.download())
    whole = cref.cip(DELTA0, W, U, nc, verts, strong)
    assert np.linalg.norm(whole) > 0 and np.linalg.norm(parts[1]) > 0
    err = ssc.rel(ssc.assemble(parts, 0, False, nc, (0, 1, 2, 3)), whole)
    print(f"1 x 1 x 1 slabs, strong {strong}: rel-L2 {err:.2e}")
    assert err <= TOL


INTEGRATED = [("pert", (0, 1, 3, 4), "mixed", False), ("box43", (0, 1, 3), "zweak", True)]


def _bound_sources(ops, slabs, nc, fields_):
    """per slab the device vectors of the whole-mesh velocity fields, their ghost planes bound"""
    hosts = [[ssc.cut_velocity(x, nc, s.z0, s.z1) for s in slabs] for x in fields_]
    devs = [[op.initialize_dof_vector(0, h) for op, h in zip(ops, hs)] for hs in hosts]
    keep = []
    for hs, ds in zip(hosts, devs):
        ghosts = _pack_ghosts(ops, slabs, ds, hs)
        for op, d, (lo, up) in zip(ops, ds, ghosts):
            if lo is not None or up is not None:
                op.cip_bind_ghosts(d, lo, up)
        keep.append(ghosts)
    return devs, keep


@pytest.mark.parametrize("mode,weight", [(0, SOURCE), (0, LIN), (nref.JACOBIAN, SOURCE), (nref.JACOBIAN, LIN)])
@pytest.mark.parametrize("mesh,bounds,masks,dg", INTEGRATED)
def test_vmult(mesh, bounds, masks, dg, mode, weight, stfem):
    """set_cip + set_cip_neighbours + bound ghosts: vmult_convection in modes 0 and jacobian with both weight choices"""
    case = ssc.Case(mesh, bounds, masks, dg, mode, None, True)
    slabs, ops, nc = _slab_operators(stfem, case, delta0=DELTA0, cip_weight=weight)
    U, P, B = ssc.fields(case)
    strong, weak, outflow = ssc.global_masks(case)
    orc = ssc.stokes_oracle(nc, ssc.vertices(mesh), strong, weak, outflow, dg)
    ku, kp = cref.vmult(orc, DELTA0, weight, mode, B, U, P, nc, ssc.vertices(mesh), strong, weak & ~outflow, 0)
    ku0, _ = nref.vmult(orc, mode, B, U, P, nc, ssc.vertices(mesh), strong, weak & ~outflow, 0)
    assert ssc.rel(ku, ku0) > 1e-2  # the term is there
    (us,), keep = _bound_sources(ops, slabs, nc, [U])
    parts_u, parts_p = [], []
    for op, s, u in zip(ops, slabs, us):
        p = op.initialize_dof_vector(1, ssc.cut(P, 1, dg, nc, s.z0, s.z1))
        b = op.initialize_dof_vector(0, ssc.cut_velocity(B, nc, s.z0, s.z1))
        ou, opr = op.initialize_dof_vector(0, np.full(u.size, 7.0)), op.initialize_dof_vector(1, np.full(p.size, -3.0))
        op.vmult(ou, opr, u, p, lin=b if mode else None, mode=mode)
        parts_u.append(ou.download()); parts_p.append(opr.download())
        assert np.all(parts_u[-1][ssc.constrained3(s.ncell, s.strong)] == 0.0)
    eu = ssc.rel(ssc.assemble(parts_u, 0, dg, nc, bounds), ku)
    ep = ssc.rel(ssc.assemble(parts_p, 1, dg, nc, bounds), kp)
    print(f"{mesh} {masks} mode {mode} weight {weight}: velocity {eu:.2e} pressure {ep:.2e}")
    assert eu <= TOL and ep <= TOL


@pytest.mark.parametrize("scheme,variable_major", [("cg2", True), ("cg2", False), ("dg2x2", True)])
@pytest.mark.parametrize("mesh,bounds,masks,dg", INTEGRATED)
def test_st_vmult(mesh, bounds, masks, dg, scheme, variable_major, stfem):
    """st_vmult_convection, jacobian, the weight from the linearisation state: cG(2) x 1 step (two sources in the fused launch set, both
    block orders) and dG(2) x 2 steps (six sources, one launch set and one binding each)"""
    mode, weight = nref.JACOBIAN, LIN
    case = ssc.Case(mesh, bounds, masks, dg, mode, scheme, variable_major)
    slabs, ops, nc = _slab_operators(stfem, case, delta0=DELTA0, cip_weight=weight)
    blocks, lin, var = ssc.fields(case)
    Alpha, Beta, ns, nt, index = ssc.weights(scheme, variable_major)
    strong, weak, outflow = ssc.global_masks(case)
    verts = ssc.vertices(mesh)
    orc = ssc.stokes_oracle(nc, verts, strong, weak, outflow, dg)
    ref = cref.st_vmult(orc, DELTA0, weight, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, strong, weak & ~outflow, 0,
                        variable_major)
    vel = [j for j, v in enumerate(var) if v == 0]
    devs, keep = _bound_sources(ops, slabs, nc, [blocks[j] for j in vel])
    parts = []
    for r, (op, s) in enumerate(zip(ops, slabs)):
        src = [None] * len(var)
        for k, j in enumerate(vel):
            src[j] = devs[k][r]
        for j, v in enumerate(var):
            if v == 1:
                src[j] = op.initialize_dof_vector(1, ssc.cut(blocks[j], 1, dg, nc, s.z0, s.z1))
        dlin = [None if x is None else op.initialize_dof_vector(0, ssc.cut_velocity(x, nc, s.z0, s.z1)) for x in lin]
        dst = [op.initialize_dof_vector(v, np.full(x.size, 11.0)) for x, v in zip(src, var)]
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, variable_major, lin=dlin, mode=mode)
        parts.append([d.download() for d in dst])
    worst = 0.0
    for j, v in enumerate(var):
        assert np.linalg.norm(ref[j]) > 0
        worst = max(worst, ssc.rel(ssc.assemble([p[j] for p in parts], v, dg, nc, bounds), ref[j]))
    print(f"{mesh} {scheme} {'vm' if variable_major else 'tm'}: worst block {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("mesh,bounds,masks,dg", INTEGRATED)
def test_mask_zero_again_is_a_context_without_neighbours_bitwise(mesh, bounds, masks, dg, stfem):
    case = ssc.Case(mesh, bounds, masks, dg, nref.JACOBIAN, None, True)
    slabs, ops, nc = _slab_operators(stfem, case, delta0=DELTA0, cip_weight=LIN)
    U, P, B = ssc.fields(case)
    r = 1  # a slab with a lower neighbour (and, on pert, an upper one)
    s, op = slabs[r], ops[r]
    fresh = _operator(stfem, case, s, delta0=DELTA0, cip_weight=LIN)
    (us,), keep = _bound_sources(ops, slabs, nc, [U])

    def run(o, u=None):
        u = o.initialize_dof_vector(0, ssc.cut_velocity(U, nc, s.z0, s.z1)) if u is None else u
        p = o.initialize_dof_vector(1, ssc.cut(P, 1, dg, nc, s.z0, s.z1))
        b = o.initialize_dof_vector(0, ssc.cut_velocity(B, nc, s.z0, s.z1))
        ou, opr = o.initialize_dof_vector(0, np.full(u.size, 7.0)), o.initialize_dof_vector(1, np.full(p.size, -3.0))
        o.vmult(ou, opr, u, p, lin=b, mode=nref.JACOBIAN)
        add = o.initialize_dof_vector(0)
        o.cip_add_slab(add, u, b, DELTA0, *keep[0][r])  # (ghosts of a side without neighbour are not read)
        return ou.download(), opr.download(), add.download()

    with_nb, ref = run(op, us[r]), run(fresh)
    assert not np.array_equal(with_nb[0], ref[0]) and not np.array_equal(with_nb[2], ref[2])
    assert np.array_equal(with_nb[1], ref[1])
    op.set_cip_neighbours(0)
    assert all(np.array_equal(x, y) for x, y in zip(run(op, us[r]), ref))  # (the binding is still there and not looked at)
    assert all(np.array_equal(x, y) for x, y in zip(run(op), ref))
    _set_neighbours(op, ssc.vertices(mesh), nc, s, ssc.is_box(case))
    assert all(np.array_equal(x, y) for x, y in zip(run(op, us[r]), with_nb))


def test_ghost_arrays_of_ghost_size(stfem):
    """cip_ghost_vector: the six planes and no more; the same bits as with larger buffers; freeing one drops the bindings that name it,
    so the next integrated call is refused instead of reading freed memory"""
    case = ssc.Case("pert", (0, 1, 3, 4), "allweak", False, 0, None, True)
    slabs, ops, nc = _slab_operators(stfem, case, delta0=DELTA0)
    U, P, W = ssc.fields(case)
    hosts = [ssc.cut_velocity(U, nc, s.z0, s.z1) for s in slabs]
    srcs = [op.initialize_dof_vector(0, h) for op, h in zip(ops, hosts)]
    big = _pack_ghosts(ops, slabs, srcs, hosts)[1]
    op, s, u = ops[1], slabs[1], srcs[1]
    lo, up = op.cip_ghost_vector(), op.cip_ghost_vector()
    assert lo.size == up.size == op.cip_ghost_size == 6 * csr.plane_size(s.ncell)
    ops[0].cip_pack(srcs[0], 1, lo)
    ops[2].cip_pack(srcs[2], 0, up)
    w = op.initialize_dof_vector(0, ssc.cut_velocity(W, nc, s.z0, s.z1))
    outs = []
    for a, b in (big, (lo, up)):
        dst = op.initialize_dof_vector(0)
        op.cip_add_slab(dst, u, w, DELTA0, a, b)
        outs.append(dst.download())
    assert np.linalg.norm(outs[0]) > 0 and np.array_equal(outs[0], outs[1])
    p = op.initialize_dof_vector(1, ssc.cut(P, 1, False, nc, s.z0, s.z1))
    ou, opr = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
    op.cip_bind_ghosts(u, lo, up)
    op.vmult(ou, opr, u, p)
    first = ou.download()
    up.free()
    with pytest.raises(stfem.StfemError) as e:
        op.vmult(ou, opr, u, p)
    assert e.value.status == INVALID and np.array_equal(ou.download(), first)


def test_refusals_leave_the_destination_alone(stfem):
    case = ssc.Case("pert", (0, 1, 3, 4), "strong", False, 0, None, True)
    nc, verts = ssc.ncell(case), ssc.vertices("pert")
    s = ssc.slabs(case)[1]
    op = _operator(stfem, case, s)
    lv, uv = csr.ghost_vertex_planes(verts, nc, s)
    U, _, _ = ssc.fields(case)
    init = np.random.default_rng(7).uniform(-1, 1, 3 * op.n_velocity)
    u, w, dst = (op.initialize_dof_vector(0, x) for x in (ssc.cut_velocity(U, nc, s.z0, s.z1),) * 2 + (init,))
    p, dstp = op.initialize_dof_vector(1), op.initialize_dof_vector(1)
    glo, gup = op.initialize_dof_vector(0), op.initialize_dof_vector(0)

    def refused(status, call):
        with pytest.raises(stfem.StfemError) as e:
            call()
        assert e.value.status == status
        assert np.array_equal(dst.download(), init)

    refused(INVALID, lambda: op.set_cip_neighbours(48 | 1, lv, uv))   # a bit outside 4 / 5
    refused(INVALID, lambda: op.set_cip_neighbours(64, lv, uv))
    refused(INVALID, lambda: op.set_cip_neighbours(48, lv, None))     # general mesh: a vertex plane is missing
    refused(INVALID, lambda: op.set_cip_neighbours(16, None, uv))
    assert "vertex plane" in stfem.lib().stfem_last_error().decode()
    op.set_cip_neighbours(48, lv, uv)
    refused(INVALID, lambda: op.cip_add_slab(dst, u, w, DELTA0, glo, None))  # a ghost array is missing
    refused(INVALID, lambda: op.cip_add_slab(dst, u, w, DELTA0, None, gup))
    refused(ALIAS, lambda: op.cip_add_slab(dst, dst, w, DELTA0, glo, gup))
    refused(ALIAS, lambda: op.cip_add_slab(dst, u, dst, DELTA0, glo, gup))
    refused(ALIAS, lambda: op.cip_add_slab(dst, u, w, DELTA0, dst, gup))
    refused(INVALID, lambda: op.cip_add_slab(dst, u, w, float("nan"), glo, gup))
    # the integrated entry points: no binding, half a binding - nothing is launched, not even the linear part
    op.set_cip(DELTA0)
    refused(INVALID, lambda: op.vmult(dst, dstp, u, p))
    assert "bound" in stfem.lib().stfem_last_error().decode()
    op.cip_bind_ghosts(u, glo, None)
    refused(INVALID, lambda: op.vmult(dst, dstp, u, p))
    Alpha, Beta, ns, nt, _ = ssc.weights("cg2", True)
    u2 = op.initialize_dof_vector(0)
    op.cip_bind_ghosts(u, glo, gup)
    dsts = [dst, op.initialize_dof_vector(0), dstp, op.initialize_dof_vector(1)]
    refused(INVALID, lambda: op.st_vmult(Alpha, Beta, ns, nt, dsts, [u, u2, p, op.initialize_dof_vector(1)]))  # the second source
    op.cip_bind_ghosts(u, None, None)  # unbound again
    refused(INVALID, lambda: op.vmult(dst, dstp, u, p))
    op.cip_bind_ghosts(u, glo, gup)
    op.vmult(dst, dstp, u, p)
    assert not np.array_equal(dst.download(), init)
