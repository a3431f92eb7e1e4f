"""The Stokes / Navier-Stokes operator at velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), stfem_stokes_create_space) on z-slabs of a
partitioned mesh: every kernel family of the degree on slabs whose interface faces are out of the strong mask, the weak set
and the outflow set, the partial sums of the interface planes added (on the host: tests/stokes_q3_slab_cases.py::assemble; on the
device: stfem_plane_pack -> copy -> stfem_plane_unpack(add) on the scalar views of the blocks - a scalar FE_Q(3) context for a velocity
block, stfem_stokes_pressure_ctx_space for an FE_Q(2) pressure block).  The degree-3 counterpart of tests/test_gpu_stokes_slabs.py.

Every expected value is a WHOLE-MESH reference: oracle.StokesOracle at pu = 3, plus tests/navier_q3_reference.py for the convection
modes, tests/stokes_pressure_q3_reference.py for the divergence, tests/cip_q3_reference.py for the CIP term;
tests/test_stokes_q3_slab_assembly_cpu.py shows that the references on the same slabs, cut and assembled by the same helpers,
reproduce them to 1e-16, and that the table reaches what it is for.  Bounds: rel-L2 <= 1e-12 per block (the project's fp64 parity
bound), the same bound on the interface planes alone, rows of strongly constrained velocity DoFs exactly 0 on every slab.  Each test
prints its largest ratio to the bound ("ratio <group> <value>").

The CIP term is held to the documented contract of the degree: a slab's term has no interface face
(stfem_stokes_set_cip_neighbours refuses a degree-3 context), so the slabs' sum equals the whole-mesh term except on the two cell
layers at every interface, where it lacks exactly the interface faces' part."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402
import stokes_pressure_q3_reference as p3  # noqa: E402
import stokes_q3_slab_cases as s3  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
UNSUPPORTED = -2
CAPS = ("STFEM_STOKES_Q3_WORKGROUPS", "STFEM_STOKES_FACE_WORKGROUPS", "STFEM_STOKES_CIP_WORKGROUPS")


@pytest.fixture(scope="module")
def stfem(oracle_mod):
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    for name in CAPS:
        monkeypatch.delenv(name, raising=False)


def _slab_operator(stfem, s, box, dg, mode=0):
    op = stfem.StokesMatrixFreeOperator.with_degree(3, s.ncell, vertices=None if box else s.vertices, lower=s.lower, upper=s.upper,
                                                    dirichlet_mask=s.strong, viscosity=s3.viscosity(mode), dg_pressure=dg)
    if s.weak or s.outflow:
        op.set_weak_boundaries_space(s3.faces_of(s.weak), s3.faces_of(s.outflow), penalty1=s3.PENALTY1, penalty2=s3.PENALTY2)
    assert op.velocity_degree == 3 and (op.n_velocity, op.n_pressure) == s3.sizes(s.ncell, dg)
    return op


def _operator(stfem, case, s):
    """the slab's operator: general meshes get the slab's vertices, a box none (the constant-Jacobian instantiation); the weak / outflow
    faces through the _space setter, and only where the slab has any"""
    return _slab_operator(stfem, s, s3.is_box(case), case.dg, case.mode)


class _Worst:
    def __init__(self, group):
        self.group, self.value = group, 0.0

    def check(self, got, want, what, zero_ok=False):
        if zero_ok and not np.any(want):  # the reference receives no contribution here: neither may the kernels' result
            assert not np.any(got), what
            return
        assert np.linalg.norm(want) > 0, what
        err = s3.rel(got, want)
        self.value = max(self.value, err / TOL)
        assert err <= TOL, (what, err)

    def report(self):
        print(f"ratio {self.group} {self.value:.3e}")


def _check_assembled(worst, case, parts_per_block, whole, variables, what="", zero_ok=False):
    """the sum of the slabs' blocks against the whole-mesh reference: per block, and on the interface planes alone (a face functional
    may leave those without any contribution: then exactly 0)"""
    nc = s3.ncell(case)
    for b, v in enumerate(variables):
        got = s3.assemble([p[b] for p in parts_per_block], v, case.dg, nc, case.bounds)
        worst.check(got, whole[b], (what, "block", b), zero_ok)
        planes = s3.interface_planes(got, v, case.dg, nc, case.bounds)
        if planes is not None:
            worst.check(planes, s3.interface_planes(whole[b], v, case.dg, nc, case.bounds), (what, "interface planes of block", b), zero_ok)


# ---------------------------------------------------------------------------------------------------------------- vmult

@pytest.mark.parametrize("case", s3.VMULT_CASES, ids=s3.case_id)
def test_vmult(case, stfem):
    """mode 0 on six mask sets and both pressure spaces, form / jacobian on the masks without a weak face; 2 and 3 slabs with the
    one-layer slabs; lin cut like the source; destinations pre-filled; a second call replays bit for bit; one call with lin = source"""
    nc = s3.ncell(case)
    U, P, B = s3.fields(case)
    worst = _Worst("modes" if case.mode else "operator")
    parts, picard = [], []
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        u, p, b = (op.initialize_dof_vector(v, s3.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in ((U, 0), (P, 1), (B, 0)))
        ou, opr = op.initialize_dof_vector(0, np.full(u.size, 7.0)), op.initialize_dof_vector(1, np.full(p.size, -3.0))  # overwritten
        lin = b if case.mode else None
        op.vmult(ou, opr, u, p, lin=lin, mode=case.mode)
        got = (ou.download(), opr.download())
        assert np.all(got[0][s3.constrained3(s.ncell, s.strong)] == 0.0)
        op.vmult(ou, opr, u, p, lin=lin, mode=case.mode)
        assert np.array_equal(ou.download(), got[0]) and np.array_equal(opr.download(), got[1])
        parts.append(got)
        if case.mode:
            op.vmult(ou, opr, u, p, lin=u, mode=case.mode)
            picard.append((ou.download(), opr.download()))
            assert np.all(picard[-1][0][s3.constrained3(s.ncell, s.strong)] == 0.0)
    _check_assembled(worst, case, parts, s3.whole_vmult(case.mesh, case.masks, case.dg, case.mode), (0, 1))
    if case.mode:
        _check_assembled(worst, case, picard, s3.whole_vmult(case.mesh, case.masks, case.dg, case.mode, True), (0, 1), "picard")
    worst.report()


# ------------------------------------------------------------------------------------------------------------- st_vmult

def _st_on_slabs(stfem, case):
    """the space-time vmult on every slab, destinations pre-filled: [dict(slab, op, dst, var)]"""
    nc = s3.ncell(case)
    blocks, lin, var = s3.fields(case)
    Alpha, Beta, ns, nt, _ = s3.weights(case.scheme, case.variable_major)
    ranks = []
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        src = [op.initialize_dof_vector(v, s3.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in zip(blocks, var)]
        dst = [op.initialize_dof_vector(v, np.full(x.size, 11.0)) for x, v in zip(src, var)]
        dlin = None
        if case.mode:  # (pressure entries: null)
            dlin = [None if x is None else op.initialize_dof_vector(0, s3.cut_velocity(x, nc, s.z0, s.z1)) for x in lin]
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, case.variable_major, lin=dlin, mode=case.mode)
        ranks.append(dict(slab=s, op=op, dst=dst, var=var, src=src, lin=dlin))
    return ranks


@pytest.mark.parametrize("case", s3.ST_CASES, ids=s3.case_id)
def test_st_vmult(case, stfem):
    """cG(2) x 1 step (two sources in one launch set, both block orderings), dG(2) x 2 steps (six sources, one launch set each,
    destinations partly overwritten and partly accumulated into); mode 0 with weak faces, jacobian without"""
    worst = _Worst("modes" if case.mode else "operator")
    ranks = _st_on_slabs(stfem, case)
    parts = [[d.download() for d in R["dst"]] for R in ranks]
    for R, p in zip(ranks, parts):
        con = s3.constrained3(R["slab"].ncell, R["slab"].strong)
        assert all(np.all(x[con] == 0.0) for x, v in zip(p, R["var"]) if v == 0)
    whole = s3.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    _check_assembled(worst, case, parts, whole, ranks[0]["var"])
    worst.report()


# ------------------------------------------------------------------------------------------------------ device exchange

def _device_exchange(stfem, case, ranks):
    """dst.compress(add) of every block through its scalar view: a velocity block is three blocks of a scalar FE_Q(3) context of the
    slab with the slab's mask, an FE_Q(2) pressure block one block of the context of stfem_stokes_pressure_ctx_space; planes packed,
    copied device to device, unpacked with add = 1.  Returns the context handles that were handed to pack / unpack."""
    L = stfem.lib()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library itself uses (already loaded)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    handed = set()
    for R in ranks:
        s, op = R["slab"], R["op"]
        R["q3"] = stfem.MatrixFreeOperator(3, s.ncell, vertices=None if s3.is_box(case) else s.vertices, lower=s.lower, upper=s.upper,
                                           dirichlet_mask=s.strong)
        assert R["q3"].n_dofs == op.n_velocity
        pc = op.pressure_ctx()  # (owned by the Stokes context)
        assert pc.value and op._space_entries
        assert case.dg or L.stfem_n_dofs(pc) == op.n_pressure
        R["q2"] = types.SimpleNamespace(_h=pc)
        R["bufs"] = {k: op.initialize_dof_vector(0) for k in ("ts", "bs", "tr", "br")}  # 3 n_u doubles each: room for three planes
    nc = s3.ncell(case)
    for b, v in enumerate(ranks[0]["var"]):
        if v == 1 and case.dg:
            continue  # cell-local DoFs: nothing to exchange
        comps, step = (3, s3.VELOCITY_STEP) if v == 0 else (1, s3.PRESSURE_STEP)
        plane = (step * nc[0] + 1) * (step * nc[1] + 1)
        views = []
        for R in ranks:
            ctx = R["q3"] if v == 0 else R["q2"]
            base, n = R["dst"][b].ptr, R["dst"][b].size // comps
            assert n == plane * (step * R["slab"].ncell[2] + 1) and comps * plane <= R["bufs"]["ts"].size
            views.append((ctx, stfem.BlockVector(ctx, device_ptrs=[base + 8 * n * c for c in range(comps)]), step * R["slab"].ncell[2]))
        for R, (ctx, view, top) in zip(ranks, views):
            handed.add(ctx._h.value)
            if R["slab"].has_upper:
                assert L.stfem_plane_pack(ctx._h, view._h, top, R["bufs"]["ts"].ptr, None) == 0
            if R["slab"].has_lower:
                assert L.stfem_plane_pack(ctx._h, view._h, 0, R["bufs"]["bs"].ptr, None) == 0
        assert hip.hipDeviceSynchronize() == 0
        D2D = 3  # hipMemcpyDeviceToDevice (between GPUs: the send / receive of exactly these buffers)
        for r, R in enumerate(ranks):
            if R["slab"].has_upper:
                assert hip.hipMemcpy(ranks[r + 1]["bufs"]["br"].ptr, R["bufs"]["ts"].ptr, comps * plane * 8, D2D) == 0
            if R["slab"].has_lower:
                assert hip.hipMemcpy(ranks[r - 1]["bufs"]["tr"].ptr, R["bufs"]["bs"].ptr, comps * plane * 8, D2D) == 0
        assert hip.hipDeviceSynchronize() == 0
        for R, (ctx, view, top) in zip(ranks, views):
            if R["slab"].has_upper:
                assert L.stfem_plane_unpack(ctx._h, view._h, top, R["bufs"]["tr"].ptr, 1, None) == 0
            if R["slab"].has_lower:
                assert L.stfem_plane_unpack(ctx._h, view._h, 0, R["bufs"]["br"].ptr, 1, None) == 0
        assert hip.hipDeviceSynchronize() == 0
        del views
    return handed


@pytest.mark.parametrize("case", s3.EXCHANGE_CASES, ids=s3.case_id)
def test_st_vmult_with_the_device_exchange(case, stfem):
    """after the exchange every slab holds the whole-mesh rows of its range, owner and ghost copy of every interface plane alike, bit
    for bit; the FE_DGP(2) carrier context is never handed to pack / unpack"""
    worst = _Worst("exchange")
    nc = s3.ncell(case)
    ranks = _st_on_slabs(stfem, case)
    handed = _device_exchange(stfem, case, ranks)
    assert all(R["q3"]._h.value in handed for R in ranks)
    assert all((R["q2"]._h.value in handed) != case.dg for R in ranks)
    whole = s3.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    got = [[d.download() for d in R["dst"]] for R in ranks]
    for R, g in zip(ranks, got):
        s = R["slab"]
        for b, v in enumerate(R["var"]):
            want = s3.cut(whole[b], v, case.dg, nc, s.z0, s.z1)
            worst.check(g[b], want, ("slab", s.z0, "block", b))
            planes = s3.slab_interface_planes(g[b], v, case.dg, s)
            if planes is not None:
                worst.check(planes, s3.slab_interface_planes(want, v, case.dg, s), ("slab", s.z0, "interface planes of block", b))
    for (lo, glo), (hi, ghi) in zip(zip(ranks, got), zip(ranks[1:], got[1:])):  # a + b on one side, b + a on the other
        for b, v in enumerate(lo["var"]):
            if v == 1 and case.dg:
                continue
            comps, step = (3, s3.VELOCITY_STEP) if v == 0 else (1, s3.PRESSURE_STEP)
            top = glo[b].reshape(comps, step * lo["slab"].ncell[2] + 1, -1)[:, -1]
            bottom = ghi[b].reshape(comps, step * hi["slab"].ncell[2] + 1, -1)[:, 0]
            assert np.array_equal(top, bottom), b
    worst.report()


# -------------------------------------------------------------------------------------------- the other entry points

@pytest.mark.parametrize("case", s3.SLICE_ADD_CASES, ids=s3.case_id)
def test_st_vmult_slice_add(case, stfem):
    """onto non-zero destinations with one zero Gamma entry: the slabs' sums equal the sums of the slabs' initial values (interface
    planes count twice, as in any vector of partial sums) plus the reference's Gamma K + Zeta M; constrained rows keep their values"""
    mode = case.mode
    worst = _Worst("modes" if mode else "operator")
    nc = s3.ncell(case)
    U, P, B = s3.fields(case)
    ku, kp = s3.whole_vmult(case.mesh, case.masks, case.dg, mode)
    mu = s3.whole_mass(case.mesh, case.masks)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    var = [(j // nt) % 2 for j in range(nb)]
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    skipped = s3.block_index(nt, 1, 0, 0)
    Gamma[skipped] = 0.0  # a velocity destination that receives the mass part alone
    n_u, n_p = s3.sizes(nc, case.dg)
    init = [rng.uniform(-1, 1, 3 * n_u if v == 0 else n_p) for v in var]
    parts, inits = [], []
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        sinit = [s3.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(init, var)]
        dst = [op.initialize_dof_vector(v, x) for x, v in zip(sinit, var)]
        u, p, b = (op.initialize_dof_vector(v, s3.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in ((U, 0), (P, 1), (B, 0)))
        op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, u, p, lin=b if mode else None, mode=mode)
        got = [d.download() for d in dst]
        con = s3.constrained3(s.ncell, s.strong)
        assert all(np.array_equal(g[con], i[con]) for g, i, v in zip(got, sinit, var) if v == 0)  # constrained rows receive nothing
        parts.append(got)
        inits.append(sinit)
    whole = []
    for j, v in enumerate(var):
        base = s3.assemble([i[j] for i in inits], v, case.dg, nc, case.bounds)
        whole.append(base + (Gamma[j] * ku + Zeta[j] * mu if v == 0 else Gamma[j] * kp))
    _check_assembled(worst, case, parts, whole, var)
    # what arrived, without the initial values: the bound on the sum above is no weaker for standing beside them
    for j, v in enumerate(var):
        added = s3.assemble([p[j] - i[j] for p, i in zip(parts, inits)], v, case.dg, nc, case.bounds)
        want = Gamma[j] * ku + Zeta[j] * mu if v == 0 else Gamma[j] * kp
        assert np.linalg.norm(added - want) <= TOL * (np.linalg.norm(want) + np.linalg.norm(whole[j])), j
    worst.report()


@pytest.mark.parametrize("case", s3.OTHER_CASES, ids=s3.case_id)
def test_st_Tvmult_and_mass_vmult(case, stfem):
    """SystemMatrixStokes::Tvmult as the reference has it (row sums over the time dofs of a step; not a transpose) and the vector mass.
    cG(2), one step: with two steps the row sums of the second step's velocity rows vanish analytically (the time derivative of a
    constant) and the reference's block is a rounding residue, which no relative bound can be held against"""
    worst = _Worst("operator")
    nc = s3.ncell(case)
    blocks, _, var = s3.fields(case._replace(scheme="cg2"))
    Alpha, Beta, ns, nt, _ = s3.weights("cg2")
    whole = s3.whole_st_Tvmult(case.mesh, case.masks, case.dg)
    U, _, _ = s3.fields(case)
    mass = s3.whole_mass(case.mesh, case.masks)
    parts, mparts = [], []
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        src = [op.initialize_dof_vector(v, s3.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in zip(blocks, var)]
        dst = [op.initialize_dof_vector(v, np.full(x.size, 3.0)) for x, v in zip(src, var)]
        op.st_Tvmult(Alpha, Beta, ns, nt, dst, src)
        parts.append([d.download() for d in dst])
        m = op.initialize_dof_vector(0, np.full(src[0].size, 5.0))
        op.mass_vmult(m, op.initialize_dof_vector(0, s3.cut_velocity(U, nc, s.z0, s.z1)))
        mparts.append([m.download()])
        con = s3.constrained3(s.ncell, s.strong)
        assert np.all(mparts[-1][0][con] == 0.0) and all(np.all(x[con] == 0.0) for x, v in zip(parts[-1], var) if v == 0)
    assert any(np.any(w) for w, v in zip(whole, var) if v == 0)
    _check_assembled(worst, case, parts, whole, var, "Tvmult", zero_ok=True)  # (the reference's rule leaves the pressure blocks empty)
    _check_assembled(worst, case, mparts, [mass], [0], "mass")
    worst.report()


@pytest.mark.parametrize("case", s3.NITSCHE_CASES, ids=s3.case_id)
def test_nitsche_rhs_and_face_points(case, stfem):
    """the Dirichlet function at each slab's own face points (stfem_stokes_face_points_space / _nitsche_rhs_space); a slab without a
    cell of face 4 / 5 - or of any weak face: the middle slab of the z-weak mask, on whose context no weak face was ever set - has no
    face points, launches cleanly and leaves the result exactly 0; against the oracle's functional at the whole mesh's points"""
    worst = _Worst("operator")
    pts, ru, rp = s3.whole_nitsche(case.mesh, case.masks, case.dg)
    parts, n_points, empty = [], 0, 0
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        sp = op.face_points_space()
        want_pts = s3.stokes_oracle(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg).face_points()
        assert sp.shape == want_pts.shape == (op.n_face_points_space(), 3)
        if len(sp):
            assert np.abs(sp - want_pts).max() < 1e-13
        n_points += len(sp)
        fu, fp = op.initialize_dof_vector(0, np.zeros(3 * op.n_velocity)), op.initialize_dof_vector(1, np.zeros(op.n_pressure))
        op.nitsche_rhs_space(s3.dirichlet(sp), fu, fp)
        parts.append((fu.download(), fp.download()))
        assert np.all(parts[-1][0][s3.constrained3(s.ncell, s.strong)] == 0.0)
        if not len(sp):
            empty += 1
            assert not parts[-1][0].any() and not parts[-1][1].any()
    assert n_points == len(pts) > 0  # every weak boundary face belongs to exactly one slab
    if case.masks == "zweak" and len(case.bounds) > 3:
        assert empty == 1 and s3.slabs(case)[1].weak == 0  # the middle slab holds no weak face at all
    _check_assembled(worst, case, parts, (ru, rp), (0, 1), zero_ok=True)
    worst.report()


@pytest.mark.parametrize("case", s3.DIVERGENCE_CASES, ids=s3.case_id)
def test_divergence_cells(case, stfem):
    """per-cell values of the slabs (stfem_stokes_divergence_space), concatenated, against the numpy divergence of the whole mesh, per
    cell and in total"""
    worst = _Worst("operator")
    nc = s3.ncell(case)
    U, _, _ = s3.fields(case)
    want, want_total = s3.whole_divergence(case.mesh)
    got, totals = [], []
    for s in s3.slabs(case):
        op = _operator(stfem, case, s)
        total, cells = op.divergence_space(op.initialize_dof_vector(0, s3.cut_velocity(U, nc, s.z0, s.z1)), cells=True)
        assert cells.shape == (s.ncell[0] * s.ncell[1] * s.ncell[2],)
        assert abs(total - np.sqrt(cells.sum())) <= TOL * total
        got.append(cells)
        totals.append(total)
    got = np.concatenate(got)
    worst.check(got, want, "cells")
    assert np.max(np.abs(got - want) / want) <= TOL  # every cell by itself: a sum of 64 non-negative terms
    assert abs(np.sqrt(np.sum(np.square(totals))) - want_total) <= TOL * want_total
    worst.report()


# ------------------------------------------------------------------------------------------------------ capped launches

def _vmult_and_st(op, U, P, blocks, var, Alpha, Beta):
    u, p = op.initialize_dof_vector(0, U), op.initialize_dof_vector(1, P)
    ou, opr = op.initialize_dof_vector(0, np.full(U.size, 7.0)), op.initialize_dof_vector(1, np.full(P.size, -3.0))
    op.vmult(ou, opr, u, p)
    src = [op.initialize_dof_vector(v, x) for x, v in zip(blocks, var)]
    dst = [op.initialize_dof_vector(v, np.full(x.size, 11.0)) for x, v in zip(blocks, var)]
    op.st_vmult(Alpha, Beta, 1, 2, dst, src)
    return [ou.download(), opr.download()] + [d.download() for d in dst]


def _capped_equals_uncapped(stfem, monkeypatch, op, U, P, blocks, var):
    """[results], cell plan and face plan (uncapped, capped): vmult and the cG(2) st_vmult with the colour launches of the cell and the
    boundary kernel capped at one workgroup, bit for bit the uncapped results, and replayed bit for bit"""
    Alpha, Beta, _, _, _ = s3.weights("cg2")
    free = _vmult_and_st(op, U, P, blocks, var, Alpha, Beta)
    plans = [(op.last_cell_plan(), op.last_face_plan())]
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")
    monkeypatch.setenv("STFEM_STOKES_FACE_WORKGROUPS", "1")
    capped = _vmult_and_st(op, U, P, blocks, var, Alpha, Beta)
    plans.append((op.last_cell_plan(), op.last_face_plan()))
    again = _vmult_and_st(op, U, P, blocks, var, Alpha, Beta)
    for j in range(len(free)):
        assert np.array_equal(capped[j], free[j]) and np.array_equal(again[j], free[j]), j
    assert plans[1][0][0] == 1 and plans[1][1][0] == 1, plans
    return free, plans


def test_capped_launches_on_the_one_layer_first_slab(stfem, monkeypatch):
    """pert (0, 1, 3, 4), mixed: the first slab, 3 x 2 x 1 cells with the upper z face neither strong nor weak nor outflow.  One
    workgroup per colour launch gives the uncapped bits.  No colour of this slab has more than two cells and it has four cells on
    weak faces, so the four cell slots of the one workgroup still walk one cell each: the plans name one workgroup and a run of 1 (runs
    of several cells on a one-layer slab: the next test)."""
    case = s3.Case("pert", (0, 1, 3, 4), "mixed", False, 0, "cg2", True)
    s = s3.slabs(case)[0]
    assert s.ncell == (3, 2, 1) and s.has_upper and not s.has_lower and s.weak == 0b000011 and s.outflow == 0b001000 and s.strong == 0b010100
    nc = s3.ncell(case)
    U, P, _ = s3.fields(case._replace(scheme=None))
    blocks, _, var = s3.fields(case)
    cutb = [s3.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(blocks, var)]
    op = _operator(stfem, case, s)
    free, plans = _capped_equals_uncapped(stfem, monkeypatch, op, s3.cut_velocity(U, nc, 0, 1), s3.cut(P, 1, False, nc, 0, 1), cutb, var)
    assert plans[1] == ((1, 1), (1, 1)), plans
    # and they are the slab's partial sums: the oracle on the slab's own mesh
    want = s3.oracle_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, False, 0, None, s3.cut_velocity(U, nc, 0, 1), s3.cut(P, 1, False, nc, 0, 1))
    want = list(want) + list(s3.oracle_st_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, False, 0, "cg2", True, cutb, None))
    worst = _Worst("operator")
    for j in range(len(free)):
        worst.check(free[j], want[j], j)
    worst.report()


WIDE = ((6, 6, 2), 0.15)  # a mesh whose one-layer first slab has nine cells in a colour and twelve on weak faces


def test_capped_launches_walk_several_cells_per_wave_on_a_one_layer_slab(stfem, monkeypatch):
    """the one-layer first slab of a 6 x 6 x 2 perturbed mesh with the masks of `mixed`: colour 3 has 3 x 3 cells and the weak faces 0
    and 1 have 12, so one workgroup (four cell slots) walks runs of 3 - last_cell_plan and last_face_plan show more than one cell per
    wave - and the result is the uncapped one bit for bit, and the oracle's on the slab's own mesh"""
    nc, distort = WIDE
    verts = nref.perturbed_vertices(nc, distort, s3.VERTEX_SEED)
    strong, weak, outflow = s3.slab_masks(*s3.global_masks(s3.Case("pert", (0, 1, 2), "mixed", False, 0, None, True)), False, True)
    s = s3.Slab(0, 1, (nc[0], nc[1], 1), s3.slab_vertices(verts, nc, 0, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 0.5), strong, weak, outflow, False, True)
    n_u, n_p = s3.sizes(s.ncell, False)
    rng = np.random.default_rng(5)
    U, P = rng.uniform(-1, 1, 3 * n_u), rng.uniform(-1, 1, n_p)
    var = [0, 0, 1, 1]
    blocks = [rng.uniform(-1, 1, 3 * n_u if v == 0 else n_p) for v in var]
    op = _slab_operator(stfem, s, False, False)
    free, plans = _capped_equals_uncapped(stfem, monkeypatch, op, U, P, blocks, var)
    assert plans[0] == ((3, 1), (3, 1)) and plans[1] == ((1, 3), (1, 3)), plans
    want = list(s3.oracle_vmult(s.ncell, s.vertices, strong, weak, outflow, False, 0, None, U, P))
    want += list(s3.oracle_st_vmult(s.ncell, s.vertices, strong, weak, outflow, False, 0, "cg2", True, blocks, None))
    worst = _Worst("operator")
    for j in range(len(free)):
        worst.check(free[j], want[j], j)
    worst.report()


# ------------------------------------------------------------------------------------------------------------------ CIP

@pytest.mark.parametrize("case", s3.CIP_CASES, ids=s3.case_id)
def test_cip_without_the_interface_faces(case, stfem):
    """The documented contract: each slab's cip_add_space is the term on the slab's own mesh; the assembled sum equals the whole-mesh
    term away from the two cell layers at every interface and lacks the interface faces' part there
    (tests/test_stokes_q3_slab_assembly_cpu.py: that part is non-zero on every DoF of those layers and more than a tenth of the term);
    vmult after set_cip_space adds the same term; stfem_stokes_set_cip_neighbours still refuses the degree with its reason"""
    worst = _Worst("cip")
    L = stfem.lib()
    nc = s3.ncell(case)
    delta0 = s3.CIP_DELTA0
    U, P, _ = s3.fields(case)
    whole, refs = s3.whole_cip(case.mesh, case.masks), s3.slab_cips(case)
    terms, full = [], []
    for s, ref in zip(s3.slabs(case), refs):
        op = _operator(stfem, case, s)
        u, p = op.initialize_dof_vector(0, s3.cut_velocity(U, nc, s.z0, s.z1)), op.initialize_dof_vector(1, s3.cut(P, 1, False, nc, s.z0, s.z1))
        dst = op.initialize_dof_vector(0, np.zeros(u.size))
        op.cip_add_space(dst, u, u, delta0)
        terms.append(dst.download())
        worst.check(terms[-1], ref, ("slab", s.z0, "cip_add_space"))
        ou, opr = op.initialize_dof_vector(0, np.full(u.size, 7.0)), op.initialize_dof_vector(1, np.full(p.size, -3.0))
        op.vmult(ou, opr, u, p)
        none = ou.download()
        op.set_cip_space(delta0)
        op.vmult(ou, opr, u, p)
        full.append((ou.download(), opr.download()))
        assert np.linalg.norm((full[-1][0] - none) - ref) <= TOL * (np.linalg.norm(none) + np.linalg.norm(none + ref)), s.z0
        layer = np.zeros(3 * (s.ncell[0] + 1) * (s.ncell[1] + 1))  # a vertex plane beyond the interface
        hp = stfem._p(layer)
        for mask, lo, up in ((16, hp, None), (32, None, hp), (48, hp, hp)):
            assert L.stfem_stokes_set_cip_neighbours(op._h, mask, lo, up) == UNSUPPORTED
            why = L.stfem_last_error().decode()
            assert "stfem_stokes_set_cip_neighbours" in why and "velocity degree 2 only" in why, why
        op.vmult(ou, opr, u, p)  # (a refused call changes nothing)
        assert np.array_equal(ou.download(), full[-1][0])
    assembled, want = s3.assemble(terms, 0, False, nc, case.bounds), s3.assemble(refs, 0, False, nc, case.bounds)
    support = s3.interface_layers(nc, case.bounds)
    worst.check(assembled, want, "the sum of the slabs' terms")
    worst.check(assembled[support], want[support], "the interface layers")
    if (~support).any():
        worst.check(assembled[~support], whole[~support], "away from the interface layers: the whole-mesh term")
    else:
        assert case.bounds == (0, 1, 3, 4)  # (every layer touches an interface)
    assert np.linalg.norm(whole - assembled) >= 0.1 * np.linalg.norm(whole)  # the interface faces are not in the slabs' sum
    ku, kp = s3.whole_vmult(case.mesh, case.masks, False, 0)
    _check_assembled(worst, case, full, (ku + want, kp), (0, 1), "vmult with the term")
    worst.report()
