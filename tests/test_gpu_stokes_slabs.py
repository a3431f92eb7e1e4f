"""The Stokes / Navier-Stokes operator on z-slabs of a partitioned mesh (BASELINE configs[4] is an 8-GPU configuration): every
kernel family on slabs whose interface faces are out of the strong mask, the weak set and the outflow set, the partial sums of the
interface planes added (on the host: tests/stokes_slab_cases.py::assemble; on the device: stfem_plane_pack -> copy ->
stfem_plane_unpack(add) on the scalar views of the blocks, as host/stfem/stokes_solver.h::StokesSystem::vmult does).

Every expected value is the WHOLE-MESH CPU oracle (oracle.StokesOracle, plus tests/navier_reference.py for the convection modes, plus
the numpy divergence of the helper module); tests/test_stokes_slab_assembly_cpu.py shows that the oracle on the same slabs, cut and
assembled by the same helpers, reproduces it to 1e-16.  Bounds: rel-L2 <= 1e-12 per block (the project's fp64 parity bound), the same
bound on the interface planes alone, rows of strongly constrained velocity DoFs exactly 0 on every slab.  Each test prints its largest
ratio to the bound ("ratio <group> <value>")."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _operator(stfem, case, s):
    """the slab's operator: general meshes get the slab's vertices (cell kernels), a box none (Kronecker path)"""
    op = stfem.StokesMatrixFreeOperator(s.ncell, vertices=None if ssc.is_box(case) else s.vertices, lower=s.lower, upper=s.upper,
                                        dirichlet_mask=s.strong, viscosity=ssc.NU, weak_boundary_ids=ssc.faces_of(s.weak),
                                        outflow_boundary_ids=ssc.faces_of(s.outflow), penalty1=ssc.PENALTY1, penalty2=ssc.PENALTY2,
                                        dg_pressure=case.dg)
    assert (op.n_velocity, op.n_pressure) == ssc.sizes(s.ncell, case.dg)
    return op


class _Worst:
    def __init__(self, group):
        self.group, self.value = group, 0.0

    def check(self, got, want, what, zero_ok=False):
        if zero_ok and not np.any(want):  # the oracle receives no contribution here: neither may the kernels' result
            assert not np.any(got), what
            return
        assert np.linalg.norm(want) > 0, what
        err = ssc.rel(got, want)
        self.value = max(self.value, err / TOL)
        assert err <= TOL, (what, err)

    def report(self):
        print(f"ratio {self.group} {self.value:.3e}")


def _check_assembled(worst, case, parts_per_block, whole, variables, what="", zero_ok=False):
    """the sum of the slabs' blocks against the whole-mesh oracle: per block, and on the interface planes alone (a face functional may
    leave those without any contribution: then exactly 0)"""
    nc = ssc.ncell(case)
    for b, v in enumerate(variables):
        got = ssc.assemble([p[b] for p in parts_per_block], v, case.dg, nc, case.bounds)
        worst.check(got, whole[b], (what, "block", b), zero_ok)
        planes = ssc.interface_planes(got, v, case.dg, nc, case.bounds)
        if planes is not None:
            worst.check(planes, ssc.interface_planes(whole[b], v, case.dg, nc, case.bounds), (what, "interface planes of block", b), True)


# ---------------------------------------------------------------------------------------------------------------- vmult

@pytest.mark.parametrize("case", ssc.VMULT_CASES, ids=ssc.case_id)
def test_vmult(case, stfem):
    """modes 0 / form / jacobian, both pressure spaces, four mask sets, 2 and 3 slabs with the one-layer slabs; lin cut like the source;
    a second call replays bit for bit; one call with lin = source (Picard)"""
    nc = ssc.ncell(case)
    U, P, B = ssc.fields(case)
    worst = _Worst("modes" if case.mode else "operator")
    parts, picard = [], []
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        u, p, b = (op.initialize_dof_vector(v, ssc.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in ((U, 0), (P, 1), (B, 0)))
        ou, opr = op.initialize_dof_vector(0, np.full(u.size, 7.0)), op.initialize_dof_vector(1, np.full(p.size, -3.0))  # overwritten
        lin = b if case.mode else None
        op.vmult(ou, opr, u, p, lin=lin, mode=case.mode)
        got = (ou.download(), opr.download())
        assert np.all(got[0][ssc.constrained3(s.ncell, s.strong)] == 0.0)
        op.vmult(ou, opr, u, p, lin=lin, mode=case.mode)
        assert np.array_equal(ou.download(), got[0]) and np.array_equal(opr.download(), got[1])
        parts.append(got)
        if case.mode:
            op.vmult(ou, opr, u, p, lin=u, mode=case.mode)
            picard.append((ou.download(), opr.download()))
            assert np.all(picard[-1][0][ssc.constrained3(s.ncell, s.strong)] == 0.0)
    _check_assembled(worst, case, parts, ssc.whole_vmult(case.mesh, case.masks, case.dg, case.mode), (0, 1))
    if case.mode:
        _check_assembled(worst, case, picard, ssc.whole_vmult(case.mesh, case.masks, case.dg, case.mode, True), (0, 1), "picard")
    worst.report()


# ------------------------------------------------------------------------------------------------------------- st_vmult

def _st_on_slabs(stfem, case):
    """the space-time vmult on every slab, destinations pre-filled: [dict(slab, op, dst, var)]"""
    nc = ssc.ncell(case)
    blocks, lin, var = ssc.fields(case)
    Alpha, Beta, ns, nt, _ = ssc.weights(case.scheme, case.variable_major)
    ranks = []
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        src = [op.initialize_dof_vector(v, ssc.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in zip(blocks, var)]
        dst = [op.initialize_dof_vector(v, np.full(x.size, 11.0)) for x, v in zip(src, var)]
        dlin = None
        if case.mode:  # (pressure entries: null)
            dlin = [None if x is None else op.initialize_dof_vector(0, ssc.cut_velocity(x, nc, s.z0, s.z1)) for x in lin]
        op.st_vmult(Alpha, Beta, ns, nt, dst, src, case.variable_major, lin=dlin, mode=case.mode)
        ranks.append(dict(slab=s, op=op, dst=dst, var=var, src=src, lin=dlin))
    return ranks


@pytest.mark.parametrize("case", ssc.ST_CASES, ids=ssc.case_id)
def test_st_vmult(case, stfem):
    """cG(2) x 1 step (the fused launch set, both block orderings), dG(2) x 2 and cG(3) x 2 steps (six sources, one launch set each,
    destinations partly overwritten and partly accumulated into), modes 0 and jacobian"""
    worst = _Worst("modes" if case.mode else "operator")
    ranks = _st_on_slabs(stfem, case)
    parts = [[d.download() for d in R["dst"]] for R in ranks]
    for R, p in zip(ranks, parts):
        con = ssc.constrained3(R["slab"].ncell, R["slab"].strong)
        assert all(np.all(x[con] == 0.0) for x, v in zip(p, R["var"]) if v == 0)
    whole = ssc.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    _check_assembled(worst, case, parts, whole, ranks[0]["var"])
    worst.report()


# ------------------------------------------------------------------------------------------------------ device exchange

def _device_exchange(stfem, case, ranks):
    """dst.compress(add) of every block through its scalar view, as StokesSystem::vmult: a velocity block is three blocks of a scalar
    FE_Q(2) context of the slab with the slab's mask, an FE_Q(1) pressure block one block of stfem_stokes_pressure_ctx; planes packed,
    copied device to device, unpacked with add = 1.  Returns the context handles that were handed to pack / unpack."""
    L = stfem.lib()
    hip = C.CDLL("libamdhip64.so")  # the runtime the library itself uses (already loaded)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    handed = set()
    for R in ranks:
        s, op = R["slab"], R["op"]
        R["q2"] = stfem.MatrixFreeOperator(2, s.ncell, vertices=None if ssc.is_box(case) else s.vertices, lower=s.lower, upper=s.upper,
                                           dirichlet_mask=s.strong)
        assert R["q2"].n_dofs == op.n_velocity
        pc = C.c_void_p()
        assert L.stfem_stokes_pressure_ctx(op._h, C.byref(pc)) == 0 and pc.value
        R["q1"] = types.SimpleNamespace(_h=pc)  # (owned by the Stokes context)
        R["bufs"] = {k: op.initialize_dof_vector(0) for k in ("ts", "bs", "tr", "br")}  # 3 n_u doubles each: room for three planes
    nc = ssc.ncell(case)
    for b, v in enumerate(ranks[0]["var"]):
        if v == 1 and case.dg:
            continue  # cell-local DoFs: nothing to exchange
        comps, step = (3, 2) if v == 0 else (1, 1)
        plane = (step * nc[0] + 1) * (step * nc[1] + 1)
        views = []
        for R in ranks:
            ctx = R["q2"] if v == 0 else R["q1"]
            base, n = R["dst"][b].ptr, R["dst"][b].size // comps
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


@pytest.mark.parametrize("case", ssc.ST_CASES, ids=ssc.case_id)
def test_st_vmult_with_the_device_exchange(case, stfem):
    """after the exchange every slab holds the oracle's whole-mesh rows of its range, owner and ghost copy of every interface plane
    alike; the FE_DGP(1) carrier context is never handed to pack / unpack"""
    worst = _Worst("exchange")
    nc = ssc.ncell(case)
    ranks = _st_on_slabs(stfem, case)
    handed = _device_exchange(stfem, case, ranks)
    if case.dg:
        assert all(R["q1"]._h.value not in handed for R in ranks)
    whole = ssc.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    got = [[d.download() for d in R["dst"]] for R in ranks]
    for R, g in zip(ranks, got):
        s = R["slab"]
        for b, v in enumerate(R["var"]):
            want = ssc.cut(whole[b], v, case.dg, nc, s.z0, s.z1)
            worst.check(g[b], want, ("slab", s.z0, "block", b))
            planes = ssc.slab_interface_planes(g[b], v, case.dg, s)
            if planes is not None:
                worst.check(planes, ssc.slab_interface_planes(want, v, case.dg, s), ("slab", s.z0, "interface planes of block", b))
    for (lo, glo), (hi, ghi) in zip(zip(ranks, got), zip(ranks[1:], got[1:])):  # a + b on one side, b + a on the other
        for b, v in enumerate(lo["var"]):
            if v == 1 and case.dg:
                continue
            comps, step = (3, 2) if v == 0 else (1, 1)
            top = glo[b].reshape(comps, step * lo["slab"].ncell[2] + 1, -1)[:, -1]
            bottom = ghi[b].reshape(comps, step * hi["slab"].ncell[2] + 1, -1)[:, 0]
            assert np.array_equal(top, bottom), b
    worst.report()


# -------------------------------------------------------------------------------------------- the other entry points
OTHER = [ssc.Case("pert", (0, 1, 3, 4), "mixed", dg, 0, None, True) for dg in (False, True)] + \
        [ssc.Case("box54", (0, 2, 3, 4), "allweak", dg, 0, None, True) for dg in (False, True)]


@pytest.mark.parametrize("mode", [0, nref.JACOBIAN])
@pytest.mark.parametrize("case", OTHER, ids=ssc.case_id)
def test_st_vmult_slice_add(case, mode, stfem):
    """onto non-zero destinations with one zero Gamma entry: the slabs' sums equal the sums of the slabs' initial values (interface
    planes count twice, as in any vector of partial sums) plus the oracle's Gamma K + Zeta M"""
    case = case._replace(mode=mode)
    worst = _Worst("modes" if mode else "operator")
    nc = ssc.ncell(case)
    U, P, B = ssc.fields(case)
    ku, kp = ssc.whole_vmult(case.mesh, case.masks, case.dg, mode)
    strong, weak, outflow = ssc.global_masks(case)
    mu, _ = ssc.stokes_oracle(nc, ssc.vertices(case.mesh), strong, weak, outflow, case.dg).apply(U, P, 0.0, 1.0)
    ns, nt = 2, 2
    nb = 2 * ns * nt
    var = [(j // nt) % 2 for j in range(nb)]
    rng = np.random.default_rng(11)
    Gamma, Zeta = rng.uniform(-1, 1, nb), rng.uniform(-1, 1, nb)
    Gamma[ssc.block_index(nt, 1, 0, 0)] = 0.0
    n_u, n_p = ssc.sizes(nc, case.dg)
    init = [rng.uniform(-1, 1, 3 * n_u if v == 0 else n_p) for v in var]
    parts, inits = [], []
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        sinit = [ssc.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(init, var)]
        dst = [op.initialize_dof_vector(v, x) for x, v in zip(sinit, var)]
        u, p, b = (op.initialize_dof_vector(v, ssc.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in ((U, 0), (P, 1), (B, 0)))
        op.st_vmult_slice_add(Gamma, Zeta, ns, nt, dst, u, p, lin=b if mode else None, mode=mode)
        got = [d.download() for d in dst]
        con = ssc.constrained3(s.ncell, s.strong)
        assert all(np.array_equal(g[con], i[con]) for g, i, v in zip(got, sinit, var) if v == 0)  # constrained rows receive nothing
        parts.append(got)
        inits.append(sinit)
    whole = []
    for j, v in enumerate(var):
        base = ssc.assemble([i[j] for i in inits], v, case.dg, nc, case.bounds)
        whole.append(base + (Gamma[j] * ku + Zeta[j] * mu.reshape(-1) if v == 0 else Gamma[j] * kp))
    _check_assembled(worst, case, parts, whole, var)
    worst.report()


@pytest.mark.parametrize("case", OTHER, ids=ssc.case_id)
def test_st_Tvmult_and_mass_vmult(case, stfem):
    """SystemMatrixStokes::Tvmult as the reference has it (row sums over the time dofs of a step; not a transpose) and the vector mass.
    cG(2), one step: with two steps the row sums of the second step's velocity rows vanish analytically (the time derivative of a
    constant) and the oracle's block is a rounding residue, which no relative bound can be held against"""
    worst = _Worst("operator")
    nc = ssc.ncell(case)
    case = case._replace(scheme="cg2")
    blocks, _, var = ssc.fields(case)
    Alpha, Beta, ns, nt, _ = ssc.weights(case.scheme)
    strong, weak, outflow = ssc.global_masks(case)
    orc = ssc.stokes_oracle(nc, ssc.vertices(case.mesh), strong, weak, outflow, case.dg)
    whole = orc.st_Tvmult(Alpha, Beta, ns, nt, blocks)
    mass, _ = orc.apply(blocks[0], np.zeros(orc.n_p), 0.0, 1.0)
    parts, mparts = [], []
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        src = [op.initialize_dof_vector(v, ssc.cut(x, v, case.dg, nc, s.z0, s.z1)) for x, v in zip(blocks, var)]
        dst = [op.initialize_dof_vector(v, np.full(x.size, 3.0)) for x, v in zip(src, var)]
        op.st_Tvmult(Alpha, Beta, ns, nt, dst, src)
        parts.append([d.download() for d in dst])
        m = op.initialize_dof_vector(0, np.full(src[0].size, 5.0))
        op.mass_vmult(m, src[0])
        mparts.append([m.download()])
        con = ssc.constrained3(s.ncell, s.strong)
        assert np.all(mparts[-1][0][con] == 0.0) and all(np.all(x[con] == 0.0) for x, v in zip(parts[-1], var) if v == 0)
    assert any(np.any(w) for w, v in zip(whole, var) if v == 0)
    _check_assembled(worst, case, parts, whole, var, "Tvmult", zero_ok=True)  # (the reference's rule leaves the pressure blocks empty)
    _check_assembled(worst, case, mparts, [mass.reshape(-1)], [0], "mass")
    worst.report()


def _dirichlet(pts):
    return np.stack([np.sin(pts[:, 0] + 2 * pts[:, 1]), pts[:, 2] ** 2 - pts[:, 0], np.cos(pts[:, 1] * pts[:, 2])], axis=1)


NITSCHE = OTHER + [ssc.Case("pert", (0, 1, 3, 4), "zweak", dg, 0, None, True) for dg in (False, True)] + \
    [ssc.Case("box43", (0, 1, 3), "zweak", False, 0, None, True)]


@pytest.mark.parametrize("case", NITSCHE, ids=ssc.case_id)
def test_nitsche_rhs(case, stfem):
    """the Dirichlet function at each slab's own face points; a slab without a cell of face 4 / 5 (or of any weak face: the middle slab
    of the z-weak mask) has no face points there and still launches cleanly; against orc.nitsche_rhs at the whole mesh's points"""
    worst = _Worst("operator")
    nc = ssc.ncell(case)
    strong, weak, outflow = ssc.global_masks(case)
    orc = ssc.stokes_oracle(nc, ssc.vertices(case.mesh), strong, weak, outflow, case.dg)
    pts = orc.face_points()
    ru, rp = orc.nitsche_rhs(_dirichlet(pts))
    parts, n_points = [], 0
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        sp = op.face_points()
        want_pts = ssc.stokes_oracle(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg).face_points()
        assert sp.shape == want_pts.shape
        if len(sp):
            assert np.abs(sp - want_pts).max() < 1e-13
        n_points += len(sp)
        fu, fp = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
        op.nitsche_rhs(_dirichlet(sp), fu, fp)
        parts.append((fu.download(), fp.download()))
        assert np.all(parts[-1][0][ssc.constrained3(s.ncell, s.strong)] == 0.0)
        if not len(sp):
            assert not parts[-1][0].any() and not parts[-1][1].any()
    assert n_points == len(pts)  # every weak boundary face belongs to exactly one slab
    if case.masks == "zweak" and len(case.bounds) > 3:
        assert all(s.weak == 0 for s in ssc.slabs(case)[1:-1])  # the middle slab holds no weak face at all
    _check_assembled(worst, case, parts, (ru.reshape(-1), rp), (0, 1))
    worst.report()


@pytest.mark.parametrize("case", [c for c in OTHER if not c.dg], ids=ssc.case_id)
def test_divergence_cells(case, stfem):
    """per-cell values of the slabs, concatenated, against the numpy Q2 divergence of the whole mesh"""
    worst = _Worst("operator")
    nc = ssc.ncell(case)
    U, _, _ = ssc.fields(case)
    want = ssc.divergence_cells(U, nc, ssc.vertices(case.mesh))
    got, totals = [], []
    for s in ssc.slabs(case):
        op = _operator(stfem, case, s)
        total, cells = op.divergence(op.initialize_dof_vector(0, ssc.cut_velocity(U, nc, s.z0, s.z1)), cells=True)
        assert cells.shape == (s.ncell[0] * s.ncell[1] * s.ncell[2],)
        got.append(cells)
        totals.append(total)
    got = np.concatenate(got)
    worst.check(got, want, "cells")
    assert np.max(np.abs(got - want) / want) <= TOL  # every cell by itself: a sum of 27 non-negative terms
    assert abs(np.sqrt(np.sum(np.square(totals))) - np.sqrt(np.sum(want))) <= TOL * np.sqrt(np.sum(want))
    worst.report()
