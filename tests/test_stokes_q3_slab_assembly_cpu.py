"""The slab harness of tests/stokes_q3_slab_cases.py without a GPU: for every case of the table the references on the slabs (slab
vertices, slab masks, sources and linearisations cut), assembled with the helpers, equal the references on the whole mesh - the CPU
oracle at pu = 3, plus tests/navier_q3_reference.py for the modes; the Nitsche functional, the reference's Tvmult, the mass and the
divergence likewise.  Bound rel-L2 <= 1e-14, the bound of tests/test_stokes_slab_assembly_cpu.py (the sums differ in the order of a few
additions per DoF; measured <= 1e-16).  A failure of tests/test_gpu_stokes_q3_slabs.py with this file green belongs to the kernels,
not to the harness.  The file also holds what the table is for, on reference values alone: the interface planes are non-zero, the
convection term and the face part are at least a tenth of what they stand beside, and the CIP term of the whole mesh differs from the
sum of the slabs' terms exactly on the two cell layers at every interface."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_q3_reference as q3  # noqa: E402
import stokes_pressure_q3_reference as p3  # noqa: E402
import stokes_q3_slab_cases as s3  # noqa: E402

TOL = 1e-14
TEETH = 0.1  # the share a term must have of the result it rides on (tests/test_gpu_navier_q3.py)
norm = np.linalg.norm


def _check_blocks(case, parts_per_block, whole, variables, zero_ok=False):
    nc = s3.ncell(case)
    for b, v in enumerate(variables):
        got = s3.assemble([p[b] for p in parts_per_block], v, case.dg, nc, case.bounds)
        if zero_ok and not np.any(whole[b]):
            assert not np.any(got), b
            continue
        assert norm(whole[b]) > 0
        err = s3.rel(got, whole[b])
        print(f"{s3.case_id(case)} block {b}: rel {err:.3e}")
        assert err <= TOL, (b, err)
        planes = s3.interface_planes(got, v, case.dg, nc, case.bounds)
        if planes is not None and (np.any(planes) or not zero_ok):
            assert s3.rel(planes, s3.interface_planes(whole[b], v, case.dg, nc, case.bounds)) <= TOL


def _planes_non_zero(case, x, variable):
    """every interface plane of a whole-mesh block, every velocity component by itself, holds a non-zero entry"""
    if variable == 1 and case.dg:
        return True
    comps = 3 if variable == 0 else 1
    planes = s3.interface_planes(x, variable, case.dg, s3.ncell(case), case.bounds).reshape(comps, len(case.bounds) - 2, -1)
    return bool(np.all(np.any(planes != 0.0, axis=2)))


@pytest.mark.parametrize("case", s3.VMULT_CASES, ids=s3.case_id)
def test_vmult_on_slabs_assembles_to_the_whole_mesh(case):
    nc = s3.ncell(case)
    U, P, B = s3.fields(case)
    for lin_is_source in ((False, True) if case.mode else (False,)):
        whole = s3.whole_vmult(case.mesh, case.masks, case.dg, case.mode, lin_is_source)
        parts = []
        for s in s3.slabs(case):
            u, p, b = (s3.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in ((U, 0), (P, 1), (U if lin_is_source else B, 0)))
            ku, kp = s3.oracle_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg, case.mode, b, u, p)
            assert np.all(ku[s3.constrained3(s.ncell, s.strong)] == 0.0)
            parts.append((ku, kp))
        _check_blocks(case, parts, whole, (0, 1))
        assert _planes_non_zero(case, whole[0], 0) and _planes_non_zero(case, whole[1], 1)
        if case.mode:  # the term is not small beside the result it is part of
            conv = s3.whole_convection(case.mesh, case.masks, case.mode, lin_is_source)
            assert norm(conv) >= TEETH * norm(whole[0]), (norm(conv), norm(whole[0]))
            assert _planes_non_zero(case, conv, 0)


@pytest.mark.parametrize("case", s3.ST_CASES, ids=s3.case_id)
def test_st_vmult_on_slabs_assembles_to_the_whole_mesh(case):
    nc = s3.ncell(case)
    blocks, lin, var = s3.fields(case)
    whole = s3.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    parts = []
    for s in s3.slabs(case):
        sb = [s3.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(blocks, var)]
        sl = [None if x is None else s3.cut_velocity(x, nc, s.z0, s.z1) for x in lin]
        parts.append(s3.oracle_st_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg, case.mode, case.scheme,
                                        case.variable_major, sb, sl))
        con = s3.constrained3(s.ncell, s.strong)
        assert all(np.all(x[con] == 0.0) for x, v in zip(parts[-1], var) if v == 0)
    _check_blocks(case, parts, whole, var)
    assert all(_planes_non_zero(case, w, v) for w, v in zip(whole, var))
    strong, weak, outflow = s3.global_masks(case)
    Alpha, Beta, ns, nt, index = s3.weights(case.scheme, case.variable_major)
    if case.mode:
        add = q3.st_convection(3, case.mode, Alpha, ns, nt, blocks, lin, index, nc, s3.vertices(case.mesh), strong)
        for j, v in enumerate(var):
            assert (add[j] is None) == (v == 1)
            if v == 0:
                assert norm(add[j]) >= TEETH * norm(whole[j]), (j, norm(add[j]), norm(whole[j]))
    if weak & ~outflow:  # the face part beside the cell part, the mass part of the time step included
        cells = s3.oracle_st_vmult(nc, s3.vertices(case.mesh), strong, 0, 0, case.dg, 0, case.scheme, case.variable_major, blocks, lin)
        for j in range(len(var)):
            assert norm(whole[j] - cells[j]) >= TEETH * norm(cells[j]), (j, norm(whole[j] - cells[j]), norm(cells[j]))


@pytest.mark.parametrize("mesh", list(s3.MESHES))
@pytest.mark.parametrize("masks", ["zweak", "allweak", "mixed"])
@pytest.mark.parametrize("dg", [False, True], ids=["q2", "dgp"])
def test_the_face_part_is_a_tenth_of_the_cell_part(mesh, masks, dg):
    (ku, kp), (cu, cp) = s3.whole_linear(mesh, masks, dg), s3.whole_linear(mesh, masks, dg, faces=False)
    shares = norm(ku - cu) / norm(cu), norm(kp - cp) / norm(cp)
    print(mesh, masks, dg, "faces / cells: velocity %.3f pressure %.3f" % shares)
    assert min(shares) >= TEETH


def test_the_table_reaches_what_it_is_for():
    ids = [s3.case_id(c) for c in s3.CASES]
    assert len(set(ids)) == len(ids)
    one_layer_middle = one_layer_first = no_weak_cell = 0
    others = s3.OTHER_CASES + s3.SLICE_ADD_CASES + s3.NITSCHE_CASES + s3.DIVERGENCE_CASES + s3.CIP_CASES + s3.EXCHANGE_CASES
    for c in s3.CASES + others:
        ss = s3.slabs(c)
        assert c.bounds in s3.BOUNDS[c.mesh]
        assert ss[0].z0 == 0 and ss[-1].z1 == s3.ncell(c)[2] and all(a.z1 == b.z0 for a, b in zip(ss, ss[1:]))
        assert not ss[0].has_lower and not ss[-1].has_upper and all(s.has_upper for s in ss[:-1]) and all(s.has_lower for s in ss[1:])
        assert not c.mode or not s3.global_masks(c)[1]  # a mode never meets a weak face
        for s in ss:
            assert not (s.strong | s.weak | s.outflow) & ((16 if s.has_lower else 0) | (32 if s.has_upper else 0))
            assert s.vertices.shape == ((s.ncell[0] + 1) * (s.ncell[1] + 1) * (s.ncell[2] + 1), 3) and int(np.prod(s.ncell)) <= 24
            one_layer_middle += s.ncell[2] == 1 and s.has_lower and s.has_upper
            one_layer_first += s.ncell[2] == 1 and not s.has_lower
            no_weak_cell += s3.global_masks(c)[1] != 0 and s.weak == 0
    assert one_layer_middle and one_layer_first and no_weak_cell
    # the z-weak three-slab case has a middle slab with no weak face at all
    zweak = [c for c in s3.VMULT_CASES + s3.NITSCHE_CASES if c.masks == "zweak" and len(c.bounds) == 4]
    assert zweak and all(s3.slabs(c)[1].weak == 0 and s3.slabs(c)[1].outflow == 0 and s3.slabs(c)[0].weak == 16 and s3.slabs(c)[2].weak == 32
                         for c in zweak)
    # faces 4 / 5 neither strong nor weak nor outflow while x / y faces are weak
    assert any(s.weak & 15 and not (s.strong | s.weak | s.outflow) & 48 for c in s3.VMULT_CASES for s in s3.slabs(c))
    assert {c.mode for c in s3.VMULT_CASES} == {0, s3.FORM, s3.JACOBIAN} and {c.dg for c in s3.CASES} == {False, True}
    assert {c.masks for c in s3.VMULT_CASES if c.mode == 0} == set(s3.MASKS)
    assert {(c.scheme, c.variable_major) for c in s3.ST_CASES} == {("cg2", True), ("cg2", False), ("dg2x2", True)}
    assert {c.mode for c in s3.ST_CASES} == {0, s3.JACOBIAN}
    assert {c.dg for c in s3.EXCHANGE_CASES} == {False, True} and len(s3.EXCHANGE_CASES) == 4


def test_cut_and_assemble_are_inverse_up_to_the_shared_planes():
    """assemble(cut(x)) counts every interface plane twice and everything else once"""
    nc, bounds = (3, 2, 4), (0, 1, 3, 4)
    rng = np.random.default_rng(1)
    for v, dg in ((0, False), (1, False), (1, True)):
        n_u, n_p = s3.sizes(nc, dg)
        assert (n_u, n_p) == (10 * 7 * 13, 10 * 24 if dg else 7 * 5 * 9)
        x = rng.uniform(-1, 1, 3 * n_u if v == 0 else n_p)
        parts = [s3.cut(x, v, dg, nc, z0, z1) for z0, z1 in zip(bounds, bounds[1:])]
        assert [p.size for p in parts] == [(3 * q3.n_velocity(3, (3, 2, z1 - z0)) if v == 0 else p3.n_pressure(2, (3, 2, z1 - z0), dg))
                                           for z0, z1 in zip(bounds, bounds[1:])]
        back = s3.assemble(parts, v, dg, nc, bounds)
        twice = np.ones_like(x)
        if not (v == 1 and dg):
            comps, step = (3, 3) if v == 0 else (1, 2)
            t = twice.reshape(comps, step * nc[2] + 1, -1)
            t[:, [step * z for z in bounds[1:-1]]] = 2.0
            planes = s3.interface_planes(x, v, dg, nc, bounds)
            assert np.array_equal(planes, x.reshape(comps, step * nc[2] + 1, -1)[:, [step, 3 * step]].reshape(-1))
        assert np.array_equal(back, twice * x)


@pytest.mark.parametrize("case", s3.NITSCHE_CASES, ids=s3.case_id)
def test_nitsche_functional_on_slabs_assembles_to_the_whole_mesh(case):
    """every weak boundary face belongs to exactly one slab.  The interface planes receive something - with the z-weak mask too, whose
    one-layer end slabs carry the normal derivative of every test function of the cell to the interface plane - except the pressure
    planes of that mask: the pressure test functions enter with their values on the face alone, and those planes are exactly 0"""
    pts, ru, rp = s3.whole_nitsche(case.mesh, case.masks, case.dg)
    parts, n_points = [], 0
    for s in s3.slabs(case):
        sp, su, spr = s3.oracle_nitsche(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg)
        assert len(sp) == 16 * sum(s.ncell[1 if f // 2 == 0 else 0] * s.ncell[1 if f // 2 == 2 else 2] for f in s3.faces_of(s.weak & ~s.outflow))
        n_points += len(sp)
        parts.append((su, spr))
    assert n_points == len(pts) > 0
    _check_blocks(case, parts, (ru, rp), (0, 1), zero_ok=True)
    assert norm(ru) > 0 and norm(rp) > 0
    for x, v in ((ru, 0), (rp, 1)):
        planes = s3.interface_planes(x, v, case.dg, s3.ncell(case), case.bounds)
        if planes is not None:
            assert (not np.any(planes)) if (case.masks, v) == ("zweak", 1) else _planes_non_zero(case, x, v)


@pytest.mark.parametrize("case", s3.OTHER_CASES, ids=s3.case_id)
def test_Tvmult_and_mass_on_slabs_assemble_to_the_whole_mesh(case):
    nc = s3.ncell(case)
    c = case._replace(scheme="cg2")
    blocks, _, var = s3.fields(c)
    Alpha, Beta, ns, nt, _ = s3.weights("cg2")
    whole = s3.whole_st_Tvmult(case.mesh, case.masks, case.dg)
    U, P, _ = s3.fields(case)
    mass = s3.whole_mass(case.mesh, case.masks)
    parts, mparts = [], []
    for s in s3.slabs(case):
        orc = s3.stokes_oracle(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg)
        parts.append(orc.st_Tvmult(Alpha, Beta, ns, nt, [s3.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(blocks, var)]))
        mparts.append([orc.apply(s3.cut_velocity(U, nc, s.z0, s.z1), np.zeros(orc.n_p), 0.0, 1.0)[0].reshape(-1)])
    assert any(np.any(w) for w, v in zip(whole, var) if v == 0)
    _check_blocks(case, parts, whole, var, zero_ok=True)
    _check_blocks(case, mparts, [mass], [0])
    assert _planes_non_zero(case, mass, 0)


@pytest.mark.parametrize("mesh", list(s3.MESHES))
def test_divergence_on_slabs_concatenates_to_the_whole_mesh(mesh):
    """and the restatement on a known field: (x, y, z) has divergence 3, every cell gives 9 |K|"""
    nc, _, up = s3.MESHES[mesh]
    verts = s3.vertices(mesh)
    if mesh == "box":  # (there the nodes lie where the trilinear map puts them: the nodal interpolant of a linear field is the field)
        X = p3.box_node_coordinates(3, nc, (0, 0, 0), up)
        cells, total = p3.divergence_cells(3, np.concatenate([X[:, 0], X[:, 1], X[:, 2]]), nc, verts)
        assert np.allclose(cells, 9 * np.prod(up) / np.prod(nc), rtol=1e-13, atol=0) and abs(total - 3 * np.sqrt(np.prod(up))) <= 1e-13
    U, _, _ = s3.fields(s3.Case(mesh, s3.BOUNDS[mesh][0], "strong", False, 0, None, True))
    whole, total = s3.whole_divergence(mesh)
    for bounds in s3.BOUNDS[mesh]:
        parts = [p3.divergence_cells(3, s3.cut_velocity(U, nc, z0, z1), (nc[0], nc[1], z1 - z0), s3.slab_vertices(verts, nc, z0, z1))
                 for z0, z1 in zip(bounds, bounds[1:])]
        assert np.all(whole > 0) and s3.rel(np.concatenate([p[0] for p in parts]), whole) <= TOL
        assert abs(np.sqrt(sum(p[1] ** 2 for p in parts)) - total) <= TOL * total


@pytest.mark.parametrize("case", s3.CIP_CASES, ids=s3.case_id)
def test_cip_of_the_slabs_lacks_exactly_the_interface_faces(case):
    """The documented contract at degree 3: a slab's CIP term has no interface face.  The whole-mesh term minus the assembled slab
    terms is the part of the interface faces: supported on the velocity DoFs of the two cell layers that touch an interface, exactly 0
    elsewhere (the other faces give the same summands in the same order) and non-zero on every DoF there (nothing is constrained)"""
    nc = s3.ncell(case)
    whole = s3.whole_cip(case.mesh, case.masks)
    assembled = s3.assemble(s3.slab_cips(case), 0, False, nc, case.bounds)
    missing = whole - assembled
    support = s3.interface_layers(nc, case.bounds)
    assert support.shape == whole.shape and support.any()
    assert np.all(missing[~support] == 0.0)
    assert np.all(missing[support] != 0.0)
    if case.bounds == (0, 2, 4):  # (with interfaces at 1 and 3 every layer touches one)
        assert (~support).any() and norm(whole[~support]) > 0
    print(s3.case_id(case), "interface faces / whole term: %.3f" % (norm(missing) / norm(whole)))
    assert norm(missing) >= TEETH * norm(whole)  # a result that did hold the interface faces would not pass for the slabs' sum
    # and the term is a tenth of the linear result it is added to (tests/test_cip_q3_reference_cpu.py::test_gpu_cases_are_not_hollow)
    assert norm(assembled) >= TEETH * norm(s3.whole_vmult(case.mesh, case.masks, False, 0)[0])
