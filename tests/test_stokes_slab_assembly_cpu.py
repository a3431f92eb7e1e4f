"""The slab harness of tests/stokes_slab_cases.py without a GPU: for every case of the table the CPU oracle on the slabs (slab vertices,
slab masks, sources and linearisations cut), assembled with the helpers, equals the oracle on the whole mesh.  Modes 1 / 2 are the
oracle plus tests/navier_reference.py.  Bound rel-L2 <= 1e-14 (the sums differ in the order of a few additions per DoF; measured
<= 1e-16).  A failure of tests/test_gpu_stokes_slabs.py with this file green belongs to the kernels, not to the harness."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

TOL = 1e-14


def _check_blocks(case, parts_per_block, whole, variables):
    nc = ssc.ncell(case)
    for b, v in enumerate(variables):
        got = ssc.assemble([p[b] for p in parts_per_block], v, case.dg, nc, case.bounds)
        assert np.linalg.norm(whole[b]) > 0
        err = ssc.rel(got, whole[b])
        print(f"{ssc.case_id(case)} block {b}: rel {err:.3e}")
        assert err <= TOL, (b, err)
        planes = ssc.interface_planes(got, v, case.dg, nc, case.bounds)
        if planes is not None:
            assert ssc.rel(planes, ssc.interface_planes(whole[b], v, case.dg, nc, case.bounds)) <= TOL


@pytest.mark.parametrize("case", ssc.VMULT_CASES, ids=ssc.case_id)
def test_vmult_on_slabs_assembles_to_the_whole_mesh(case):
    nc = ssc.ncell(case)
    U, P, B = ssc.fields(case)
    whole = ssc.whole_vmult(case.mesh, case.masks, case.dg, case.mode)
    parts = []
    for s in ssc.slabs(case):
        u, p, b = (ssc.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in ((U, 0), (P, 1), (B, 0)))
        ku, kp = ssc.oracle_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg, case.mode, b, u, p)
        assert np.all(ku[ssc.constrained3(s.ncell, s.strong)] == 0.0)
        parts.append((ku, kp))
    _check_blocks(case, parts, whole, (0, 1))


@pytest.mark.parametrize("case", ssc.ST_CASES, ids=ssc.case_id)
def test_st_vmult_on_slabs_assembles_to_the_whole_mesh(case):
    nc = ssc.ncell(case)
    blocks, lin, var = ssc.fields(case)
    whole = ssc.whole_st_vmult(case.mesh, case.masks, case.dg, case.mode, case.scheme, case.variable_major)
    parts = []
    for s in ssc.slabs(case):
        sb = [ssc.cut(x, v, case.dg, nc, s.z0, s.z1) for x, v in zip(blocks, var)]
        sl = [None if x is None else ssc.cut_velocity(x, nc, s.z0, s.z1) for x in lin]
        parts.append(ssc.oracle_st_vmult(s.ncell, s.vertices, s.strong, s.weak, s.outflow, case.dg, case.mode, case.scheme,
                                         case.variable_major, sb, sl))
    _check_blocks(case, parts, whole, var)


def test_the_table_reaches_what_it_is_for():
    ids = [ssc.case_id(c) for c in ssc.CASES]
    assert len(set(ids)) == len(ids)
    one_layer_middle = one_layer_first = no_weak_cell = 0
    for c in ssc.CASES:
        ss = ssc.slabs(c)
        assert ss[0].z0 == 0 and ss[-1].z1 == ssc.ncell(c)[2] and all(a.z1 == b.z0 for a, b in zip(ss, ss[1:]))
        assert not ss[0].has_lower and not ss[-1].has_upper and all(s.has_upper for s in ss[:-1]) and all(s.has_lower for s in ss[1:])
        for s in ss:
            assert not (s.strong | s.weak | s.outflow) & ((16 if s.has_lower else 0) | (32 if s.has_upper else 0))
            one_layer_middle += s.ncell[2] == 1 and s.has_lower and s.has_upper
            one_layer_first += s.ncell[2] == 1 and not s.has_lower
            no_weak_cell += ssc.global_masks(c)[1] != 0 and s.weak == 0
    assert one_layer_middle and one_layer_first and no_weak_cell
    assert {c.mode for c in ssc.VMULT_CASES} == {0, nref.FORM, nref.JACOBIAN} and {c.dg for c in ssc.CASES} == {False, True}
    assert {(c.scheme, c.variable_major) for c in ssc.ST_CASES} == {("cg2", True), ("cg2", False), ("dg2x2", True), ("cg3x2", True)}


def test_cut_and_assemble_are_inverse_up_to_the_shared_planes():
    """assemble(cut(x)) counts every interface plane twice and everything else once"""
    nc, bounds = (3, 2, 4), (0, 1, 3, 4)
    rng = np.random.default_rng(1)
    for v, dg in ((0, False), (1, False), (1, True)):
        n_u, n_p = ssc.sizes(nc, dg)
        x = rng.uniform(-1, 1, 3 * n_u if v == 0 else n_p)
        back = ssc.assemble([ssc.cut(x, v, dg, nc, z0, z1) for z0, z1 in zip(bounds, bounds[1:])], v, dg, nc, bounds)
        twice = np.ones_like(x)
        if not (v == 1 and dg):
            comps, step = (3, 2) if v == 0 else (1, 1)
            t = twice.reshape(comps, step * nc[2] + 1, -1)
            t[:, [step * z for z in bounds[1:-1]]] = 2.0
        assert np.array_equal(back, twice * x)


def test_divergence_restatement_on_a_known_field():
    """(x, y, z) has divergence 3: every cell gives 9 |K|, on the perturbed mesh too; slabs concatenate"""
    nc = ssc.MESHES["pert"][0]
    verts = ssc.vertices("pert")
    # the known field on the box (there the Q2 nodes lie on the uniform lattice), the perturbed mesh for the partition identity
    box = ssc.vertices("box43")
    nb = ssc.MESHES["box43"][0]
    up = ssc.MESHES["box43"][2]
    z, y, x = np.meshgrid(*[np.linspace(0, up[d], 2 * nb[d] + 1) for d in (2, 1, 0)], indexing="ij")
    cells = ssc.divergence_cells(np.concatenate([x.ravel(), y.ravel(), z.ravel()]), nb, box)
    assert np.allclose(cells, 9 * np.prod(up) / np.prod(nb), rtol=1e-13, atol=0)
    u = np.random.default_rng(2).uniform(-1, 1, 3 * nref.n_velocity(nc))
    whole = ssc.divergence_cells(u, nc, verts)
    parts = [ssc.divergence_cells(ssc.cut_velocity(u, nc, z0, z1), (nc[0], nc[1], z1 - z0), ssc.slab_vertices(verts, nc, z0, z1))
             for z0, z1 in ((0, 1), (1, 3), (3, 4))]
    assert np.all(whole > 0) and ssc.rel(np.concatenate(parts), whole) <= TOL
