"""The CIP interior-face term on z-slabs, on the CPU: the slab rule of tests/cip_slab_reference.py - own-side contributions, the
neighbour read through two ghost DoF planes and one ghost vertex plane, zeros on the sender's constrained DoFs - summed over the
slabs, is the whole-mesh term of tests/cip_reference.py.  Both sides are the same float sums in another order, hence 1e-13.
Also recorded here: the conditioning of the specs of the per-cell Vanka blocks on slabs (cip_slab_reference.VANKA_SLAB_SPECS)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import cip_slab_reference as csr  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

TOL = 1e-13
DELTA0 = 1.0
CASES = [(mesh, bounds, masks) for mesh in ("pert", "box43") for bounds in ssc.BOUNDS[mesh] for masks in ("strong", "allweak")]


def _case(mesh, bounds, masks):
    return ssc.Case(mesh, bounds, masks, False, 0, None, True)


def _fields(case):
    U, _, B = ssc.fields(case)
    return U, B  # source, weight velocity


@pytest.mark.parametrize("mesh,bounds,masks", CASES, ids=["-".join([m, "".join(map(str, b)), k]) for m, b, k in CASES])
def test_slabs_sum_to_the_whole_mesh_term(mesh, bounds, masks):
    case = _case(mesh, bounds, masks)
    nc, verts = ssc.ncell(case), ssc.vertices(mesh)
    strong = ssc.global_masks(case)[0]
    U, Wt = _fields(case)
    whole = cref.cip(DELTA0, Wt, U, nc, verts, strong)
    assert np.linalg.norm(whole) > 0
    slabs = ssc.slabs(case)
    u_parts = [ssc.cut_velocity(U, nc, s.z0, s.z1) for s in slabs]
    w_parts = [ssc.cut_velocity(Wt, nc, s.z0, s.z1) for s in slabs]
    ghosts = csr.slab_ghosts(u_parts, slabs)
    parts, inner = [], []
    for r, s in enumerate(slabs):
        lv, uv = csr.ghost_vertex_planes(verts, nc, s)
        parts.append(csr.cip_slab(DELTA0, w_parts[r], u_parts[r], s.ncell, s.vertices, s.strong, csr.neighbour_mask(s), ghosts[r][0],
                                  ghosts[r][1], lv, uv))
        inner.append(csr.cip_slab(DELTA0, w_parts[r], u_parts[r], s.ncell, s.vertices, s.strong))
    err = ssc.rel(ssc.assemble(parts, 0, False, nc, bounds), whole)
    print("slab sum against the whole mesh: %.3e" % err)
    assert err <= TOL
    # not hollow: without the interface faces the slabs' sum is far off
    missing = ssc.rel(ssc.assemble(inner, 0, False, nc, bounds), whole)
    print("without the interface faces: %.3e" % missing)
    assert missing > 1e-2


@pytest.mark.parametrize("name", list(csr.VANKA_SLAB_SPECS))
def test_vanka_slab_cases_are_not_hollow_and_well_conditioned(name, oracle_mod):
    """what tests/test_stokes_vanka_cip_reference_cpu.py records for its cases, for the specs of the Vanka blocks on slabs: the term
    changes the reference vmult by at least 1e-2 relative and cond_max <= 1e6 (with eps = 2.2e-16 that leaves 1e-10 for the applied
    blocks).  Measured: pert224_jac cond_max 3.0e4 without / 4.2e4 with the term, change 6.0e-2; pert223_form_dgp_cg2_tm 1.7e3 /
    2.0e3, 3.4e-2; pert323_jac_weakx 4.1e2 / 4.2e2, 4.2e-2."""
    import stokes_vanka_cip_reference as scr
    import stokes_vanka_reference as svr
    p = svr.problem(csr.VANKA_SLAB_SPECS[name])
    base = svr.reference(p)
    ref = scr.with_cip(base, p, scr.DELTA0, p.lin)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    change = ssc.rel(np.concatenate(ref.vmult(X)), np.concatenate(base.vmult(X)))
    print("%-26s change of vmult %.2e  cond_max %.3e (without the term %.3e)" % (name, change, ref.cond_max, base.cond_max))
    assert change >= 1e-2
    assert ref.cond_max <= 1e6 and base.cond_max <= 1e6
    for bounds in csr.VANKA_SLAB_CUTS[name]:
        assert bounds[0] == 0 and bounds[-1] == p.nc[2] and all(a < b for a, b in zip(bounds, bounds[1:]))


def test_mask_zero_is_the_term_on_the_slab_alone():
    """a slab without neighbours is a mesh of its own"""
    case = _case("pert", (0, 2, 4), "strong")
    nc, verts = ssc.ncell(case), ssc.vertices("pert")
    U, Wt = _fields(case)
    s = ssc.slabs(case)[0]
    u, w = ssc.cut_velocity(U, nc, s.z0, s.z1), ssc.cut_velocity(Wt, nc, s.z0, s.z1)
    assert ssc.rel(csr.cip_slab(DELTA0, w, u, s.ncell, s.vertices, s.strong), cref.cip(DELTA0, w, u, s.ncell, s.vertices, s.strong)) <= TOL


def test_pack_zeroes_the_senders_constrained_dofs():
    """a one-layer last slab under a strongly constrained global top: the plane the lower neighbour reads as its second ghost plane is
    that boundary, and only the sender knows"""
    case = _case("box43", (0, 1, 3), "strong")
    nc = ssc.ncell(case)
    U, _ = _fields(case)
    first, last = ssc.slabs(case)
    plane = csr.plane_size(nc)
    up = csr.pack(ssc.cut_velocity(U, nc, first.z0, first.z1), first.ncell, first.strong, 1).reshape(3, 2, plane)
    whole = np.asarray(U).reshape(3, 2 * nc[2] + 1, plane)
    free = ~ssc.constrained3(nc, 63).reshape(3, 2 * nc[2] + 1, plane)
    assert np.array_equal(up[:, 0], np.where(free[:, 0], whole[:, 0], 0.0))  # the global bottom plane: all constrained
    assert not up[:, 0].any() and up[:, 1].any()
    down = csr.pack(ssc.cut_velocity(U, nc, last.z0, last.z1), last.ncell, last.strong, 0).reshape(3, 2, plane)
    assert np.array_equal(down, np.where(free[:, 3:5], whole[:, 3:5], 0.0))
