"""The dense restatement of the per-cell Stokes Vanka blocks with the CIP term (tests/stokes_vanka_cip_reference.py) checked by
properties on the CPU, and the two facts the bounds of tests/test_gpu_stokes_vanka_cip.py rest on: the term changes the smoother of
every GPU case (the test is not hollow), and the blocks stay as well conditioned as those of tests/test_gpu_stokes_vanka_linearised.py,
whose 1e-10 the GPU test keeps.

Recorded (this file prints them), delta0 = 1, NU = 0.7, DT = 0.05, states in [-1, 1]: the term changes vmult by at least 1e-2
relative (2.8e-2 ... 1.0e-1 over the cases); cond_max 3.3e2 ... 1.3e5 with the term against 1.5e2 ... 1.15e5 without."""
import numpy as np
import pytest

import cip_reference as cref
import navier_reference as nref
import stokes_vanka_cip_reference as scr
import stokes_vanka_reference as svr


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def meshes(oracle_mod):
    """name -> (ncell, vertices) of every case mesh, and the mode-0 one"""
    out = {name: (svr.problem(spec).nc, svr.problem(spec).verts) for name, spec in scr.CASES.items()}
    out["mode0"] = (svr.problem(scr.MODE0).nc, svr.problem(scr.MODE0).verts)
    return out


@pytest.fixture(scope="module")
def matrices(meshes):
    """name -> (C(w), w) with a random w read without constraints"""
    out = {}
    for k, (name, (nc, verts)) in enumerate(meshes.items()):
        w = np.random.default_rng(40 + k).uniform(-1, 1, 3 * nref.n_velocity(nc))
        out[name] = (scr.cip_matrix(1.0, w, nc, verts, 0), w)
    return out


def test_matrix_times_vector_is_the_term(meshes, matrices):
    """(a) C(w) u equals cip_reference.cip(1, w, u, ..., dirichlet_mask=0), abs 1e-14"""
    for name, (nc, verts) in meshes.items():
        C, w = matrices[name]
        u = np.random.default_rng(3).uniform(-1, 1, 3 * nref.n_velocity(nc))
        want = cref.cip(1.0, w, u, nc, verts, 0).reshape(3, -1)
        got = u.reshape(3, -1) @ C.T
        err = np.abs(got - want).max()
        print("%-26s |C u - cip| %.2e" % (name, err))
        assert err < 1e-14


def test_matrix_is_symmetric_and_positive_semidefinite(matrices):
    """(b), (d)"""
    for name, (C, _) in matrices.items():
        asym = np.linalg.norm(C - C.T) / np.linalg.norm(C)
        print("%-26s asymmetry %.2e" % (name, asym))
        assert asym < 1e-14
        u = np.random.default_rng(9).uniform(-1, 1, (5, C.shape[0]))
        assert all(v @ C @ v >= 0.0 for v in u)
        assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() > -1e-13 * np.abs(C).max()


def test_linear_fields_have_no_gradient_jump(meshes, matrices):
    """(c) C 1 = 0 and C (x, y, z) = 0, perturbed meshes too: 1e-13"""
    for name, (nc, verts) in meshes.items():
        C, _ = matrices[name]
        X = cref.dof_points(nc, verts)
        for field in (np.ones(C.shape[0]), X[:, 0], X[:, 1], X[:, 2]):
            assert np.abs(C @ field).max() < 1e-13, name


def test_centre_block_of_333_has_shares_of_all_54_faces():
    """(e) every interior face of the 3 x 3 x 3 box adds to the centre cell's restricted 27 x 27 block; its own six faces alone miss
    a large part of it"""
    nc = (3, 3, 3)
    verts = cref.box_vertices(nc)
    w = np.random.default_rng(1).uniform(-1, 1, 3 * nref.n_velocity(nc))
    dofs = nref._cell_dofs(nc, 1, 1, 1)
    nf = scr.n_interior_faces(nc)
    assert nf == 54
    full = scr.cip_matrix(1.0, w, nc, verts, 0)[np.ix_(dofs, dofs)]
    own, total = np.zeros_like(full), np.zeros_like(full)
    for k, (dofsA, dofsB, *_rest) in enumerate(scr.face_pairs(nc, verts)):
        share = scr.cip_matrix(1.0, w, nc, verts, 0, faces={k})[np.ix_(dofs, dofs)]
        assert np.abs(share).max() > 1e-6 * np.abs(full).max(), k
        total += share
        if set(dofsA) == set(dofs) or set(dofsB) == set(dofs):
            own += share
    assert rel(total, full) < 1e-13
    print("own six faces alone: off by %.2f (relative Frobenius norm)" % rel(own, full))
    assert rel(own, full) > 0.1


@pytest.mark.parametrize("name", list(scr.CASES) + ["mode0"])
def test_gpu_cases_are_not_hollow_and_well_conditioned(name, oracle_mod):
    """(f), (g): the term changes the reference vmult by at least 1e-2 relative, and cond_max <= 1e6"""
    p, base, ref = scr.mode0() if name == "mode0" else scr.case(name)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    change = rel(np.concatenate(ref.vmult(X)), np.concatenate(base.vmult(X)))
    print("%-26s change of vmult %.2e  cond_max %.3e (without the term %.3e)" % (name, change, ref.cond_max, base.cond_max))
    assert change >= 1e-2
    assert ref.cond_max <= 1e6


def test_constrained_diagonal_keeps_the_cip_diagonal(oracle_mod):
    """rows and columns of strongly constrained DoFs are dropped and the diagonal, the CIP diagonal included, is kept"""
    p, base, ref = scr.case("pert412_jac_free")
    con = np.flatnonzero(ref.constrained)
    assert con.size
    K0, K1 = base.K[0], ref.K[0]
    off = K1[con].copy()
    off[np.arange(con.size), con] = 0.0
    assert not off.any() and not (K1[:, con] - np.diag(K1.diagonal())[:, con]).any()
    assert np.all(K1[con, con] >= K0[con, con]) and np.any(K1[con, con] > K0[con, con])
