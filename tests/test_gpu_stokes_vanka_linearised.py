"""Cell-patch Vanka smoother of the linearised two-variable system with one block per cell (stfem_stokes_vanka_create_linearised /
_update; the reference's reinit_asm, include/stmg.h:929-965, 704-742): the HIP set-up (cell matrices of A(b), assembly, Gauss-Jordan)
and the streaming apply against the dense numpy restatement tests/stokes_vanka_reference.py.  fp64, rel-L2 per block and overall.

Tolerance: the 1e-10 that tests/test_gpu_stokes_vanka.py uses for inverted blocks.  tests/test_stokes_vanka_reference_cpu.py records the
largest cond(B_c) of these cases, 1.2e5 (perturbed 3 x 2 x 2, jacobian, weak faces), against 1.1e5 over the plain Stokes cases of that
file: within a factor of 10, so its tolerance holds here."""
import importlib

import numpy as np
import pytest

import stokes_vanka_reference as svr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _operator(stfem, p):
    return stfem.StokesMatrixFreeOperator(p.nc, vertices=p.verts if p.pert else None, dirichlet_mask=p.mask, viscosity=p.nu,
                                          weak_boundary_ids=[f for f in range(6) if p.weak >> f & 1], dg_pressure=p.dg)


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) if x is not None else None for v, x in zip(p.var, host)]


def _smoother(stfem, op, p, lin_host=None):
    """(smoother, device linearisation vectors - kept alive by the caller)"""
    dlin = _device(op, p, p.lin if lin_host is None else lin_host) if p.mode else None
    return stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=dlin, mode=p.mode, per_cell=True), dlin


def _apply(op, p, V, X):
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, 9.0) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    return [d.download() for d in dst], src, dst


@pytest.mark.parametrize("name", [n for n in svr.CASES if n != "cell_jac_dgp"])
def test_per_cell_blocks_vs_reference(name, stfem, oracle_mod):
    p, ref = svr.case(name)
    op = _operator(stfem, p)
    assert (op.n_velocity, op.n_pressure) == (p.n_u, p.n_p)
    V, dlin = _smoother(stfem, op, p)
    assert V.n_classes == int(np.prod(p.nc))  # one block per cell
    rng = np.random.default_rng(3)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    Y, src, dst = _apply(op, p, V, X)
    want = ref.vmult(X)
    overall = rel(np.concatenate(Y), np.concatenate(want))
    per_block = [rel(Y[b], want[b]) for b in range(p.nb)]
    print(name, "overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block))
    assert overall < TOL
    assert max(per_block) < TOL, per_block
    if name == "box333":  # the same blocks as the class variant of the box
        Vc = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta)
        assert Vc.n_classes == 27
        Yc, _, _ = _apply(op, p, Vc, X)
        assert rel(np.concatenate(Y), np.concatenate(Yc)) < TOL
    # repeat apply: reproducible; the relaxation step dst += omega V src
    V.vmult(dst, src)
    assert all(np.array_equal(d.download(), y) for d, y in zip(dst, Y))
    V.step(dst, 0.6, True, src)
    assert rel(np.concatenate([d.download() for d in dst]), 1.6 * np.concatenate(Y)) < 1e-12
    with pytest.raises(stfem.StfemError):
        V.vmult(src, src)


def test_general_mesh_through_the_plain_create(stfem, oracle_mod):
    """stfem_stokes_vanka_create on a general mesh forwards to one block per cell, mode 0"""
    p, ref = svr.case("pert232")
    op = _operator(stfem, p)
    V = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta)
    assert V.n_classes == int(np.prod(p.nc))
    X = [np.random.default_rng(4).uniform(-1, 1, n) for n in p.sizes]
    Y, _, _ = _apply(op, p, V, X)
    assert rel(np.concatenate(Y), np.concatenate(ref.vmult(X))) < TOL


def test_single_cell_inverts_the_linearised_operator(stfem):
    p = svr.problem(svr.CASES["cell_jac_dgp"])
    op = _operator(stfem, p)
    V, dlin = _smoother(stfem, op, p)
    rng = np.random.default_rng(6)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    x, ax, y = _device(op, p, X), _device(op, p, [np.zeros(n) for n in p.sizes]), _device(op, p, [np.zeros(n) for n in p.sizes])
    op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, ax, x, variable_major=p.variable_major, lin=dlin, mode=p.mode)
    V.vmult(y, ax)
    got = np.concatenate([v.download() for v in y])
    print("V A x - x: %.3e" % rel(got, np.concatenate(X)))
    assert rel(got, np.concatenate(X)) < TOL


def test_update_equals_a_fresh_create_bitwise(stfem):
    p = svr.problem(svr.CASES["pert322_jac_weak"])
    q = svr.problem(svr.CASES["pert322_jac_weak"], seed=12)  # the same problem, other linearisation states
    assert not np.array_equal(p.lin[0], q.lin[0])
    op = _operator(stfem, p)
    V, keep1 = _smoother(stfem, op, p)
    X = [np.random.default_rng(7).uniform(-1, 1, n) for n in p.sizes]
    Y1, _, _ = _apply(op, p, V, X)
    lin2 = _device(op, p, q.lin)
    V.update(lin2)
    Y2, _, _ = _apply(op, p, V, X)
    W, keep2 = _smoother(stfem, op, p, q.lin)
    Y3, _, _ = _apply(op, p, W, X)
    assert rel(np.concatenate(Y2), np.concatenate(Y1)) > 1e-6  # the blocks did change
    assert all(np.array_equal(a, b) for a, b in zip(Y2, Y3))
    # equal pointers are one state: every time dof linearised about the first vector, whichever way it is said
    same = [lin2[0] if v == 0 else None for v in p.var]
    V.update(same)
    Y4, _, _ = _apply(op, p, V, X)
    qq = [q.lin[0] if v == 0 else None for v in p.var]
    W2, keep3 = _smoother(stfem, op, p, [None if a is None else a.copy() for a in qq])  # distinct pointers, equal values
    Y5, _, _ = _apply(op, p, W2, X)
    assert all(np.array_equal(a, b) for a, b in zip(Y4, Y5))


def test_refusals(stfem):
    import ctypes as C
    p = svr.problem(svr.CASES["pert322_jac_weak"])
    op = _operator(stfem, p)
    lib = stfem.lib()
    lin = _device(op, p, p.lin)
    ptrs = (C.c_void_p * p.nb)(*[getattr(v, "ptr", v) for v in lin])
    bv = (C.c_int32 * p.nb)(*p.var)
    A, B = np.ascontiguousarray(p.Alpha), np.ascontiguousarray(p.Beta)
    dp = C.POINTER(C.c_double)

    def create(nb, bv_, mode, lin_):
        h = C.c_void_p(1)  # must come back null
        rc = lib.stfem_stokes_vanka_create_linearised(op._h, nb, bv_, A.ctypes.data_as(dp), B.ctypes.data_as(dp), mode, lin_, C.byref(h))
        assert not h.value
        return rc

    assert create(p.nb, bv, 3, ptrs) == -1        # STFEM_ERR_INVALID_ARGUMENT: a mode outside 0..2
    assert create(p.nb, bv, -1, ptrs) == -1
    assert create(p.nb, bv, 2, None) == -1        # no linearisation with a mode that needs one
    holes = (C.c_void_p * p.nb)(*[None] * p.nb)
    assert create(p.nb, bv, 2, holes) == -1       # a null entry of a velocity block
    bv9 = (C.c_int32 * 9)(*([0, 1] * 4 + [1]))
    A9 = np.eye(9)
    h = C.c_void_p(1)
    assert lib.stfem_stokes_vanka_create_linearised(op._h, 9, bv9, A9.ctypes.data_as(dp), A9.ctypes.data_as(dp), 0, None, C.byref(h)) == -2
    assert not h.value                            # STFEM_ERR_UNSUPPORTED: more than VK_MAX_BLOCKS blocks
    bv7 = (C.c_int32 * 7)(*[0] * 7)               # 567 rows > VK_MAX_ROWS
    h = C.c_void_p(1)
    assert lib.stfem_stokes_vanka_create_linearised(op._h, 7, bv7, A9.ctypes.data_as(dp), A9.ctypes.data_as(dp), 0, None, C.byref(h)) == -2
    assert not h.value
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=None, mode=2)
    assert e.value.status == -1
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=lin, mode=3)
    assert e.value.status == -1
    # the class blocks of a box hold the linear operator only
    box = svr.problem(svr.CASES["box333"])
    Vc = stfem.StokesPreconditionVanka(_operator(stfem, box), box.var, box.Alpha, box.Beta)
    with pytest.raises(stfem.StfemError) as e:
        Vc.update(None)
    assert e.value.status == -2


def test_relaxation_follows_the_reference_history(stfem, oracle_mod):
    """eight sweeps x <- x + omega V (f - A_jac x) on the perturbed 3 x 3 x 2 mesh: the residual norms of the device operator and
    smoother equal those of the restatement to 1e-8 relative (the history itself decreases: the CPU test)"""
    p, _, f, want = svr.relaxation()
    op = _operator(stfem, p)
    V, dlin = _smoother(stfem, op, p)
    x = _device(op, p, [np.zeros(n) for n in p.sizes])
    r = _device(op, p, [np.zeros(n) for n in p.sizes])
    norms = []
    for _ in range(svr.RELAX_SWEEPS):
        op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, r, x, variable_major=p.variable_major, lin=dlin, mode=p.mode)
        res = [f[i] - r[i].download() for i in range(p.nb)]
        norms.append(np.sqrt(sum(np.sum(q * q) for q in res)))
        for i in range(p.nb):
            r[i].upload(res[i])
        V.step(x, svr.RELAX_OMEGA, True, r)
    print("history:", " ".join("%.6e" % v for v in norms))
    assert np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)
