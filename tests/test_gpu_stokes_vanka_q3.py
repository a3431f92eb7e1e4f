"""Per-cell Vanka smoother of the Stokes system at velocity degree 3 (stfem_stokes_vanka_create_space; FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)):
the HIP set-up (cell matrices at the 4 x 4 x 4 Gauss points, assembly, Gauss-Jordan) and the streaming apply against the dense numpy
restatement tests/stokes_vanka_q3_reference.py.  fp64, rel-L2 per block and overall.

Tolerance: the 1e-10 of tests/test_gpu_stokes_vanka_linearised.py, which stands on blocks of cond 1.2e5;
tests/test_stokes_vanka_q3_reference_cpu.py holds every case here below ten times that (the largest: 1.0e6), so it carries over."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stokes_vanka_q3_reference as q3r
import stokes_vanka_reference as svr

pytestmark = pytest.mark.gpu
TOL = 1e-10
ERR_ALIAS = -6  # STFEM_ERR_ALIAS


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("STFEM_VANKA_SETUP_LAYERS", raising=False)


def _operator(stfem, p, vertices="as the case"):
    verts = (p.verts if p.pert else None) if isinstance(vertices, str) else vertices
    return stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=p.dg)


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) for v, x in zip(p.var, host)]


def _apply(op, p, V, X):
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, 9.0) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    return [d.download() for d in dst], src, dst


def _source(p, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n) for n in p.sizes]


@pytest.mark.parametrize("name", list(q3r.CASES))
def test_blocks_vs_reference(name, stfem, oracle_mod):
    p, ref = q3r.case(name)
    op = _operator(stfem, p)
    assert (op.n_velocity, op.n_pressure) == (p.n_u, p.n_p)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    assert V.n_classes == int(np.prod(p.nc)) and V.setup_batches >= 1  # one block per cell
    X = _source(p)
    Y, src, dst = _apply(op, p, V, X)
    want = ref.vmult(X)
    overall = rel(np.concatenate(Y), np.concatenate(want))
    per_block = [rel(Y[b], want[b]) for b in range(p.nb)]
    print(name, "rows", p.rows, "overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block))
    assert overall < TOL
    assert max(per_block) < TOL, per_block
    # two applies give identical bits; update without a linearisation rebuilds the same blocks; the relaxation step
    V.vmult(dst, src)
    assert all(np.array_equal(d.download(), y) for d, y in zip(dst, Y))
    V.update(None)
    V.vmult(dst, src)
    assert all(np.array_equal(d.download(), y) for d, y in zip(dst, Y))
    D0 = [np.random.default_rng(20 + b).uniform(-1, 1, n) for b, n in enumerate(p.sizes)]
    for d, d0 in zip(dst, D0):
        d.upload(d0)
    V.step(dst, 0.6, True, src)
    got = np.concatenate([d.download() for d in dst])
    assert np.linalg.norm(got - (np.concatenate(D0) + 0.6 * np.concatenate(Y))) <= 1e-14 * np.linalg.norm(got)
    with pytest.raises(stfem.StfemError) as e:
        V.vmult(src, src)
    assert e.value.status == ERR_ALIAS


@pytest.mark.parametrize("name", ["cell_free_dgp", "cell_free_q2"])
def test_single_cell_inverts_the_operator(name, stfem):
    p = q3r.problem(q3r.CASES[name])
    op = _operator(stfem, p)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    X = _source(p, 6)
    zeros = [np.zeros(n) for n in p.sizes]
    x, ax, y = _device(op, p, X), _device(op, p, zeros), _device(op, p, zeros)
    op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, ax, x, variable_major=p.variable_major)
    V.vmult(y, ax)
    got = np.concatenate([v.download() for v in y])
    print(name, "V A x - x: %.3e" % rel(got, np.concatenate(X)))
    assert rel(got, np.concatenate(X)) < TOL


def test_setup_in_batches_is_bit_identical(stfem, monkeypatch):
    p = q3r.problem(q3r.CASES["box223_dgp"])
    op = _operator(stfem, p)
    X = _source(p)
    V1 = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    assert V1.setup_batches == 1
    Y1, _, _ = _apply(op, p, V1, X)
    monkeypatch.setenv("STFEM_VANKA_SETUP_LAYERS", "1")
    V3 = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    assert V3.setup_batches == 3
    Y3, _, _ = _apply(op, p, V3, X)
    assert all(np.array_equal(a, b) for a, b in zip(Y1, Y3))


def test_box_context_equals_the_mesh_given_as_vertices(stfem, oracle_mod):
    p, ref = q3r.case("box322_q2")
    X = _source(p)
    box = _operator(stfem, p, vertices=None)
    Yb, _, _ = _apply(box, p, stfem.StokesPreconditionVanka.for_space(box, p.var, p.Alpha, p.Beta), X)
    gen = _operator(stfem, p, vertices=stfem.mesh_vertices(p.nc))
    Yg, _, _ = _apply(gen, p, stfem.StokesPreconditionVanka.for_space(gen, p.var, p.Alpha, p.Beta), X)
    print("box vs vertices: %.3e" % rel(np.concatenate(Yb), np.concatenate(Yg)))
    assert rel(np.concatenate(Yb), np.concatenate(Yg)) < TOL
    assert max(rel(a, b) for a, b in zip(Yb, Yg)) < TOL


def test_degree_2_through_the_descriptor_is_create_linearised_bitwise(stfem):
    p = svr.problem(svr.CASES["pert232"])
    op = stfem.StokesMatrixFreeOperator(p.nc, vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=p.dg)
    X = _source(p)

    def apply(V):
        src = [op.initialize_dof_vector(v, x) for v, x in zip(p.var, X)]
        dst = [op.initialize_dof_vector(v, np.full(n, 9.0)) for v, n in zip(p.var, p.sizes)]
        V.vmult(dst, src)
        return [d.download() for d in dst]

    Ya = apply(stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta))
    Yb = apply(stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, mode=0, per_cell=True))
    assert np.linalg.norm(np.concatenate(Ya)) > 0
    assert all(np.array_equal(a, b) for a, b in zip(Ya, Yb))


def test_refusals(stfem):
    p = q3r.problem(q3r.TOO_MANY_ROWS)  # dG(2): six blocks, 657 rows
    assert p.nb == 6 and sum(192 if v == 0 else 27 for v in p.var) == 657
    op = _operator(stfem, p)
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    assert e.value.status == -2 and "512" in str(e.value) and "657" in str(e.value)
    q = q3r.problem(q3r.CASES["box223_dgp"])
    oq = _operator(stfem, q)
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka.for_space(oq, q.var, q.Alpha, q.Beta, reserved=(0, 0, 0, 5))
    assert e.value.status == -1 and "reserved[3]" in str(e.value)
    # the handle comes back null from the C entry itself
    L, dp = stfem.lib(), C.POINTER(C.c_double)
    d = stfem._StokesVankaSpaceDesc()
    bv = (C.c_int32 * p.nb)(*p.var)
    A, B = np.ascontiguousarray(p.Alpha), np.ascontiguousarray(p.Beta)
    d.n_blocks, d.block_variable, d.Alpha, d.Beta = p.nb, bv, A.ctypes.data_as(dp), B.ctypes.data_as(dp)
    h = C.c_void_p(1)
    assert L.stfem_stokes_vanka_create_space(op._h, C.byref(d), C.byref(h)) == -2 and not h.value
    # the old constructor keeps refusing a degree-3 context
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka(oq, q.var, q.Alpha, q.Beta)
    assert e.value.status == -2 and "velocity degree 2 only" in str(e.value)
    # a destination that is a source
    V = stfem.StokesPreconditionVanka.for_space(oq, q.var, q.Alpha, q.Beta)
    x = _device(oq, q, _source(q))
    ptr = (C.c_void_p * q.nb)(*[v.ptr for v in x])
    assert L.stfem_stokes_vanka_vmult(V._h, ptr, ptr, None) == ERR_ALIAS
    assert L.stfem_stokes_vanka_step(V._h, ptr, 0.5, 1, ptr, None) == ERR_ALIAS


@pytest.mark.parametrize("omega", [q3r.RELAX_OMEGA, 0.7])
def test_relaxation_follows_the_reference_history(omega, stfem, oracle_mod):
    """eight sweeps x <- x + omega V (f - A x) on the perturbed 2 x 2 x 2 mesh, FE_DGP(2), cG(1), nu = 1: the residual norms of the
    device operator and smoother equal those of the restatement to 1e-8 relative, and decrease (CPU: 12.7 -> 0.713 at omega 0.5,
    12.7 -> 0.343 at omega 0.7)"""
    p, ref, f, want = q3r.relaxation()
    if omega != q3r.RELAX_OMEGA:
        want = q3r.relaxation_history(p, ref, f, omega)
    op = _operator(stfem, p)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    zeros = [np.zeros(n) for n in p.sizes]
    x, r = _device(op, p, zeros), _device(op, p, zeros)
    norms = []
    for _ in range(q3r.RELAX_SWEEPS):
        op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, r, x, variable_major=p.variable_major)
        res = [f[i] - r[i].download() for i in range(p.nb)]
        norms.append(np.sqrt(sum(np.sum(q * q) for q in res)))
        for i in range(p.nb):
            r[i].upload(res[i])
        V.step(x, omega, True, r)
    print("omega", omega, "history:", " ".join("%.6e" % v for v in norms))
    assert np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)
    assert all(b < a for a, b in zip(norms, norms[1:]))
