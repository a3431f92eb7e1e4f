"""Per-cell Vanka smoother of the LINEARISED Stokes operator at velocity degree 3 (stfem_stokes_vanka_create_linearised_space;
FE_Q(3)^3 x FE_Q(2) / FE_DGP(2)): the HIP set-up with the convection term in the cell matrices, a launch per linearisation state, and the
streaming apply against the dense numpy restatement tests/stokes_vanka_q3_linearised_reference.py.  fp64, rel-L2 per block and overall.

Tolerance: the 1e-10 of tests/test_gpu_stokes_vanka_q3.py; tests/test_stokes_vanka_q3_linearised_reference_cpu.py holds every case here
below the same condition bound (the term moves the conditions by under 1 %) and shows that the term is visible in each (the apply
differs from the mode-0 apply by 4e-3 ... 2e-2, the bound asserted here is 1e-4)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stokes_vanka_q3_linearised_reference as lq3
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


def _operator(stfem, p):
    return stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=p.verts if p.pert else None, dirichlet_mask=p.mask, viscosity=p.nu,
                                                      dg_pressure=p.dg)


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) for v, x in zip(p.var, host)]


def _states(op, lin):
    """device copies of the states; the pressure entries stay None"""
    return [None if b is None else op.initialize_dof_vector(0, b) for b in lin]


def _apply(op, p, V, X):
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, 9.0) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    return [d.download() for d in dst], src, dst


def _source(p, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n) for n in p.sizes]


def _same(Ya, Yb):
    return all(np.array_equal(a, b) for a, b in zip(Ya, Yb))


@pytest.mark.parametrize("name", list(lq3.CASES))
def test_blocks_vs_reference(name, stfem, oracle_mod):
    p, mode, lin, ref, _ = lq3.case(name)
    op = _operator(stfem, p)
    lv = _states(op, lin)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=mode)
    assert V.n_classes == int(np.prod(p.nc)) and V.setup_batches >= 1  # one block per cell
    X = _source(p)
    Y, src, dst = _apply(op, p, V, X)
    want = ref.vmult(X)
    overall = rel(np.concatenate(Y), np.concatenate(want))
    per_block = [rel(Y[b], want[b]) for b in range(p.nb)]
    Y0, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta), X)
    visible = rel(np.concatenate(Y), np.concatenate(Y0))
    print(name, "mode", mode, "rows", p.rows, "overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block),
          "differs from mode 0 by %.2e" % visible)
    assert overall < TOL
    assert max(per_block) < TOL, per_block
    assert visible >= lq3.VISIBLE
    # two applies give identical bits; the relaxation step; the alias refusal
    V.vmult(dst, src)
    assert _same([d.download() for d in dst], Y)
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
def test_single_cell_inverts_the_linearised_operator(name, stfem):
    """one unconstrained cell: V (A(b) x) = x, A(b) applied through the operator's st_vmult in the mode"""
    p = q3r.problem(q3r.CASES[name])
    mode, lin = lq3.CASES[name], lq3.states(p)
    op = _operator(stfem, p)
    lv = _states(op, lin)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=mode)
    X = _source(p, 6)
    zeros = [np.zeros(n) for n in p.sizes]
    x, ax, y = _device(op, p, X), _device(op, p, zeros), _device(op, p, zeros)
    op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, ax, x, variable_major=p.variable_major, lin=lv, mode=mode)
    V.vmult(y, ax)
    got = np.concatenate([v.download() for v in y])
    print(name, "mode", mode, "V A(b) x - x: %.3e" % rel(got, np.concatenate(X)))
    assert rel(got, np.concatenate(X)) < TOL


@pytest.mark.parametrize("name", ["pert222_dgp_cg2", "box322_q2"])
def test_mode_0_through_the_new_entry_is_create_space_bitwise(name, stfem):
    p = q3r.problem(q3r.CASES[name])
    op = _operator(stfem, p)
    X = _source(p)
    Y, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta), X)
    assert np.linalg.norm(np.concatenate(Y)) > 0
    # lin null: the C entry itself (for_space without lin and mode goes to stfem_stokes_vanka_create_space)
    V = stfem.StokesPreconditionVanka.__new__(stfem.StokesPreconditionVanka)
    bv, A, B = V._blocks(op, p.var, p.Alpha, p.Beta, None)
    d = stfem._StokesVankaLinearisedSpaceDesc()
    d.n_blocks, d.block_variable, d.Alpha, d.Beta, d.mode, d.lin_blocks = p.nb, bv, stfem._p(A), stfem._p(B), 0, None
    h = C.c_void_p()
    assert stfem.lib().stfem_stokes_vanka_create_linearised_space(op._h, C.byref(d), C.byref(h)) == 0 and h.value
    V._h = h
    assert _same(_apply(op, p, V, X)[0], Y)
    # lin given: not read
    lv = _states(op, lq3.states(p))
    Vl = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=0)
    assert _same(_apply(op, p, Vl, X)[0], Y)
    Vl.update(None)
    assert _same(_apply(op, p, Vl, X)[0], Y)


def test_degree_2_through_the_new_entry_is_create_linearised_bitwise(stfem):
    p = svr.problem(svr.CASES["pert322_jac_weak"])
    op = stfem.StokesMatrixFreeOperator(p.nc, vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=p.dg,
                                        weak_boundary_ids=[f for f in range(6) if p.weak >> f & 1])
    X = _source(p)
    lv = _states(op, p.lin)
    Ya, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=p.mode), X)
    Yb, _, _ = _apply(op, p, stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=lv, mode=p.mode, per_cell=True), X)
    assert p.mode == 2 and np.linalg.norm(np.concatenate(Ya)) > 0
    assert _same(Ya, Yb)


def test_update_equals_a_fresh_smoother_bitwise(stfem):
    p = q3r.problem(q3r.CASES["pert222_dgp_cg2"])
    op = _operator(stfem, p)
    X = _source(p)
    lin_a, lin_b = _states(op, lq3.states(p)), _states(op, lq3.states(p, seed=12))
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lin_a, mode=2)
    Ya, _, _ = _apply(op, p, V, X)
    Yb, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lin_b, mode=2), X)
    assert rel(np.concatenate(Ya), np.concatenate(Yb)) > 1e-4
    V.update(lin_b)
    assert _same(_apply(op, p, V, X)[0], Yb)
    V.update(lin_a)
    assert _same(_apply(op, p, V, X)[0], Ya)
    # the refusals of update are those of degree 2
    with pytest.raises(stfem.StfemError) as e:
        V.update(None)
    assert e.value.status == -1
    with pytest.raises(stfem.StfemError) as e:
        V.update([None] * p.nb)
    assert e.value.status == -1
    assert _same(_apply(op, p, V, X)[0], Ya)


def test_one_buffer_for_both_time_dofs_equals_two_of_equal_content(stfem):
    p = q3r.problem(q3r.CASES["pert222_dgp_cg2"])
    op = _operator(stfem, p)
    X = _source(p)
    b = lq3.states(p)[p.var.index(0)]
    one = op.initialize_dof_vector(0, b)
    shared = [one if v == 0 else None for v in p.var]
    twice = [op.initialize_dof_vector(0, b) if v == 0 else None for v in p.var]
    Y1, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=shared, mode=2), X)
    Y2, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=twice, mode=2), X)
    assert np.linalg.norm(np.concatenate(Y1)) > 0 and _same(Y1, Y2)


def test_constrained_entries_and_pressure_entries_of_lin_are_not_read(stfem):
    """NaN in the strongly constrained entries of the states and in a pressure-sized dummy changes no bit"""
    p = q3r.problem(q3r.CASES["pert222_q2_cg2_freex"])
    op = _operator(stfem, p)
    X = _source(p)
    lin = lq3.states(p)
    Y, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=_states(op, lin), mode=1), X)
    cu = np.tile(q3r.constrained(p.nc, p.mask), 3)
    assert 0 < cu.sum() < cu.size
    dummy = op.initialize_dof_vector(1, np.full(p.n_p, np.nan))
    poisoned = [dummy if b is None else op.initialize_dof_vector(0, np.where(cu, np.nan, b)) for b in lin]
    Yn, _, _ = _apply(op, p, stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=poisoned, mode=1), X)
    assert np.all(np.isfinite(np.concatenate(Yn))) and _same(Y, Yn)


def test_setup_in_batches_is_bit_identical(stfem, monkeypatch):
    """three batches of one cell layer against one batch, two states (two time steps at once on the mesh of box223_dgp)"""
    spec = list(q3r.CASES["box223_dgp"])
    spec[5], spec[8] = 2, 404  # two time steps at once: four blocks, a state per step
    p = q3r.problem(tuple(spec))
    assert p.nb == 4
    op = _operator(stfem, p)
    lv = _states(op, lq3.states(p))
    assert len({v.ptr for v in lv if v is not None}) == 2
    X = _source(p)
    V1 = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=2)
    assert V1.setup_batches == 1
    Y1, _, _ = _apply(op, p, V1, X)
    monkeypatch.setenv("STFEM_VANKA_SETUP_LAYERS", "1")
    V3 = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=2)
    assert V3.setup_batches == 3
    Y3, _, _ = _apply(op, p, V3, X)
    assert np.linalg.norm(np.concatenate(Y1)) > 0 and _same(Y1, Y3)


def test_refusals(stfem):
    q = q3r.problem(q3r.CASES["box223_dgp"])
    oq = _operator(stfem, q)
    lv = _states(oq, lq3.states(q))
    for kw, reason in ((dict(lin=lv, mode=3), "mode = 3"), (dict(lin=None, mode=2), "needs lin_blocks"),
                       (dict(lin=[None] * q.nb, mode=1), "lin_blocks[0] of a velocity block is null")):
        with pytest.raises(stfem.StfemError) as e:
            stfem.StokesPreconditionVanka.for_space(oq, q.var, q.Alpha, q.Beta, **kw)
        assert e.value.status == -1 and reason in str(e.value), str(e.value)
    # dG(2) with a mode: six blocks, 657 rows
    p = q3r.problem(q3r.TOO_MANY_ROWS)
    assert p.nb == 6 and sum(192 if v == 0 else 27 for v in p.var) == 657
    op = _operator(stfem, p)
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=_states(op, lq3.states(p)), mode=2)
    assert e.value.status == -2 and "512" in str(e.value) and "657" in str(e.value)
    # the entries of degree 2 keep refusing a degree-3 context
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka(oq, q.var, q.Alpha, q.Beta, lin=lv, mode=2)
    assert e.value.status == -2 and "velocity degree 2 only" in str(e.value)


def test_relaxation_follows_the_reference_history(stfem, oracle_mod):
    """eight sweeps x <- x + 0.5 V (f - A(b) x) on the perturbed 2 x 2 x 2 mesh, FE_DGP(2), cG(1), nu = 1, jacobian about
    0.5 uniform(-1, 1): the residual norms of the device operator and smoother equal those of the restatement to 1e-8 relative (CPU:
    12.68 -> 0.7131, decreasing; tests/test_stokes_vanka_q3_linearised_reference_cpu.py)"""
    p, mode, lin, ref, f, want = lq3.relaxation()
    op = _operator(stfem, p)
    lv = _states(op, lin)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta, lin=lv, mode=mode)
    zeros = [np.zeros(n) for n in p.sizes]
    x, r = _device(op, p, zeros), _device(op, p, zeros)
    norms = []
    for _ in range(q3r.RELAX_SWEEPS):
        op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, r, x, variable_major=p.variable_major, lin=lv, mode=mode)
        res = [f[i] - r[i].download() for i in range(p.nb)]
        norms.append(np.sqrt(sum(np.sum(q * q) for q in res)))
        for i in range(p.nb):
            r[i].upload(res[i])
        V.step(x, q3r.RELAX_OMEGA, True, r)
    print("history:", " ".join("%.6e" % v for v in norms))
    assert np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)
