"""Per-cell Stokes Vanka blocks of the operator WITH the CIP term (stfem_stokes_vanka_create_linearised_cip / _update): the HIP set-up
(stokes_cip_cell_matrices_kernel, the CIP branch of stokes_vanka_assemble_kernel) against the dense numpy restatement
tests/stokes_vanka_cip_reference.py.  fp64, rel-L2 per block and overall.

Tolerance: the 1e-10 of tests/test_gpu_stokes_vanka_linearised.py; tests/test_stokes_vanka_cip_reference_cpu.py holds the condition
numbers of these cases within that file's range (cond_max <= 1.3e5 here, 1.15e5 there) and shows that the term changes every case's
vmult by at least 1e-2, eight orders above the bound.

Run as a program (the batch test starts it in a fresh process): <file> <case> <out.npy> applies the smoother of the case to the test's
vector and saves the result and the batch count."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stokes_vanka_cip_reference as scr  # noqa: E402
import stokes_vanka_reference as svr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
KNOB = "STFEM_VANKA_SETUP_LAYERS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _smoother(stfem, op, p, lin_host=None, delta0=scr.DELTA0, per_cell=True):
    """(smoother, device linearisation vectors - kept alive by the caller)"""
    host = p.lin if lin_host is None else lin_host
    dlin = _device(op, p, host) if any(x is not None for x in host) else None
    return stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=dlin, mode=p.mode, per_cell=per_cell, delta0=delta0), dlin


def _apply(op, p, V, X):
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, 9.0) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    return [d.download() for d in dst]


def _x(p):
    return [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]


def _check_against(name, p, ref, base, Y, X):
    want = ref.vmult(X)
    overall = rel(np.concatenate(Y), np.concatenate(want))
    per_block = [rel(Y[b], want[b]) for b in range(p.nb)]
    hollow = rel(np.concatenate(Y), np.concatenate(base.vmult(X)))
    print(name, "overall %.3e" % overall, "largest block %.3e" % max(per_block), "ratio to the bound %.3e" % (max(overall, *per_block) / TOL),
          "| against the blocks without the term %.3e" % hollow)
    assert overall < TOL
    assert max(per_block) < TOL, per_block
    assert hollow > 1e-3  # (the device blocks do hold the term)


@pytest.mark.parametrize("name", list(scr.CASES))
def test_blocks_with_the_term_vs_reference(name, stfem, oracle_mod, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    p, base, ref = scr.case(name)
    op = _operator(stfem, p)
    assert (op.n_velocity, op.n_pressure) == (p.n_u, p.n_p)
    V, dlin = _smoother(stfem, op, p)
    assert V.n_classes == int(np.prod(p.nc)) and V.setup_batches == 1
    X = _x(p)
    Y = _apply(op, p, V, X)
    _check_against(name, p, ref, base, Y, X)
    # two creates agree bit for bit
    W, dlin2 = _smoother(stfem, op, p)
    Z = _apply(op, p, W, X)
    assert all(np.array_equal(a, b) for a, b in zip(Y, Z))
    # delta0 = 0 through the new entry point: the blocks of _create_linearised, bit for bit
    lib = stfem.lib()
    h = C.c_void_p()
    bv = (C.c_int32 * p.nb)(*p.var)
    A, B = np.ascontiguousarray(p.Alpha), np.ascontiguousarray(p.Beta)
    dp = C.POINTER(C.c_double)
    ptrs = (C.c_void_p * p.nb)(*[getattr(v, "ptr", v) for v in dlin])
    assert lib.stfem_stokes_vanka_create_linearised_cip(op._h, p.nb, bv, A.ctypes.data_as(dp), B.ctypes.data_as(dp), p.mode, ptrs, 0.0,
                                                        C.byref(h)) == 0
    V0 = object.__new__(stfem.StokesPreconditionVanka)  # (the wrapper's own delta0 = 0 does not go through the new entry point)
    V0.op, V0.nb, V0._h = op, p.nb, h
    Y0 = _apply(op, p, V0, X)
    V1, _ = _smoother(stfem, op, p, delta0=0.0)
    Y1 = _apply(op, p, V1, X)
    assert all(np.array_equal(a, b) for a, b in zip(Y0, Y1))
    assert rel(np.concatenate(Y1), np.concatenate(base.vmult(X))) < TOL


def test_batched_setup_in_a_fresh_process_equals_one_batch(stfem, oracle_mod, monkeypatch, tmp_path):
    """box224_jac_dg1, one cell layer per batch (four batches, windows that start below the batch, faces to cells outside the patch and
    outside the batch) in a child process against the one-batch set-up here: bit for bit"""
    name = "box224_jac_dg1"
    monkeypatch.delenv(KNOB, raising=False)
    p, base, ref = scr.case(name)
    op = _operator(stfem, p)
    V, dlin = _smoother(stfem, op, p)
    assert V.setup_batches == 1
    X = _x(p)
    one = np.concatenate(_apply(op, p, V, X))
    out = tmp_path / "batched.npy"
    env = dict(os.environ, **{KNOB: "1"})
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.load(out)
    assert int(got[-1]) == 4  # setup_batches
    assert np.array_equal(got[:-1], one)


def test_mesh_without_interior_face_equals_the_blocks_without_the_term(stfem):
    p = svr.problem(scr.CELL)
    op = _operator(stfem, p)
    X = _x(p)
    V1, keep1 = _smoother(stfem, op, p, delta0=1.0)
    V0, keep0 = _smoother(stfem, op, p, delta0=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(_apply(op, p, V1, X), _apply(op, p, V0, X)))


def test_update_equals_a_fresh_create_bitwise(stfem, oracle_mod):
    name = "pert232_form_dgp_cg2_tm"
    p, base, ref = scr.case(name)
    lin2_host = scr.other_states(name)
    assert not np.array_equal(p.lin[p.index(0, 0, 0)], lin2_host[p.index(0, 0, 0)])
    op = _operator(stfem, p)
    V, keep1 = _smoother(stfem, op, p)
    X = _x(p)
    Y1 = _apply(op, p, V, X)
    lin2 = _device(op, p, lin2_host)
    V.update(lin2)  # keeps the delta0 of creation
    Y2 = _apply(op, p, V, X)
    W, keep2 = _smoother(stfem, op, p, lin2_host)
    Y3 = _apply(op, p, W, X)
    assert rel(np.concatenate(Y2), np.concatenate(Y1)) > 1e-6  # the blocks did change
    assert all(np.array_equal(a, b) for a, b in zip(Y2, Y3))
    W0, keep3 = _smoother(stfem, op, p, lin2_host, delta0=0.0)
    assert rel(np.concatenate(Y2), np.concatenate(_apply(op, p, W0, X))) > 1e-3  # and still hold the term


def test_mode0_with_lin_as_weight(stfem, oracle_mod):
    p, base, ref = scr.mode0()
    assert p.mode == 0
    op = _operator(stfem, p)
    V, dlin = _smoother(stfem, op, p)
    X = _x(p)
    _check_against("mode0", p, ref, base, _apply(op, p, V, X), X)
    with pytest.raises(stfem.StfemError) as e:
        V.update(None)  # the weight is needed again
    assert e.value.status == -1


def test_refusals(stfem):
    p = svr.problem(scr.CASES["pert412_jac_free"])
    op = _operator(stfem, p)
    lib = stfem.lib()
    lin = _device(op, p, p.lin)
    ptrs = (C.c_void_p * p.nb)(*[getattr(v, "ptr", v) for v in lin])
    holes = (C.c_void_p * p.nb)(*[None] * p.nb)
    bv = (C.c_int32 * p.nb)(*p.var)
    A, B = np.ascontiguousarray(p.Alpha), np.ascontiguousarray(p.Beta)
    dp = C.POINTER(C.c_double)

    def create(mode, lin_, delta0):
        h = C.c_void_p(1)  # must come back null
        rc = lib.stfem_stokes_vanka_create_linearised_cip(op._h, p.nb, bv, A.ctypes.data_as(dp), B.ctypes.data_as(dp), mode, lin_, delta0,
                                                          C.byref(h))
        assert not h.value
        return rc, lib.stfem_last_error().decode()

    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, why = create(2, ptrs, bad)
        assert rc == -1 and "delta0" in why  # STFEM_ERR_INVALID_ARGUMENT
    for mode in (0, 1, 2):
        rc, why = create(mode, None, 1.0)
        assert rc == -1 and "lin_blocks" in why
        rc, why = create(mode, holes, 1.0)
        assert rc == -1 and "lin_blocks[" in why
    with pytest.raises(stfem.StfemError) as e:
        stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=None, mode=0, delta0=1.0)
    assert e.value.status == -1


def test_relaxation_follows_the_reference_history(stfem, oracle_mod):
    """eight sweeps x <- x + omega V (f - A x), A the device operator with set_cip(1, CIP_WEIGHT_LINEARISATION) in jacobian mode on the
    perturbed 3 x 3 x 2 mesh, V the smoother with the term: the residual norms equal those of the restatement to 1e-8 relative"""
    p, _, f, want = scr.relaxation()
    op = _operator(stfem, p)
    op.set_cip(scr.DELTA0, stfem.CIP_WEIGHT_LINEARISATION)
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
    print("reference:", " ".join("%.6e" % v for v in want))
    assert np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)


if __name__ == "__main__":
    case_name, out_path = sys.argv[1], sys.argv[2]
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    prob = svr.problem(scr.CASES[case_name])
    oper = _operator(mod, prob)
    smoother, keep = _smoother(mod, oper, prob)
    y = np.concatenate(_apply(oper, prob, smoother, _x(prob)))
    np.save(out_path, np.concatenate([y, [float(smoother.setup_batches)]]))
