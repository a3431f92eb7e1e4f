"""Per-cell Vanka smoother of the Stokes system at velocity degree 3 over an operator WITH weak (Nitsche) faces
(stfem_stokes_vanka_create_space after stfem_stokes_set_weak_boundaries_space): the face phases of the cell matrices at the 4 x 4 Gauss
points of a face, against the dense numpy restatement tests/stokes_q3_faces_reference.py.  fp64, rel-L2 per block and overall.

Tolerance: the 1e-10 of tests/test_gpu_stokes_vanka_q3.py; tests/test_stokes_q3_faces_reference_cpu.py holds every case here under the
same conditioning cap (the largest: 2.75e5)."""
import importlib

import numpy as np
import pytest

import stokes_q3_faces_reference as fr

pytestmark = pytest.mark.gpu
TOL = 1e-10


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
    monkeypatch.delenv("STFEM_STOKES_FACE_WORKGROUPS", raising=False)


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) for v, x in zip(p.var, host)]


@pytest.mark.parametrize("name", list(fr.VANKA_CASES))
def test_blocks_with_faces_vs_reference(name, stfem, oracle_mod):
    p, ref = fr.case(name)
    op = fr.vanka_operator(stfem, p)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    assert V.n_classes == int(np.prod(p.nc))  # one block per cell
    rng = np.random.default_rng(3)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, 9.0) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    Y = [d.download() for d in dst]
    want = ref.vmult(X)
    overall = rel(np.concatenate(Y), np.concatenate(want))
    per_block = [rel(Y[b], want[b]) for b in range(p.nb)]
    print(name, "rows", p.rows, "overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block))
    assert overall < TOL
    assert max(per_block) < TOL, per_block
    V.update(None)  # rebuilds the same blocks
    V.vmult(dst, src)
    assert all(np.array_equal(d.download(), y) for d, y in zip(dst, Y))


def test_relaxation_with_faces_follows_the_reference_history(stfem, oracle_mod):
    """eight sweeps x <- x + omega V (f - A x) of the operator with weak faces on the perturbed 2 x 2 x 2 mesh, FE_DGP(2), cG(1),
    nu = 1: the residual norms of the device operator and smoother equal those of the restatement to 1e-8 relative, and decrease
    (CPU: 15.9 -> 0.726 at omega 0.5)"""
    p, ref, f, want = fr.relaxation()
    op = fr.vanka_operator(stfem, p)
    V = stfem.StokesPreconditionVanka.for_space(op, p.var, p.Alpha, p.Beta)
    zeros = [np.zeros(n) for n in p.sizes]
    x, r = _device(op, p, zeros), _device(op, p, zeros)
    norms = []
    for _ in range(fr.RELAX_SWEEPS):
        op.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, r, x, variable_major=p.variable_major)
        res = [f[i] - r[i].download() for i in range(p.nb)]
        norms.append(np.sqrt(sum(np.sum(q * q) for q in res)))
        for i in range(p.nb):
            r[i].upload(res[i])
        V.step(x, fr.RELAX_OMEGA, True, r)
    print("history:", " ".join("%.6e" % v for v in norms))
    assert np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)
    assert all(b < a for a, b in zip(norms, norms[1:]))
