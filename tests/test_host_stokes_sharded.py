"""The partitioned Stokes / Navier-Stokes system of the C++ mirror (host/stfem/stokes_solver.h: StokesSpaces::set_partition, the comm
branches of StokesSystem::vmult / form, the reducing inner product and Gram-Schmidt step) through its caller
host/test_host_stokes_sharded, rebuilt from the CPU oracle with the self-loop rule of
tests/test_gpu_comm.py::test_cpp_caller_runs_partitioned: on the one-rank communicator with the rank itself as both neighbours every
interface partial returns to its sender (both interface planes of every velocity component and of the FE_Q(1) pressure double;
FE_DGP(1) pressure DoFs are cell-local and unchanged), and inner products count owned planes once (all but the top plane; every
FE_DGP(1) entry).  Vectors rel-L2 <= 1e-12, scalars 1e-12 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12
NC, UPPER, NU, MASK = (4, 3, 3), (1.0, 0.75, 1.25), 0.3, 63 & ~48


def _planes(x, v, dg):
    """a block as [component][z plane][plane] (None: FE_DGP(1) pressure)"""
    if v == 1 and dg:
        return None
    comps, step = (3, 2) if v == 0 else (1, 1)
    return x.reshape(comps, step * NC[2] + 1, -1)


def _doubled(x, v, dg):
    out = np.array(x, dtype=np.float64)
    p = _planes(out, v, dg)
    if p is not None:
        p[:, 0] *= 2
        p[:, -1] *= 2
    return out


def _dot(a, b, var, dg):
    """the partitioned inner product: owned entries only"""
    total = 0.0
    for x, y, v in zip(a, b, var):
        px, py = _planes(x, v, dg), _planes(y, v, dg)
        total += float(np.sum(x * y)) if px is None else float(np.sum(px[:, :-1] * py[:, :-1]))
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [False, True])
def test_cpp_stokes_caller_runs_partitioned(dg, tmp_path):
    orc_mod = ssc.oracle()
    exe = os.path.join(HOST, "test_host_stokes_sharded")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = tmp_path / "stokes_sharded.bin"
    res = subprocess.run([exe, *map(str, NC), str(int(dg)), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"ranks=1 blocks=4 carrier={int(dg)}" in res.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    nb = int(raw[:8].view(np.uint64)[0])
    sizes = [int(v) for v in raw[8:8 + 8 * nb].view(np.uint64)]
    off = 8 + 8 * nb
    n_u, n_p = ssc.sizes(NC, dg)
    var = [0, 0, 1, 1]  # BlockSlice(1, 2, 2), variable-major
    assert nb == 4 and sizes == [3 * n_u if v == 0 else n_p for v in var]

    def blocks():
        nonlocal off
        v = []
        for n in sizes:
            v.append(raw[off:off + 8 * n].view(np.float64).copy())
            off += 8 * n
        return v

    X, LIN, Y, F, GS = (blocks() for _ in range(5))
    xy, h0, h1, norm_after = raw[off:off + 32].view(np.float64)
    assert off + 32 == raw.size
    verts = nref.perturbed_vertices(NC, 0.0, 0, (0, 0, 0), UPPER)
    orc = orc_mod.StokesOracle(NC, verts, MASK, NU, dg_pressure=dg)
    A, B, _, _ = orc_mod.time_weights(orc_mod.CGP, 2, 1.0 / 32, 1)
    Alpha, Beta = np.zeros((4, 4)), np.zeros((4, 4))
    index = lambda it, v, d: ssc.block_index(2, it, v, d)  # noqa: E731
    for a in range(2):
        for b in range(2):
            Alpha[index(0, 0, a), index(0, 0, b)] = Alpha[index(0, 0, a), index(0, 1, b)] = Alpha[index(0, 1, a), index(0, 0, b)] = A[a, b]
            Beta[index(0, 0, a), index(0, 0, b)] = B[a, b]
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        for j, v in enumerate(var):
            assert np.linalg.norm(want[j]) > 0
            err = ssc.rel(got[j], want[j])
            worst = max(worst, err / TOL)
            assert err <= TOL, (what, j, err)

    # vmult: the jacobian about lin; form: the weak form about lin; then the add-exchange on the self-loop
    ref = {m: [_doubled(x, v, dg) for x, v in zip(nref.st_vmult(orc, m, Alpha, Beta, 1, 2, X, LIN, index, NC, verts, MASK), var)]
           for m in (nref.FORM, nref.JACOBIAN)}
    close(Y, ref[nref.JACOBIAN], "vmult")
    close(F, ref[nref.FORM], "form")
    assert ssc.rel(np.concatenate(Y), np.concatenate(F)) > 1e-3  # two different modes
    # the partitioned inner product
    want = _dot(X, ref[nref.JACOBIAN], var, dg)
    assert abs(want) > 1e-3 * np.sqrt(_dot(X, X, var, dg) * _dot(ref[nref.JACOBIAN], ref[nref.JACOBIAN], var, dg))  # (no cancellation)
    worst = max(worst, abs(xy - want) / abs(want) / TOL)
    assert abs(xy - want) <= TOL * abs(want)
    # the Gram-Schmidt step of partitioned vectors: the modified scheme with reducing inner products
    w = [y.copy() for y in ref[nref.JACOBIAN]]
    hs = []
    for basis in (X, LIN):
        hs.append(_dot(w, basis, var, dg))
        w = [wi - hs[-1] * bi for wi, bi in zip(w, basis)]
    close(GS, w, "gram-schmidt")
    for got, want in ((h0, hs[0]), (h1, hs[1]), (norm_after, np.sqrt(_dot(w, w, var, dg)))):
        worst = max(worst, abs(got - want) / abs(want) / TOL)
        assert abs(got - want) <= TOL * abs(want)
    print(f"ratio caller {worst:.3e}")
