"""The C++ mirror at velocity degree 3 (host/stfem/stokes.h: StokesMatrixFreeOperator<3, double>(mesh, 3, ...) through
stfem_stokes_create_space, SystemMatrixStokes over it) through its caller host/test_host_stokes_q3, against the CPU oracle at pu = 3,
rel-L2 <= 1e-12 per block.  The caller counts the constructor's refusals (weak / outflow ids, delta0, a nonlinear treatment, degree
4) and the alias refusal itself."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [0, 1], ids=["FE_Q2", "FE_DGP2"])
def test_cpp_degree_3_caller(dg, tmp_path):
    """(3, 2, 2) cells, perturbed, cG(2) with one step: vmult, the reference's Tvmult and vmult_slice_add (Gamma, Zeta)"""
    from oracle import oracle
    nc, nu, mask = (3, 2, 2), 0.5, 0b111011
    stfem = importlib.import_module("dealii-stfem_amd")
    exe = os.path.join(HOST, "test_host_stokes_q3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_stokes_q3"], stdout=subprocess.DEVNULL)
    out = tmp_path / "q3.bin"
    res = subprocess.run([exe, *map(str, nc), str(dg), str(nu), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "exceptions=7" in res.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    nb = int(raw[:8].view(np.uint64)[0]); off = 8
    X, sizes = [], []
    for _ in range(nb):
        n = int(raw[off:off + 8].view(np.uint64)[0]); off += 8
        X.append(raw[off:off + 8 * n].view(np.float64).copy()); off += 8 * n
        sizes.append(n)

    def blocks():
        nonlocal off
        v = []
        for n in sizes:
            v.append(raw[off:off + 8 * n].view(np.float64).copy()); off += 8 * n
        return v

    orc = oracle.StokesOracle(nc, stfem.mesh_vertices(nc, distort=0.1, seed=99), mask, nu, pu=3, dg_pressure=bool(dg))
    ns, nt = 1, 2
    assert nb == 4 and sizes == [3 * orc.n_u] * 2 + [orc.n_p] * 2
    Alpha, Beta, Gamma, Zeta = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 32, ns)

    def close(got, want, what):
        for b in range(nb):
            assert np.linalg.norm(want[b]) > 0, (what, b)
            assert np.linalg.norm(got[b] - want[b]) <= TOL * np.linalg.norm(want[b]), (what, b)

    close(blocks(), orc.st_vmult(Alpha, Beta, ns, nt, X), "vmult")
    got, want = blocks(), orc.st_Tvmult(Alpha, Beta, ns, nt, X)
    for b in range(nb):
        assert np.linalg.norm(got[b] - want[b]) <= TOL * max(np.linalg.norm(want[b]), 1.0), ("Tvmult", b)
    iu, ip = stfem.stokes_block_index(nt, 0, 0, 1), stfem.stokes_block_index(nt, 0, 1, 1)
    ku, kp = orc.apply(X[iu], X[ip])
    mu, _ = orc.apply(X[iu], X[ip], 0.0, 1.0)
    g, z = Gamma.reshape(-1), Zeta.reshape(-1)
    assert g.size == nb
    want = [X[b] + (g[b] * ku.reshape(-1) + z[b] * mu.reshape(-1) if b < nt else g[b] * kp) for b in range(nb)]
    close(blocks(), want, "vmult_slice_add")
    assert off == raw.size
