"""The C++ mirror with the CIP interior-face term (host/stfem/stokes.h: the StokesMatrixFreeOperator constructor with delta0 = 1,
set_cip_weight, SystemMatrixStokes and NavierStokesOperator over it) through its caller host/test_host_cip, against the linear oracle
plus the numpy restatements of the convection term and of the CIP term (tests/navier_reference.py, tests/cip_reference.py), rel-L2 <=
1e-12."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import navier_reference as nref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(0, 2, 1), (1, 2, 2)])
def test_cpp_cip_caller(case, tmp_path):
    """(3, 2, 4) cells, perturbed, delta0 = 1: cG(2) with one step (the fused launch set), dG(2) with two steps (one set per source).
    residual = rhs - form(x) and vmult = form (Explicit) / jacobian (Implicit) with the source weight of the constructor and with the
    linearisation weight, every time dof with its own linearisation velocity; the refusals (a weight outside 0..1, outflow_penalty
    with a nonlinear treatment, a non-finite delta0) are counted by the caller itself."""
    from oracle import oracle
    nc, nu, delta0 = (3, 2, 4), 0.5, 1.0
    ttype, r, ns = case
    stfem = importlib.import_module("dealii-stfem_amd")
    exe = os.path.join(HOST, "test_host_cip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = tmp_path / "cip.bin"
    res = subprocess.run([exe, *map(str, nc), str(ttype), str(r), str(ns), str(nu), str(delta0), str(out)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "exceptions=5" in res.stdout
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

    lin, rhs = blocks(), blocks()
    mask = 63
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=99)
    orc = oracle.StokesOracle(nc, verts, mask, nu)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(ttype, r, 1.0 / 32, ns)
    nt = r if ttype == 0 else r + 1
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d)  # noqa: E731
    ref = {(m, w): cref.st_vmult(orc, delta0, w, m, Alpha, Beta, ns, nt, X, lin, index, nc, verts, mask)
           for m in (nref.FORM, nref.JACOBIAN) for w in (cref.SOURCE, cref.LINEARISATION)}
    plain = {m: nref.st_vmult(orc, m, Alpha, Beta, ns, nt, X, lin, index, nc, verts, mask) for m in (nref.FORM, nref.JACOBIAN)}

    def close(got, exp, what):
        for b in range(nb):
            assert np.linalg.norm(exp[b]) > 0
            err = np.linalg.norm(got[b] - exp[b]) / np.linalg.norm(exp[b])
            assert np.linalg.norm(got[b] - exp[b]) <= TOL * np.linalg.norm(exp[b]) + 1e-14, (what, b, err)

    iu = index(0, 0, 0)
    for m in plain:  # the term is a visible part of what is compared, and the two weights give two results
        for w in (cref.SOURCE, cref.LINEARISATION):
            assert np.linalg.norm(ref[m, w][iu] - plain[m][iu]) > 1e-2 * np.linalg.norm(plain[m][iu])
        assert np.linalg.norm(ref[m, 0][iu] - ref[m, 1][iu]) > 1e-3 * np.linalg.norm(ref[m, 0][iu])
    for treatment, vmult_mode in (("Explicit", nref.FORM), ("Implicit", nref.JACOBIAN)):
        for w in (cref.SOURCE, cref.LINEARISATION):
            close(blocks(), [rhs[b] - ref[nref.FORM, w][b] for b in range(nb)], f"{treatment} residual, weight {w}")
            close(blocks(), ref[vmult_mode, w], f"{treatment} vmult, weight {w}")
    # the spatial operator alone, linearised about time dof (0, 0), linearisation weight
    ip = index(0, 1, 0)
    for mode in (nref.FORM, nref.JACOBIAN):
        ku, kp = cref.vmult(orc, delta0, cref.LINEARISATION, mode, lin[iu], X[iu], X[ip], nc, verts, mask)
        gu = raw[off:off + 8 * sizes[iu]].view(np.float64); off += 8 * sizes[iu]
        gp = raw[off:off + 8 * sizes[ip]].view(np.float64); off += 8 * sizes[ip]
        assert np.linalg.norm(gu - ku) <= TOL * np.linalg.norm(ku)
        assert np.linalg.norm(gp - kp) <= TOL * np.linalg.norm(kp) + 1e-14
    assert off == raw.size
