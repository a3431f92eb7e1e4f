"""The C++ mirror of the Navier-Stokes side (host/stfem/stokes.h: NonlinearTreatment, StokesMatrixFreeOperator::set_data / form /
vmult, SystemMatrixStokes with a linearisation vector, NavierStokesOperator) through its caller host/test_host_navier, against the
linear oracle plus the numpy restatement of the convection term (tests/navier_reference.py), rel-L2 <= 1e-12."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(0, 2, 1, 0), (1, 2, 2, 0), (0, 2, 1, 0b100011)])
def test_cpp_navier_caller(case, tmp_path):
    """(3, 2, 4) cells, perturbed: cG(2) with one step (the fused path), dG(2) with two steps (six time dofs: one set of launches per
    source), cG(2) with weak boundary ids 0, 1, 5.  residual = rhs - form(x) with both treatments, vmult = form (Explicit) / jacobian
    (Implicit), every time dof with its own linearisation velocity; the refusals are counted by the caller itself."""
    from oracle import oracle
    nc, nu = (3, 2, 4), 0.5
    ttype, r, ns, weak = case
    stfem = importlib.import_module("dealii-stfem_amd")
    exe = os.path.join(HOST, "test_host_navier")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = tmp_path / "navier.bin"
    res = subprocess.run([exe, *map(str, nc), str(ttype), str(r), str(ns), str(nu), str(out)] + ([str(weak)] if weak else []),
                         capture_output=True, text=True, timeout=300)
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
    mask = 63 & ~weak
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=99)
    orc = oracle.StokesOracle(nc, verts, mask, nu, weak_mask=weak)
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(ttype, r, 1.0 / 32, ns)
    nt = r if ttype == 0 else r + 1
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d)  # noqa: E731
    ref = {m: nref.st_vmult(orc, m, Alpha, Beta, ns, nt, X, lin, index, nc, verts, mask, weak) for m in (nref.FORM, nref.JACOBIAN)}

    def close(got, exp, what):
        for b in range(nb):
            assert np.linalg.norm(exp[b]) > 0
            assert np.linalg.norm(got[b] - exp[b]) <= TOL * np.linalg.norm(exp[b]) + 1e-14, (what, b)

    for treatment, vmult_mode in (("Explicit", nref.FORM), ("Implicit", nref.JACOBIAN)):
        close(blocks(), [rhs[b] - ref[nref.FORM][b] for b in range(nb)], treatment + " residual")
        close(blocks(), ref[vmult_mode], treatment + " vmult")
    # the spatial operator alone, linearised about time dof (0, 0)
    iu, ip = index(0, 0, 0), index(0, 1, 0)
    for mode in (nref.FORM, nref.JACOBIAN):
        ku, kp = nref.vmult(orc, mode, lin[iu], X[iu], X[ip], nc, verts, mask, weak)
        gu = raw[off:off + 8 * sizes[iu]].view(np.float64); off += 8 * sizes[iu]
        gp = raw[off:off + 8 * sizes[ip]].view(np.float64); off += 8 * sizes[ip]
        assert np.linalg.norm(gu - ku) <= TOL * np.linalg.norm(ku)
        assert np.linalg.norm(gp - kp) <= TOL * np.linalg.norm(kp) + 1e-14
    assert off == raw.size
