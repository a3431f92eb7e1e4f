"""The C++ mirror's StokesMatrixFreeOperator::compute_drag_lift (host/stfem/stokes.h) through its caller host/test_host_drag_lift:
Poiseuille flow on [0, Lx] x [0, 1] x [0, Lz] with the walls y = 0, 1 strongly constrained, against the closed forms of the six faces
within 1e-12 A (A from the numpy restatement tests/drag_lift_reference.py), the scale argument, and the several-pairs form: five
pairs k (u, p) of one call, compared bit for bit with the single calls by the caller itself and with k times the closed form here."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drag_lift_reference as dref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [0, 1])
def test_cpp_drag_lift_caller(dg):
    nc, L, nu, c0 = (3, 2, 2), (2.0, 1.0, 1.5), 0.7, 1.3
    exe = os.path.join(HOST, "test_host_drag_lift")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    res = subprocess.run([exe, *map(str, nc), str(dg), str(L[0]), str(L[2]), str(nu), str(c0)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pairs_equal=1" in res.stdout and "exceptions=3" in res.stdout
    got = {}
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] in ("face", "pair"):
            got[w[0], int(w[1])] = np.array([float(v) for v in w[2:5]])
        elif w[0] in ("all", "scaled"):
            got[w[0]] = np.array([float(v) for v in w[1:4]])
    u, p, verts = dref.poiseuille(nc, L, nu, c0, bool(dg))
    want = {f: np.array(v, dtype=float) for f, v in dref.poiseuille_forces(L, nu, c0).items()}
    for f in range(6):
        _, _, A = dref.drag_lift(u, p, nc, verts, nu, 1 << f, plain=True, dg_pressure=bool(dg))
        assert np.max(np.abs(got["face", f] - want[f])) <= TOL * A, (f, got["face", f], want[f])
    _, _, A3 = dref.drag_lift(u, p, nc, verts, nu, 8, plain=True, dg_pressure=bool(dg))
    assert np.max(np.abs(got["scaled"] + 2.5 * want[3])) <= TOL * 2.5 * A3
    _, _, A = dref.drag_lift(u, p, nc, verts, nu, 63, plain=True, dg_pressure=bool(dg))
    assert np.max(np.abs(got["all"])) <= TOL * A
    _, _, A23 = dref.drag_lift(u, p, nc, verts, nu, 12, plain=True, dg_pressure=bool(dg))
    for k in range(1, 6):
        assert np.max(np.abs(got["pair", k] - k * (want[2] + want[3]))) <= TOL * k * A23, k
