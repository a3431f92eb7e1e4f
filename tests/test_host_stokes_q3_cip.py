"""The C++ mirror at velocity degree 3 with the CIP interior-face term (host/stfem/stokes.h: StokesMatrixFreeOperator<3, double>(mesh,
StokesSpace{3, ..., delta0}) through stfem_stokes_set_cip_space, set_cip_weight and cip_add over an operator made by descriptor) through
its caller host/test_host_stokes_q3_cip, against the CPU oracle at pu = 3 plus the numpy restatement of the term
(tests/cip_q3_reference.py), rel-L2 <= 1e-12 per block.  The caller counts the refusals itself: the first constructor with delta0 != 0
at degree 3 still throws, and so does PreconditionVankaStokes with delta0 != 0 over a degree-3 operator."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cip_q3_reference as c3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = c3.TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [0, 1], ids=["FE_Q2", "FE_DGP2"])
def test_cpp_degree_3_cip_caller(dg, tmp_path):
    """(3, 2, 2) cells, perturbed, x+ and y+ strong, delta0 = 2.5: vmult with the term (both weights: without a nonlinear treatment the
    same bits), without it, and cip_add with a weight velocity of its own"""
    from oracle import oracle
    nc, nu, mask, delta0 = (3, 2, 2), 0.5, 0b001010, 2.5
    stfem = importlib.import_module("dealii-stfem_amd")
    exe = os.path.join(HOST, "test_host_stokes_q3_cip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_stokes_q3_cip"], stdout=subprocess.DEVNULL)
    out = tmp_path / "q3_cip.bin"
    res = subprocess.run([exe, *map(str, nc), str(dg), str(nu), str(delta0), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "exceptions=2" in res.stdout and "weight=1" in res.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    off = 0
    X = []
    for _ in range(4):  # x = (u, p), then w = (velocity, pressure: unused)
        n = int(raw[off:off + 8].view(np.uint64)[0]); off += 8
        X.append(raw[off:off + 8 * n].view(np.float64).copy()); off += 8 * n

    def take(n):
        nonlocal off
        v = raw[off:off + 8 * n].view(np.float64).copy(); off += 8 * n
        return v

    verts = stfem.mesh_vertices(nc, distort=0.1, seed=99)
    orc = oracle.StokesOracle(nc, verts, mask, nu, pu=3, dg_pressure=bool(dg))
    assert [x.size for x in X] == [3 * orc.n_u, orc.n_p] * 2
    U, P, W = X[0], X[1], X[2]
    ku, kp = orc.apply(U, P)
    ku = ku.reshape(-1)
    own, other = delta0 * c3.cip(3, 1.0, U, U, nc, verts, mask), delta0 * c3.cip(3, 1.0, W, U, nc, verts, mask)
    assert np.linalg.norm(own) >= 0.1 * np.linalg.norm(ku)  # the term is no small part of what is compared
    with_u, with_p = take(U.size), take(P.size)
    again_u, again_p = take(U.size), take(P.size)
    none_u, none_p = take(U.size), take(P.size)
    added = take(U.size)
    assert off == raw.size
    for what, got, want in (("vmult u", with_u, ku + own), ("vmult p", with_p, kp), ("no cip u", none_u, ku), ("no cip p", none_p, kp),
                            ("cip_add", added, ku + other)):
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(what, "%.2e" % err)
        assert np.linalg.norm(want) > 0 and err <= TOL, what
    assert np.array_equal(again_u, with_u) and np.array_equal(again_p, with_p) and np.array_equal(with_p, none_p)
    assert np.linalg.norm((added - none_u) - other) <= TOL * (np.linalg.norm(ku) + np.linalg.norm(ku + other))
