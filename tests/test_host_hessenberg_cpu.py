"""HessenbergLeastSquares (host/stfem/hessenberg.h), the dense part shared by SolverFGMRES and GMG::coarse_gmres: the Givens
update column by column and the back-substitution, against numpy.linalg.lstsq on the same matrix.  Plain host code: no device."""
import os
import subprocess

import numpy as np

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "host")


def test_hessenberg_least_squares_vs_lstsq():
    subprocess.check_call(["make", "-C", HOST, "test_host_hessenberg"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(HOST, "test_host_hessenberg")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = [line.split() for line in res.stdout.splitlines()]
    beta = float(next(r[1] for r in rows if r[0] == "beta"))
    H = np.array([[float(v) for v in r[1:]] for r in rows if r[0] == "H"])
    residuals = np.array([float(r[1]) for r in rows if r[0] == "residual"])
    y = np.array([float(v) for v in next(r[1:] for r in rows if r[0] == "y")])
    assert H.shape == (5, 4) and np.all(np.tril(H, -2) == 0) and np.all(np.diag(H, -1) != 0)  # upper Hessenberg, unreduced
    # the bar below is cond * eps (1e3 * 2.2e-16) with a factor of about 10 in hand
    assert np.linalg.cond(H) < 1e3
    b = np.zeros(5)
    b[0] = beta
    want_residuals = []
    for j in range(1, 5):  # the leading (j + 1) x j problems: what the solver controls after each Arnoldi step
        yj = np.linalg.lstsq(H[:j + 1, :j], b[:j + 1], rcond=None)[0]
        want_residuals.append(np.linalg.norm(b[:j + 1] - H[:j + 1, :j] @ yj))
    print("residuals", residuals, "lstsq", want_residuals, "y", y, "lstsq", yj)
    assert residuals.shape == (4,) and np.allclose(residuals, want_residuals, rtol=1e-12, atol=0.0)
    assert y.shape == (4,) and np.allclose(y, yj, rtol=1e-12, atol=0.0)
