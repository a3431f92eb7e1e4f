"""The Navier-Stokes slab driver (host/navier_convergence.cpp: TimeIntegratorNavierStokes - Newton / Picard around FGMRES, preconditioned by
the per-cell Vanka smoother of the linearised operator or by a V-cycle of the linearised GMGStokes levels) against the dense restatement
tests/navier_slab_reference.py::navier_convergence_row_3d.  The discrete solution does not depend on the iteration and both sides iterate
to a relative residual of 1e-12, so the bar on the four error columns is the Stokes driver's own (tests/test_gpu_stokes_driver.py):
rtol 1e-6, atol 1e-9; |div u_h| at the end time is compared with the same bar.  The step counts stay below the driver's cap (40) and
every slab reports convergence, so a run that stalls fails."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_slab_reference as nsr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
CAP = 40  # max_nonlinear of the driver


def _exe(name):
    exe = os.path.join(HOST, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    return exe


@functools.lru_cache(maxsize=None)
def _reference(ttype, k, refinement, nu, dg):
    from oracle import oracle
    oracle.build()
    oracle.lib().stfo_set_threads(min(8, len(os.sched_getaffinity(0))))
    return nsr.navier_convergence_row_3d(ttype, k, refinement, nu=nu, dg_pressure=dg)


@functools.lru_cache(maxsize=None)
def _run(ttype, k, refinement, treatment, mg, dg, nu):
    args = [_exe("navier_convergence"), str(ttype), str(k), str(refinement), f"treatment={treatment}", f"nu={nu}"]
    if mg:
        args.append(f"mg={mg}")
    if dg:
        args.append("dg=1")
    res = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stderr)
    return [float(v) for v in res.stdout.split()]


# (time type, degree, refinement, treatment, multigrid levels, FE_DGP(1) pressure, viscosity)
CASES = [
    (0, 1, 1, "newton", 0, False, 1.0),
    (1, 1, 1, "picard", 0, False, 1.0),
    (0, 1, 2, "newton", 2, False, 1.0),
    (0, 2, 1, "newton", 0, False, 0.1),
    (0, 1, 2, "newton", 2, True, 1.0),
]


@pytest.mark.parametrize("ttype,k,refinement,treatment,mg,dg,nu", CASES)
def test_driver_row_vs_restatement(ttype, k, refinement, treatment, mg, dg, nu):
    row = _run(ttype, k, refinement, treatment, mg, dg, nu)
    want = _reference(ttype, k, refinement, nu, dg)
    n = 2 ** refinement
    nt = k if ttype == 0 else k + 1
    assert len(row) == 17
    assert row[:4] == [n ** 3, 3 * (2 * n + 1) ** 3, 4 * n ** 3 if dg else (n + 1) ** 3, nt]
    print("driver", row[4:8], row[11], "restatement", want)
    assert np.allclose(row[4:8], want[:4], rtol=1e-6, atol=1e-9), (row[4:8], want[:4])
    assert np.isclose(row[11], want[4], rtol=1e-6, atol=1e-9), (row[11], want[4])
    assert row[16] == 1 and 1 <= row[15] < CAP, row               # every slab converged, below the cap
    assert row[9] >= 1.0 and row[10] >= row[9]                    # at least one linear solve per slab, one iteration per solve
    assert abs(row[12] + row[13] + row[14] - 1.0) < 2e-4          # the three wall-time shares


@pytest.mark.parametrize("ttype", [0, 1])
def test_newton_takes_no_more_steps_than_picard(ttype):
    newton = _run(ttype, 1, 1, "newton", 0, False, 1.0)
    picard = _run(ttype, 1, 1, "picard", 0, False, 1.0)
    assert np.allclose(newton[4:8], picard[4:8], rtol=1e-6, atol=1e-9)  # the same discrete solution
    assert newton[9] <= picard[9], (newton[9], picard[9])
    assert max(newton[15], picard[15]) < CAP and newton[16] == picard[16] == 1


def test_bad_argument_is_refused():
    res = subprocess.run([_exe("navier_convergence"), "0", "1", "1", "treatment=quasi"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2
