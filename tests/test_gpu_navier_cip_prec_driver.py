"""The Navier-Stokes slab driver (host/navier_convergence.cpp) with the CIP term in the preconditioner, cipprec=1: the run's delta0 goes
to the blocks of the per-cell Vanka smoother (RelaxedVankaStokes) or, with mg=, to every multigrid level (GMGStokes: level operators and
level smoothers).  Every slab still reaches the nonlinear tolerance below the step limit, and the errors are those of the run with
cipprec=0: both stop at a relative nonlinear residual of 1e-12 on the same discrete problem - the preconditioner changes the path, not
the solution; tests/test_gpu_navier_cip_driver.py and tests/test_gpu_navier_driver.py observe at least 11 common digits between runs at
that tolerance, 1e-8 leaves three orders over that.  cipprec=1 with delta0=0 is the run without either argument.  Nonlinear steps and
FGMRES iterations per slab with and without cipprec are printed, not asserted (profiles/stokes_cip.txt records them)."""
import functools
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
CAP = 40  # max_nonlinear of the driver
SHARES = (12, 13, 14)  # the wall-time shares of the row: measured, different in every run

# positional arguments and the named ones but delta0 / cipprec: 2^3 cells with the relaxed smoother, 4^3 cells with two levels
RUNS = {
    "newton": ("0", "1", "1", "treatment=newton"),
    "picard": ("0", "1", "1", "treatment=picard"),
    "newton_mg2": ("0", "1", "2", "treatment=newton", "mg=2"),
}


def _exe(name):
    exe = os.path.join(HOST, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    return exe


@functools.lru_cache(maxsize=None)
def _run(*args):
    res = subprocess.run([_exe("navier_convergence"), *args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout, res.stderr


@pytest.mark.parametrize("name", list(RUNS))
def test_converges_to_the_errors_of_the_run_without_cipprec(name):
    out, log = _run(*RUNS[name], "delta0=1", "cipprec=1")
    base, _ = _run(*RUNS[name], "delta0=1", "cipprec=0")
    row, row0 = [float(v) for v in out.split()], [float(v) for v in base.split()]
    print(log)
    print(f"{name}: nonlinear steps per slab {row[9]:.2f} (cipprec=0: {row0[9]:.2f}), FGMRES iterations per slab {row[10]:.2f} "
          f"(cipprec=0: {row0[10]:.2f}), most steps in a slab {int(row[15])} (cipprec=0: {int(row0[15])})")
    assert len(row) == len(row0) == 17
    assert row[16] == 1 and 1 <= row[15] < CAP, row  # every slab reached nltol below the step limit
    for a, b in zip(row[4:8], row0[4:8]):
        assert abs(a - b) <= 1e-8 * abs(b), (row[4:8], row0[4:8])


def test_cipprec_without_delta0_prints_the_row_of_today():
    """character for character, but for the three wall-time shares, which no two runs print alike"""
    for name in ("newton", "picard"):
        without, _ = _run(*RUNS[name])
        with_prec, _ = _run(*RUNS[name], "cipprec=1", "delta0=0")
        a, b = without.split(), with_prec.split()
        assert len(a) == len(b) == 17
        assert [t for i, t in enumerate(a) if i not in SHARES] == [t for i, t in enumerate(b) if i not in SHARES], (without, with_prec)
        assert without.endswith("\n") and with_prec.endswith("\n") and without.count("\n") == with_prec.count("\n") == 1
