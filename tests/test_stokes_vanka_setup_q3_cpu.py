"""Index helpers of the one-block-per-cell Stokes smoother at velocity degree 3 (csrc/stfem_vanka_setup.h: neighbour and face tables of
the cell's 192 + 27 / 10 DoFs, row -> cell DoF, the apply's row table) on the CPU: csrc/test_stokes_vanka_setup_q3.cpp checks them
against a brute-force enumeration of the global numbering and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_stokes_vanka_setup_q3_program():
    subprocess.check_call(["make", "-C", CSRC, "test_stokes_vanka_setup_q3"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_stokes_vanka_setup_q3")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
