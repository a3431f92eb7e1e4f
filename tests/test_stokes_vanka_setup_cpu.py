"""Index helpers of the one-block-per-cell Stokes smoother (csrc/stfem_vanka_setup.h: neighbour table of the cell's DoFs per variable,
row -> cell DoF, distinct linearisation states) on the CPU: csrc/test_stokes_vanka_setup.cpp checks them against the global numbering
and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_stokes_vanka_setup_program():
    subprocess.check_call(["make", "-C", CSRC, "test_stokes_vanka_setup"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_stokes_vanka_setup")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
