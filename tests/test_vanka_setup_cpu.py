"""Host set-up steps of the cell-patch smoothers (csrc/stfem_vanka_setup.h: Gauss-Jordan inverse, block classes, cell lists, tile
plans, finish_block) on the CPU: csrc/test_vanka_setup.cpp checks them and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_vanka_setup_program():
    subprocess.check_call(["make", "-C", CSRC, "test_vanka_setup"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_vanka_setup")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
