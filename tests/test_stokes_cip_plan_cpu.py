"""The grid of a CIP colour launch and what stfem_stokes_last_cip_plan reports of it (csrc/stfem_stokes_cip_plan.h: workgroups under
the device limit and the cap of STFEM_STOKES_CIP_WORKGROUPS, passes of the grid-stride loop, the cells of a colour) on the CPU:
csrc/test_stokes_cip_plan.cpp checks them with exact comparisons and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_stokes_cip_plan_program():
    subprocess.check_call(["make", "-C", CSRC, "test_stokes_cip_plan"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_stokes_cip_plan")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
