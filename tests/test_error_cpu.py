"""The library's one error record (csrc/stfem_error.cpp: stfem_set_error and the eight accessors) on the CPU: format and returned
status, truncation, a message built from the current text, one record behind every accessor, one record per thread.
csrc/test_error.cpp checks them and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_error_program():
    subprocess.check_call(["make", "-C", CSRC, "test_error"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_error")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
