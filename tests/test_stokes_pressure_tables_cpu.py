"""The host-side 1D tables of the degree-2 pressure spaces (csrc/host_tables.cpp: the orthonormal Legendre functions, the FE_Q(2)
Lagrange functions, and the tables of the FE_DGP(2) embedding into the two halves of a cell that the transfer kernel takes by value) on
the CPU: csrc/test_stokes_pressure_tables.cpp checks them against quadrature with the library's own Gauss rule and exits with status 0."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-stfem_amd", "csrc")


def test_stokes_pressure_tables_program():
    subprocess.check_call(["make", "-C", CSRC, "test_stokes_pressure_tables"], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CSRC, "test_stokes_pressure_tables")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
