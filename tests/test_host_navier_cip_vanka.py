"""The C++ mirror of the smoother of the linearised operator with the CIP term in its blocks (host/stfem/stokes.h: the delta0 argument of
PreconditionVankaStokes; host/stfem/stokes_solver.h: the trailing delta0 of RelaxedVankaStokes) through its caller
host/test_host_navier_cip_vanka, against the values the caller computes with the same linearisation through the C-ABI
(stfem_stokes_vanka_create_linearised_cip / _step): the same kernels on the same data, so the two agree bit for bit."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(0, 2, 1), (1, 1, 1)])
def test_cpp_navier_cip_vanka_caller(case):
    """(3, 2, 2) cells, perturbed, Implicit treatment, delta0 = 1: cG(2) (four blocks, two linearisation states) and dG(1).  Created about
    one vector, updated to a second, one step: equal to a C-ABI smoother created about the second with the same delta0; the update and
    the term changed the blocks; delta0 = 0 is the constructor without it; one sweep of RelaxedVankaStokes with the given damping is
    that step; two refusals."""
    ttype, r, ns = case
    exe = os.path.join(HOST, "test_host_navier_cip_vanka")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_navier_cip_vanka"], stdout=subprocess.DEVNULL)
    res = subprocess.run([exe, "3", "2", "2", str(ttype), str(r), str(ns), "0.5", "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = dict(re.findall(r"(\w+)=(\S+)", res.stdout))
    nt = r if ttype == 0 else r + 1
    assert int(out["blocks"]) == 2 * nt * ns and int(out["cells"]) == 12
    assert float(out["mirror_vs_capi"]) == 0.0
    assert int(out["update_changed"]) == 1 and int(out["term_changed"]) == 1
    assert float(out["zero_vs_plain"]) == 0.0
    assert float(out["relaxed_vs_step"]) == 0.0
    assert int(out["exceptions"]) == 2
