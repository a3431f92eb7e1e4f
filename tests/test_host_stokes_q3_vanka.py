"""The C++ mirror of the Stokes Vanka smoother at velocity degree 3 (host/stfem/stokes.h: PreconditionVankaStokes over a
StokesMatrixFreeOperator<3, double> of degree 3 goes through stfem_stokes_vanka_create_space) through its caller
host/test_host_stokes_q3_vanka, on case box222_q2_cg2 against tests/stokes_vanka_q3_reference.py at 1e-10 overall and per block.  The
caller itself counts the repeat (same bits), the accumulating step and the alias refusal."""
import os
import subprocess

import numpy as np
import pytest

import stokes_vanka_q3_reference as q3r

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-10


@pytest.mark.gpu
def test_cpp_degree_3_vanka_caller(tmp_path, oracle_mod):
    p, ref = q3r.case("box222_q2_cg2")
    assert p.variable_major and p.nb == 4 and not p.pert and not p.dg
    exe = os.path.join(HOST, "test_host_stokes_q3_vanka")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_stokes_q3_vanka"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(3)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.uint64(p.nb).tobytes())
        for x in X:
            f.write(np.uint64(x.size).tobytes())
            f.write(x.tobytes())
    res = subprocess.run([exe, *map(str, p.nc), "0", repr(p.nu), repr(q3r.DT), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"blocks=4 cells={int(np.prod(p.nc))} checks=3" in res.stdout, res.stdout
    raw = np.fromfile(fout, dtype=np.float64)
    assert raw.size == sum(p.sizes)
    Y = np.split(raw, np.cumsum(p.sizes)[:-1])
    want = ref.vmult(X)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    overall, per_block = rel(raw, np.concatenate(want)), [rel(Y[b], want[b]) for b in range(p.nb)]
    print("overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block))
    assert overall < TOL and max(per_block) < TOL
