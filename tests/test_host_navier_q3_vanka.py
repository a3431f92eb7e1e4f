"""The C++ mirror of the Stokes Vanka smoother of the linearised operator at velocity degree 3 (host/stfem/stokes.h: the second
constructor of PreconditionVankaStokes over a StokesMatrixFreeOperator<3, double> of degree 3 goes through
stfem_stokes_vanka_create_linearised_space) through its caller host/test_host_navier_q3_vanka, on the 2 x 2 x 2 box of case box222_q2_cg2
with the Implicit (jacobian) and the Explicit (form) treatment against tests/stokes_vanka_q3_linearised_reference.py at 1e-10 overall
and per block.  The caller itself counts that update reproduces a fresh construction bit for bit, the way back, and the refusal of
delta0 != 0."""
import os
import subprocess

import numpy as np
import pytest

import stokes_vanka_q3_linearised_reference as lq3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-10


def _write(path, blocks):
    with open(path, "wb") as f:
        f.write(np.uint64(len(blocks)).tobytes())
        for x in blocks:
            f.write(np.uint64(x.size).tobytes())
            f.write(x.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("treatment", ["implicit", "explicit"])
def test_cpp_degree_3_linearised_vanka_caller(treatment, tmp_path, oracle_mod):
    p, mode, lin, ref, base = lq3.case("box222_q2_cg2")
    assert p.variable_major and p.nb == 4 and not p.pert and not p.dg and mode == lq3.JACOBIAN
    if treatment == "explicit":
        mode, ref = lq3.FORM, lq3.reference(p, base, lq3.FORM, lin)
    exe = os.path.join(HOST, "test_host_navier_q3_vanka")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_navier_q3_vanka"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(3)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    fin, flin, fout = tmp_path / "in.bin", tmp_path / "lin.bin", tmp_path / "out.bin"
    _write(fin, X)
    _write(flin, [np.zeros(n) if b is None else b for b, n in zip(lin, p.sizes)])
    res = subprocess.run([exe, *map(str, p.nc), "0", repr(p.nu), repr(lq3.DT), str(mode), str(fin), str(flin), str(fout)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"blocks=4 cells={int(np.prod(p.nc))} checks=4" in res.stdout, res.stdout
    raw = np.fromfile(fout, dtype=np.float64)
    assert raw.size == sum(p.sizes)
    Y = np.split(raw, np.cumsum(p.sizes)[:-1])
    want = ref.vmult(X)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    overall, per_block = rel(raw, np.concatenate(want)), [rel(Y[b], want[b]) for b in range(p.nb)]
    print(treatment, "overall %.3e" % overall, "blocks", " ".join("%.2e" % e for e in per_block))
    assert overall < TOL and max(per_block) < TOL
