"""The solver-side C++ classes over an operator of velocity degree 3 (host/stfem/stokes_solver.h: StokesSpaces, StokesBlockVector,
StokesSystem, RelaxedVankaStokes, the zero-mean shift of StokesSlab; host/stfem/stokes.h: compute_divergence) through their caller
host/test_host_stokes_q3_relaxed, on the perturbed 2 x 2 x 2 mesh of relaxation() in tests/stokes_vanka_q3_reference.py (FE_DGP(2),
cG(1), viscosity 1): the residual history of sweeps x <- x + omega V (f - A x) with a GIVEN relaxation and one iteration equals the
restatement's to 1e-8 relative, the bar tests/test_gpu_stokes_vanka_q3.py holds for `step` - for the linear smoother and, after
set_data, for the smoother of the operator linearised about the states of tests/stokes_vanka_q3_linearised_reference.py.  With
relaxation 0 the estimated omega is finite, positive and the same in two constructions (no value is pinned: the reference holds none).
After the zero-mean shift weights . p / volume is <= 1e-13 max |p|; compute_divergence equals the restatement
(tests/stokes_pressure_q3_reference.py) and the Python veneer for the same vector to 1e-12.  The caller itself counts the degree the
spaces report, the given relaxation, the total without a cell vector, that the shift had something to do, and the refusals of
set_partition, of GMGStokes::vmult and of the slab's force quadrature."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import stokes_pressure_q3_reference as R
import stokes_vanka_q3_linearised_reference as lq3
import stokes_vanka_q3_reference as q3r

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")


def _write(path, blocks):
    with open(path, "wb") as f:
        f.write(np.uint64(len(blocks)).tobytes())
        for x in blocks:
            f.write(np.uint64(x.size).tobytes())
            f.write(x.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("treatment", ["linear", "linearised"])
def test_cpp_degree_3_relaxed_vanka_caller(treatment, tmp_path, oracle_mod):
    if treatment == "linear":
        p, ref, f, want = q3r.relaxation()
        mode, lin = 0, None
    else:
        p, mode, lin, ref, f, want = lq3.relaxation()
    assert p.variable_major and p.nb == 2 and p.pert and p.dg and p.ns == 1 and p.nt == 1 and p.mask == 63
    exe = os.path.join(HOST, "test_host_stokes_q3_relaxed")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_stokes_q3_relaxed"], stdout=subprocess.DEVNULL)
    # the vector whose divergence is taken: the linearisation state, or a random velocity in f's place (non-zero boundary entries)
    states = [np.zeros(n) if b is None else b for b, n in zip(lin, p.sizes)] if lin is not None else None
    fv, fl, ff, fc = tmp_path / "vertices.bin", tmp_path / "lin.bin", tmp_path / "f.bin", tmp_path / "cells.bin"
    np.ascontiguousarray(p.verts, dtype=np.float64).tofile(fv)
    _write(ff, f)
    _write(fl, states if states is not None else [np.zeros(n) for n in p.sizes])
    sweeps = q3r.RELAX_SWEEPS
    res = subprocess.run([exe, *map(str, p.nc), "1", repr(p.nu), repr(q3r.DT), str(mode), repr(q3r.RELAX_OMEGA), str(sweeps), str(fv), str(ff), str(fl),
                          str(fc)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(line.split(" ", 1) for line in res.stdout.strip().splitlines())
    assert lines["checks"] == "7", res.stdout
    norms = [float(v) for v in lines["history"].split()]
    print(treatment, "history:", " ".join("%.6e" % v for v in norms))
    assert len(norms) == sweeps and np.allclose(norms, want, rtol=1e-8, atol=0.0), (norms, want)
    assert all(b < a for a, b in zip(norms, norms[1:]))
    w1, w2 = (float(v) for v in lines["omega"].split())
    print(treatment, "estimated omega", w1)
    assert np.isfinite(w1) and w1 > 0.0 and w1 == w2
    mean, pmax = float(lines["mean"].split()[0]), float(lines["mean"].split()[2])
    print(treatment, "mean after the shift", mean, "max |p|", pmax)
    assert pmax > 1.0 and abs(mean) <= 1e-13 * pmax
    # compute_divergence: the restatement, and the Python veneer for the same vector
    u = (states if states is not None else f)[0]
    ref_cells, ref_total = R.divergence_cells(3, u, p.nc, p.verts)
    cells, total = np.fromfile(fc, dtype=np.float64), float(lines["divergence"])
    assert cells.shape == ref_cells.shape
    assert np.linalg.norm(cells - ref_cells) <= 1e-12 * np.linalg.norm(ref_cells) and abs(total - ref_total) <= 1e-12 * ref_total
    stfem = importlib.import_module("dealii-stfem_amd")
    op = stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=True)
    py_total, py_cells = op.divergence_space(op.initialize_dof_vector(0, u), cells=True)
    assert abs(total - py_total) <= 1e-12 * py_total and np.linalg.norm(cells - py_cells) <= 1e-12 * np.linalg.norm(py_cells)
