"""Guard-band tests of the entries of include/stfem_stokes_pressure_space.h that read or write a caller's device array, at velocity
degree 3: stfem_stokes_divergence_space, stfem_stokes_pressure_difference_space, stfem_stokes_dgp_prolongate_space and
stfem_stokes_dgp_restrict_space on packed caller-owned views.

The scheme is that of tests/test_gpu_guard_bands_stokes_q3_convection.py: each call runs on arrays in allocations of their own (`plain`)
and on views of one guarded arena (tests/guard_arena.py); plain agrees with the numpy restatement
(tests/stokes_pressure_q3_reference.py) within the parity bound, the arena result - returned host values included - equals plain bit
for bit, and every guard and source byte of the arena is unchanged."""
import importlib

import numpy as np
import pytest

import stokes_pressure_q3_reference as R
from guard_arena import Spec, guard_case, poison

pytestmark = pytest.mark.gpu

PLACEMENTS = ["aligned", "packed"]
TOL = 1e-12
LOWER, UPPER = (0.0, 0.0, 0.0), (1.0, 0.7, 1.3)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()  # raises if the HIP library is missing: no fallback
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)


def pvec(name, data, nc, dg, role="source"):
    return Spec(name, data, role, None if dg else tuple(2 * c + 1 for c in nc))


def within(ref, scale=None):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    scale = np.linalg.norm(ref) if scale is None else scale

    def check(got):
        err = np.linalg.norm(got - ref)
        print(f"|got - ref| = {err:.3e}, bound {TOL:.1e} x {scale:.3e}")
        assert scale > 0 and err <= TOL * scale, (err, TOL * scale)
    return check


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mesh", ["box", "pert"])
def test_divergence_space(mesh, placement, stfem):
    """stfem_stokes_divergence_space with the per-cell output an arena view of n_cells doubles"""
    nc, distort, (lower, upper) = {"box": ((2, 3, 2), 0.0, ((0.0, -0.5, 0.25), (1.0, 0.25, 1.75))), "pert": ((3, 2, 2), 0.15, ((0, 0, 0), (1, 1, 1)))}[mesh]
    verts = stfem.mesh_vertices(nc, lower=lower, upper=upper, distort=distort, seed=77)
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=verts if distort else None, lower=lower, upper=upper, dirichlet_mask=0b011101)
    u = np.random.default_rng(11).uniform(-1, 1, 3 * op.n_velocity)
    ref_cells, ref_total = R.divergence_cells(3, u, nc, verts)

    def returned(total):
        assert abs(total - ref_total) <= TOL * ref_total

    guard_case(stfem, placement, [Spec("u", u, "source", tuple(3 * c + 1 for c in nc)), Spec("cells", poison(op.n_cells, np.float64), "destination", nc)],
               lambda ptr: op.divergence_space(ptr["u"], cells=ptr["cells"]), {"cells": within(ref_cells)}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dg", [False, True], ids=["FE_Q2", "FE_DGP2"])
def test_pressure_difference_space(dg, placement, stfem):
    nc, nq = (3, 2, 2), 3
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, lower=LOWER, upper=UPPER, dg_pressure=dg)
    rng = np.random.default_rng(4)
    coeffs, exact = rng.uniform(-1, 1, op.n_pressure), rng.uniform(-1, 1, (op.n_cells, nq ** 3))
    ref = R.pressure_difference(2, nc, LOWER, UPPER, nq, coeffs, exact, dg)

    def returned(got):
        assert abs(got[0] - ref[0]) <= 1e-12 * ref[0] and abs(got[1] - ref[1]) <= 1e-13 * ref[1], (got, ref)

    guard_case(stfem, placement, [pvec("p", coeffs, nc, dg)], lambda ptr: op.pressure_difference(nq, ptr["p"], exact), {}, returned=returned)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("add", [False, True], ids=["set", "add"])
def test_dgp_transfers_space(add, placement, stfem):
    """stfem_stokes_dgp_prolongate_space / _restrict_space between 3 x 1 x 2 and 6 x 2 x 4 cells, FE_DGP(2)"""
    nf, ncoarse = (6, 2, 4), (3, 1, 2)
    fine = stfem.StokesMatrixFreeOperator.with_degree(3, nf, dg_pressure=True)
    coarse = stfem.StokesMatrixFreeOperator.with_degree(3, ncoarse, dg_pressure=True)
    rng = np.random.default_rng(6)
    c, f = rng.uniform(-1, 1, coarse.n_pressure), rng.uniform(-1, 1, fine.n_pressure)
    yf, yc = rng.uniform(-1, 1, fine.n_pressure), rng.uniform(-1, 1, coarse.n_pressure)
    Pm = R.dgp_embedding(2, nf)
    Pc, Rf = Pm @ c, Pm.T @ f
    guard_case(stfem, placement, [pvec("c", c, ncoarse, True), pvec("f", yf if add else poison(f.size, np.float64), nf, True, "destination")],
               lambda ptr: stfem.stokes_dgp_prolongate(fine, coarse, ptr["f"], ptr["c"], add=add), {"f": within(yf + Pc if add else Pc, scale=np.linalg.norm(Pc))})
    guard_case(stfem, placement, [pvec("f", f, nf, True), pvec("c", yc if add else poison(c.size, np.float64), ncoarse, True, "destination")],
               lambda ptr: stfem.stokes_dgp_restrict(fine, coarse, ptr["c"], ptr["f"], add=add), {"c": within(yc + Rf if add else Rf, scale=np.linalg.norm(Rf))})
