"""GPU parity of stfem_stokes_divergence (StokesMatrixFreeOperator::compute_divergence, reference include/operators.h:1391-1439)
against the numpy restatement tests/navier_slab_reference.py::divergence_cells from the full 3D tables of tests/navier_reference.py: per cell sum_q (div u_h)^2 JxW at the 3 x 3 x 3 Gauss
points with the MappingQ1 Jacobian from the eight vertices, the total sqrt(sum of the cells).  Tolerance rel 1e-12, the project's
fp64 parity tolerance.  Meshes: a lone cell (seven idle half-waves), an anisotropic 2 x 3 x 2 box (no vertices handed in: the
library's own lattice) and a 3 x 2 x 2 mesh perturbed by 0.15 (12 cells: two workgroups, the second half empty)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402
import navier_slab_reference as nsr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
BOX = ((0.0, -0.5, 0.25), (1.0, 0.25, 1.75))  # hx = 1/2, hy = 1/4, hz = 3/4
MESHES = {"cell": ((1, 1, 1), 0.0, ((0, 0, 0), (1, 1, 1))), "box": ((2, 3, 2), 0.0, BOX), "pert": ((3, 2, 2), 0.15, ((0, 0, 0), (1, 1, 1)))}
MASKS = [63, 0b011101]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _setup(stfem, mesh, mask):
    nc, distort, (lo, up) = MESHES[mesh]
    verts = stfem.mesh_vertices(nc, lower=lo, upper=up, distort=distort, seed=77)
    op = stfem.StokesMatrixFreeOperator(nc, vertices=verts if distort else None, lower=lo, upper=up, dirichlet_mask=mask)
    return op, nc, verts


def reference(u, ncell, vertices):
    return nsr.divergence_cells(u, ncell, vertices)


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_random_field_plain_read(mesh, mask, stfem):
    op, nc, verts = _setup(stfem, mesh, mask)
    u = np.random.default_rng(11).uniform(-1, 1, 3 * op.n_velocity)
    con = np.tile(nref.constrained(nc, mask), 3)
    assert np.all(u[con] != 0.0)
    du = op.initialize_dof_vector(0, u)
    total, cells = op.divergence(du, cells=True)
    ref_cells, ref_total = reference(u, nc, verts)
    print(f"{mesh} mask {mask}: cells rel {rel(cells, ref_cells):.3e}, total rel {abs(total - ref_total) / ref_total:.3e}")
    assert cells.shape == ref_cells.shape
    assert rel(cells, ref_cells) <= TOL
    assert np.max(np.abs(cells - ref_cells) / ref_cells) <= TOL  # every cell by itself: a sum of 27 non-negative terms
    assert abs(total - ref_total) <= TOL * ref_total
    # the total alone (no cell array) is the same number
    assert op.divergence(du) == total
    # the check tells a plain read from read_dof_values: with the constrained entries read as zero the answer is another one
    _, zeroed = reference(np.where(con, 0.0, u), nc, verts)
    assert abs(zeroed - ref_total) > 1e-3 * ref_total


def test_divergence_free_field(stfem):
    """(x^2, -2 x y, 0) lies in FE_Q(2)^3 and has no divergence: the total is rounding, <= 1e-13 of ||u||"""
    op, nc, verts = _setup(stfem, "box", 63)
    lo, up = BOX
    ax = [np.linspace(lo[d], up[d], 2 * nc[d] + 1) for d in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    u = np.concatenate([(x * x).ravel(), (-2 * x * y).ravel(), np.zeros(x.size)])
    total, cells = op.divergence(op.initialize_dof_vector(0, u), cells=True)
    print(f"divergence-free field: total {total:.3e}, ||u|| {np.linalg.norm(u):.3e}")
    assert np.all(cells >= 0.0)
    assert total <= 1e-13 * np.linalg.norm(u)
    # and a field with a known divergence: (x, y, z) has div = 3, the total is 3 sqrt(volume)
    u = np.concatenate([x.ravel(), y.ravel(), z.ravel()])
    total = op.divergence(op.initialize_dof_vector(0, u))
    vol = np.prod(np.array(up) - np.array(lo))
    assert abs(total - 3 * np.sqrt(vol)) <= TOL * 3 * np.sqrt(vol)


def test_two_calls_agree_bitwise(stfem):
    op, nc, verts = _setup(stfem, "pert", 63)
    du = op.initialize_dof_vector(0, np.random.default_rng(12).uniform(-1, 1, 3 * op.n_velocity))
    t1, c1 = op.divergence(du, cells=True)
    t2, c2 = op.divergence(du, cells=True)
    assert t1 == t2 and np.array_equal(c1, c2)


def test_null_pointers_refused(stfem):
    op, nc, verts = _setup(stfem, "box", 63)
    du = op.initialize_dof_vector(0, np.random.default_rng(13).uniform(-1, 1, 3 * op.n_velocity))
    sentinel = np.full(op.n_pressure, -7.25)
    dc = op.initialize_dof_vector(1, sentinel)
    total = C.c_double(-1.0)
    lib = stfem.lib()
    assert lib.stfem_stokes_divergence(op._h, None, dc.ptr, C.byref(total), None) == -1  # STFEM_ERR_INVALID_ARGUMENT
    assert lib.stfem_stokes_divergence(op._h, du.ptr, dc.ptr, None, None) == -1
    assert lib.stfem_stokes_divergence(None, du.ptr, dc.ptr, C.byref(total), None) == -1
    assert total.value == -1.0
    assert np.array_equal(dc.download(), sentinel)
    with pytest.raises(stfem.StfemError):
        op.divergence(None)
    # the same call with its arguments in place writes the first n_cells entries and no more
    assert lib.stfem_stokes_divergence(op._h, du.ptr, dc.ptr, C.byref(total), None) == 0
    got = dc.download()
    assert np.all(got[:op.n_cells] > 0.0) and np.array_equal(got[op.n_cells:], sentinel[op.n_cells:])
