"""GPU parity of stfem_stokes_divergence_space (include/stfem_stokes_pressure_space.h; compute_divergence, reference
include/operators.h:1391-1439) at velocity degree 3 against the numpy restatement tests/stokes_pressure_q3_reference.py::
divergence_cells: per cell sum_q (div u_h)^2 JxW at the 4 x 4 x 4 Gauss points with the MappingQ1 Jacobian from the eight vertices,
the total sqrt(sum of the cells).  Tolerance rel 1e-12, the project's fp64 parity tolerance.  Meshes: an anisotropic 3 x 2 x 2 box
(no vertices handed in), the same cells perturbed by 0.15 (12 cells: three workgroups of four waves), and 5 x 1 x 1 cells (two
workgroups, the second with three idle waves; with one workgroup a tail).  The degree-2 context through the _space entry gives the
bits of stfem_stokes_divergence."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_q3_reference as nq3  # noqa: E402
import stokes_pressure_q3_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
UNSUPPORTED = -2
BOX = ((0.0, -0.5, 0.25), (1.0, 0.25, 1.75))
UNIT = ((0, 0, 0), (1, 1, 1))
MESHES = {"box": ((3, 2, 2), 0.0, BOX), "pert": ((3, 2, 2), 0.15, UNIT), "five": ((5, 1, 1), 0.15, UNIT)}
MASKS = [0, 0b011101]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv("STFEM_STOKES_Q3_WORKGROUPS", raising=False)


def _setup(stfem, mesh, mask, degree=3, dg=False):
    nc, distort, (lo, up) = MESHES[mesh]
    verts = stfem.mesh_vertices(nc, lower=lo, upper=up, distort=distort, seed=77)
    op = stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=verts if distort else None, lower=lo, upper=up, dirichlet_mask=mask,
                                                    dg_pressure=dg)
    return op, nc, verts


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_random_field_plain_read(mesh, mask, stfem):
    op, nc, verts = _setup(stfem, mesh, mask)
    assert op.space() == (3, 0, 1.0)
    with pytest.raises(stfem.StfemError) as e:
        op.last_divergence_plan()  # no divergence launch yet
    assert e.value.status == UNSUPPORTED and b"stfem_stokes_last_divergence_plan" in stfem.lib().stfem_last_error()
    u = np.random.default_rng(11).uniform(-1, 1, 3 * op.n_velocity)
    con = np.tile(nq3.constrained(3, nc, mask), 3)
    assert np.all(u[con] != 0.0)
    du = op.initialize_dof_vector(0, u)
    total, cells = op.divergence_space(du, cells=True)
    ref_cells, ref_total = R.divergence_cells(3, u, nc, verts)
    print(f"{mesh} mask {mask}: cells rel {rel(cells, ref_cells):.3e}, total rel {abs(total - ref_total) / ref_total:.3e}")
    assert cells.shape == ref_cells.shape
    assert rel(cells, ref_cells) <= TOL
    assert np.max(np.abs(cells - ref_cells) / ref_cells) <= TOL  # every cell by itself: a sum of 64 non-negative terms
    assert abs(total - ref_total) <= TOL * ref_total
    n = int(np.prod(nc))
    assert op.last_divergence_plan() == ((n + 3) // 4, 1)
    # the total alone (cell_out = NULL) is the same number
    assert op.divergence_space(du) == total
    if mask:  # the check tells a plain read from read_dof_values: with the constrained entries read as zero the answer is another one
        _, zeroed = R.divergence_cells(3, np.where(con, 0.0, u), nc, verts)
        assert abs(zeroed - ref_total) > 1e-3 * ref_total


@pytest.mark.parametrize("mesh", ["pert", "five"])
def test_capped_workgroups_and_reproducible(mesh, stfem, monkeypatch):
    """STFEM_STOKES_Q3_WORKGROUPS=1: one workgroup walks all cells, a wave several where the mesh has more than four; the same bits as
    uncapped, and as a second call"""
    op, nc, verts = _setup(stfem, mesh, 63, dg=True)
    n = int(np.prod(nc))
    du = op.initialize_dof_vector(0, np.random.default_rng(12).uniform(-1, 1, 3 * op.n_velocity))
    t1, c1 = op.divergence_space(du, cells=True)
    assert op.last_divergence_plan() == ((n + 3) // 4, 1)
    t2, c2 = op.divergence_space(du, cells=True)
    assert t1 == t2 and np.array_equal(c1, c2)
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")
    t3, c3 = op.divergence_space(du, cells=True)
    plan = op.last_divergence_plan()
    assert plan == (1, (n + 3) // 4), plan
    if mesh == "pert":
        assert plan[1] == 3  # 12 cells, four waves
    assert t1 == t3 and np.array_equal(c1, c3)
    ref_cells, ref_total = R.divergence_cells(3, du.download(), nc, verts)
    assert rel(c3, ref_cells) <= TOL and abs(t3 - ref_total) <= TOL * ref_total


def test_solenoidal_cubic_and_known_divergence(stfem):
    """the curl of a quartic potential with components in Q3 lies in FE_Q(3)^3 and has no divergence: the total is rounding,
    <= 1e-13 of ||u||; (x, y, z) has div = 3"""
    op, nc, verts = _setup(stfem, "box", 63)
    lo, up = BOX
    x = R.box_node_coordinates(3, nc, lo, up)
    u = R.solenoidal_cubic(x)
    total, cells = op.divergence_space(op.initialize_dof_vector(0, u), cells=True)
    print(f"solenoidal cubic: total {total:.3e}, ||u|| {np.linalg.norm(u):.3e}")
    assert np.all(cells >= 0.0)
    assert total <= 1e-13 * np.linalg.norm(u)
    total = op.divergence_space(op.initialize_dof_vector(0, x.T.ravel()))
    vol = np.prod(np.array(up) - np.array(lo))
    assert abs(total - 3 * np.sqrt(vol)) <= TOL * 3 * np.sqrt(vol)


@pytest.mark.parametrize("mesh", ["box", "pert"])
def test_degree_2_through_space_entry_is_bit_identical(mesh, stfem, monkeypatch):
    nc, distort, (lo, up) = MESHES[mesh]
    verts = stfem.mesh_vertices(nc, lower=lo, upper=up, distort=distort, seed=77)
    kw = dict(vertices=verts if distort else None, lower=lo, upper=up, dirichlet_mask=0b011101)
    old, new = stfem.StokesMatrixFreeOperator(nc, **kw), stfem.StokesMatrixFreeOperator.with_degree(2, nc, **kw)
    assert new.space() == (2, 0, 1.0) and old.space() == (2, 0, 1.0)
    u = np.random.default_rng(13).uniform(-1, 1, 3 * old.n_velocity)
    t_old, c_old = old.divergence(old.initialize_dof_vector(0, u), cells=True)
    t_new, c_new = new.divergence_space(new.initialize_dof_vector(0, u), cells=True)
    assert t_old == t_new and np.array_equal(c_old, c_new)
    plan = new.last_divergence_plan()
    monkeypatch.setenv("STFEM_STOKES_Q3_WORKGROUPS", "1")  # the degree-2 launch is not changed by it
    t_cap, c_cap = new.divergence_space(new.initialize_dof_vector(0, u), cells=True)
    assert new.divergence(new.initialize_dof_vector(0, u)) == t_old  # (the entry of stfem.h on the same context)
    assert new.last_divergence_plan() == plan == ((int(np.prod(nc)) + 7) // 8, 1)
    assert t_cap == t_old and np.array_equal(c_cap, c_old)
    ref_cells, ref_total = R.divergence_cells(2, u, nc, verts)
    assert rel(c_new, ref_cells) <= TOL and abs(t_new - ref_total) <= TOL * ref_total


def test_null_pointers_refused_and_the_old_entry_refuses(stfem):
    op, nc, verts = _setup(stfem, "box", 63)
    du = op.initialize_dof_vector(0, np.random.default_rng(13).uniform(-1, 1, 3 * op.n_velocity))
    sentinel = np.full(op.n_pressure, -7.25)
    dc = op.initialize_dof_vector(1, sentinel)
    total = C.c_double(-1.0)
    lib = stfem.lib()
    assert lib.stfem_stokes_divergence_space(op._h, None, dc.ptr, C.byref(total), None) == -1  # STFEM_ERR_INVALID_ARGUMENT
    assert lib.stfem_stokes_divergence_space(op._h, du.ptr, dc.ptr, None, None) == -1
    assert lib.stfem_stokes_divergence_space(None, du.ptr, dc.ptr, C.byref(total), None) == -1
    assert lib.stfem_stokes_divergence(op._h, du.ptr, dc.ptr, C.byref(total), None) == UNSUPPORTED  # the entry of stfem.h: degree 2 only
    assert b"velocity degree 2 only" in lib.stfem_last_error()
    with pytest.raises(stfem.StfemError) as e:  # (and so the wrapper that calls it)
        op.divergence(du)
    assert e.value.status == UNSUPPORTED
    assert total.value == -1.0
    assert np.array_equal(dc.download(), sentinel)
    # the same call with its arguments in place writes the first n_cells entries and no more
    assert lib.stfem_stokes_divergence_space(op._h, du.ptr, dc.ptr, C.byref(total), None) == 0
    got = dc.download()
    assert np.all(got[:op.n_cells] > 0.0) and np.array_equal(got[op.n_cells:], sentinel[op.n_cells:])
