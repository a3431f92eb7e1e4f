"""The numpy restatement of compute_drag_lift (tests/drag_lift_reference.py) against closed forms, so that the GPU tests do not check
the kernel against a restatement that is only checked against itself.  Every comparison within 1e-12 A, A = sum |tau_k| JxW over the
contributing face points and components (what the restatement returns as the scale of a rounding bound)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drag_lift_reference as dref  # noqa: E402
import navier_reference as nref  # noqa: E402

TOL = 1e-12
NU, CONST, LBOX = 0.7, 1.3, (2.0, 1.0, 1.5)


@pytest.mark.parametrize("dg", [False, True])
@pytest.mark.parametrize("ncell", [(2, 2, 2), (3, 1, 2)])
def test_poiseuille_closed_forms(ncell, dg):
    """u = (y (1 - y), 0, 0), p = -2 nu x + c lie exactly in the spaces: every face, and all six together (0)"""
    u, p, verts = dref.poiseuille(ncell, LBOX, NU, CONST, dg)
    want = dref.poiseuille_forces(LBOX, NU, CONST)
    for f in range(6):
        force, items, A = dref.drag_lift(u, p, ncell, verts, NU, 1 << f, dg_pressure=dg, plain=True)
        assert A > 0 and items.shape == (dref.n_items(ncell, 1 << f), 3)
        assert np.max(np.abs(force - np.array(want[f]))) <= TOL * A, (f, force, want[f])
    force, items, A = dref.drag_lift(u, p, ncell, verts, NU, 63, dg_pressure=dg, plain=True)
    assert np.max(np.abs(force)) <= TOL * A
    assert len(items) == 2 * (ncell[0] * ncell[1] + ncell[1] * ncell[2] + ncell[0] * ncell[2])
    # with the no-slip walls read as constrained (mask 12) nothing changes: the field is zero there
    again, _, _ = dref.drag_lift(u, p, ncell, verts, NU, 63, dirichlet_mask=12, dg_pressure=dg, plain=False)
    assert np.array_equal(again, force)


def test_closed_surface_of_a_perturbed_mesh():
    """constant p, u = 0, all six faces: the rule integrates n dA of a trilinear face exactly, and the surface is closed"""
    ncell = (3, 2, 2)
    verts = nref.perturbed_vertices(ncell, 0.15, 5)
    rng = np.random.default_rng(3)
    # (perturbed_vertices moves interior vertices only; move the boundary ones too so that the faces are truly trilinear)
    verts = verts + 0.05 * rng.uniform(-1, 1, verts.shape)
    p = np.full(int(np.prod([n + 1 for n in ncell])), 2.5)
    force, items, A = dref.drag_lift(np.zeros(3 * nref.n_velocity(ncell)), p, ncell, verts, NU, 63)
    assert A > 1.0 and np.max(np.abs(items)) > 0.1
    assert np.max(np.abs(force)) <= TOL * A
    pd = np.zeros(4 * int(np.prod(ncell))); pd[0::4] = 2.5
    force, _, A = dref.drag_lift(np.zeros(3 * nref.n_velocity(ncell)), pd, ncell, verts, NU, 63, dg_pressure=True)
    assert np.max(np.abs(force)) <= TOL * A


def test_rigid_rotation_has_no_traction():
    """u = omega x x, p = 0: the symmetric gradient vanishes at every point, so does every item"""
    ncell = (2, 3, 2)
    verts = nref.perturbed_vertices(ncell, 0.15, 6)
    X = dref.velocity_lattice(ncell, verts)
    omega = np.array([0.3, -1.1, 0.7])
    u = np.cross(omega, X).T.reshape(-1)
    scale = NU * np.linalg.norm(omega) * 6.0  # nu |grad u| times the surface of the unit box: what the terms that cancel amount to
    force, items, A = dref.drag_lift(u, np.zeros(int(np.prod([n + 1 for n in ncell]))), ncell, verts, NU, 63, plain=True)
    assert np.max(np.abs(items)) <= TOL * scale and np.max(np.abs(force)) <= TOL * scale
    assert A <= 1e-12 * scale


def test_linearity_and_reading_rule():
    ncell = (2, 2, 3)
    verts = nref.perturbed_vertices(ncell, 0.1, 7)
    rng = np.random.default_rng(8)
    nu_, npr = 3 * nref.n_velocity(ncell), int(np.prod([n + 1 for n in ncell]))
    u1, u2, p1, p2 = rng.uniform(-1, 1, nu_), rng.uniform(-1, 1, nu_), rng.uniform(-1, 1, npr), rng.uniform(-1, 1, npr)
    mask = 0b100110
    f1, i1, A1 = dref.drag_lift(u1, p1, ncell, verts, NU, mask, dirichlet_mask=63)
    f2, i2, A2 = dref.drag_lift(u2, p2, ncell, verts, NU, mask, dirichlet_mask=63)
    f3, i3, A3 = dref.drag_lift(2 * u1 - 3 * u2, 2 * p1 - 3 * p2, ncell, verts, NU, mask, dirichlet_mask=63)
    bound = TOL * (2 * A1 + 3 * A2)
    assert np.max(np.abs(f3 - (2 * f1 - 3 * f2))) <= bound and np.max(np.abs(i3 - (2 * i1 - 3 * i2))) <= bound
    fs, is_, As = dref.drag_lift(u1, p1, ncell, verts, NU, mask, dirichlet_mask=63, scale=-2.5)
    assert np.max(np.abs(fs + 2.5 * f1)) <= TOL * 2.5 * A1 and np.array_equal(is_, i1) and As == A1  # items and A are unscaled
    # the plain read sees the stored boundary values: another answer; without constraints both rules are one
    fp, _, _ = dref.drag_lift(u1, p1, ncell, verts, NU, mask, dirichlet_mask=63, plain=True)
    assert np.max(np.abs(fp - f1)) > 1e-3 * A1
    fa, _, _ = dref.drag_lift(u1, p1, ncell, verts, NU, mask, dirichlet_mask=0, plain=False)
    assert np.array_equal(fa, fp)
    # a mask is the sum of its faces, item for item
    parts = [dref.drag_lift(u1, p1, ncell, verts, NU, 1 << f, dirichlet_mask=63) for f in (1, 2, 5)]
    assert np.array_equal(np.concatenate([q[1] for q in parts]), i1)
