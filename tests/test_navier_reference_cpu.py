"""The numpy restatement of the convection modes (tests/navier_reference.py) checked against what it must satisfy by construction,
and the C-ABI of the modes checked without a GPU: the symbols exist and refuse bad arguments before anything touches a device."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


def _node_coordinates(ncell):
    nd = [2 * n + 1 for n in ncell]
    z, y, x = np.meshgrid(*[np.linspace(0, 1, nd[d]) for d in (2, 1, 0)], indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


@pytest.mark.parametrize("mode", [nref.FORM, nref.JACOBIAN])
def test_three_point_rule_is_exact_for_trilinear_fields(mode):
    """trilinear u, b on a Cartesian 2 x 2 x 2 mesh: the integrand has degree <= 5 per direction (1 + 1 + 2, and the constant
    Jacobian), so Gauss(3) and Gauss(6) integrate it exactly and agree to rounding"""
    nc = (2, 2, 2)
    verts = nref.perturbed_vertices(nc, 0.0, 0)
    x, y, z = _node_coordinates(nc)
    rng = np.random.default_rng(3)

    def trilinear():
        c = rng.uniform(-1, 1, (3, 8))
        mono = np.stack([np.ones_like(x), x, y, z, x * y, y * z, x * z, x * y * z])
        return (c @ mono).reshape(-1)

    u, b = trilinear(), trilinear()
    r3 = nref.convection_cells(mode, b, u, nc, verts, 0, nq=3)
    r6 = nref.convection_cells(mode, b, u, nc, verts, 0, nq=6)
    assert np.linalg.norm(r3) > 1e-3
    assert rel(r3, r6) <= 1e-13


@pytest.mark.parametrize("dg_pressure", [False, True])
def test_newton_identity(dg_pressure, oracle_mod):
    """F(w) = L w + C_form(w, w) is quadratic: F(u + d) = F(u) + J(u) d + C_form(d, d) with J(u) d = L d + C_jacobian(u, d), for
    random Q2 fields on a perturbed 2 x 2 x 2 mesh; L is the existing linear oracle"""
    nc, mask, nu = (2, 2, 2), 0b111011, 0.3
    verts = nref.perturbed_vertices(nc, 0.15, 7)
    orc = oracle_mod.StokesOracle(nc, verts, mask, nu, dg_pressure=dg_pressure)
    rng = np.random.default_rng(11)
    u, d = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, 3 * orc.n_u)
    p, dp = rng.uniform(-1, 1, orc.n_p), rng.uniform(-1, 1, orc.n_p)

    def F(w, q):
        return nref.vmult(orc, nref.FORM, w, w, q, nc, verts, mask)

    fu, fp = F(u + d, p + dp)
    gu, gp = F(u, p)
    ju, jp = nref.vmult(orc, nref.JACOBIAN, u, d, dp, nc, verts, mask)
    cdd = nref.convection(nref.FORM, d, d, nc, verts, mask)
    assert np.linalg.norm(cdd) > 1e-3 * np.linalg.norm(fu)
    assert np.linalg.norm(fu - (gu + ju + cdd)) <= 1e-13 * np.linalg.norm(fu)
    assert np.linalg.norm(fp - (gp + jp)) <= 1e-13 * np.linalg.norm(fp)


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    mod.lib()
    return mod


NEW = ["stfem_stokes_vmult_convection", "stfem_stokes_st_vmult_convection", "stfem_stokes_st_vmult_slice_add_convection"]


def test_convection_entry_points_exported_and_refuse_bad_arguments(stfem):
    """the three entry points of the modes are exported and listed in SIGNATURES; a mode outside 0..2, a null linearisation with a
    mode other than 0 and null arguments are STFEM_ERR_INVALID_ARGUMENT (-1) - decided before the context is looked at, so a block
    of zeros stands in for it here and no device is needed"""
    raw = C.CDLL(stfem.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in stfem.SIGNATURES, name
    assert (stfem.CONVECTION_FORM, stfem.CONVECTION_JACOBIAN) == (1, 2)
    L = stfem.lib()
    ctx = C.create_string_buffer(1 << 16)  # never dereferenced by a refusal
    bufs = [np.zeros(8) for _ in range(6)]
    du, dp, su, sp, lin, w = (b.ctypes.data for b in bufs)
    A = np.zeros((2, 2))
    pA = A.ctypes.data_as(C.POINTER(C.c_double))
    vp2 = C.c_void_p * 2
    dst, src, lb = vp2(du, dp), vp2(su, sp), vp2(lin, None)
    for mode in (-1, 3, 7):
        assert L.stfem_stokes_vmult_convection(ctx, mode, du, dp, su, sp, lin, None) == -1
        assert L.stfem_stokes_st_vmult_convection(ctx, mode, 1, 1, 1, pA, pA, dst, src, lb, None) == -1
        assert L.stfem_stokes_st_vmult_slice_add_convection(ctx, mode, 1, 1, 1, pA, pA, dst, su, sp, lin, None) == -1
    for mode in (1, 2):  # no linearisation state
        assert L.stfem_stokes_vmult_convection(ctx, mode, du, dp, su, sp, None, None) == -1
        assert L.stfem_stokes_st_vmult_convection(ctx, mode, 1, 1, 1, pA, pA, dst, src, None, None) == -1
        assert L.stfem_stokes_st_vmult_convection(ctx, mode, 1, 1, 1, pA, pA, dst, src, vp2(None, None), None) == -1
        assert L.stfem_stokes_st_vmult_slice_add_convection(ctx, mode, 1, 1, 1, pA, pA, dst, su, sp, None, None) == -1
    for mode in (0, 1, 2):  # null context / vectors
        assert L.stfem_stokes_vmult_convection(None, mode, du, dp, su, sp, lin, None) == -1
        assert L.stfem_stokes_vmult_convection(ctx, mode, None, dp, su, sp, lin, None) == -1
        assert L.stfem_stokes_st_vmult_convection(None, mode, 1, 1, 1, pA, pA, dst, src, lb, None) == -1
        assert L.stfem_stokes_st_vmult_convection(ctx, mode, 1, 1, 1, pA, pA, None, src, lb, None) == -1
        assert L.stfem_stokes_st_vmult_slice_add_convection(ctx, mode, 1, 1, 1, pA, pA, dst, None, sp, lin, None) == -1
    # aliasing is a status too: the linearisation may be the source, never a destination
    assert L.stfem_stokes_vmult_convection(ctx, 1, du, dp, su, sp, du, None) == -6
    assert L.stfem_stokes_st_vmult_convection(ctx, 2, 1, 1, 1, pA, pA, dst, src, vp2(du, None), None) == -6
    assert L.stfem_stokes_st_vmult_slice_add_convection(ctx, 1, 1, 1, 1, pA, pA, dst, su, sp, du, None) == -6
    assert all(np.all(b == 0) for b in bufs)
