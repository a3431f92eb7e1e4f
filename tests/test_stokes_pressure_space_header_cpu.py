"""The companion header include/stfem_stokes_pressure_space.h (the pressure space helpers, the FE_DGP transfers and the divergence
functional for a Stokes context of either velocity degree, the getter of a context's space and the diagnostic of the divergence
kernel): include/stfem.h includes it after the four other companions, the library exports the nine symbols it declares, the Python
veneer binds exactly those in PRESSURE_SPACE_SIGNATURES, and they stand in none of the five other tables and headers.  The argument
refusals of the seven _space entries are decided without a device and are those of the entries of stfem.h without the suffix, status
for status.  No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

SPACE_FORMS = {"stfem_stokes_pressure_ctx_space", "stfem_stokes_pressure_mean_vectors_space", "stfem_stokes_pressure_quadrature_points_space",
               "stfem_stokes_pressure_difference_space", "stfem_stokes_dgp_prolongate_space", "stfem_stokes_dgp_restrict_space",
               "stfem_stokes_divergence_space"}
NAMES = SPACE_FORMS | {"stfem_stokes_get_space", "stfem_stokes_last_divergence_plan"}
INVALID = -1


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    mod.lib()
    return mod


def declared_in(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(stfem_[a-z0-9_]+)\s*\(", text))


def test_companion_header_symbols_exported_and_bound(stfem):
    text = open(stfem.HEADER_PATH).read()
    assert re.search(r'^#include "stfem_stokes_pressure_space.h"$', text, flags=re.M)
    assert (text.index('#include "stfem_stokes_space.h"') < text.index('#include "stfem_stokes_vanka_space.h"')
            < text.index('#include "stfem_stokes_convection_space.h"') < text.index('#include "stfem_stokes_vanka_linearised_space.h"')
            < text.index('#include "stfem_stokes_pressure_space.h"'))
    head = open(stfem.PRESSURE_SPACE_HEADER_PATH).read()
    assert "#ifndef STFEM_H\n#error" in head
    declared = declared_in(stfem.PRESSURE_SPACE_HEADER_PATH)
    assert declared == NAMES
    raw = C.CDLL(stfem.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/stfem_stokes_pressure_space.h but not exported"
    assert declared == set(stfem.PRESSURE_SPACE_SIGNATURES)
    for table in (stfem.SIGNATURES, stfem.SPACE_SIGNATURES, stfem.VANKA_SPACE_SIGNATURES, stfem.CONVECTION_SPACE_SIGNATURES,
                  stfem.VANKA_LINEARISED_SPACE_SIGNATURES):
        assert not declared & set(table)
    for path in (stfem.HEADER_PATH, stfem.SPACE_HEADER_PATH, stfem.VANKA_SPACE_HEADER_PATH, stfem.CONVECTION_SPACE_HEADER_PATH,
                 stfem.VANKA_LINEARISED_SPACE_HEADER_PATH):
        assert not declared & declared_in(path)
    # the argument lists are those of the entries without the suffix
    for name in SPACE_FORMS:
        assert stfem.PRESSURE_SPACE_SIGNATURES[name] == stfem.SIGNATURES[name[: -len("_space")]]
        assert getattr(stfem.lib(), name).argtypes == stfem.SIGNATURES[name[: -len("_space")]][1]
    assert stfem.PRESSURE_SPACE_SIGNATURES["stfem_stokes_last_divergence_plan"] == stfem.SPACE_SIGNATURES["stfem_stokes_last_cell_plan"]
    assert [a.__name__ for a in stfem.PRESSURE_SPACE_SIGNATURES["stfem_stokes_get_space"][1]] == ["c_void_p", "LP__StokesSpaceDesc"]


def test_refusals_without_a_device(stfem):
    """decided on the arguments before the context is read or the device touched: the same with and without a GPU.  The context of
    these calls is a block of zeros that no accepted call could use, the arrays are host addresses no accepted call could read - every
    call must be refused before either is looked at, by the _space entry exactly as by the entry without the suffix."""
    L = stfem.lib()
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    ctx2 = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    bufs = [np.zeros(8) for _ in range(4)]
    a, b, c, d = (x.ctypes.data for x in bufs)
    pa, pb, pc = (stfem._p(x) for x in bufs[:3])
    handle = C.c_void_p(7)

    def both(name, status, *args):
        for entry in (name, name + "_space"):
            got = getattr(L, "stfem_stokes_" + entry)(*args)
            assert got == status, (entry, got, status, args)

    # ---- pressure_ctx: (ctx, out)
    both("pressure_ctx", INVALID, None, C.byref(handle))
    both("pressure_ctx", INVALID, ctx, None)
    assert handle.value == 7
    # ---- pressure_mean_vectors: (ctx, ones, weights, volume)
    for hole in range(4):
        args = [ctx, pa, pb, pc]
        args[hole] = None
        both("pressure_mean_vectors", INVALID, *args)
    # ---- pressure_quadrature_points: (ctx, nq, out)
    both("pressure_quadrature_points", INVALID, None, 2, pa)
    both("pressure_quadrature_points", INVALID, ctx, 2, None)
    for nq in (0, -1, 9):
        both("pressure_quadrature_points", INVALID, ctx, nq, pa)
    # ---- pressure_difference: (ctx, nq, p, exact, out, stream)
    for hole in (0, 2, 3, 4):
        args = [ctx, 2, a, pb, pc, None]
        args[hole] = None
        both("pressure_difference", INVALID, *args)
    for nq in (0, -3, 9):
        both("pressure_difference", INVALID, ctx, nq, a, pb, pc, None)
    # ---- the transfers: (fine, coarse, dst, src, add, stream)
    for entry in ("dgp_prolongate", "dgp_restrict"):
        for hole in range(4):
            args = [ctx, ctx2, a, b, 0, None]
            args[hole] = None
            both(entry, INVALID, *args)
    # ---- divergence: (ctx, u, cell_out, total, stream); cell_out may be null, so a null context decides
    both("divergence", INVALID, None, a, b, pc, None)
    both("divergence", INVALID, ctx, None, b, pc, None)
    both("divergence", INVALID, ctx, a, b, None, None)
    both("divergence", INVALID, None, a, None, pc, None)
    # ---- the getter and the diagnostic
    sd = stfem._StokesSpaceDesc()
    sd.velocity_degree = 77
    assert L.stfem_stokes_get_space(None, C.byref(sd)) == INVALID and L.stfem_stokes_get_space(ctx, None) == INVALID
    assert sd.velocity_degree == 77
    out = (C.c_int32 * 2)(5, 6)
    assert L.stfem_stokes_last_divergence_plan(None, out) == INVALID and L.stfem_stokes_last_divergence_plan(ctx, None) == INVALID
    assert list(out) == [5, 6]
    assert all(np.all(x == 0.0) for x in bufs)
