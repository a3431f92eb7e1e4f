"""The companion header include/stfem_stokes_boundary_space.h (the weak faces for a Stokes context of either velocity degree and the
diagnostic of the boundary kernel): include/stfem.h includes it after the five other companions, the library exports the five symbols
it declares, the Python veneer binds exactly those in BOUNDARY_SPACE_SIGNATURES, and they stand in none of the six other tables and
headers.  The argument refusals are decided without a device and are those of the entries of stfem.h without the suffix, status for
status.  No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

NAMES = {"stfem_stokes_set_weak_boundaries_space", "stfem_stokes_n_face_points_space", "stfem_stokes_face_points_space",
         "stfem_stokes_nitsche_rhs_space", "stfem_stokes_last_face_plan"}
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
    assert re.search(r'^#include "stfem_stokes_boundary_space.h"$', text, flags=re.M)
    assert text.index('#include "stfem_stokes_pressure_space.h"') < text.index('#include "stfem_stokes_boundary_space.h"')
    head = open(stfem.BOUNDARY_SPACE_HEADER_PATH).read()
    assert "#ifndef STFEM_H\n#error" in head
    declared = declared_in(stfem.BOUNDARY_SPACE_HEADER_PATH)
    assert declared == NAMES
    raw = C.CDLL(stfem.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/stfem_stokes_boundary_space.h but not exported"
    assert declared == set(stfem.BOUNDARY_SPACE_SIGNATURES)
    for table in (stfem.SIGNATURES, stfem.SPACE_SIGNATURES, stfem.VANKA_SPACE_SIGNATURES, stfem.CONVECTION_SPACE_SIGNATURES,
                  stfem.VANKA_LINEARISED_SPACE_SIGNATURES, stfem.PRESSURE_SPACE_SIGNATURES):
        assert not declared & set(table)
    for path in (stfem.HEADER_PATH, stfem.SPACE_HEADER_PATH, stfem.VANKA_SPACE_HEADER_PATH, stfem.CONVECTION_SPACE_HEADER_PATH,
                 stfem.VANKA_LINEARISED_SPACE_HEADER_PATH, stfem.PRESSURE_SPACE_HEADER_PATH):
        assert not declared & declared_in(path)
    # the argument lists are those of the entries without the suffix
    for name in NAMES - {"stfem_stokes_last_face_plan"}:
        assert stfem.BOUNDARY_SPACE_SIGNATURES[name] == stfem.SIGNATURES[name[: -len("_space")]]
    assert stfem.BOUNDARY_SPACE_SIGNATURES["stfem_stokes_last_face_plan"] == stfem.SPACE_SIGNATURES["stfem_stokes_last_cell_plan"]


def test_refusals_without_a_device(stfem):
    """decided on the arguments before the context is read or the device touched: the context of these calls is a block of zeros that
    no accepted call could use, the arrays are host addresses no accepted call could read"""
    L = stfem.lib()
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    bufs = [np.zeros(8) for _ in range(3)]
    g = bufs[0].ctypes.data_as(C.POINTER(C.c_double))
    du, dp = bufs[1].ctypes.data, bufs[2].ctypes.data

    def both(name, status, *args):
        for entry in (name, name + "_space"):
            got = getattr(L, "stfem_stokes_" + entry)(*args)
            assert got == status, (entry, got, status)

    both("set_weak_boundaries", INVALID, None, 1, 0, 20.0, 10.0)
    for weak, outflow in ((-1, 0), (64, 0), (1, -1), (1, 64)):
        both("set_weak_boundaries", INVALID, ctx, weak, outflow, 20.0, 10.0)
    both("face_points", INVALID, None, g)
    both("face_points", INVALID, ctx, None)
    both("nitsche_rhs", INVALID, None, g, du, dp, None)
    for hole in (1, 2, 3):
        args = [ctx, g, du, dp, None]
        args[hole] = None
        both("nitsche_rhs", INVALID, *args)
    assert L.stfem_stokes_n_face_points(None) == 0 and L.stfem_stokes_n_face_points_space(None) == 0
    out = (C.c_int32 * 2)()
    assert L.stfem_stokes_last_face_plan(None, out) == INVALID and L.stfem_stokes_last_face_plan(ctx, None) == INVALID
    assert all(np.all(x == 0.0) for x in bufs)
