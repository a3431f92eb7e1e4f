"""The companion header include/stfem_stokes_convection_space.h (the convection modes for a Stokes context of either velocity degree
and the diagnostic of the convection kernels): include/stfem.h includes it after the two other companions, the library exports the
four symbols it declares, the Python veneer binds exactly those in CONVECTION_SPACE_SIGNATURES, and they stand in none of the three
other tables and headers.  The argument refusals of the three operator entries are decided without a device and are those of the
entries of stfem.h without the suffix, status for status.  No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

NAMES = {"stfem_stokes_vmult_convection_space", "stfem_stokes_st_vmult_convection_space", "stfem_stokes_st_vmult_slice_add_convection_space",
         "stfem_stokes_last_convection_plan"}
INVALID, ALIAS = -1, -6


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
    assert re.search(r'^#include "stfem_stokes_convection_space.h"$', text, flags=re.M)
    assert (text.index('#include "stfem_stokes_space.h"') < text.index('#include "stfem_stokes_vanka_space.h"')
            < text.index('#include "stfem_stokes_convection_space.h"'))
    head = open(stfem.CONVECTION_SPACE_HEADER_PATH).read()
    assert "#ifndef STFEM_H\n#error" in head
    declared = declared_in(stfem.CONVECTION_SPACE_HEADER_PATH)
    assert declared == NAMES
    raw = C.CDLL(stfem.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/stfem_stokes_convection_space.h but not exported"
    assert declared == set(stfem.CONVECTION_SPACE_SIGNATURES)
    for table in (stfem.SIGNATURES, stfem.SPACE_SIGNATURES, stfem.VANKA_SPACE_SIGNATURES):
        assert not declared & set(table)
    for path in (stfem.HEADER_PATH, stfem.SPACE_HEADER_PATH, stfem.VANKA_SPACE_HEADER_PATH):
        assert not declared & declared_in(path)
    # the argument lists are those of the entries without the suffix
    for name in NAMES - {"stfem_stokes_last_convection_plan"}:
        assert stfem.CONVECTION_SPACE_SIGNATURES[name] == stfem.SIGNATURES[name[: -len("_space")]]
    assert stfem.CONVECTION_SPACE_SIGNATURES["stfem_stokes_last_convection_plan"] == stfem.SPACE_SIGNATURES["stfem_stokes_last_cell_plan"]


def test_refusals_without_a_device(stfem):
    """decided on the arguments before the context is read or the device touched: the same with and without a GPU.  The context of
    these calls is a block of zeros that no accepted call could use, the arrays are host addresses no accepted call could read - every
    call must be refused before either is looked at, by the _space entry exactly as by the entry without the suffix."""
    L = stfem.lib()
    ctx = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    bufs = [np.zeros(8) for _ in range(8)]
    du, dp, u, p, b, du2, dp2, b2 = (x.ctypes.data for x in bufs)
    A = np.eye(4)
    Ap, ones = stfem._p(A), stfem._p(np.ones(4))
    two, four = (C.c_void_p * 2), (C.c_void_p * 4)
    dst, src, lin = four(du, du2, dp, dp2), four(u, u + 8, p, p + 8), four(b, b2, None, None)

    def both(name, status, *args):
        for entry in (name, name + "_space"):
            got = getattr(L, "stfem_stokes_" + entry)(*args)
            assert got == status, (entry, got, status, args)

    # ---- vmult: (ctx, mode, dst_u, dst_p, src_u, src_p, lin_u, stream)
    both("vmult_convection", INVALID, None, 1, du, dp, u, p, b, None)
    for hole in range(2, 6):
        args = [ctx, 1, du, dp, u, p, b, None]
        args[hole] = None
        both("vmult_convection", INVALID, *args)
    for mode in (-1, 3):
        both("vmult_convection", INVALID, ctx, mode, du, dp, u, p, b, None)
    for mode in (1, 2):
        both("vmult_convection", INVALID, ctx, mode, du, dp, u, p, None, None)
    both("vmult_convection", ALIAS, ctx, 0, u, dp, u, p, None, None)
    both("vmult_convection", ALIAS, ctx, 2, du, p, u, p, b, None)
    both("vmult_convection", ALIAS, ctx, 1, du, dp, u, p, du, None)
    both("vmult_convection", ALIAS, ctx, 1, du, dp, u, p, dp, None)
    # ---- st_vmult: (ctx, mode, ns, nt, variable_major, Alpha, Beta, dst_blocks, src_blocks, lin_blocks, stream), cG(2): four blocks
    both("st_vmult_convection", INVALID, None, 1, 1, 2, 1, Ap, Ap, dst, src, lin, None)
    for hole in (5, 6, 7, 8):
        args = [ctx, 1, 1, 2, 1, Ap, Ap, dst, src, lin, None]
        args[hole] = None
        both("st_vmult_convection", INVALID, *args)
    both("st_vmult_convection", INVALID, ctx, 1, 0, 2, 1, Ap, Ap, dst, src, lin, None)
    both("st_vmult_convection", INVALID, ctx, 1, 1, 0, 1, Ap, Ap, dst, src, lin, None)
    for mode in (-1, 3):
        both("st_vmult_convection", INVALID, ctx, mode, 1, 2, 1, Ap, Ap, dst, src, lin, None)
    both("st_vmult_convection", INVALID, ctx, 2, 1, 2, 1, Ap, Ap, dst, src, None, None)                   # a mode without lin
    both("st_vmult_convection", INVALID, ctx, 2, 1, 2, 1, Ap, Ap, dst, src, four(b, None, None, None), None)  # ... without one velocity entry
    both("st_vmult_convection", INVALID, ctx, 0, 1, 2, 1, Ap, Ap, four(du, None, dp, dp2), src, None, None)
    both("st_vmult_convection", ALIAS, ctx, 0, 1, 2, 1, Ap, Ap, four(du, u + 8, dp, dp2), src, None, None)  # a destination that is a source
    both("st_vmult_convection", ALIAS, ctx, 1, 1, 2, 1, Ap, Ap, dst, src, four(b, du2, None, None), None)   # a destination that is lin
    # ---- st_vmult_slice_add: (ctx, mode, ns, nt, variable_major, Gamma, Zeta, dst_blocks, src_u, src_p, lin_u, stream)
    both("st_vmult_slice_add_convection", INVALID, None, 1, 1, 2, 1, ones, ones, dst, u, p, b, None)
    for hole in (5, 6, 7, 8, 9):
        args = [ctx, 1, 1, 2, 1, ones, ones, dst, u, p, b, None]
        args[hole] = None
        both("st_vmult_slice_add_convection", INVALID, *args)
    for mode in (-1, 3):
        both("st_vmult_slice_add_convection", INVALID, ctx, mode, 1, 2, 1, ones, ones, dst, u, p, b, None)
    both("st_vmult_slice_add_convection", INVALID, ctx, 1, 1, 2, 1, ones, ones, dst, u, p, None, None)
    both("st_vmult_slice_add_convection", INVALID, ctx, 0, 1, 1, 1, ones, ones, two(du, None), u, p, None, None)
    both("st_vmult_slice_add_convection", ALIAS, ctx, 0, 1, 2, 1, ones, ones, four(du, u, dp, dp2), u, p, None, None)
    both("st_vmult_slice_add_convection", ALIAS, ctx, 0, 1, 2, 1, ones, ones, four(du, du2, dp, p), u, p, None, None)
    both("st_vmult_slice_add_convection", ALIAS, ctx, 2, 1, 2, 1, ones, ones, four(du, du2, dp, dp2), u, p, du2, None)
    # ---- the diagnostic
    out = (C.c_int32 * 2)()
    assert L.stfem_stokes_last_convection_plan(None, out) == INVALID and L.stfem_stokes_last_convection_plan(ctx, None) == INVALID
    assert all(np.all(x == 0.0) for x in bufs)
