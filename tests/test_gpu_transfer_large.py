"""The space-transfer paths that only larger meshes select (csrc/stfem_transfer.hip), against tests/transfer_line_reference.py:
  * cell_prolongate_yz_kernel, taken when fine nx x coarse ncy x coarse ncz >= 150000 (and not for the fp64 Q4 h-transfer, nor
    for a shape it is not instantiated for: three passes, the x pass once),
  * cell_restrict_march_kernel with segments of several coarse cells (nseg = min(ncell, ceil(262144 / lines), 64) < ncell): the
    carry of w[] and u0 from one cell to the next, segments of unequal length,
  * stfem_transfer_restrict with add = 0 (no caller elsewhere).  The restriction runs z, y, x and hands `add` to its last pass only,
    the table-driven x pass (axis_apply_kernel): the march kernels overwrite their intermediates under either entry point, so what
    add = 0 newly reaches is the overwrite of that final pass, checked on a NaN-filled destination with exact zeros in the
    constrained rows.
Every case asserts through MGTwoLevelTransfer.last_path that it ran the path it is named for, so a changed threshold makes the
test fail instead of going quiet.  Tolerances: those of test_gpu_stmg.py::test_space_transfer_vs_oracle (1e-13 / 2e-6 rel-L2) -
the number of terms per output entry does not grow with the mesh.  The inputs are fp32-representable in both precisions, so one
reference serves a shape's double and float case."""
import functools
import importlib

import numpy as np
import pytest

import transfer_line_reference as tlr

pytestmark = pytest.mark.gpu

MIXED_A = 2 | 4 | 32   # x upper, y lower, z upper: flags_y != flags_z
MIXED_B = 1 | 8 | 16   # x lower, y upper, z lower
NB = 3

# name: (fine degree, fine cells, coarse degree, coarse cells, mask, fused in double, fused in float, y marches several cells)
# coarse cell counts along y and z that the longest segment of a marched pass does not divide: segments of unequal length
CASES = {
    "h_q1":        (1, (200, 74, 74), 1, (100, 37, 37), MIXED_A, True, True, True),    # (1, 2): 275 169 y-z threads
    "h_q2_mask63": (2, (100, 58, 58), 2, (50, 29, 29), 63, True, True, True),          # (2, 4): 169 041
    "h_q2_mask0":  (2, (100, 58, 58), 2, (50, 29, 29), 0, True, True, True),
    "h_q2_mixed":  (2, (100, 58, 58), 2, (50, 29, 29), MIXED_B, True, True, True),
    "h_q3":        (3, (60, 58, 58), 3, (30, 29, 29), 63, True, True, True),           # (3, 6): 152 221
    "h_q4":        (4, (66, 48, 52), 4, (33, 24, 26), MIXED_B, False, True, True),     # (4, 8): 165 360; fp64 is `heavy`: three passes
    "p_q3_q2":     (3, (60, 37, 37), 2, (60, 37, 37), MIXED_A, True, True, True),      # (2, 3): 247 789
    "p_q3_q1":     (3, (40, 47, 47), 1, (40, 47, 47), 63, True, True, True),           # (1, 3): 267 289
    "p_q2_q1":     (2, (33, 49, 49), 1, (33, 49, 49), 0, True, True, False),           # (1, 2): 160 867; only z marches several cells
    # (1, 6): 172 040 threads would fuse, but cell_prolongate_yz_kernel has no such instantiation: three passes are planned
    "hp_q3_q1":    (3, (130, 40, 44), 1, (65, 20, 22), MIXED_A, False, False, False),
}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=1)
def reference(name):
    """inputs and the float64 results of one shape (kept for the shape's next case; never modified)"""
    from oracle import stmg_oracle
    pf, ncf, pc, ncc, mask = CASES[name][:5]
    F = tlr.line_factors(pf, ncf, mask, pc, ncc, mask)
    n_f, n_c = int(np.prod([f.shape[0] for f in F])), int(np.prod([f.shape[1] for f in F]))
    rng = np.random.default_rng(11)
    Uc = rng.uniform(-1, 1, (NB, n_c)).astype(np.float32).astype(float)
    Uf = rng.uniform(-1, 1, (NB, n_f)).astype(np.float32).astype(float)
    out = dict(Uc=Uc, Uf=Uf, PUc=tlr.prolongate(F, Uc), RUf=tlr.restrict(F, Uf),
               con_f=stmg_oracle.constrained_mask(pf, ncf, mask), con_c=stmg_oracle.constrained_mask(pc, ncc, mask))
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("number", ["double", "float"])
@pytest.mark.parametrize("name", list(CASES))
def test_large_mesh_transfer_paths(name, number):
    stfem = importlib.import_module("dealii-stfem_amd")
    pf, ncf, pc, ncc, mask, fused64, fused32, y_marches = CASES[name]
    fused = fused64 if number == "double" else fused32
    tol = 1e-13 if number == "double" else 2e-6
    ref = reference(name)
    Uc, Uf, con_f, con_c = ref["Uc"], ref["Uf"], ref["con_f"], ref["con_c"]
    fine = stfem.MatrixFreeOperator(pf, ncf, dirichlet_mask=mask, number=number)
    coarse = stfem.MatrixFreeOperator(pc, ncc, dirichlet_mask=mask, number=number)
    T = stfem.MGTwoLevelTransfer(fine, coarse)
    assert (pf * ncf[0] + 1) * ncc[1] * ncc[2] >= 150000
    uc, uf = stfem.BlockVector(coarse, NB).upload(Uc), stfem.BlockVector(fine, NB).upload(Uf)

    # prolongation, overwrite: every entry of a NaN-filled destination is written, constrained rows with exact zeros
    out_f = stfem.BlockVector(fine, NB).upload(np.full(Uf.shape, np.nan))
    T.prolongate(out_f, uc)
    assert T.last_path[0] == int(fused)
    got = out_f.download()
    err = rel(got, ref["PUc"])
    print(f"{name} {number}: prolongate fused={T.last_path[0]} rel-L2 {err:.3e}")
    assert np.isfinite(got).all() and err < tol
    assert np.all(got[:, con_f] == 0)
    # prolongation, add: constrained rows untouched
    out_f.upload(Uf)
    T.prolongate_and_add(out_f, uc)
    assert T.last_path[0] == int(fused)
    got = out_f.download()
    err = rel(got, Uf + ref["PUc"])
    print(f"{name} {number}: prolongate_and_add rel-L2 {err:.3e}")
    assert err < tol
    assert np.array_equal(got[:, con_f], Uf[:, con_f])
    del out_f

    # restriction (stfem_transfer_restrict with add = 0) into a NaN-filled destination
    out_c = stfem.BlockVector(coarse, NB).upload(np.full(Uc.shape, np.nan))
    T.restrict(out_c, uf)
    path = T.last_path
    print(f"{name} {number}: restriction marches (y, z) = {path[1:]} of {ncc[1:]} coarse cells")
    assert path[2] >= 2  # several coarse cells per thread along z
    assert path[1] >= 2 if y_marches else path[1] == 1
    # a pass whose segments cannot all have the reported (longest) length: segments of unequal length
    assert any(path[d] >= 2 and ncc[d] % path[d] != 0 for d in (1, 2))
    got = out_c.download()
    err = rel(got, ref["RUf"])
    print(f"{name} {number}: restrict rel-L2 {err:.3e}")
    assert np.isfinite(got).all() and err < tol
    assert np.all(got[:, con_c] == 0)
    # restriction march, add
    out_c.upload(Uc)
    T.restrict_and_add(out_c, uf)
    assert T.last_path == path
    got = out_c.download()
    err = rel(got, Uc + ref["RUf"])
    print(f"{name} {number}: restrict_and_add rel-L2 {err:.3e}")
    assert err < tol
    assert np.array_equal(got[:, con_c], Uc[:, con_c])
