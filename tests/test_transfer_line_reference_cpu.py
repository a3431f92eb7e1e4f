"""tests/transfer_line_reference.py (three 1D factors assembled cell by cell along a line, applied axis by axis) against the
cell-by-cell 3D assembly of oracle/stmg_oracle.py::space_prolongation, P and P^T, on the shapes of
tests/test_gpu_stmg.py::test_space_transfer_vs_oracle.  The two are sums of the same products in another order: 1e-14 rel-L2."""
import numpy as np
import pytest
import scipy.sparse as sp

import transfer_line_reference as tlr

SHAPES = [
    (2, (4, 4, 4), 2, (2, 2, 2), 63),
    (4, (4, 2, 6), 4, (2, 1, 3), 63),
    (3, (3, 2, 2), 1, (3, 2, 2), 63),
    (4, (2, 3, 2), 2, (2, 3, 2), 63 & ~48),
    (2, (4, 2, 2), 1, (2, 1, 1), 0),
    (1, (6, 4, 4), 1, (3, 2, 2), 63 & ~3),
    (4, (4, 2, 4), 3, (2, 1, 2), 63),
    (3, (2, 4, 2), 2, (1, 2, 1), 63 & ~12),
    (2, (4, 2, 4), 2, (2, 2, 2), 63),
]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


@pytest.mark.parametrize("pf,ncf,pc,ncc,mask", SHAPES)
def test_line_reference_equals_cellwise_oracle(pf, ncf, pc, ncc, mask):
    from oracle import stmg_oracle
    P = stmg_oracle.space_prolongation(pf, ncf, mask, pc, ncc, mask)
    F = tlr.line_factors(pf, ncf, mask, pc, ncc, mask)
    rng = np.random.default_rng(5)
    Uc, Uf = rng.uniform(-1, 1, (3, P.shape[1])), rng.uniform(-1, 1, (3, P.shape[0]))
    assert rel(tlr.prolongate(F, Uc), (P @ Uc.T).T) < 1e-14
    assert rel(tlr.restrict(F, Uf), (P.T @ Uf.T).T) < 1e-14
    # the matrix itself, not only its action on two vectors
    K = sp.kron(F[2], sp.kron(F[1], F[0]))
    assert abs(K - P).max() < 1e-14


def test_mixed_mask_differs_between_y_and_z():
    """a mask that constrains different ends along y and z: the factors must follow the direction's own bits"""
    mask = 2 | 4 | 32  # x upper, y lower, z upper
    from oracle import stmg_oracle
    P = stmg_oracle.space_prolongation(2, (2, 4, 4), mask, 2, (1, 2, 2), mask)
    F = tlr.line_factors(2, (2, 4, 4), mask, 2, (1, 2, 2), mask)
    assert abs(F[1] - F[2]).max() > 0.5
    Uc = np.random.default_rng(6).uniform(-1, 1, (2, P.shape[1]))
    assert rel(tlr.prolongate(F, Uc), (P @ Uc.T).T) < 1e-14
