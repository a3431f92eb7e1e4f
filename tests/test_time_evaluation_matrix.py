"""get_time_evaluation_matrix (reference include/fe_time.h:308-326) for the basis of get_time_basis: the temporal Lagrange basis on the
Gauss-Lobatto (cG) / right Gauss-Radau (dG) points at the samples s / (samples - 1), against direct Lagrange evaluation in numpy.  Host
tables only: no GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

CASES = [(0, r) for r in range(1, 5)] + [(1, r) for r in range(0, 4)]


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def lagrange(nodes, x):
    """[x][node], the product formula"""
    V = np.ones((len(x), len(nodes)))
    for j, xj in enumerate(nodes):
        for k, xk in enumerate(nodes):
            if k != j:
                V[:, j] *= (x - xk) / (xj - xk)
    return V


@pytest.mark.parametrize("samples", [2, 5, 11])
@pytest.mark.parametrize("ttype,r", CASES)
def test_against_direct_lagrange_evaluation(ttype, r, samples, stfem):
    T = stfem.get_time_evaluation_matrix(ttype, r, samples)
    nodes = stfem.fe_time_points(ttype, r)
    assert T.shape == (samples, r + 1)
    x = np.arange(samples) / (samples - 1)
    assert np.max(np.abs(T - lagrange(nodes, x))) <= 1e-14
    assert np.max(np.abs(T.sum(axis=1) - 1.0)) <= 1e-14  # a partition of unity
    # a basis node at 0 or 1 makes the first / last row a unit vector: both ends for cG (Lobatto), the right end for dG (Radau)
    unit_last = np.zeros(r + 1); unit_last[-1] = 1.0
    assert nodes[-1] == 1.0 and np.max(np.abs(T[-1] - unit_last)) <= 1e-14
    if ttype == 0:
        unit_first = np.zeros(r + 1); unit_first[0] = 1.0
        assert nodes[0] == 0.0 and np.max(np.abs(T[0] - unit_first)) <= 1e-14
    elif r > 0:
        assert nodes[0] > 0.0 and np.count_nonzero(np.abs(T[0]) > 1e-3) > 1  # no node at 0: an extrapolation of all of them
    # it reproduces polynomials of the basis degree from their nodal values
    if r > 0:
        assert np.max(np.abs(T @ nodes ** r - x ** r)) <= 1e-14


def test_refused_arguments(stfem):
    L = stfem.lib()
    dims = (C.c_int32 * 2)(7, 7)
    assert L.stfem_time_evaluation_matrix(0, 0, 5, None, dims) < 0   # cG(0) does not exist
    assert L.stfem_time_evaluation_matrix(2, 1, 5, None, dims) < 0   # no such type
    assert L.stfem_time_evaluation_matrix(1, 9, 5, None, dims) < 0   # degree
    assert L.stfem_time_evaluation_matrix(1, 1, 1, None, dims) < 0   # one sample: the step 1 / (samples - 1) does not exist
    assert L.stfem_time_evaluation_matrix(1, 1, 5, None, None) < 0
    assert tuple(dims) == (7, 7)
    assert L.stfem_time_evaluation_matrix(1, 1, 5, None, dims) == 0 and tuple(dims) == (5, 2)
    with pytest.raises(stfem.StfemError):
        stfem.get_time_evaluation_matrix(0, 0, 5)
