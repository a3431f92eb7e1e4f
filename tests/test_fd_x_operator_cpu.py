"""The parity-packed 1D mass and stiffness tables of the pencil sweep's x step (csrc/host_tables.h: fd_M1, fd_K1), read from the
library through `host/print_tables fd` for FE_Q(1) .. FE_Q(5).  No GPU.

The tables are unpacked (layout of host_tables.h) and compared with M1 = S^T diag(w) S and K1 = D^T diag(w) D assembled here from
the library's own nodes, quadrature points and weights, in extended precision (numpy longdouble), so that the reference's own
rounding is below what is measured.  The bound is not a guess: the route the kernel took before, W^T W and W^T diag(fd_lam) W from
the double tables fd_W / fd_lam, is measured against the same matrices in the same test, and the new tables must be no worse.

Measured (max |difference| / max |entry|, x86-64, longdouble = 80-bit):
  p   M1 packed   M1 = W^T W   K1 packed   K1 = W^T diag(lam) W
  1   8.4e-17     1.7e-16      0.0e+00     2.2e-16
  2   4.8e-17     4.8e-17      7.0e-17     1.2e-15
  3   1.4e-16     1.4e-16      3.1e-16     7.5e-16
  4   2.2e-16     1.1e-15      8.7e-16     1.4e-15
  5   2.8e-16     3.8e-16      9.7e-16     1.2e-15
(what is left in the packed tables is the rounding of the library's S and D tables and of the quadrature sums)
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
LD = np.longdouble


@pytest.fixture(scope="module")
def tables():
    """{p: {name: values}} as printed by the library's host tables"""
    subprocess.check_call(["make", "-C", HOST, "print_tables"], stdout=subprocess.DEVNULL)
    out, cur = {}, None
    for line in subprocess.check_output([os.path.join(HOST, "print_tables"), "fd"], text=True).splitlines():
        f = line.split()
        if f[0] == "p":
            cur = out.setdefault(int(f[1]), {"n": int(f[3])})
        else:
            cur[f[0]] = np.array([float(v) for v in f[1:]])
    assert sorted(out) == [1, 2, 3, 4, 5]
    return out


def sym_index(m, i, j):
    i, j = min(i, j), max(i, j)
    return i * m - i * (i - 1) // 2 + (j - i)


def unpack(t, n):
    """the full n x n matrix of a parity-packed table"""
    h = n // 2
    ne = n - h
    assert len(t) == ne * (ne + 1) // 2 + h * (h + 1) // 2
    odd0 = ne * (ne + 1) // 2
    X = np.zeros((n, n))
    for i in range(ne):
        for j in range(ne):
            e = t[sym_index(ne, i, j)]
            o = t[odd0 + sym_index(h, i, j)] if i < h and j < h else 0.0
            if i < h and j < h:
                X[i, j] = X[n - 1 - i, n - 1 - j] = e + o
                X[i, n - 1 - j] = X[n - 1 - i, j] = e - o
            elif i < h:          # column of the middle node
                X[i, j] = X[n - 1 - i, j] = e
            elif j < h:          # row of the middle node
                X[i, j] = X[i, n - 1 - j] = e
            else:
                X[i, j] = e
    return X


def full_W(fd_W, n):
    h = n // 2
    ne = n - h
    W = np.zeros((n, n))
    for m in range(ne):
        for i in range(ne):
            W[m, i] = W[m, n - 1 - i] = fd_W[m * ne + i]
    for m in range(h):
        for i in range(h):
            W[ne + m, i] = fd_W[ne * ne + m * h + i]
            W[ne + m, n - 1 - i] = -fd_W[ne * ne + m * h + i]
    return W


def reference_pair(nodes, xq, wq):
    """M1, K1 from the Lagrange basis on `nodes` at the quadrature points, in extended precision"""
    x, q, w = nodes.astype(LD), xq.astype(LD), wq.astype(LD)
    n = len(x)
    S, D = np.zeros((n, n), LD), np.zeros((n, n), LD)
    for a in range(n):
        others = [b for b in range(n) if b != a]
        den = np.prod([x[a] - x[b] for b in others])
        for k in range(n):
            S[k, a] = np.prod([q[k] - x[b] for b in others]) / den
            D[k, a] = sum(np.prod([q[k] - x[c] for c in others if c != b]) for b in others) / den
    return S.T @ (w[:, None] * S), D.T @ (w[:, None] * D)


def discrepancy(X, ref):
    return float(np.abs(X.astype(LD) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5])
def test_packed_pair_vs_numpy_and_vs_the_transform_route(p, tables):
    t = tables[p]
    n = t["n"]
    assert n == p + 1
    M1, K1 = reference_pair(t["nodes"], t["xq"], t["wq"])
    M, K = unpack(t["fd_M1"], n), unpack(t["fd_K1"], n)
    W = full_W(t["fd_W"], n)
    Mw, Kw = W.T @ W, W.T @ (t["fd_lam"][:, None] * W)
    dM, dMw, dK, dKw = discrepancy(M, M1), discrepancy(Mw, M1), discrepancy(K, K1), discrepancy(Kw, K1)
    print(f"p {p}: M1 packed {dM:.1e}, W^T W {dMw:.1e}; K1 packed {dK:.1e}, W^T diag(lam) W {dKw:.1e}")
    # no worse than the route through the transform tables (whose own discrepancy is rounding: a few 1e-16)
    assert dMw < 1e-14 and dKw < 1e-14
    assert dM <= dMw and dK <= dKw
    # symmetric and persymmetric, exactly (only the unique entries are stored)
    for X in (M, K):
        assert np.array_equal(X, X.T) and np.array_equal(X, X[::-1, ::-1])
    # M1 is positive definite, K1 positive semi-definite with the constants in its kernel
    assert np.linalg.eigvalsh(M).min() > 0
    assert np.abs(K @ np.ones(n)).max() < 1e-13 * np.abs(K).max() and np.linalg.eigvalsh(K).min() > -1e-13 * np.abs(K).max()
