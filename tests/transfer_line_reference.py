"""Line form of the space transfer for meshes too large for oracle/stmg_oracle.py::space_prolongation (which visits every
fine cell in Python): the same rule, applied along ONE line per direction.  Per fine cell of a line: the local embedding of
its parent's (or its own coarser-degree) Lagrange basis, weighted by the inverse valence of the fine node, added into the 1D
matrix; rows and columns of the nodes on faces with the zero boundary condition zeroed.  The valence of a node of the 3D
mesh is the product of its three line valences and a DoF is constrained iff one of its three line indices is, so the 3D
matrix is the Kronecker product of the three factors; they are applied axis by axis in float64.
tests/test_transfer_line_reference_cpu.py holds this against space_prolongation on the small shapes.
TEST INFRASTRUCTURE ONLY: nothing here calls the product."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as _o


def _lagrange(nodes, x):
    nodes = np.asarray(nodes, float)
    out = np.ones(len(nodes))
    for a in range(len(nodes)):
        for m in range(len(nodes)):
            if m != a:
                out[a] *= (x - nodes[m]) / (nodes[a] - nodes[m])
    return out


def line_factor(p_f, n_f, lo_f, hi_f, p_c, n_c, lo_c, hi_c):
    """P1 [p_f n_f + 1, p_c n_c + 1] (csr) of a line of n_f fine on n_c coarse cells; lo / hi: that end is constrained"""
    r = n_f // n_c
    assert n_f == r * n_c and r in (1, 2)
    gf, gc = _o.gauss_lobatto(p_f + 1), _o.gauss_lobatto(p_c + 1)
    local = [np.array([_lagrange(gc, (s + x) / r) for x in gf]) for s in range(r)]
    nd_f, nd_c = p_f * n_f + 1, p_c * n_c + 1
    valence = np.zeros(nd_f)
    for c in range(n_f):
        valence[c * p_f:c * p_f + p_f + 1] += 1
    P = np.zeros((nd_f, nd_c))
    for c in range(n_f):
        f = np.arange(c * p_f, c * p_f + p_f + 1)
        k = np.arange((c // r) * p_c, (c // r) * p_c + p_c + 1)
        P[np.ix_(f, k)] += local[c % r] / valence[f][:, None]
    if lo_f:
        P[0, :] = 0
    if hi_f:
        P[-1, :] = 0
    if lo_c:
        P[:, 0] = 0
    if hi_c:
        P[:, -1] = 0
    return sp.csr_matrix(P)


def line_factors(p_f, nc_f, mask_f, p_c, nc_c, mask_c):
    """[Px, Py, Pz]; masks as dirichlet_mask (bit 2d: lower, 2d + 1: upper face of direction d)"""
    return [line_factor(p_f, nc_f[d], mask_f >> (2 * d) & 1, mask_f >> (2 * d + 1) & 1,
                        p_c, nc_c[d], mask_c >> (2 * d) & 1, mask_c >> (2 * d + 1) & 1) for d in range(3)]


def _apply_axis(A, U, axis):
    """A along `axis` of U"""
    V = np.moveaxis(U, axis, 0)
    shape = V.shape
    W = A @ np.ascontiguousarray(V).reshape(shape[0], -1)
    return np.moveaxis(W.reshape((A.shape[0],) + shape[1:]), 0, axis)


def _apply(factors, U, nd_in):
    """(Fz (x) Fy (x) Fx) on every row of U [nb, N], x fastest"""
    U = np.asarray(U, float)
    V = U.reshape(U.shape[0], nd_in[2], nd_in[1], nd_in[0])
    for d in range(3):
        V = _apply_axis(factors[d], V, 3 - d)
    return np.ascontiguousarray(V).reshape(U.shape[0], -1)


def prolongate(factors, Uc):
    """P Uc for Uc [nb, N_c]"""
    return _apply(factors, Uc, [f.shape[1] for f in factors])


def restrict(factors, Uf):
    """P^T Uf for Uf [nb, N_f]"""
    return _apply([f.T.tocsr() for f in factors], Uf, [f.shape[0] for f in factors])
