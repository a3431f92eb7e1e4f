"""Plain numpy restatement of the cell term of the Navier-Stokes modes of StokesMatrixFreeOperator (reference
include/operators.h:1525-1575) for a velocity of any degree, written independently of the kernels and of tests/navier_reference.py
(which is FE_Q(2) in closed form): a loop over cells with the full 3D tables of the Lagrange basis on the Gauss-Lobatto nodes at the
Gauss(nq)^3 points (numpy's own rule), the MappingQ1 Jacobian from the eight vertices, no sum factorisation, read_dof_values
semantics.  A helper of tests/test_navier_q3_reference_cpu.py, tests/test_gpu_navier_q3.py, tests/test_host_navier_q3.py and
tests/test_gpu_guard_bands_stokes_q3_convection.py, not a test module.

Vectors: velocity 3 * n_u doubles, component-major, every component numbered lexicographically on the (degree ncell + 1)^3 lattice
(x fastest); vertices [(ncell + 1)^3][3], x fastest.  Modes: 1 = form, 2 = jacobian."""
import numpy as np

FORM, JACOBIAN = 1, 2
EPS10 = 10 * np.finfo(np.float64).eps


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def gauss_lobatto01(degree):
    """the degree + 1 Gauss-Lobatto points on [0, 1]: the end points and the roots of P_degree'"""
    inner = np.polynomial.legendre.Legendre.basis(degree).deriv().roots() if degree > 1 else np.zeros(0)
    return 0.5 * (np.concatenate([[-1.0], np.sort(np.real(inner)), [1.0]]) + 1.0)


def lagrange_1d(nodes, x):
    """values and derivatives [point][node] of the Lagrange basis on `nodes`, from the product formulas"""
    x = np.asarray(x, dtype=np.float64)
    n = len(nodes)
    S, D = np.ones((len(x), n)), np.zeros((len(x), n))
    for a in range(n):
        for m in range(n):
            if m != a:
                S[:, a] *= (x - nodes[m]) / (nodes[a] - nodes[m])
        for k in range(n):
            if k == a:
                continue
            term = np.full(len(x), 1.0 / (nodes[a] - nodes[k]))
            for m in range(n):
                if m != a and m != k:
                    term *= (x - nodes[m]) / (nodes[a] - nodes[m])
            D[:, a] += term
    return S, D


def tables_3d(nodes, pts):
    """phi [point][n^3], dphi [point][n^3][3] of the tensor Lagrange basis on `nodes` at the reference points pts [point][3]; function
    a + n b + n^2 c"""
    n = len(nodes)
    SD = [lagrange_1d(nodes, pts[:, d]) for d in range(3)]
    phi, dphi = np.zeros((len(pts), n ** 3)), np.zeros((len(pts), n ** 3, 3))
    for c in range(n):
        for b in range(n):
            for a in range(n):
                f = a + n * (b + n * c)
                phi[:, f] = SD[0][0][:, a] * SD[1][0][:, b] * SD[2][0][:, c]
                dphi[:, f, 0] = SD[0][1][:, a] * SD[1][0][:, b] * SD[2][0][:, c]
                dphi[:, f, 1] = SD[0][0][:, a] * SD[1][1][:, b] * SD[2][0][:, c]
                dphi[:, f, 2] = SD[0][0][:, a] * SD[1][0][:, b] * SD[2][1][:, c]
    return phi, dphi


def lattice(degree, ncell):
    return [degree * n + 1 for n in ncell]


def n_velocity(degree, ncell):
    return int(np.prod(lattice(degree, ncell)))


def constrained(degree, ncell, dirichlet_mask):
    """[n_u] bool: the strongly constrained DoFs of a velocity component (bit 2 d + s: side s of direction d)"""
    nd = lattice(degree, ncell)
    iz, iy, ix = np.meshgrid(np.arange(nd[2]), np.arange(nd[1]), np.arange(nd[0]), indexing="ij")
    idx = (ix, iy, iz)
    con = np.zeros(ix.shape, dtype=bool)
    for d in range(3):
        if dirichlet_mask >> (2 * d) & 1:
            con |= idx[d] == 0
        if dirichlet_mask >> (2 * d + 1) & 1:
            con |= idx[d] == nd[d] - 1
    return con.reshape(-1)


def node_coordinates(degree, ncell):
    """[n_u][3]: the DoF positions of a velocity component on the unit box with uniform cells (nodal interpolation of a function)"""
    gl = gauss_lobatto01(degree)
    ax = [np.concatenate([(c + gl[:-1]) / n for c in range(n)] + [[1.0]]) for n in ncell]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def box_vertices(ncell, lower=(0, 0, 0), upper=(1, 1, 1)):
    ax = [np.linspace(lower[d], upper[d], ncell[d] + 1) for d in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def _cell_dofs(degree, ncell, cx, cy, cz):
    nd, n = lattice(degree, ncell), degree + 1
    return np.array([(degree * cx + a) + nd[0] * ((degree * cy + b) + nd[1] * (degree * cz + c))
                     for c in range(n) for b in range(n) for a in range(n)])


def _cell_vertices(ncell, vertices, cx, cy, cz):
    nv = [n + 1 for n in ncell]
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return np.array([V[(cx + i) + nv[0] * ((cy + j) + nv[1] * (cz + k))] for k in range(2) for j in range(2) for i in range(2)])


def _read(vec, degree, ncell, dirichlet_mask):
    """read_dof_values: entries on strongly constrained DoFs read as 0"""
    w = np.array(vec, dtype=np.float64).reshape(3, n_velocity(degree, ncell))
    w[:, constrained(degree, ncell, dirichlet_mask)] = 0.0
    return w


def convection_cells(degree, mode, b, u, ncell, vertices, dirichlet_mask, nq=None):
    """[3][n_u]: v -> - int (u (x) b) : grad v (form), - int (b (x) u + u (x) b) : grad v (jacobian) with the Gauss(nq)^3 rule,
    nq = degree + 1 unless given"""
    assert mode in (FORM, JACOBIAN)
    nq = degree + 1 if nq is None else nq
    xq, wq = gauss01(nq)
    pts = np.array([[xq[qa], xq[qb], xq[qc]] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    wts = np.array([wq[qa] * wq[qb] * wq[qc] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    phi, dphi = tables_3d(gauss_lobatto01(degree), pts)
    _, dN = tables_3d(np.array([0.0, 1.0]), pts)  # the trilinear mapping, vertex i + 2 j + 4 k
    U, B = _read(u, degree, ncell, dirichlet_mask), _read(b, degree, ncell, dirichlet_mask)
    out = np.zeros_like(U)
    for cz in range(ncell[2]):
        for cy in range(ncell[1]):
            for cx in range(ncell[0]):
                dofs = _cell_dofs(degree, ncell, cx, cy, cz)
                V = _cell_vertices(ncell, vertices, cx, cy, cz)
                J = np.einsum("vd,qve->qde", V, dN)              # dx_d / dxi_e
                Jinv = np.linalg.inv(J)                           # dxi_e / dx_j = Jinv[q][e][j]
                JxW = np.linalg.det(J) * wts
                grad = np.einsum("qne,qej->qnj", dphi, Jinv)      # d phi_n / dx_j
                uq, bq = U[:, dofs] @ phi.T, B[:, dofs] @ phi.T   # [3][q]
                F = -np.einsum("iq,jq->qij", uq, bq)
                if mode == JACOBIAN:
                    F -= np.einsum("iq,jq->qij", bq, uq)
                out[:, dofs] += np.einsum("q,qij,qnj->in", JxW, F, grad)
    out[:, constrained(degree, ncell, dirichlet_mask)] = 0.0
    return out


def convection(degree, mode, b, u, ncell, vertices, dirichlet_mask):
    """what mode 1 / 2 adds to the velocity rows of the linear operator, flat [3 n_u]"""
    return convection_cells(degree, mode, b, u, ncell, vertices, dirichlet_mask).reshape(-1)


def st_convection(degree, mode, Alpha, ns, nt, blocks, lin, index, ncell, vertices, dirichlet_mask):
    """per destination block the sum over the source time dofs (it, id), linearised about lin[index(it, 0, id)], of the convective
    result weighted with Alpha(index(jt, 0, jd), index(it, 0, id)) under the 10-eps skip rule (operators.h:835-866); None where nothing
    arrives (the pressure blocks)"""
    add = [None] * (2 * ns * nt)
    for it in range(ns):
        for d in range(nt):
            i = index(it, 0, d)
            conv = convection(degree, mode, lin[i], blocks[i], ncell, vertices, dirichlet_mask)
            for jt in range(ns):
                for jd in range(nt):
                    j = index(jt, 0, jd)
                    if abs(Alpha[j, i]) > EPS10:
                        add[j] = Alpha[j, i] * conv if add[j] is None else add[j] + Alpha[j, i] * conv
    return add
