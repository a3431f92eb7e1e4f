"""Plain numpy restatement of the convection term of the Navier-Stokes modes of StokesMatrixFreeOperator (reference
include/operators.h:1525-1575, 1738-1743), written independently of the kernels: a loop over cells with the full 3D tables of
FE_Q(2) on {0, 1/2, 1} at the Gauss(n) points, the MappingQ1 Jacobian from the eight vertices, no sum factorisation.  A helper of
tests/test_navier_reference_cpu.py, tests/test_gpu_navier.py and tests/test_host_navier.py, not a test module.

Vectors: velocity 3 * n_u doubles, component-major, every component numbered lexicographically on the (2 ncell + 1)^3 lattice
(x fastest); vertices [(ncell + 1)^3][3], x fastest.  Modes: 1 = form, 2 = jacobian."""
import numpy as np

FORM, JACOBIAN = 1, 2
EPS10 = 10 * np.finfo(np.float64).eps


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def q2_1d(x):
    """values and derivatives [point][node] of the quadratic Lagrange basis on the nodes 0, 1/2, 1"""
    x = np.asarray(x, dtype=np.float64)
    S = np.stack([(2 * x - 1) * (x - 1), 4 * x * (1 - x), x * (2 * x - 1)], axis=1)
    D = np.stack([4 * x - 3, 4 - 8 * x, 4 * x - 1], axis=1)
    return S, D


def q1_1d(x):
    x = np.asarray(x, dtype=np.float64)
    return np.stack([1 - x, x], axis=1), np.stack([-np.ones_like(x), np.ones_like(x)], axis=1)


def tables_3d(pts):
    """phi [point][27], dphi [point][27][3] of FE_Q(2)^1 and the same of the trilinear mapping ([point][8], [point][8][3]) at the
    reference points pts [point][3]; node n = a + 3 b + 9 c (vertex v = i + 2 j + 4 k)"""
    out = []
    for f, m in ((q2_1d, 3), (q1_1d, 2)):
        S = [f(pts[:, d])[0] for d in range(3)]
        D = [f(pts[:, d])[1] for d in range(3)]
        phi = np.zeros((len(pts), m ** 3)); dphi = np.zeros((len(pts), m ** 3, 3))
        for c in range(m):
            for b in range(m):
                for a in range(m):
                    n = a + m * (b + m * c)
                    phi[:, n] = S[0][:, a] * S[1][:, b] * S[2][:, c]
                    dphi[:, n, 0] = D[0][:, a] * S[1][:, b] * S[2][:, c]
                    dphi[:, n, 1] = S[0][:, a] * D[1][:, b] * S[2][:, c]
                    dphi[:, n, 2] = S[0][:, a] * S[1][:, b] * D[2][:, c]
        out += [phi, dphi]
    return out


def n_velocity(ncell):
    return int(np.prod([2 * n + 1 for n in ncell]))


def constrained(ncell, dirichlet_mask):
    """[n_u] bool: the strongly constrained DoFs of a velocity component (bit 2 d + s: side s of direction d)"""
    nd = [2 * n + 1 for n in ncell]
    iz, iy, ix = np.meshgrid(np.arange(nd[2]), np.arange(nd[1]), np.arange(nd[0]), indexing="ij")
    idx = (ix, iy, iz)
    con = np.zeros(ix.shape, dtype=bool)
    for d in range(3):
        if dirichlet_mask >> (2 * d) & 1:
            con |= idx[d] == 0
        if dirichlet_mask >> (2 * d + 1) & 1:
            con |= idx[d] == nd[d] - 1
    return con.reshape(-1)


def _cell_dofs(ncell, cx, cy, cz):
    nd = [2 * n + 1 for n in ncell]
    return np.array([(2 * cx + a) + nd[0] * ((2 * cy + b) + nd[1] * (2 * cz + c)) for c in range(3) for b in range(3) for a in range(3)])


def _cell_vertices(ncell, vertices, cx, cy, cz):
    nv = [n + 1 for n in ncell]
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return np.array([V[(cx + i) + nv[0] * ((cy + j) + nv[1] * (cz + k))] for k in range(2) for j in range(2) for i in range(2)])


def _read(vec, ncell, dirichlet_mask):
    """read_dof_values: entries on strongly constrained DoFs read as 0"""
    w = np.array(vec, dtype=np.float64).reshape(3, n_velocity(ncell))
    w[:, constrained(ncell, dirichlet_mask)] = 0.0
    return w


def convection_cells(mode, b, u, ncell, vertices, dirichlet_mask, nq=3):
    """[3][n_u]: v -> - int (u (x) b) : grad v (form), - int (b (x) u + u (x) b) : grad v (jacobian) with the Gauss(nq)^3 rule"""
    assert mode in (FORM, JACOBIAN)
    xq, wq = gauss01(nq)
    pts = np.array([[xq[qa], xq[qb], xq[qc]] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    wts = np.array([wq[qa] * wq[qb] * wq[qc] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    phi, dphi, _, dN = tables_3d(pts)
    U, B = _read(u, ncell, dirichlet_mask), _read(b, ncell, dirichlet_mask)
    out = np.zeros_like(U)
    for cz in range(ncell[2]):
        for cy in range(ncell[1]):
            for cx in range(ncell[0]):
                dofs = _cell_dofs(ncell, cx, cy, cz)
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
    out[:, constrained(ncell, dirichlet_mask)] = 0.0
    return out


def convection_faces(b, u, ncell, vertices, dirichlet_mask, weak_mask, outflow_mask=0, nq=3):
    """[3][n_u]: v -> - int_F min(b.n, 0) u.v over the faces of weak_mask that are not in outflow_mask (face 2 d + s), Gauss(nq)^2"""
    xq, wq = gauss01(nq)
    U, B = _read(u, ncell, dirichlet_mask), _read(b, ncell, dirichlet_mask)
    out = np.zeros_like(U)
    for f in range(6):
        if not (weak_mask & ~outflow_mask) >> f & 1:
            continue
        d, s = f // 2, f % 2
        t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
        pts = np.zeros((nq * nq, 3)); wts = np.zeros(nq * nq)
        for q2 in range(nq):
            for q1 in range(nq):
                pts[q1 + nq * q2, d], pts[q1 + nq * q2, t1], pts[q1 + nq * q2, t2] = s, xq[q1], xq[q2]
                wts[q1 + nq * q2] = wq[q1] * wq[q2]
        phi, _, _, dN = tables_3d(pts)
        for c2 in range(ncell[t2]):
            for c1 in range(ncell[t1]):
                cc = [0, 0, 0]
                cc[d], cc[t1], cc[t2] = (ncell[d] - 1 if s else 0), c1, c2
                dofs = _cell_dofs(ncell, *cc)
                V = _cell_vertices(ncell, vertices, *cc)
                J = np.einsum("vd,qve->qde", V, dN)
                Jinv = np.linalg.inv(J)
                m = (1.0 if s else -1.0) * Jinv[:, d, :]          # J^-T e_d, outward
                length = np.linalg.norm(m, axis=1)
                normal = m / length[:, None]
                JxW = np.abs(np.linalg.det(J)) * length * wts
                uq, bq = U[:, dofs] @ phi.T, B[:, dofs] @ phi.T
                inflow = np.minimum(np.einsum("iq,qi->q", bq, normal), 0.0)
                out[:, dofs] += np.einsum("q,iq,qn->in", -inflow * JxW, uq, phi)
    out[:, constrained(ncell, dirichlet_mask)] = 0.0
    return out


def convection(mode, b, u, ncell, vertices, dirichlet_mask, weak_mask=0, outflow_mask=0):
    """what mode 1 / 2 adds to the velocity rows of the linear operator, flat [3 n_u]"""
    r = convection_cells(mode, b, u, ncell, vertices, dirichlet_mask)
    if weak_mask & ~outflow_mask:
        r = r + convection_faces(b, u, ncell, vertices, dirichlet_mask, weak_mask, outflow_mask)
    return r.reshape(-1)


def vmult(orc, mode, b, u, p, ncell, vertices, dirichlet_mask, weak_mask=0, outflow_mask=0):
    """the expected full result: the existing linear oracle (oracle.StokesOracle.apply) plus the term above"""
    ku, kp = orc.apply(u, p)
    ku = ku.reshape(-1).copy()
    if mode:
        ku += convection(mode, b, u, ncell, vertices, dirichlet_mask, weak_mask, outflow_mask)
    return ku, kp


def st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, ncell, vertices, dirichlet_mask, weak_mask=0, outflow_mask=0,
             variable_major=True):
    """oracle.StokesOracle.st_vmult plus, per source time dof (it, id) linearised about lin[index(it, 0, id)], the convective result
    scattered with Alpha(index(jt, 0, jd), index(it, 0, id)) and the 10-eps skip rule (operators.h:835-866)"""
    dst = orc.st_vmult(Alpha, Beta, ns, nt, blocks, variable_major)
    if not mode:
        return dst
    for it in range(ns):
        for d in range(nt):
            i = index(it, 0, d)
            conv = convection(mode, lin[i], blocks[i], ncell, vertices, dirichlet_mask, weak_mask, outflow_mask)
            for jt in range(ns):
                for jd in range(nt):
                    j = index(jt, 0, jd)
                    if abs(Alpha[j, i]) > EPS10:
                        dst[j] = dst[j] + Alpha[j, i] * conv
    return dst


def perturbed_vertices(ncell, distort, seed, lower=(0, 0, 0), upper=(1, 1, 1)):
    """structured vertex grid with the interior vertices moved by up to distort * h per direction"""
    rng = np.random.default_rng(seed)
    nv = [n + 1 for n in ncell]
    h = [(upper[d] - lower[d]) / ncell[d] for d in range(3)]
    V = np.zeros((nv[2], nv[1], nv[0], 3))
    for k in range(nv[2]):
        for j in range(nv[1]):
            for i in range(nv[0]):
                V[k, j, i] = [lower[0] + i * h[0], lower[1] + j * h[1], lower[2] + k * h[2]]
                if 0 < i < ncell[0] and 0 < j < ncell[1] and 0 < k < ncell[2]:
                    V[k, j, i] += distort * np.array(h) * rng.uniform(-1, 1, 3)
    return V.reshape(-1, 3)
