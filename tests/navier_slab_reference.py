"""Dense numpy restatements around the Navier-Stokes slab solve, written from the formulas and independently of the kernels:

  convection_matrix          the convection term of tests/navier_reference.py as a dense matrix, assembled cell by cell (vectorised over
                             the cells) from navier_reference.tables_3d;
  divergence_cells           StokesMatrixFreeOperator::compute_divergence (reference include/operators.h:1391-1439), values read plain;
  navier_convergence_row_3d  the recipe of oracle/slab_oracle.py::stokes_convergence_row_3d with the convection term and a dense Newton
                             iteration with the exact Jacobian (relative residual 1e-12) in place of the single LU solve;
  linearised_level           dense matrix and per-cell Vanka smoother of one multigrid level of the operator linearised about a velocity
                             (Stokes oracle + dense convection), for oracle/stmg_oracle.py::Multigrid.

A helper of tests/test_navier_slab_reference_cpu.py, tests/test_gpu_navier_driver.py, tests/test_gpu_navier_mg.py and
tests/test_gpu_stokes_divergence.py, not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402

FORM, JACOBIAN = nref.FORM, nref.JACOBIAN
EPS10 = nref.EPS10


def _rule(nq=3):
    xq, wq = nref.gauss01(nq)
    pts = np.array([[xq[qa], xq[qb], xq[qc]] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    wts = np.array([wq[qa] * wq[qb] * wq[qc] for qc in range(nq) for qb in range(nq) for qa in range(nq)])
    return pts, wts


def _cells(ncell, vertices):
    """DoFs [cell][27] and vertices [cell][8][3] of all cells, cells lexicographic (x fastest)"""
    dofs = np.array([nref._cell_dofs(ncell, cx, cy, cz) for cz in range(ncell[2]) for cy in range(ncell[1]) for cx in range(ncell[0])])
    V = np.array([nref._cell_vertices(ncell, vertices, cx, cy, cz) for cz in range(ncell[2]) for cy in range(ncell[1]) for cx in range(ncell[0])])
    return dofs, V


def _geometry(ncell, vertices):
    pts, wts = _rule()
    phi, dphi, _, dN = nref.tables_3d(pts)
    dofs, V = _cells(ncell, vertices)
    J = np.einsum("cvd,qve->cqde", V, dN)                       # dx_d / dxi_e
    grad = np.einsum("qne,cqej->cqnj", dphi, np.linalg.inv(J))  # d phi_n / dx_j
    return dofs, phi, grad, np.linalg.det(J) * wts


def divergence_cells(u, ncell, vertices):
    """([n_cells] sum_q (div u_h)^2 JxW, sqrt of their sum): the values of u are used as stored (read_dof_values_plain)"""
    dofs, _, grad, JxW = _geometry(ncell, vertices)
    U = np.asarray(u, dtype=np.float64).reshape(3, nref.n_velocity(ncell))
    div = np.einsum("icn,cqni->cq", U[:, dofs], grad)
    cells = np.sum(div * div * JxW, axis=1)
    return cells, np.sqrt(np.sum(cells))


def convection_matrix(mode, b, ncell, vertices, dirichlet_mask, weak_mask=0, outflow_mask=0):
    """[3 n_u][3 n_u]: u -> navier_reference.convection(mode, b, u, ...): rows and columns of strongly constrained DoFs are zero, b is read
    with its constrained entries as zero"""
    assert mode in (FORM, JACOBIAN)
    Nu = nref.n_velocity(ncell)
    dofs, phi, grad, JxW = _geometry(ncell, vertices)
    B = nref._read(b, ncell, dirichlet_mask)
    bq = np.einsum("icn,qn->ciq", B[:, dofs], phi)              # b_i at the points
    bg = np.einsum("cjq,cqnj->cqn", bq, grad)                   # b . grad phi_n
    M = np.zeros((3 * Nu, 3 * Nu))
    rows, cols = dofs[:, :, None], dofs[:, None, :]
    Cf = -np.einsum("cq,cqn,qm->cnm", JxW, bg, phi)             # - int (u (x) b) : grad v, the same for every component
    for i in range(3):
        np.add.at(M, (i * Nu + rows, i * Nu + cols), Cf)
    if mode == JACOBIAN:                                        # - int (b (x) u) : grad v
        Cj = -np.einsum("cq,ciq,qm,cqnj->cinjm", JxW, bq, phi, grad)
        for i in range(3):
            for j in range(3):
                np.add.at(M, (i * Nu + rows, j * Nu + cols), Cj[:, i, :, j, :])
    weak = weak_mask & ~outflow_mask
    if weak:                                                    # - int_F min(b.n, 0) u.v (navier_reference.convection_faces)
        xq, wq = nref.gauss01(3)
        for f in range(6):
            if not weak >> f & 1:
                continue
            d, s = f // 2, f % 2
            t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
            pts = np.zeros((9, 3)); wts = np.zeros(9)
            for q2 in range(3):
                for q1 in range(3):
                    pts[q1 + 3 * q2, d], pts[q1 + 3 * q2, t1], pts[q1 + 3 * q2, t2] = s, xq[q1], xq[q2]
                    wts[q1 + 3 * q2] = wq[q1] * wq[q2]
            fphi, _, _, fdN = nref.tables_3d(pts)
            for c2 in range(ncell[t2]):
                for c1 in range(ncell[t1]):
                    cc = [0, 0, 0]
                    cc[d], cc[t1], cc[t2] = (ncell[d] - 1 if s else 0), c1, c2
                    fd = nref._cell_dofs(ncell, *cc)
                    V = nref._cell_vertices(ncell, vertices, *cc)
                    J = np.einsum("vd,qve->qde", V, fdN)
                    m = (1.0 if s else -1.0) * np.linalg.inv(J)[:, d, :]
                    length = np.linalg.norm(m, axis=1)
                    fJxW = np.abs(np.linalg.det(J)) * length * wts
                    inflow = np.minimum(np.einsum("iq,qi->q", B[:, fd] @ fphi.T, m / length[:, None]), 0.0)
                    loc = np.einsum("q,qn,qm->nm", -inflow * fJxW, fphi, fphi)
                    for i in range(3):
                        M[np.ix_(i * Nu + fd, i * Nu + fd)] += loc
    con = np.tile(nref.constrained(ncell, dirichlet_mask), 3)
    M[con, :] = 0.0
    M[:, con] = 0.0
    return M


def _exact_convection(X, Y, Z, t):
    """(u . grad) u of the exact velocity of oracle/slab_oracle.py (divergence-free, zero on the boundary)"""
    from oracle import slab_oracle as so
    u, g = so.stokes3d_exact_u(X, Y, Z, t), so.stokes3d_exact_grad_u(X, Y, Z, t)
    return tuple(sum(u[j] * g[i][j] for j in range(3)) for i in range(3))


def navier_convergence_row_3d(ttype, k, refinement, nu=1.0, dg_pressure=False, convection=True, tol=1e-12, details=None):
    """(u: L-inf L-inf, L2 L2, L2 H1-semi; p: L2 L2; |div u_h| at the end time) of the Navier-Stokes problem with the exact solution of
    oracle/slab_oracle.py::stokes_convergence_row_3d and the force extended by (u . grad) u; the same discretisation, right-hand-side
    recipe, zero-mean shift and error quadratures.  Per time dof the convection is the weak form about that time dof's own velocity
    (include/operators.h:835-866); the previous-slab term is the j = 0 term of the same sum.  Per slab a dense Newton iteration with the
    exact Jacobian from the previous solution to a relative residual `tol`.  convection=False: the Stokes problem (one Newton step solves
    it).  details: a dict that receives the residual histories per slab."""
    from oracle import oracle as o, slab_oracle as so_
    n = 2 ** refinement
    h = 1.0 / n
    tau = 2.0 ** -(refinement + 1)
    nc = (n, n, n)
    verts = np.array([[i * h, j * h, kk * h] for kk in range(n + 1) for j in range(n + 1) for i in range(n + 1)], dtype=float)
    so = o.StokesOracle(nc, verts, 0, nu, dg_pressure=dg_pressure)
    Nu, Np = so.n_u, so.n_p
    ndu, ndp = 2 * n + 1, n + 1
    ntot = 3 * Nu + Np
    K = np.zeros((ntot, ntot))
    M = np.zeros((3 * Nu, 3 * Nu))
    e = np.zeros(ntot)
    for j in range(ntot):
        e[j] = 1.0
        ou, op = so.apply(e[:3 * Nu], e[3 * Nu:], 1.0, 0.0)
        K[:3 * Nu, j], K[3 * Nu:, j] = ou.reshape(-1), op
        if j < 3 * Nu:
            M[:, j] = so.apply(e[:3 * Nu], np.zeros(Np), 0.0, 1.0)[0].reshape(-1)
        e[j] = 0.0
    iu = np.arange(ndu ** 3).reshape(ndu, ndu, ndu)
    free1 = iu[1:-1, 1:-1, 1:-1].ravel()
    free = np.concatenate([c * Nu + free1 for c in range(3)])
    nf = len(free)
    pidx = 3 * Nu + np.arange(Np)
    KS_uu, Bt, Bm = K[np.ix_(free, free)], K[np.ix_(free, pidx)], K[np.ix_(pidx, free)]   # nu K, -B^T, B
    MM = M[np.ix_(free, free)]
    A1, B1, G1, Z1 = o.time_weights(ttype, k, tau, 1)
    nt = A1.shape[0]
    NU, NP = nf, Np
    N = nt * (NU + NP)
    ub = lambda a: slice(a * NU, (a + 1) * NU)                     # noqa: E731
    pb = lambda a: slice(nt * NU + a * NP, nt * NU + (a + 1) * NP)  # noqa: E731
    sysm = np.zeros((N, N))
    for a in range(nt):
        for b in range(nt):
            sysm[ub(a), ub(b)] += A1[a, b] * KS_uu + B1[a, b] * MM
            sysm[ub(a), pb(b)] += A1[a, b] * Bt
            sysm[pb(a), ub(b)] += A1[a, b] * Bm
    keep = np.ones(N, dtype=bool)
    for a in range(nt):
        keep[nt * NU + a * NP] = False       # the pressure is determined up to a constant: pin one value, shift to zero mean afterwards
    if ttype == o.CGP:
        rKu, rKp, rM = G1[:, 0], G1[:, 0], Z1[:, 0]
    else:
        rKu, rKp, rM = np.zeros(nt), np.zeros(nt), G1[:, 0]
    Su, _ = o.shape_tables(2)
    xq, wq = o.gauss(3)

    def full(uf):
        U = np.zeros(3 * Nu)
        U[free] = uf
        return U

    def conv(mode, uf):
        """the convection matrix about the velocity uf on the free DoFs (zero without convection)"""
        if not convection:
            return np.zeros((NU, NU))
        return convection_matrix(mode, full(uf), nc, verts, 63)[np.ix_(free, free)]

    def load_vector(t):
        F = np.zeros((3, ndu, ndu, ndu))
        W = h ** 3 * np.einsum("i,j,k->ijk", wq, wq, wq)
        for cz in range(n):
            for cy in range(n):
                for cx in range(n):
                    X, Y, Zc = h * (cx + xq)[None, None, :], h * (cy + xq)[None, :, None], h * (cz + xq)[:, None, None]
                    f = so_.stokes3d_force(X, Y, Zc, t, nu)
                    if convection:
                        f = tuple(a + b for a, b in zip(f, _exact_convection(X, Y, Zc, t)))
                    for c in range(3):
                        F[c, 2 * cz:2 * cz + 3, 2 * cy:2 * cy + 3, 2 * cx:2 * cx + 3] += np.einsum("zyx,za,yb,xc->abc", W * f[c], Su, Su, Su)
        return F.reshape(3 * Nu)[free]

    tq_int = o.gauss_radau_right(k + 1) if ttype == o.DG else o.gauss_lobatto(k + 1)
    et, ewt = o.gauss(k + 1)
    Ltime, _ = so_.lagrange_eval(tq_int, et)
    eu, ewu = o.gauss(3)
    ep, ewp = o.gauss(2)
    Eu, dEu = so_.lagrange_eval(o.gauss_lobatto(3), eu)
    Ep, _ = so_.lagrange_eval(o.gauss_lobatto(2), ep)

    def errors_u(uf, t):
        U = full(uf).reshape(3, ndu, ndu, ndu)
        l2 = h1 = l8 = 0.0
        W = h ** 3 * np.einsum("i,j,k->ijk", ewu, ewu, ewu)
        for cz in range(n):
            for cy in range(n):
                for cx in range(n):
                    X, Y, Zc = h * (cx + eu)[None, None, :], h * (cy + eu)[None, :, None], h * (cz + eu)[:, None, None]
                    ue, ge = so_.stokes3d_exact_u(X, Y, Zc, t), so_.stokes3d_exact_grad_u(X, Y, Zc, t)
                    for c in range(3):
                        loc = U[c, 2 * cz:2 * cz + 3, 2 * cy:2 * cy + 3, 2 * cx:2 * cx + 3]
                        uh = np.einsum("ac,bd,ef,cdf->abe", Eu, Eu, Eu, loc)
                        ux = np.einsum("ac,bd,ef,cdf->abe", Eu, Eu, dEu, loc) / h
                        uy = np.einsum("ac,bd,ef,cdf->abe", Eu, dEu, Eu, loc) / h
                        uz = np.einsum("ac,bd,ef,cdf->abe", dEu, Eu, Eu, loc) / h
                        l2 += np.sum(W * (uh - ue[c]) ** 2)
                        h1 += np.sum(W * ((ux - ge[c][0]) ** 2 + (uy - ge[c][1]) ** 2 + (uz - ge[c][2]) ** 2))
                        l8 = max(l8, np.abs(uh - ue[c]).max())
        return l2, l8, h1

    def errors_p(pf, t):
        P = pf.reshape(n, n, n, 4) if dg_pressure else pf.reshape(ndp, ndp, ndp)
        l2 = 0.0
        W = h ** 3 * np.einsum("i,j,k->ijk", ewp, ewp, ewp)
        lg = np.sqrt(3.0) * (2 * ep - 1)  # deal.II's Legendre basis of FE_DGP(1): 1, l(xi), l(eta), l(zeta)
        for cz in range(n):
            for cy in range(n):
                for cx in range(n):
                    X, Y, Zc = h * (cx + ep)[None, None, :], h * (cy + ep)[None, :, None], h * (cz + ep)[:, None, None]
                    if dg_pressure:
                        c = P[cz, cy, cx]
                        ph = c[0] + c[1] * lg[None, None, :] + c[2] * lg[None, :, None] + c[3] * lg[:, None, None]
                    else:
                        ph = np.einsum("ac,bd,ef,cdf->abe", Ep, Ep, Ep, P[cz:cz + 2, cy:cy + 2, cx:cx + 2])
                    l2 += np.sum(W * (ph - so_.stokes3d_exact_p(X, Y, Zc, t)) ** 2)
        return l2

    if dg_pressure:
        mean_w = np.zeros(Np)
        mean_w[0::4] = h ** 3
        one_p = np.zeros(Np)
        one_p[0::4] = 1.0
    else:
        w1 = np.full(ndp, h)
        w1[0] = w1[-1] = h / 2
        mean_w = np.einsum("i,j,k->ijk", w1, w1, w1).ravel()
        one_p = np.ones(Np)
    prev_u, prev_p = np.zeros(NU), np.zeros(NP)
    time = 0.0
    acc_l2 = acc_h1 = acc_p = 0.0
    acc_l8 = -1.0
    histories = []
    while time < 1.0 - 1e-12:
        rhs = np.zeros(N)
        KSu = KS_uu @ prev_u + Bt @ prev_p + conv(FORM, prev_u) @ prev_u   # the weak form at the previous end value
        KSp = Bm @ prev_u
        Mu = MM @ prev_u
        for a in range(nt):
            rhs[ub(a)] = rKu[a] * KSu + rM[a] * Mu
            rhs[pb(a)] = rKp[a] * KSp
        for j, xi in enumerate(tq_int):
            F = load_vector(time + tau * xi)
            if ttype == o.DG:
                rhs[ub(j)] += A1[j, j] * F
            elif j == 0:
                for i in range(nt):
                    rhs[ub(i)] += -G1[i, 0] * F
            else:
                rhs[ub(j - 1)] += A1[j - 1, j - 1] * F
        # Newton from the previous solution: R(z) = sysm z + sum_b A1[a, b] C(u_b) u_b - rhs, J = sysm + A1[a, b] C_jacobian(u_b)
        sol = np.zeros(N)
        for a in range(nt):
            sol[ub(a)], sol[pb(a)] = prev_u, prev_p
        for a in range(nt):
            sol[nt * NU + a * NP] = 0.0   # (the pinned value)
        hist = []
        for _ in range(30):
            res = sysm @ sol - rhs
            for b in range(nt):
                cb = conv(FORM, sol[ub(b)]) @ sol[ub(b)]
                for a in range(nt):
                    res[ub(a)] += A1[a, b] * cb
            hist.append(np.linalg.norm(res[keep]))
            if hist[-1] <= tol * hist[0]:
                break
            Jm = sysm.copy()
            for b in range(nt):
                cj = conv(JACOBIAN, sol[ub(b)])
                for a in range(nt):
                    Jm[ub(a), ub(b)] += A1[a, b] * cj
            step = np.zeros(N)
            step[keep] = np.linalg.solve(Jm[np.ix_(keep, keep)], -res[keep])
            sol += step
        histories.append(hist)
        xu = [sol[ub(a)] for a in range(nt)]
        xp = [sol[pb(a)] - np.dot(mean_w, sol[pb(a)]) * one_p for a in range(nt)]
        for q in range(k + 1):
            if ttype == o.DG:
                uf = sum(Ltime[q, i] * xu[i] for i in range(nt))
                pf = sum(Ltime[q, i] * xp[i] for i in range(nt))
            else:
                uf = Ltime[q, 0] * prev_u + sum(Ltime[q, i] * xu[i - 1] for i in range(1, k + 1))
                pf = Ltime[q, 0] * prev_p + sum(Ltime[q, i] * xp[i - 1] for i in range(1, k + 1))
            t = time + tau * et[q]
            l2, l8, h1 = errors_u(uf, t)
            acc_l2 += tau * ewt[q] * l2
            acc_h1 += tau * ewt[q] * h1
            acc_l8 = max(acc_l8, l8)
            acc_p += tau * ewt[q] * errors_p(pf, t)
        prev_u, prev_p = xu[-1], xp[-1]
        time += tau
    if details is not None:
        details["residuals"] = histories
    return acc_l8, np.sqrt(acc_l2), np.sqrt(acc_h1), np.sqrt(acc_p), divergence_cells(full(prev_u), nc, verts)[1]


def inject(lin, ncell_fine):
    """the velocity lin [3 n_u] of a mesh at the nodes of the mesh with half the cells per direction (nodal interpolation: the coarse
    FE_Q(2) nodes are fine nodes)"""
    nd = [2 * c + 1 for c in ncell_fine]
    return np.ascontiguousarray(np.asarray(lin).reshape(3, nd[2], nd[1], nd[0])[:, ::2, ::2, ::2]).reshape(-1)


def stokes_matrices(nc, nu, weak=0, dg=False):
    """(K [3 n_u + n_p]^2, M [3 n_u]^2, cells): the Stokes operator (nu K, -B^T; B, 0; Nitsche terms of the weak faces) and the vector
    mass of the unit cube with nc uniform cells WITHOUT strong constraints, assembled cell by cell from the oracle on ONE cell of that
    size (a cell's matrix depends on which of its faces lie on a weak boundary face only); cells: the (velocity, pressure) DoFs per cell.
    The oracle applied to the unit vectors of the whole mesh gives the same matrices, two orders of magnitude more slowly
    (tests/test_navier_slab_reference_cpu.py compares the two)."""
    from oracle import oracle as o
    h = [1.0 / c for c in nc]
    verts1 = np.array([[i * h[0], j * h[1], k * h[2]] for k in range(2) for j in range(2) for i in range(2)])
    ndu, ndp = [2 * c + 1 for c in nc], [c + 1 for c in nc]
    Nu = int(np.prod(ndu))
    Np = 4 * int(np.prod(nc)) if dg else int(np.prod(ndp))
    K, M = np.zeros((3 * Nu + Np, 3 * Nu + Np)), np.zeros((3 * Nu, 3 * Nu))
    local, cells, cell = {}, [], 0
    for cz in range(nc[2]):
        for cy in range(nc[1]):
            for cx in range(nc[0]):
                cc = (cx, cy, cz)
                wm = sum(1 << (2 * d + s) for d in range(3) for s in range(2) if weak >> (2 * d + s) & 1 and cc[d] == (nc[d] - 1 if s else 0))
                if wm not in local:
                    one = o.StokesOracle((1, 1, 1), verts1, 0, nu, weak_mask=wm, dg_pressure=bool(dg))
                    n1 = 81 + one.n_p
                    Kl, Ml, e = np.zeros((n1, n1)), np.zeros((81, 81)), np.zeros(n1)
                    for j in range(n1):
                        e[j] = 1.0
                        ou, op = one.apply(e[:81], e[81:], 1.0, 0.0)
                        Kl[:81, j], Kl[81:, j] = ou.reshape(-1), op
                        if j < 81:
                            Ml[:, j] = one.apply(e[:81], np.zeros(one.n_p), 0.0, 1.0)[0].reshape(-1)
                        e[j] = 0.0
                    local[wm] = (Kl, Ml)
                Kl, Ml = local[wm]
                iu1 = nref._cell_dofs(nc, cx, cy, cz)
                iu = np.concatenate([c * Nu + iu1 for c in range(3)])
                if dg:
                    ip = 4 * cell + np.arange(4)
                else:
                    ip = np.array([(cx + i) + ndp[0] * ((cy + j) + ndp[1] * (cz + k)) for k in range(2) for j in range(2) for i in range(2)])
                idx = np.concatenate([iu, 3 * Nu + ip])
                K[np.ix_(idx, idx)] += Kl
                M[np.ix_(iu, iu)] += Ml
                cells.append((iu, ip))
                cell += 1
    return K, M, cells


def _constrain(A, con, keep_diagonal):
    """rows and columns of the constrained DoFs dropped (with or without the diagonal kept)"""
    A = A.copy()
    d = A.diagonal().copy()
    A[con, :] = 0.0
    A[:, con] = 0.0
    if keep_diagonal:
        A[con, con] = d[con]
    return A


def linearised_level(stfem, nc, ttype, r, tau, nu, dg, omega, degree, mode, lin, mask=63, weak=0):
    """dense matrix and per-cell Vanka smoother of one level (unit cube, nc uniform cells) of the system linearised about
    lin[time dof] (velocities [3 n_u]); -> (dict for oracle/stmg_oracle.py::Multigrid, block sizes in BlockSlice(1, 2, nt) order).
    The matrix: Alpha (x) (Stokes + convection about the source time dof's velocity) + Beta (x) mass with the rows and columns of
    the strongly constrained DoFs zero, as the operator applies it.  The smoother: the steps of tests/stokes_vanka_reference.py (the
    reference's PreconditionVanka on the assembled matrices: constrained rows and columns dropped with the diagonal kept, valence
    weights, one inverse per cell) with the dense convection of this file."""
    nt = r if ttype == 0 else r + 1
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(ttype, r, tau, 1)
    Alpha, Beta = np.asarray(Alpha, float), np.asarray(Beta, float)
    var = [(b // nt) % 2 for b in range(2 * nt)]
    verts = stfem.mesh_vertices(nc)
    K, M, cells = stokes_matrices(nc, nu, weak, dg)
    nu_ = nref.n_velocity(nc)
    n_p = K.shape[0] - 3 * nu_
    cu = np.tile(nref.constrained(nc, mask), 3)
    con = np.concatenate([cu, np.zeros(n_p, bool)])
    bs = [3 * nu_ if v == 0 else n_p for v in var]
    off = np.concatenate([[0], np.cumsum(bs)])
    nb, N = len(bs), off[-1]
    rng = [np.arange(3 * nu_), 3 * nu_ + np.arange(n_p)]   # the rows of a variable in K
    # the level operator
    Ka, Ma = _constrain(K, con, False), _constrain(M, cu, False)
    A = np.zeros((N, N))
    for bi in range(nb):
        for bj in range(nb):
            iv, jv = var[bi], var[bj]
            if abs(Alpha[bi, bj]) > EPS10:
                A[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] += Alpha[bi, bj] * Ka[np.ix_(rng[iv], rng[jv])]
            if iv == 0 and jv == 0 and abs(Beta[bi, bj]) > EPS10:
                A[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] += Beta[bi, bj] * Ma
    for i in range(nt):       # source time dof i (block i: the velocity blocks come first), linearised about lin[i]
        C = convection_matrix(mode, lin[i], nc, verts, mask, weak)
        for j in range(nt):
            if abs(Alpha[j, i]) > EPS10:
                A[off[j]:off[j + 1], off[i]:off[i + 1]] += Alpha[j, i] * C
    # the smoother's matrices: assembled on the unconstrained mesh (b read with its constrained entries as zero), then constrained
    Ks = []
    for i in range(nt):
        bm = np.array(lin[i], dtype=np.float64).reshape(-1)
        bm[cu] = 0.0
        Kb = K.copy()
        Kb[:3 * nu_, :3 * nu_] += convection_matrix(mode, bm, nc, verts, 0, weak)
        Ks.append(_constrain(Kb, con, True))
    Ms = _constrain(M, cu, True)
    valu, valp = np.zeros(3 * nu_), np.zeros(n_p)
    for iu, ip in cells:
        valu[iu] += 1.0
        valp[ip] += 1.0
    blocks = []
    for iu, ip in cells:
        idx = [iu, 3 * nu_ + ip]
        val = [valu[iu], valp[ip]]
        o2 = np.concatenate([[0], np.cumsum([len(idx[v]) for v in var])])
        Bk = np.zeros((o2[-1], o2[-1]))
        for bi in range(nb):
            for bj in range(nb):
                iv, jv = var[bi], var[bj]
                blk = Alpha[bi, bj] * Ks[bj if jv == 0 else 0][np.ix_(idx[iv], idx[jv])]   # (pressure columns carry no convection)
                if iv == 0 and jv == 0:
                    blk = blk + Beta[bi, bj] * Ms[np.ix_(iu, iu)]
                Bk[o2[bi]:o2[bi + 1], o2[bj]:o2[bj + 1]] = val[iv][:, None] * blk
        blocks.append(np.linalg.inv(Bk))

    def smoother(rv):
        src = [rv[off[b]:off[b + 1]] for b in range(nb)]
        dst = [np.zeros_like(b) for b in src]
        for (iu, ip), Binv in zip(cells, blocks):
            y = Binv @ np.concatenate([src[b][iu if v == 0 else ip] for b, v in enumerate(var)])
            o3 = 0
            for b, v in enumerate(var):
                ii = iu if v == 0 else ip
                dst[b][ii] += y[o3:o3 + len(ii)]
                o3 += len(ii)
        return np.concatenate(dst)

    return dict(A=A, smoother=smoother, omega=omega, n_iterations=degree), bs
