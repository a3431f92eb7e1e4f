"""The dense levels of tests/navier_slab_reference.py::linearised_level WITH the CIP term on the level (GMGStokes with
AdditionalData::delta0; the reference hands stokes_parameters.delta0 to the operator of every multigrid level and cuts the Vanka blocks
out of that operator's matrix, tests/tp_03stokes.cc:610-623, 655-726): Alpha[j, i] C(lin_i) is added to the level operator and to the
smoother's matrices, C the dense scalar matrix of tests/stokes_vanka_cip_reference.py::cip_matrix on the three velocity components.
  level operator: u and w read with the level's constraints and constrained rows zero, as cip_reference.cip(..., dirichlet_mask=mask);
  smoother: assembled on the unconstrained mesh with w read with the constraints, then rows and columns of constrained DoFs dropped
  with the diagonal - the CIP diagonal included - kept.
The steps are those of linearised_level, restated here because its smoother is closed over its own matrices.  A helper of
tests/test_gpu_navier_cip_mg.py, not a test module."""
import numpy as np
import scipy.linalg

import navier_reference as nref
import navier_slab_reference as nsr
import stokes_vanka_cip_reference as scr

EPS10 = nref.EPS10


def _three(C):
    return scipy.linalg.block_diag(C, C, C)


def linearised_level_cip(stfem, nc, ttype, r, tau, nu, dg, omega, degree, mode, lin, delta0, mask=63, weak=0):
    """-> (dict for oracle/stmg_oracle.py::Multigrid, block sizes in BlockSlice(1, 2, nt) order); delta0 = 0: linearised_level's own"""
    nt = r if ttype == 0 else r + 1
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(ttype, r, tau, 1)
    Alpha, Beta = np.asarray(Alpha, float), np.asarray(Beta, float)
    var = [(b // nt) % 2 for b in range(2 * nt)]
    verts = stfem.mesh_vertices(nc)
    K, M, cells = nsr.stokes_matrices(nc, nu, weak, dg)
    nu_ = nref.n_velocity(nc)
    n_p = K.shape[0] - 3 * nu_
    cu1 = nref.constrained(nc, mask)
    cu = np.tile(cu1, 3)
    con = np.concatenate([cu, np.zeros(n_p, bool)])
    bs = [3 * nu_ if v == 0 else n_p for v in var]
    off = np.concatenate([[0], np.cumsum(bs)])
    nb, N = len(bs), off[-1]
    rng = [np.arange(3 * nu_), 3 * nu_ + np.arange(n_p)]
    # the CIP matrices of the time dofs: w read with the level's constraints
    Cs = [scr.cip_matrix(delta0, lin[i], nc, verts, mask) for i in range(nt)]
    # the level operator
    Ka, Ma = nsr._constrain(K, con, False), nsr._constrain(M, cu, False)
    A = np.zeros((N, N))
    for bi in range(nb):
        for bj in range(nb):
            iv, jv = var[bi], var[bj]
            if abs(Alpha[bi, bj]) > EPS10:
                A[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] += Alpha[bi, bj] * Ka[np.ix_(rng[iv], rng[jv])]
            if iv == 0 and jv == 0 and abs(Beta[bi, bj]) > EPS10:
                A[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] += Beta[bi, bj] * Ma
    for i in range(nt):       # source time dof i (block i: the velocity blocks come first), linearised about lin[i]
        C = nsr.convection_matrix(mode, lin[i], nc, verts, mask, weak) + _three(nsr._constrain(Cs[i], cu1, False))
        for j in range(nt):
            if abs(Alpha[j, i]) > EPS10:
                A[off[j]:off[j + 1], off[i]:off[i + 1]] += Alpha[j, i] * C
    # the smoother's matrices
    Ks = []
    for i in range(nt):
        bm = np.array(lin[i], dtype=np.float64).reshape(-1)
        bm[cu] = 0.0
        Kb = K.copy()
        Kb[:3 * nu_, :3 * nu_] += nsr.convection_matrix(mode, bm, nc, verts, 0, weak) + _three(Cs[i])
        Ks.append(nsr._constrain(Kb, con, True))
    Ms = nsr._constrain(M, cu, True)
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
                blk = Alpha[bi, bj] * Ks[bj if jv == 0 else 0][np.ix_(idx[iv], idx[jv])]
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
