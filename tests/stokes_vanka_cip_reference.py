"""Dense numpy restatement of the per-cell Stokes Vanka blocks of the operator WITH the CIP term
(stfem_stokes_vanka_create_linearised_cip; the reference cuts its blocks out of compute_system_matrix of an operator that holds delta0,
tests/tp_03stokes.cc:610-623, 655-726).  The dense scalar matrix C(w) of a mesh is assembled face pair by face pair from the formulas
of tests/cip_reference.py with no strong constraints on u; the entries of w on strongly constrained DoFs are read as 0.  It is added,
constrained like K (rows and columns of constrained DoFs zeroed, the diagonal kept), to the three component-diagonal velocity blocks of
StokesVankaReference.K[s] of an instance built by tests/stokes_vanka_reference.py; the weight velocity is the linearisation state of the
column block in every mode.  The blocks are then built again in that helper's own steps.  Written from the formulas, not from the
kernels.  A helper of tests/test_stokes_vanka_cip_reference_cpu.py and tests/test_gpu_stokes_vanka_cip.py, not a test module; it also
holds the cases the two share, built once per process."""
import copy
import functools

import numpy as np

import cip_reference as cref
import navier_reference as nref
import stokes_vanka_reference as svr

DELTA0 = 1.0

# (mesh, perturbed, mode, FE_DGP pressure, time type (0 cG, 1 dG), degree, time steps at once, dirichlet mask, weak mask, variable-major)
CASES = {
    "box333_jac": ((3, 3, 3), False, 2, False, 0, 1, 1, 63, 0, True),          # all 27 neighbour patterns, the centre cell with 54 faces
    "pert232_form_dgp_cg2_tm": ((2, 3, 2), True, 1, True, 0, 2, 1, 63, 0, False),  # general geometry, two states, time-major
    "pert322_jac_weak": svr.CASES["pert322_jac_weak"],                         # unconstrained x faces, weak terms beside the CIP term
    "box224_jac_dg1": ((2, 2, 4), False, 2, False, 1, 1, 1, 63, 0, True),      # 4 cells in z: faces to cells outside the patch
    "pert412_jac_free": ((4, 1, 2), True, 2, True, 0, 1, 1, 0b110000, 0, True),  # 4 cells in x, a one-cell-thick direction
}
# a mode-0 run: the plain Stokes blocks plus the term, `lin` read as the weight only
MODE0 = ((2, 3, 2), True, 0, False, 0, 1, 1, 63, 0, True)
CELL = ((1, 1, 1), False, 2, True, 0, 1, 1, 0, 0, True)  # no interior face


def face_pairs(ncell, vertices, nq=3):
    """every interior face as (dofsA, dofsB, dnA[q][27], dnB[q][27], normal[q][3], phiA[q][27], JxW[q]): cell A, its xi_d = 1 side, and
    the neighbour B in direction d; normal, JxW (and h_F^2 = sum JxW) of side A, each side's normal derivative with its own Jacobian"""
    for d in range(3):
        ptsA, wts = cref.face_rule(d, 1.0, nq)
        ptsB, _ = cref.face_rule(d, 0.0, nq)
        phiA, dphiA, _, dNA = nref.tables_3d(ptsA)
        _, dphiB, _, dNB = nref.tables_3d(ptsB)
        for cz in range(ncell[2]):
            for cy in range(ncell[1]):
                for cx in range(ncell[0]):
                    A = [cx, cy, cz]
                    if A[d] == ncell[d] - 1:
                        continue
                    B = list(A); B[d] += 1
                    JA = np.einsum("vd,qve->qde", nref._cell_vertices(ncell, vertices, *A), dNA)
                    JB = np.einsum("vd,qve->qde", nref._cell_vertices(ncell, vertices, *B), dNB)
                    JinvA, JinvB = np.linalg.inv(JA), np.linalg.inv(JB)
                    m = JinvA[:, d, :]
                    length = np.linalg.norm(m, axis=1)
                    normal = m / length[:, None]
                    JxW = np.abs(np.linalg.det(JA)) * length * wts
                    dnA = np.einsum("qne,qej,qj->qn", dphiA, JinvA, normal)
                    dnB = np.einsum("qne,qej,qj->qn", dphiB, JinvB, normal)
                    yield nref._cell_dofs(ncell, *A), nref._cell_dofs(ncell, *B), dnA, dnB, normal, phiA, JxW


def cip_matrix(delta0, w, ncell, vertices, w_mask, faces=None):
    """the dense scalar [n_u][n_u] matrix of u -> C(w; u) per component, no constraint on u; w read with the mask w_mask.  faces: only
    these positions of the face_pairs sequence"""
    W = nref._read(w, ncell, w_mask)
    n = nref.n_velocity(ncell)
    C = np.zeros((n, n))
    for k, (dofsA, dofsB, dnA, dnB, normal, phiA, JxW) in enumerate(face_pairs(ncell, vertices)):
        if faces is not None and k not in faces:
            continue
        wn = np.einsum("iq,qi->q", W[:, dofsA] @ phiA.T, normal)
        c = delta0 * (JxW.sum() / cref.PA) * wn * wn * JxW
        # the jump [d_n u] = dnA u_A - dnB u_B tested with + dnA on A and - dnB on B (the face nodes are in both lists: four additions)
        C[np.ix_(dofsA, dofsA)] += np.einsum("q,qa,qb->ab", c, dnA, dnA)
        C[np.ix_(dofsA, dofsB)] -= np.einsum("q,qa,qb->ab", c, dnA, dnB)
        C[np.ix_(dofsB, dofsA)] -= np.einsum("q,qa,qb->ab", c, dnB, dnA)
        C[np.ix_(dofsB, dofsB)] += np.einsum("q,qa,qb->ab", c, dnB, dnB)
    return C


def n_interior_faces(ncell):
    return sum((ncell[d] - 1) * ncell[(d + 1) % 3] * ncell[(d + 2) % 3] for d in range(3))


def with_cip(base, p, delta0, lin):
    """a copy of the StokesVankaReference `base` of problem p whose matrices hold Alpha-scaled C(lin_j; .) too; base is left unchanged"""
    ref = copy.copy(base)
    nu_ = base.n_u
    conu = nref.constrained(p.nc, p.mask)
    states, sel = [], [0] * p.nb  # the distinct weight velocities of the velocity column blocks, by identity (as the library has it)
    for j in range(p.nb):
        if p.var[j] != 0:
            continue
        at = [s for s, b in enumerate(states) if b is lin[j]]
        if not at:
            states.append(lin[j])
            at = [len(states) - 1]
        sel[j] = at[0]
    ref.K = []
    for s, b in enumerate(states):
        j0 = [j for j in range(p.nb) if p.var[j] == 0 and sel[j] == s][0]
        Kb = base.K[base.sel[j0]].copy()
        Cs = cip_matrix(delta0, b, p.nc, p.verts, p.mask)
        d = Cs.diagonal().copy()
        Cs[conu, :] = 0.0
        Cs[:, conu] = 0.0
        Cs[conu, conu] = d[conu]
        for c in range(3):
            Kb[c * nu_:(c + 1) * nu_, c * nu_:(c + 1) * nu_] += Cs
        ref.K.append(Kb)
    ref.sel = sel
    # the blocks again: the steps of StokesVankaReference.__init__
    valu, valp = np.zeros(3 * nu_), np.zeros(base.n_p)
    for iu, ip in base.cells:
        valu[iu] += 1.0
        valp[ip] += 1.0
    ref.blocks, ref.cond = [], []
    for iu, ip in base.cells:
        idx = [iu, 3 * nu_ + ip]
        val = [valu[iu], valp[ip]]
        size = [len(iu), len(ip)]
        off = np.concatenate([[0], np.cumsum([size[v] for v in base.var])])
        B = np.zeros((off[-1], off[-1]))
        for bi in range(p.nb):
            for bj in range(p.nb):
                iv, jv = base.var[bi], base.var[bj]
                blk = base.Alpha[bi, bj] * ref.K[ref.sel[bj]][np.ix_(idx[iv], idx[jv])]
                if iv == 0 and jv == 0:
                    blk = blk + base.Beta[bi, bj] * base.M[np.ix_(iu, iu)]
                B[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] = val[iv][:, None] * blk
        ref.cond.append(np.linalg.cond(B))
        ref.blocks.append(np.linalg.inv(B))
    ref.cond_max = max(ref.cond)
    return ref


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, reference without the term, reference with delta0 = DELTA0) of a case of CASES, built once per process"""
    if CASES[name] is svr.CASES.get(name):
        p, base = svr.case(name)
    else:
        p = svr.problem(CASES[name])
        base = svr.reference(p)
    return p, base, with_cip(base, p, DELTA0, p.lin)


def other_states(name, seed=12):
    """the linearisation states of the same case from another seed"""
    return svr.problem(CASES[name], seed=seed).lin


@functools.lru_cache(maxsize=None)
def mode0():
    """(problem of MODE0 with weight velocities in p.lin, reference without the term, with it)"""
    p = svr.problem(MODE0)
    q = svr.problem(MODE0[:2] + (2,) + MODE0[3:])  # the states a mode would get
    p.lin = q.lin
    base = svr.reference(p)
    return p, base, with_cip(base, p, DELTA0, p.lin)


def st_vmult(p, delta0, blocks, lin=None):
    """the linearised space-time operator with the term weighted by the linearisation (the constrained operator, as the device applies it
    with set_cip(delta0, CIP_WEIGHT_LINEARISATION))"""
    return cref.st_vmult(svr.operator_oracle(p), delta0, cref.LINEARISATION, p.mode, p.Alpha, p.Beta, p.ns, p.nt, blocks,
                         p.lin if lin is None else lin, p.index, p.nc, p.verts, p.mask, p.weak, 0, p.variable_major)


@functools.lru_cache(maxsize=None)
def relaxation():
    """(problem, reference, f, residual norms) of svr.RELAX_SWEEPS sweeps x <- x + omega V (f - A x) from x = 0 on the mesh of svr.RELAX,
    operator and smoother both with the term"""
    p = svr.problem(svr.RELAX, viscosity=svr.RELAX_NU, b_scale=svr.RELAX_B)
    ref = with_cip(svr.reference(p), p, DELTA0, p.lin)
    f = svr.right_hand_side(p)
    x = [np.zeros(n) for n in p.sizes]
    norms = []
    for _ in range(svr.RELAX_SWEEPS):
        Ax = st_vmult(p, DELTA0, x)
        res = [f[i] - Ax[i] for i in range(p.nb)]
        norms.append(float(np.sqrt(sum(np.sum(q * q) for q in res))))
        y = ref.vmult(res)
        x = [x[i] + svr.RELAX_OMEGA * y[i] for i in range(p.nb)]
    return p, ref, f, norms
