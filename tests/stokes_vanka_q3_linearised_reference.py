"""Dense numpy restatement of the per-cell Vanka smoother of the LINEARISED Stokes operator at velocity degree 3
(stfem_stokes_vanka_create_linearised_space): tests/stokes_vanka_q3_reference.py::StokesVankaQ3Reference with K of column block j
replaced by K + C(b_j), b_j the linearisation state of that block (reinit_asm, include/stmg.h:929-965; operators.h:835-866).  C(b) is the
dense matrix of the convection term
    form:      C(b)[(i, a), (j, b')] = - int delta_ij phi_b' (b . grad phi_a)
    jacobian:  ... - int b_i phi_b' d_j phi_a
(operators.h:1554-1567), assembled per cell on the unconstrained mesh from the formulas with the tables of tests/navier_q3_reference.py
(Gauss(4)^3 points, Lagrange basis on the Gauss-Lobatto nodes, MappingQ1), b read with the entries on strongly constrained DoFs as 0;
constrained rows and columns are then dropped as for K, the diagonal kept.  Written from the formulas, not from the kernels.  A helper of
tests/test_stokes_vanka_q3_linearised_reference_cpu.py and the GPU tests of the linearised degree-3 smoother, not a test module; it holds
the cases they share, built once per process.  The states are generated as in tests/stokes_vanka_reference.py::problem: a different
b_scale * uniform(-1, 1) per velocity block, seed 11."""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_q3_reference as nq3  # noqa: E402
import stokes_vanka_q3_reference as q3r  # noqa: E402

FORM, JACOBIAN = nq3.FORM, nq3.JACOBIAN
NU, DT, DISTORT, COND_BOUND = q3r.NU, q3r.DT, q3r.DISTORT, q3r.COND_BOUND
SEED, B_SCALE = 11, 1.0
VISIBLE = 1e-4  # the least relative difference of the apply with the mode from the mode-0 apply

# the mesh shapes of q3r.CASES, each with a mode
CASES = {
    "cell_free_dgp": JACOBIAN,
    "cell_free_q2": FORM,
    "pert222_dgp_cg2": JACOBIAN,        # time-major, two states, 404 rows
    "box222_q2_cg2": JACOBIAN,          # a box context without vertices, 438 rows
    "pert222_q2_cg2_freex": FORM,       # unconstrained x faces: b is non-zero on the boundary
    "box122_dgp_2steps": JACOBIAN,      # four blocks, a state per time step
    "box322_q2": JACOBIAN,              # a cell with both x neighbours
    "box223_dgp": FORM,                 # three cell layers
    "box221_q2_dg0": JACOBIAN,
}
RELAX_MODE, RELAX_B = JACOBIAN, 0.5    # on q3r.RELAX with q3r.RELAX_NU, RELAX_OMEGA, RELAX_SWEEPS


def convection_matrix(mode, b, ncell, vertices, dirichlet_mask):
    """C(b) [3 n_u][3 n_u] on the unconstrained mesh; b [3 n_u] is read with its entries on strongly constrained DoFs as 0"""
    assert mode in (FORM, JACOBIAN)
    nc = tuple(ncell)
    n_u = q3r.n_velocity(nc)
    nd = [3 * c + 1 for c in nc]
    nv = [c + 1 for c in nc]
    xq, wq = nq3.gauss01(4)
    pts = np.array([[xq[qa], xq[qb], xq[qc]] for qc in range(4) for qb in range(4) for qa in range(4)])
    wts = np.array([wq[qa] * wq[qb] * wq[qc] for qc in range(4) for qb in range(4) for qa in range(4)])
    phi, dphi = nq3.tables_3d(nq3.gauss_lobatto01(3), pts)      # [q][64], [q][64][3]
    _, dN = nq3.tables_3d(np.array([0.0, 1.0]), pts)            # the trilinear mapping, vertex i + 2 j + 4 k
    B = np.array(b, dtype=np.float64).reshape(3, n_u)
    B[:, q3r.constrained(nc, dirichlet_mask)] = 0.0
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    Cm = np.zeros((3 * n_u, 3 * n_u))
    for cz in range(nc[2]):
        for cy in range(nc[1]):
            for cx in range(nc[0]):
                dofs = np.array([(3 * cx + a) + nd[0] * ((3 * cy + bb) + nd[1] * (3 * cz + c))
                                 for c in range(4) for bb in range(4) for a in range(4)])
                Vc = np.array([V[(cx + i) + nv[0] * ((cy + j) + nv[1] * (cz + k))] for k in range(2) for j in range(2) for i in range(2)])
                J = np.einsum("vd,qve->qde", Vc, dN)             # dx_d / dxi_e
                JxW = np.linalg.det(J) * wts
                grad = np.einsum("qne,qej->qnj", dphi, np.linalg.inv(J))  # d phi_n / dx_j
                bq = np.einsum("in,qn->qi", B[:, dofs], phi)     # b at the points [q][3]
                same = -np.einsum("q,qn,qmj,qj->mn", JxW, phi, grad, bq)  # [row a][column b']
                for i in range(3):
                    gi = i * n_u + dofs
                    Cm[np.ix_(gi, gi)] += same
                    if mode == JACOBIAN:
                        for j in range(3):
                            Cm[np.ix_(gi, j * n_u + dofs)] -= np.einsum("q,q,qn,qm->mn", JxW, bq[:, i], phi, grad[:, :, j])
    return Cm


class StokesVankaQ3LinearisedReference:
    """the blocks of `base` (a StokesVankaQ3Reference of the same problem) with K + C(lin[j]) in column block j; mode 0: base's own"""

    def __init__(self, base, ncell, vertices, dirichlet_mask, mode, lin):
        self.base, self.var, self.cells = base, base.var, base.cells
        nu_, np_ = base.n_u, base.n_p
        nblk = len(self.var)
        states, self.sel = [], [0] * nblk
        if mode:
            for j in range(nblk):
                if self.var[j] != 0:
                    continue
                at = [s for s, b in enumerate(states) if b is lin[j]]
                if not at:
                    states.append(lin[j])
                    at = [len(states) - 1]
                self.sel[j] = at[0]
        cu = base.constrained[:3 * nu_]
        self.K = []
        for b in states:
            Cb = convection_matrix(mode, b, ncell, vertices, dirichlet_mask)
            d = Cb.diagonal().copy()
            Cb[cu, :] = 0.0
            Cb[:, cu] = 0.0
            Cb[cu, cu] = d[cu]
            Kb = base.K.copy()
            Kb[:3 * nu_, :3 * nu_] += Cb
            self.K.append(Kb)
        if not mode:
            self.K = [base.K]
        valu, valp = np.zeros(3 * nu_), np.zeros(np_)
        for iu, ip in self.cells:
            valu[iu] += 1.0
            valp[ip] += 1.0
        self.blocks, self.cond = [], []
        for iu, ip in self.cells:
            idx = [iu, 3 * nu_ + ip]
            val = [valu[iu], valp[ip]]
            size = [len(iu), len(ip)]
            off = np.concatenate([[0], np.cumsum([size[v] for v in self.var])])
            B = np.zeros((off[-1], off[-1]))
            for bi in range(nblk):
                for bj in range(nblk):
                    iv, jv = self.var[bi], self.var[bj]
                    blk = base.Alpha[bi, bj] * self.K[self.sel[bj]][np.ix_(idx[iv], idx[jv])]
                    if iv == 0 and jv == 0:
                        blk = blk + base.Beta[bi, bj] * base.M[np.ix_(iu, iu)]
                    B[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] = val[iv][:, None] * blk
            self.cond.append(np.linalg.cond(B))
            self.blocks.append(np.linalg.inv(B))
        self.rows = int(self.blocks[0].shape[0])
        self.cond_max = max(self.cond)

    vmult = q3r.StokesVankaQ3Reference.vmult


def _stfem():
    return importlib.import_module("dealii-stfem_amd")


def block_index(p):
    stfem = _stfem()
    return lambda it, v, d: stfem.stokes_block_index(p.nt, it, v, d, p.variable_major)


def states(p, b_scale=B_SCALE, seed=SEED):
    """lin in BlockSlice order: a different b_scale * uniform(-1, 1) per velocity block, None for the pressure blocks"""
    index = block_index(p)
    rng = np.random.default_rng(seed)
    lin = [None] * p.nb
    for it in range(p.ns):
        for d in range(p.nt):
            lin[index(it, 0, d)] = b_scale * rng.uniform(-1, 1, 3 * p.n_u)
    return lin


def reference(p, base, mode, lin):
    return StokesVankaQ3LinearisedReference(base, p.nc, p.verts, p.mask, mode, lin)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, mode, states, reference with the mode, the mode-0 reference) of a case of CASES, built once per process"""
    p, base = q3r.case(name)
    mode, lin = CASES[name], states(p)
    return p, mode, lin, reference(p, base, mode, lin), base


def st_vmult(p, mode, lin, blocks):
    """the constrained linearised space-time operator of the problem on host blocks, as the device applies it"""
    out = [np.array(np.ravel(b), dtype=np.float64) for b in q3r.st_vmult(p, blocks)]
    if mode:
        add = nq3.st_convection(3, mode, p.Alpha, p.ns, p.nt, blocks, lin, block_index(p), p.nc, p.verts, p.mask)
        for j, a in enumerate(add):
            if a is not None:
                out[j] += a
    return out


def relaxation_history(p, ref, mode, lin, f, omega, sweeps=q3r.RELAX_SWEEPS):
    """residual norms of x <- x + omega V (f - A(b) x) from x = 0"""
    x = [np.zeros(n) for n in p.sizes]
    norms = []
    for _ in range(sweeps):
        Ax = st_vmult(p, mode, lin, x)
        res = [f[i] - Ax[i] for i in range(p.nb)]
        norms.append(float(np.sqrt(sum(np.sum(q * q) for q in res))))
        y = ref.vmult(res)
        x = [x[i] + omega * y[i] for i in range(p.nb)]
    return norms


@functools.lru_cache(maxsize=None)
def relaxation():
    """(problem, mode, states, reference, f, residual norms) of q3r.RELAX_SWEEPS sweeps with omega = q3r.RELAX_OMEGA on the perturbed
    2 x 2 x 2 mesh, FE_DGP(2), cG(1), viscosity 1, jacobian about 0.5 uniform(-1, 1)"""
    p, base, f, _ = q3r.relaxation()
    lin = states(p, b_scale=RELAX_B)
    ref = reference(p, base, RELAX_MODE, lin)
    return p, RELAX_MODE, lin, ref, f, relaxation_history(p, ref, RELAX_MODE, lin, f, q3r.RELAX_OMEGA)
