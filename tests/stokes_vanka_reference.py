"""Dense numpy restatement of the cell-patch Vanka smoother of the LINEARISED two-variable system, one block per cell (what the
reference's reinit_asm builds, include/stmg.h:929-965, 704-742, compute_block_matrix.h:50-139): the assembled matrix of the whole mesh
column by column - oracle.StokesOracle on the unconstrained mesh plus tests/navier_reference.convection(mode, b, e_j, ...,
dirichlet_mask=0) per distinct linearisation state b (read as the operator reads it: entries on strongly constrained DoFs count as
zero) - then exactly the steps of oracle/vanka_oracle.py::StokesVankaOracle, with the column blocks of source time dof (it, id) taken
from the matrix of b = lin[index(it, 0, id)] (operators.h:835-866).  Written from the formulas, not from the kernels.  A helper of
tests/test_stokes_vanka_reference_cpu.py and tests/test_gpu_stokes_vanka_linearised.py, not a test module; it also holds the cases the
two share, built once per process."""
import functools
import importlib
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402

NU, DT, DISTORT = 0.7, 0.05, 0.15


class StokesVankaReference:
    def __init__(self, ncell, vertices, dirichlet_mask, viscosity, block_variable, Alpha, Beta, mode=0, lin=None, weak_mask=0, outflow_mask=0,
                 penalty1=20.0, penalty2=10.0, dg_pressure=False):
        from oracle import oracle as _o
        self.nc = tuple(ncell)
        self.var = list(block_variable)
        self.Alpha, self.Beta = np.asarray(Alpha, float), np.asarray(Beta, float)
        weak = weak_mask & ~outflow_mask
        free = _o.StokesOracle(self.nc, vertices, 0, viscosity, weak_mask=weak, penalty1=penalty1, penalty2=penalty2, dg_pressure=dg_pressure)
        nu_, np_ = free.n_u, free.n_p
        self.n_u, self.n_p = nu_, np_
        n = 3 * nu_ + np_
        K = np.zeros((n, n))
        M = np.zeros((3 * nu_, 3 * nu_))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            ou, op = free.apply(e[:3 * nu_], e[3 * nu_:], 1.0, 0.0)
            K[:3 * nu_, j], K[3 * nu_:, j] = ou.reshape(-1), op
            if j < 3 * nu_:
                mu, _ = free.apply(e[:3 * nu_], np.zeros(np_), 0.0, 1.0)
                M[:, j] = mu.reshape(-1)
            e[j] = 0.0
        cu = np.tile(nref.constrained(self.nc, dirichlet_mask), 3)
        con = np.concatenate([cu, np.zeros(np_, bool)])
        # the distinct linearisation states of the velocity column blocks, and the assembled matrix of each
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
        else:
            states = [None]
        self.K = []
        for b in states:
            Kb = K.copy()
            if mode:
                bm = np.array(b, dtype=np.float64).reshape(-1)
                bm[cu] = 0.0
                eu = np.zeros(3 * nu_)
                for j in range(3 * nu_):
                    eu[j] = 1.0
                    Kb[:3 * nu_, j] += nref.convection(mode, bm, eu, self.nc, vertices, 0, weak, 0)
                    eu[j] = 0.0
            d = Kb.diagonal().copy()
            Kb[con, :] = 0.0
            Kb[:, con] = 0.0
            Kb[con, con] = d[con]
            self.K.append(Kb)
        d = M.diagonal().copy()
        M[cu, :] = 0.0
        M[:, cu] = 0.0
        M[cu, cu] = d[cu]
        self.M, self.constrained = M, con
        # cell DoF lists per variable and the valences
        ndu = [2 * c + 1 for c in self.nc]
        ndp = [c + 1 for c in self.nc]
        self.cells = []
        valu, valp = np.zeros(3 * nu_), np.zeros(np_)
        cell = 0
        for cz in range(self.nc[2]):
            for cy in range(self.nc[1]):
                for cx in range(self.nc[0]):
                    k, j, i = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
                    iu = ((2 * cx + i) + ndu[0] * ((2 * cy + j) + ndu[1] * (2 * cz + k))).ravel()
                    iu = np.concatenate([c * nu_ + iu for c in range(3)])
                    if dg_pressure:
                        ip = 4 * cell + np.arange(4)
                    else:
                        k, j, i = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
                        ip = ((cx + i) + ndp[0] * ((cy + j) + ndp[1] * (cz + k))).ravel()
                    self.cells.append((iu, ip))
                    valu[iu] += 1.0
                    valp[ip] += 1.0
                    cell += 1
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
                    blk = self.Alpha[bi, bj] * self.K[self.sel[bj]][np.ix_(idx[iv], idx[jv])]
                    if iv == 0 and jv == 0:
                        blk = blk + self.Beta[bi, bj] * M[np.ix_(iu, iu)]
                    B[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] = val[iv][:, None] * blk
            self.cond.append(np.linalg.cond(B))
            self.blocks.append(np.linalg.inv(B))
        self.cond_max = max(self.cond)

    def vmult(self, src_blocks):
        """src_blocks: list of arrays in BlockSlice order (velocity 3 n_u, pressure n_p); returns the same shapes"""
        src = [np.asarray(b, float).reshape(-1) for b in src_blocks]
        dst = [np.zeros_like(b) for b in src]
        for (iu, ip), Binv in zip(self.cells, self.blocks):
            loc = np.concatenate([src[b][iu if v == 0 else ip] for b, v in enumerate(self.var)])
            y = Binv @ loc
            o = 0
            for b, v in enumerate(self.var):
                ii = iu if v == 0 else ip
                dst[b][ii] += y[o:o + len(ii)]
                o += len(ii)
        return dst


# ---- the cases of the GPU test: the smallest shapes that reach every index branch (1 - 4 time dofs, 85 ... 340 rows)
# (mesh, perturbed, mode, FE_DGP pressure, time type (0 cG, 1 dG), degree, time steps at once, dirichlet mask, weak mask, variable-major)
CASES = {
    "box333": ((3, 3, 3), False, 0, False, 0, 1, 1, 63, 0, True),            # all 27 neighbour patterns; equals the class variant
    "pert232": ((2, 3, 2), True, 0, False, 0, 1, 1, 63, 0, True),
    "pert322_jac_weak": ((3, 2, 2), True, 2, False, 0, 2, 1, 63 & ~3, 3, False),  # cG(2), time-major, weak x faces, a b per time dof
    "box223_form_dgp": ((2, 2, 3), False, 1, True, 1, 1, 1, 63, 0, True),
    "box222_jac_dgp_2steps": ((2, 2, 2), False, 2, True, 1, 1, 2, 63, 0, True),  # 8 blocks, 340 rows
    "cell_jac_dgp": ((1, 1, 1), False, 2, True, 0, 1, 1, 0, 0, True),        # one unconstrained cell: the exact inverse
    # the weak-face terms beyond the x faces of pert322_jac_weak: y and z faces, both sides, FE_DGP on a face, every mode on a face
    "pert222_form_dgp_weak_all": ((2, 2, 2), True, 1, True, 0, 1, 1, 0, 63, True),  # all six faces weak, FE_DGP, form
    "pert222_lin_weak_yz": ((2, 2, 2), True, 0, False, 0, 1, 1, 3, 60, True),       # y and z faces weak, no mode, x faces strong
    "pert222_jac_weak_all": ((2, 2, 2), True, 2, False, 0, 1, 1, 0, 63, True),      # all six faces weak, FE_Q, jacobian
}
RELAX = ((3, 3, 2), True, 2, True, 0, 1, 1, 63, 0, True)
RELAX_NU, RELAX_B, RELAX_OMEGA, RELAX_SWEEPS = 1.0, 0.5, 0.5, 8


def _stfem():
    return importlib.import_module("dealii-stfem_amd")


def problem(spec, viscosity=NU, b_scale=1.0, seed=11):
    """everything a case needs but the reference blocks: mesh, block layout, time weights in block order, linearisation states"""
    stfem = _stfem()
    nc, pert, mode, dg, ttype, r, ns, mask, weak, variable_major = spec
    nt = r if ttype == 0 else r + 1
    nb = 2 * nt * ns
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(ttype, r, DT, ns)
    index = lambda it, v, d: stfem.stokes_block_index(nt, it, v, d, variable_major)  # noqa: E731
    perm = [0] * nb  # the matrices of get_fe_time_weights_stokes are in variable-major block order
    var = [0] * nb
    for it in range(ns):
        for v in range(2):
            for d in range(nt):
                perm[index(it, v, d)] = stfem.stokes_block_index(nt, it, v, d, True)
                var[index(it, v, d)] = v
    Alpha, Beta = Alpha[np.ix_(perm, perm)], Beta[np.ix_(perm, perm)]
    verts = nref.perturbed_vertices(nc, DISTORT, 21) if pert else stfem.mesh_vertices(nc)
    n_u = nref.n_velocity(nc)
    n_p = 4 * int(np.prod(nc)) if dg else int(np.prod([c + 1 for c in nc]))
    rng = np.random.default_rng(seed)
    lin = [None] * nb
    if mode:
        for it in range(ns):
            for d in range(nt):
                lin[index(it, 0, d)] = b_scale * rng.uniform(-1, 1, 3 * n_u)  # a different state per time dof
    return types.SimpleNamespace(nc=nc, pert=pert, mode=mode, dg=dg, ns=ns, nt=nt, nb=nb, mask=mask, weak=weak, variable_major=variable_major,
                                 var=var, Alpha=Alpha, Beta=Beta, verts=verts, n_u=n_u, n_p=n_p, lin=lin, nu=viscosity, index=index,
                                 sizes=[3 * n_u if v == 0 else n_p for v in var])


def reference(p, lin=None):
    return StokesVankaReference(p.nc, p.verts, p.mask, p.nu, p.var, p.Alpha, p.Beta, mode=p.mode, lin=p.lin if lin is None else lin,
                                weak_mask=p.weak, dg_pressure=p.dg)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, reference) of a case of CASES, built once per process"""
    p = problem(CASES[name])
    return p, reference(p)


def operator_oracle(p):
    from oracle import oracle as _o
    return _o.StokesOracle(p.nc, p.verts, p.mask, p.nu, weak_mask=p.weak, dg_pressure=p.dg)


def st_vmult(p, blocks, lin=None):
    """the linearised space-time operator of the problem on host blocks (the constrained operator, as the device applies it)"""
    return nref.st_vmult(operator_oracle(p), p.mode, p.Alpha, p.Beta, p.ns, p.nt, blocks, p.lin if lin is None else lin, p.index, p.nc,
                         p.verts, p.mask, p.weak, 0, p.variable_major)


def right_hand_side(p, seed=5):
    """random blocks with zeros in the strongly constrained velocity rows (the operator returns exact zeros there)"""
    rng = np.random.default_rng(seed)
    f = [rng.uniform(-1, 1, n) for n in p.sizes]
    cu = np.tile(nref.constrained(p.nc, p.mask), 3)
    for b, v in enumerate(p.var):
        if v == 0:
            f[b][cu] = 0.0
    return f


@functools.lru_cache(maxsize=None)
def relaxation():
    """(problem, reference, f, residual norms) of RELAX_SWEEPS sweeps x <- x + omega V (f - A_jac x) from x = 0 on the perturbed
    3 x 3 x 2 mesh; viscosity, |b| and omega are chosen so that the history decreases (tests/test_stokes_vanka_reference_cpu.py)"""
    p = problem(RELAX, viscosity=RELAX_NU, b_scale=RELAX_B)
    ref = reference(p)
    f = right_hand_side(p)
    x = [np.zeros(n) for n in p.sizes]
    norms = []
    for _ in range(RELAX_SWEEPS):
        Ax = st_vmult(p, x)
        res = [f[i] - Ax[i] for i in range(p.nb)]
        norms.append(float(np.sqrt(sum(np.sum(q * q) for q in res))))
        y = ref.vmult(res)
        x = [x[i] + RELAX_OMEGA * y[i] for i in range(p.nb)]
    return p, ref, f, norms
