"""The weak (Nitsche) faces of the Stokes operator at velocity degree 3 (stfem_stokes_set_weak_boundaries_space,
include/stfem_stokes_boundary_space.h): the cases the CPU and GPU tests share, the consistency identity of the faces, and the dense
numpy restatement of the per-cell Vanka smoother over an operator WITH weak faces - the construction of
tests/stokes_vanka_q3_reference.py::StokesVankaQ3Reference with the assembled matrix taken from
oracle.StokesOracle(..., pu=3, weak_mask=...).  A helper, not a test module; everything is built once per process."""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stokes_vanka_q3_reference as q3r  # noqa: E402

NU, DISTORT, COND_BOUND = q3r.NU, q3r.DISTORT, q3r.COND_BOUND
TOL = 1e-12  # the operator tolerance of tests/test_gpu_stokes_q3.py, rel-L2 per block

# ---- the operator cases: cells, distortion, seed, strong mask, weak mask, viscosity, box (created without vertices)
OPERATOR_CASES = {
    "1x1x1_six_faces": ((1, 1, 1), 0.15, 4, 0, 63, 0.7, False),                 # one cell carrying six faces
    # the y faces weak AND strongly constrained (their DoFs read as 0 and are not written, the face terms reach the others), z natural
    "2x1x2_y_strong": ((2, 1, 2), 0.15, 5, 0b001100, 0b001111, 0.3, False),
    "5x4x3": ((5, 4, 3), 0.15, 77, 63 & ~0b100101, 0b100101, 0.9, False),       # colour populations no multiples of four; cells on 2 or 3 weak faces
    "3x2x2_box": ((3, 2, 2), 0.0, 0, 0, 0b000011, 0.7, True),
}
CAPPED = "5x4x3"
DGP = [False, True]
DGP_IDS = ["FE_Q2", "FE_DGP2"]


def _stfem():
    return importlib.import_module("dealii-stfem_amd")


def vertices_of(nc, distort, seed):
    stfem = _stfem()
    return stfem.mesh_vertices(nc, distort=distort, seed=seed) if distort else stfem.mesh_vertices(nc)


@functools.lru_cache(maxsize=None)
def operator_oracle(name, dgp):
    from oracle import oracle
    nc, distort, seed, mask, weak, nu, _ = OPERATOR_CASES[name]
    return oracle.StokesOracle(nc, vertices_of(nc, distort, seed), mask, nu, pu=3, weak_mask=weak, dg_pressure=dgp)


@functools.lru_cache(maxsize=None)
def operator_reference(name, dgp):
    """one random (u, p) and the oracle's K_S (u, p) with the faces, without them, and M u: computed once and shared"""
    from oracle import oracle
    orc = operator_oracle(name, dgp)
    nc, distort, seed, mask, weak, nu, _ = OPERATOR_CASES[name]
    rng = np.random.default_rng(21)
    U, P = rng.uniform(-1, 1, 3 * orc.n_u), rng.uniform(-1, 1, orc.n_p)
    ku, kp = orc.apply(U, P)
    mu, _ = orc.apply(U, P, 0.0, 1.0)
    cu, cp = oracle.StokesOracle(nc, vertices_of(nc, distort, seed), mask, nu, pu=3, dg_pressure=dgp).apply(U, P)
    res = dict(U=U, P=P, ku=ku.reshape(-1), kp=kp, mu=mu.reshape(-1), cell_u=cu.reshape(-1), cell_p=cp)
    for v in res.values():
        v.setflags(write=False)
    return res


def device_operator(stfem, name, dgp, **faces):
    nc, distort, seed, mask, weak, nu, box = OPERATOR_CASES[name]
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=None if box else vertices_of(nc, distort, seed), dirichlet_mask=mask,
                                                    viscosity=nu, dg_pressure=dgp)
    op.set_weak_boundaries_space([f for f in range(6) if weak >> f & 1], **faces)
    return op


# ---- the consistency identity: an affinely sheared 2 x 1 x 2 mesh, all six faces weak, nothing strongly constrained
IDENTITY_NC, IDENTITY_NU = (2, 1, 2), 0.7
SHEAR = np.array([[1.0, 0.2, 0.1], [0.0, 0.9, 0.15], [0.05, 0.0, 1.1]])
GL3 = np.array([0.0, 0.5 - 0.5 / np.sqrt(5.0), 0.5 + 0.5 / np.sqrt(5.0), 1.0])  # Gauss-Lobatto nodes of FE_Q(3)
GL2 = np.array([0.0, 0.5, 1.0])


def _lattice(nc, nodes):
    """physical coordinates [node][3] of the node lattice (x fastest) of the sheared unit cube"""
    deg = len(nodes) - 1
    axes = [np.array([(c + nodes[a]) / n for c in range(n) for a in range(deg)] + [1.0]) for n in nc]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) @ SHEAR.T


def identity_vertices():
    return np.ascontiguousarray(_stfem().mesh_vertices(IDENTITY_NC).reshape(-1, 3) @ SHEAR.T)


def identity_fields(dgp):
    """u = (y^2, z^2, x^2) at the velocity nodes, p = x + 2 y z at the FE_Q(2) nodes or p = 0 (FE_DGP(2)), f = - nu Laplace u + grad p at
    the velocity nodes; g(points) = u at the face points"""
    X = _lattice(IDENTITY_NC, GL3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    U = np.concatenate([y * y, z * z, x * x])
    if dgp:
        P = np.zeros(10 * int(np.prod(IDENTITY_NC)))
        F = np.concatenate([np.full(x.size, -2.0 * IDENTITY_NU)] * 3)
    else:
        Xp = _lattice(IDENTITY_NC, GL2)
        P = Xp[:, 0] + 2.0 * Xp[:, 1] * Xp[:, 2]
        F = np.concatenate([-2.0 * IDENTITY_NU + np.ones_like(x), -2.0 * IDENTITY_NU + 2.0 * z, -2.0 * IDENTITY_NU + 2.0 * y])
    g = lambda pts: np.stack([pts[:, 1] ** 2, pts[:, 2] ** 2, pts[:, 0] ** 2], axis=1)  # noqa: E731
    return U, P, F, g


@functools.lru_cache(maxsize=None)
def identity_oracle(dgp):
    from oracle import oracle
    return oracle.StokesOracle(IDENTITY_NC, identity_vertices(), 0, IDENTITY_NU, pu=3, weak_mask=63, dg_pressure=dgp)


# ---- the per-cell Vanka smoother over an operator with weak faces
class StokesVankaQ3FacesReference(q3r.StokesVankaQ3Reference):
    """StokesVankaQ3Reference with the Nitsche terms of the weak faces in the assembled matrix; vmult is inherited"""

    def __init__(self, ncell, vertices, dirichlet_mask, viscosity, block_variable, Alpha, Beta, dg_pressure=False, weak_mask=0):
        from oracle import oracle as _o
        self.nc = tuple(ncell)
        self.var = list(block_variable)
        self.Alpha, self.Beta = np.asarray(Alpha, float), np.asarray(Beta, float)
        free = _o.StokesOracle(self.nc, vertices, 0, viscosity, pu=3, weak_mask=weak_mask, dg_pressure=dg_pressure)
        nu_, np_ = free.n_u, free.n_p
        assert (nu_, np_) == (q3r.n_velocity(self.nc), q3r.n_pressure(self.nc, dg_pressure))
        self.n_u, self.n_p = nu_, np_
        n = 3 * nu_ + np_
        K = np.zeros((n, n))
        M = np.zeros((3 * nu_, 3 * nu_))
        e = np.zeros(n)
        zp = np.zeros(np_)
        for j in range(n):
            e[j] = 1.0
            ou, op = free.apply(e[:3 * nu_], e[3 * nu_:], 1.0, 0.0)
            K[:3 * nu_, j], K[3 * nu_:, j] = ou.reshape(-1), op
            if j < 3 * nu_:
                mu, _ = free.apply(e[:3 * nu_], zp, 0.0, 1.0)
                M[:, j] = mu.reshape(-1)
            e[j] = 0.0
        cu = np.tile(q3r.constrained(self.nc, dirichlet_mask), 3)
        con = np.concatenate([cu, np.zeros(np_, bool)])
        d = K.diagonal().copy()
        K[con, :] = 0.0
        K[:, con] = 0.0
        K[con, con] = d[con]
        d = M.diagonal().copy()
        M[cu, :] = 0.0
        M[:, cu] = 0.0
        M[cu, cu] = d[cu]
        self.K, self.M, self.constrained = K, M, con
        ndu = [3 * c + 1 for c in self.nc]
        ndp = [2 * c + 1 for c in self.nc]
        self.cells = []
        valu, valp = np.zeros(3 * nu_), np.zeros(np_)
        cell = 0
        for cz in range(self.nc[2]):
            for cy in range(self.nc[1]):
                for cx in range(self.nc[0]):
                    k, j, i = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
                    iu = ((3 * cx + i) + ndu[0] * ((3 * cy + j) + ndu[1] * (3 * cz + k))).ravel()
                    iu = np.concatenate([c * nu_ + iu for c in range(3)])
                    if dg_pressure:
                        ip = 10 * cell + np.arange(10)
                    else:
                        k, j, i = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
                        ip = ((2 * cx + i) + ndp[0] * ((2 * cy + j) + ndp[1] * (2 * cz + k))).ravel()
                    self.cells.append((iu, ip))
                    valu[iu] += 1.0
                    valp[ip] += 1.0
                    cell += 1
        nblk = len(self.var)
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
                    blk = self.Alpha[bi, bj] * K[np.ix_(idx[iv], idx[jv])]
                    if iv == 0 and jv == 0:
                        blk = blk + self.Beta[bi, bj] * M[np.ix_(iu, iu)]
                    B[off[bi]:off[bi + 1], off[bj]:off[bj + 1]] = val[iv][:, None] * blk
            self.cond.append(np.linalg.cond(B))
            self.blocks.append(np.linalg.inv(B))
        self.rows = int(self.blocks[0].shape[0])
        self.cond_max = max(self.cond)


# name: (spec of tests/stokes_vanka_q3_reference.py - mesh, perturbed, FE_DGP, cG, degree 1, one step, strong mask, variable-major, rows -, weak mask)
VANKA_CASES = {
    "pert222_q2_weak_x-_y-": (((2, 2, 2), True, False, 0, 1, 1, 63 & ~0b000101, True, 219), 0b000101),
    "pert222_dgp_weak_upper": (((2, 2, 2), True, True, 0, 1, 1, 63 & ~0b101010, True, 202), 0b101010),
    "box222_dgp_all_weak": (((2, 2, 2), False, True, 0, 1, 1, 0, True, 202), 63),
    "pert221_q2_z_strong": (((2, 2, 1), True, False, 0, 1, 1, 0b110000, True, 219), 0b001111),
    "box122_q2_weak_x": (((1, 2, 2), False, False, 0, 1, 1, 63 & ~0b000011, True, 219), 0b000011),
}
RELAX = "pert222_dgp_weak_upper"
RELAX_NU, RELAX_OMEGA, RELAX_SWEEPS = q3r.RELAX_NU, q3r.RELAX_OMEGA, q3r.RELAX_SWEEPS


def problem(name, viscosity=NU):
    spec, weak = VANKA_CASES[name]
    p = q3r.problem(spec, viscosity)
    p.weak = weak
    return p


def reference(p):
    return StokesVankaQ3FacesReference(p.nc, p.verts, p.mask, p.nu, p.var, p.Alpha, p.Beta, dg_pressure=p.dg, weak_mask=p.weak)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, reference) of a case of VANKA_CASES, built once per process"""
    p = problem(name)
    return p, reference(p)


def vanka_operator(stfem, p):
    op = stfem.StokesMatrixFreeOperator.with_degree(3, p.nc, vertices=p.verts if p.pert else None, dirichlet_mask=p.mask, viscosity=p.nu,
                                                    dg_pressure=p.dg)
    op.set_weak_boundaries_space([f for f in range(6) if p.weak >> f & 1])
    return op


def st_vmult(p, blocks):
    """the constrained space-time operator with the weak faces on host blocks, as the device applies it"""
    from oracle import oracle as _o
    orc = _o.StokesOracle(p.nc, p.verts, p.mask, p.nu, pu=3, weak_mask=p.weak, dg_pressure=p.dg)
    return orc.st_vmult(p.Alpha, p.Beta, p.ns, p.nt, blocks, variable_major=p.variable_major)


def relaxation_history(p, ref, f, omega, sweeps=RELAX_SWEEPS):
    """residual norms of x <- x + omega V (f - A x) from x = 0"""
    x = [np.zeros(n) for n in p.sizes]
    norms = []
    for _ in range(sweeps):
        Ax = st_vmult(p, x)
        res = [f[i] - np.ravel(Ax[i]) for i in range(p.nb)]
        norms.append(float(np.sqrt(sum(np.sum(q * q) for q in res))))
        y = ref.vmult(res)
        x = [x[i] + omega * y[i] for i in range(p.nb)]
    return norms


@functools.lru_cache(maxsize=None)
def relaxation():
    """(problem, reference, f, residual norms) of RELAX_SWEEPS sweeps with omega = RELAX_OMEGA on the case RELAX at viscosity 1"""
    p = problem(RELAX, viscosity=RELAX_NU)
    ref = reference(p)
    f = q3r.right_hand_side(p)
    return p, ref, f, relaxation_history(p, ref, f, RELAX_OMEGA)
