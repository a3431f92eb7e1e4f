"""Plain numpy restatement of the CIP interior-face term of StokesMatrixFreeOperator (delta0 != 0; reference
include/operators.h:1605-1633 with get_h_face, 182-209) for a velocity of any degree, written independently of the kernels: a loop
over face PAIRS (cell A, its xi_d = 1 side, and the neighbour B in direction d, its xi_d = 0 side) with the full 3D tables of
FE_Q(degree) (tests/navier_q3_reference.py::tables_3d) of both cells at the Gauss(degree + 1)^2 face points, the MappingQ1 Jacobian
from the eight vertices, no sum factorisation.  As in the reference the normal, the face JxW, h_F and the weight velocity are those of
the interior side A; both sides' test functions are integrated (1628-1632).

  C(w; u)(v) = sum_F int_F delta_F(w) [d_n u] . [d_n v] dA,   [d_n u] = (grad u|_A - grad u|_B) n,
  delta_F(w) = delta0 h_F^2 / pa (w.n)^2,  h_F = sqrt(sum_q JxW_face),  pa = degree^3.5

UNPINNED, like tests/cip_reference.py (the closed-form FE_Q(2) restatement): no number held by the reference reaches this term.  It is
held by properties and, at degree 2, by that module (tests/test_cip_q3_reference_cpu.py).  A helper of that module,
tests/test_gpu_stokes_q3_cip.py, tests/test_gpu_guard_bands_stokes_q3_cip.py and tests/test_host_stokes_q3_cip.py, not a test module.
Vectors and vertices as in tests/navier_q3_reference.py."""
import functools
import importlib

import numpy as np

import navier_q3_reference as qref

SOURCE, LINEARISATION = 0, 1
TOL = 1e-12  # rel-L2, the tolerance of the degree-3 operator tests (tests/stokes_q3_faces_reference.py::TOL)

# The meshes of the GPU tests: name -> (ncell, lower, upper, distort); vertex seed 77.  Cartesian ones (distort 0) run without
# vertices on the device.  "box" has three different edge lengths (0.25, 0.5, 0.3).
MESHES = {
    "pair": ((2, 1, 1), (0, 0, 0), (2, 1, 1), 0.0),
    "column": ((1, 1, 3), (0, 0, 0), (1, 1, 1), 0.0),
    "cube": ((2, 2, 2), (0, 0, 0), (1, 1, 1), 0.0),
    "box": ((4, 3, 2), (0, 0, 0), (1.0, 1.5, 0.6), 0.0),
    "pert": ((3, 2, 4), (0, 0, 0), (1, 1, 1), 0.15),
}
MASKS = [63, 0b111011, 0]
VERTEX_SEED, FIELD_SEED, NU = 77, 5, 0.3
# delta0 of every (mesh, mask) the GPU tests use, so that the term alone is at least a tenth of the linear operator's velocity result
# (tests/test_cip_q3_reference_cpu.py::test_gpu_cases_are_not_hollow, the threshold of the degree-2 test): 1 unless listed.  The
# degree-3 term is smaller against nu K u than the degree-2 one (pa = 46.8 against 11.3, and |K u| grows with the degree): with
# delta0 = 1 the one face of 2 x 1 x 1 cells gives 0.06 .. 0.09 of it and 2 x 2 x 2 cells 0.12, the others 0.17 .. 0.8.
DELTA0 = {("pert", 0b111011): 1.5, ("pert", 0): 0.75,  # (not 1: a result that ignored delta0 would pass)
          ("pair", 63): 4.0, ("pair", 0b111011): 4.0, ("pair", 0): 4.0, ("cube", 63): 2.0, ("cube", 0b111011): 2.0, ("cube", 0): 2.0}


def delta0_of(mesh, mask):
    return DELTA0.get((mesh, mask), 1.0)


# delta0 of the several-source cases on the meshes without vertices (tests/test_gpu_stokes_q3_cip.py::test_st_vmult_on_boxes): there
# the term stands beside the mass part of a time step 1 / 16 and, in jacobian mode, beside the convection term, and has to be a tenth
# of each compared block, which that test asserts on the reference values
ST_DELTA0 = {("cube", 63): 8.0, ("cube", 0b111011): 8.0, ("cube", 0): 8.0}  # (2 x 2 x 2: with delta0 = 1 the term is 0.03 .. 0.12 of a block)


def st_delta0_of(mesh, mask):
    return ST_DELTA0.get((mesh, mask), 4.0)


def pa(degree):
    return float(degree) ** 3.5


def mesh_vertices(mesh):
    """the vertices of a mesh of MESHES, from the library's host-side generator (what the device operator of a perturbed mesh gets)"""
    stfem = importlib.import_module("dealii-stfem_amd")
    nc, lower, upper, distort = MESHES[mesh]
    return stfem.mesh_vertices(nc, lower=lower, upper=upper, distort=distort, seed=VERTEX_SEED)


def face_rule(d, side, nq):
    """reference points [nq^2][3] (q = q1 + nq q2, the lower tangential axis fastest) and weights of the face xi_d = side"""
    xq, wq = qref.gauss01(nq)
    t1, t2 = (1 if d == 0 else 0), (1 if d == 2 else 2)
    pts, wts = np.zeros((nq * nq, 3)), np.zeros(nq * nq)
    for q2 in range(nq):
        for q1 in range(nq):
            pts[q1 + nq * q2, d], pts[q1 + nq * q2, t1], pts[q1 + nq * q2, t2] = side, xq[q1], xq[q2]
            wts[q1 + nq * q2] = wq[q1] * wq[q2]
    return pts, wts


def cip(degree, delta0, w, u, ncell, vertices, dirichlet_mask):
    """flat [3 n_u]: v -> C(w; u)(v); entries of u and w on strongly constrained DoFs read as 0, constrained rows receive nothing"""
    nodes, corners = qref.gauss_lobatto01(degree), np.array([0.0, 1.0])
    U, W = qref._read(u, degree, ncell, dirichlet_mask), qref._read(w, degree, ncell, dirichlet_mask)
    out = np.zeros_like(U)
    for d in range(3):
        ptsA, wts = face_rule(d, 1.0, degree + 1)
        ptsB, _ = face_rule(d, 0.0, degree + 1)
        phiA, dphiA = qref.tables_3d(nodes, ptsA)
        _, dphiB = qref.tables_3d(nodes, ptsB)
        _, dNA = qref.tables_3d(corners, ptsA)  # the trilinear mapping, vertex i + 2 j + 4 k
        _, dNB = qref.tables_3d(corners, ptsB)
        for cz in range(ncell[2]):
            for cy in range(ncell[1]):
                for cx in range(ncell[0]):
                    A = [cx, cy, cz]
                    if A[d] == ncell[d] - 1:
                        continue
                    B = list(A)
                    B[d] += 1
                    dofsA, dofsB = qref._cell_dofs(degree, ncell, *A), qref._cell_dofs(degree, ncell, *B)
                    JA = np.einsum("vd,qve->qde", qref._cell_vertices(ncell, vertices, *A), dNA)
                    JB = np.einsum("vd,qve->qde", qref._cell_vertices(ncell, vertices, *B), dNB)
                    JinvA, JinvB = np.linalg.inv(JA), np.linalg.inv(JB)
                    m = JinvA[:, d, :]                                       # J^-T e_d
                    length = np.linalg.norm(m, axis=1)
                    normal = m / length[:, None]
                    JxW = np.abs(np.linalg.det(JA)) * length * wts
                    h2 = JxW.sum()                                           # h_F^2 (get_h_face: area^(1 / (dim - 1)))
                    dnA = np.einsum("qne,qej,qj->qn", dphiA, JinvA, normal)  # d_n phi_n, each side with its own Jacobian
                    dnB = np.einsum("qne,qej,qj->qn", dphiB, JinvB, normal)
                    wn = np.einsum("iq,qi->q", W[:, dofsA] @ phiA.T, normal)
                    delta = delta0 * (h2 / pa(degree)) * wn * wn
                    jump = U[:, dofsA] @ dnA.T - U[:, dofsB] @ dnB.T         # [3][q]
                    out[:, dofsA] += np.einsum("q,iq,qn->in", delta * JxW, jump, dnA)
                    out[:, dofsB] -= np.einsum("q,iq,qn->in", delta * JxW, jump, dnB)
    out[:, qref.constrained(degree, ncell, dirichlet_mask)] = 0.0
    return out.reshape(-1)


def weight_of(weight, mode, b, u):
    """the weight velocity of a source u linearised about b: the linearisation velocity with choice 1 and a mode, else the source"""
    return b if (weight == LINEARISATION and mode and b is not None) else u


def dof_points(degree, ncell, vertices):
    """[n_u][3]: the physical positions of the FE_Q(degree) support points under the trilinear mapping"""
    gl = qref.gauss_lobatto01(degree)
    ref = np.array([[gl[a], gl[b], gl[c]] for c in range(degree + 1) for b in range(degree + 1) for a in range(degree + 1)])
    N, _ = qref.tables_3d(np.array([0.0, 1.0]), ref)
    X = np.zeros((qref.n_velocity(degree, ncell), 3))
    for cz in range(ncell[2]):
        for cy in range(ncell[1]):
            for cx in range(ncell[0]):
                X[qref._cell_dofs(degree, ncell, cx, cy, cz)] = N @ qref._cell_vertices(ncell, vertices, cx, cy, cz)
    return X


# ---- what the GPU tests share: per (mesh, mask) one random (u, p, w) and the term, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def fields(mesh, n=4):
    """n random velocity fields of the mesh at degree 3 (read-only)"""
    nc = MESHES[mesh][0]
    rng = np.random.default_rng(FIELD_SEED)
    out = [rng.uniform(-1, 1, 3 * qref.n_velocity(3, nc)) for _ in range(n)]
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def term(mesh, mask, iw, iu):
    """C(fields[iw]; fields[iu]) at degree 3 with delta0 = 1 (the term is linear in delta0), read-only"""
    nc = MESHES[mesh][0]
    f = fields(mesh)
    c = cip(3, 1.0, f[iw], f[iu], nc, mesh_vertices(mesh), mask)
    c.setflags(write=False)
    return c


def device_operator(stfem, mesh, mask, dgp=False, degree=3):
    nc, lower, upper, distort = MESHES[mesh]
    return stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=mesh_vertices(mesh) if distort else None, lower=lower, upper=upper,
                                                      dirichlet_mask=mask, viscosity=NU, dg_pressure=dgp)
