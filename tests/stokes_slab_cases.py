"""The Stokes / Navier-Stokes operator on z-slabs of a partitioned mesh: the case table and the cutting / assembling helpers shared by
tests/test_stokes_slab_assembly_cpu.py (the oracle on the slabs, cut and summed, equals the oracle on the whole mesh) and
tests/test_gpu_stokes_slabs.py (the kernels on the slabs against the oracle on the whole mesh).  Plain numpy and the CPU oracle; no
GPU, not a test module.

The contract: a slab is the cell layers [z0, z1) of the global mesh with its own operator; the faces 4 / 5 it shares with a
neighbour are taken out of the strong mask, the weak set and the outflow set (they are no boundary); the operator leaves PARTIAL sums
in the interface planes of every velocity component and of the FE_Q(1) pressure, and the sum over the slabs (the add-exchange) is the
whole-mesh result.  FE_DGP(1) pressure DoFs are cell-local: the slabs' blocks are concatenated.

Layouts: velocity 3 * n_u, component-major, every component lexicographic on the (2 ncell + 1)^3 lattice (x fastest); FE_Q(1) pressure
lexicographic on the (ncell + 1)^3 lattice; FE_DGP(1) pressure 4 per cell, cells lexicographic (z slowest); vertices
[(ncell + 1)^3][3], x fastest."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navier_reference as nref  # noqa: E402

NU, PENALTY1, PENALTY2 = 0.3, 20.0, 10.0

# ncell, distortion of the interior vertices (0: an axis-aligned box, no vertex array handed to the library: Kronecker path), upper corner
MESHES = {
    "pert": ((3, 2, 4), 0.15, (1.0, 1.0, 1.0)),    # general mesh: cell / coupling / boundary kernels in eight colour launches
    "box54": ((5, 4, 4), 0.0, (1.0, 0.75, 1.25)),  # unequal extents
    "box43": ((4, 3, 3), 0.0, (1.25, 1.0, 0.75)),
}
# (strong mask, weak faces, outflow faces), face 2 d + s
MASKS = {
    "strong": (63, (), ()),
    "zweak": (0b001111, (4, 5), ()),             # x / y strong, z faces weak: face 4 on the first slab only, face 5 on the last
    "allweak": (0, (0, 1, 2, 3, 4, 5), ()),      # nothing strong: weak x / y faces cut by every interface
    "mixed": (0b010100, (0, 1, 5), (3,)),        # weak 0, 1, 5, outflow 3, faces 2 and 4 strong
}
# slab bounds in cell layers: two slabs; three with one-layer slabs at both ends and a middle slab holding two interfaces; a one-layer
# middle slab, both of whose DoF planes at the ends are interface planes; a one-layer first slab
BOUNDS = {"pert": ((0, 2, 4), (0, 1, 3, 4), (0, 2, 3, 4)), "box54": ((0, 1, 3, 4), (0, 2, 3, 4)), "box43": ((0, 1, 3),)}
# time schemes: (type, degree, steps at once); None is the plain spatial vmult
SCHEMES = {"cg2": ("cg", 2, 1), "dg2x2": ("dg", 2, 2), "cg3x2": ("cg", 3, 2)}

Case = collections.namedtuple("Case", "mesh bounds masks dg mode scheme variable_major")
Slab = collections.namedtuple("Slab", "z0 z1 ncell vertices lower upper strong weak outflow has_lower has_upper")


def case_id(c):
    return "-".join([c.mesh, "".join(str(b) for b in c.bounds), c.masks, "dgp" if c.dg else "q1", "mode%d" % c.mode] +
                    ([c.scheme, "vm" if c.variable_major else "tm"] if c.scheme else []))


def _table():
    vmult = [Case(mesh, bounds, masks, dg, mode, None, True)
             for mesh in ("pert", "box54", "box43") for bounds in BOUNDS[mesh]
             for masks in MASKS for dg in (False, True) for mode in (0, nref.FORM, nref.JACOBIAN)]
    st = [Case(mesh, bounds, masks, dg, mode, scheme, vm)
          for mesh, bounds, masks in (("pert", (0, 1, 3, 4), "mixed"), ("box43", (0, 1, 3), "zweak"))
          for scheme, vm in (("cg2", True), ("cg2", False), ("dg2x2", True), ("cg3x2", True))
          for dg in (False, True) for mode in (0, nref.JACOBIAN)]
    return vmult, st


VMULT_CASES, ST_CASES = _table()
CASES = VMULT_CASES + ST_CASES


def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


# ---- meshes and slabs

def ncell(case):
    return MESHES[case.mesh][0]


def is_box(case):
    return MESHES[case.mesh][1] == 0.0


@functools.lru_cache(maxsize=None)
def vertices(mesh):
    nc, distort, upper = MESHES[mesh]
    v = nref.perturbed_vertices(nc, distort, 77, (0, 0, 0), upper)
    v.setflags(write=False)
    return v


def face_mask(faces):
    return sum(1 << f for f in faces)


def slab_vertices(verts, nc, z0, z1):
    """the global vertex array cut at the vertex planes [z0 : z1 + 1]"""
    plane = (nc[0] + 1) * (nc[1] + 1)
    return np.ascontiguousarray(np.asarray(verts).reshape(nc[2] + 1, plane, 3)[z0:z1 + 1]).reshape(-1, 3)


def slab_masks(strong, weak, outflow, has_lower, has_upper):
    """(strong, weak, outflow) bit masks of the slab: faces 4 / 5 are cleared from all three wherever the slab has a neighbour"""
    keep = 63 & ~(16 if has_lower else 0) & ~(32 if has_upper else 0)
    return strong & keep, weak & keep, outflow & keep


def global_masks(case):
    strong, weak, outflow = MASKS[case.masks]
    return strong, face_mask(weak), face_mask(outflow)


def slabs(case):
    nc, _, upper = MESHES[case.mesh]
    verts = vertices(case.mesh)
    strong, weak, outflow = global_masks(case)
    out = []
    for r in range(len(case.bounds) - 1):
        z0, z1 = case.bounds[r], case.bounds[r + 1]
        lo, hi = r > 0, r < len(case.bounds) - 2
        s, w, o = slab_masks(strong, weak, outflow, lo, hi)
        out.append(Slab(z0, z1, (nc[0], nc[1], z1 - z0), slab_vertices(verts, nc, z0, z1), (0.0, 0.0, upper[2] * z0 / nc[2]),
                        (upper[0], upper[1], upper[2] * z1 / nc[2]), s, w, o, lo, hi))
    return out


def faces_of(mask):
    return [f for f in range(6) if mask >> f & 1]


# ---- cutting and assembling

def sizes(nc, dg):
    n_u = nref.n_velocity(nc)
    n_p = 4 * nc[0] * nc[1] * nc[2] if dg else (nc[0] + 1) * (nc[1] + 1) * (nc[2] + 1)
    return n_u, n_p


def cut_velocity(x, nc, z0, z1):
    """[3][2 z0 : 2 z1 + 1][plane]"""
    plane = (2 * nc[0] + 1) * (2 * nc[1] + 1)
    return np.asarray(x).reshape(3, 2 * nc[2] + 1, plane)[:, 2 * z0:2 * z1 + 1].reshape(-1).copy()


def cut_q1(x, nc, z0, z1):
    """[z0 : z1 + 1][plane]"""
    plane = (nc[0] + 1) * (nc[1] + 1)
    return np.asarray(x).reshape(nc[2] + 1, plane)[z0:z1 + 1].reshape(-1).copy()


def cut_dgp(x, nc, z0, z1):
    """cells [z0 : z1), z slowest"""
    return np.asarray(x).reshape(nc[2], -1)[z0:z1].reshape(-1).copy()


def cut(x, variable, dg, nc, z0, z1):
    if variable == 0:
        return cut_velocity(x, nc, z0, z1)
    return cut_dgp(x, nc, z0, z1) if dg else cut_q1(x, nc, z0, z1)


def assemble(parts, variable, dg, nc, bounds):
    """the sum of the slabs' results into a whole-mesh array: interface planes receive both sides' partial sums (the add-exchange);
    FE_DGP(1) pressure blocks are concatenated"""
    assert len(parts) == len(bounds) - 1
    if variable == 1 and dg:
        return np.concatenate([np.asarray(p).reshape(-1) for p in parts])
    comps, step = (3, 2) if variable == 0 else (1, 1)
    plane = (step * nc[0] + 1) * (step * nc[1] + 1)
    total = np.zeros((comps, step * nc[2] + 1, plane))
    for r, p in enumerate(parts):
        z0, z1 = bounds[r], bounds[r + 1]
        total[:, step * z0:step * z1 + 1] += np.asarray(p).reshape(comps, step * (z1 - z0) + 1, plane)
    return total.reshape(-1)


def interface_planes(x, variable, dg, nc, bounds):
    """the entries of a whole-mesh array in the interface planes alone (None: FE_DGP(1) pressure has none)"""
    if variable == 1 and dg:
        return None
    comps, step = (3, 2) if variable == 0 else (1, 1)
    plane = (step * nc[0] + 1) * (step * nc[1] + 1)
    return np.asarray(x).reshape(comps, step * nc[2] + 1, plane)[:, [step * z for z in bounds[1:-1]]].reshape(-1).copy()


def slab_interface_planes(x, variable, dg, slab):
    """the entries of a slab array in its own interface planes (first and / or last DoF plane)"""
    if variable == 1 and dg:
        return None
    comps, step = (3, 2) if variable == 0 else (1, 1)
    nc = slab.ncell
    plane = (step * nc[0] + 1) * (step * nc[1] + 1)
    which = ([0] if slab.has_lower else []) + ([step * nc[2]] if slab.has_upper else [])
    return np.asarray(x).reshape(comps, step * nc[2] + 1, plane)[:, which].reshape(-1).copy()


def constrained3(nc, strong):
    """[3 n_u] bool: the strongly constrained velocity DoFs"""
    return np.tile(nref.constrained(nc, strong), 3)


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


# ---- time schemes

def block_index(nt, it, v, d, variable_major=True):
    """BlockSlice::index, two variables"""
    return it * 2 * nt + (v * nt + d if variable_major else d * 2 + v)


def weights(scheme, variable_major=True):
    """(Alpha, Beta, ns, nt, index) of get_fe_time_weights_stokes: the scalar matrices scattered into the (variable, time dof) block
    structure - Alpha everywhere but pressure-pressure, Beta velocity-velocity only"""
    orc = oracle()
    kind, r, ns = SCHEMES[scheme]
    A, B, _, _ = orc.time_weights(orc.CGP if kind == "cg" else orc.DG, r, 1.0 / 16, ns)
    n = A.shape[0]
    nt = n // ns
    index = lambda it, v, d: block_index(nt, it, v, d, variable_major)  # noqa: E731
    Alpha, Beta = np.zeros((2 * n, 2 * n)), np.zeros((2 * n, 2 * n))
    for a in range(n):
        for b in range(n):
            for iv in range(2):
                for jv in range(2):
                    if (iv, jv) != (1, 1):
                        Alpha[index(a // nt, iv, a % nt), index(b // nt, jv, b % nt)] = A[a, b]
            Beta[index(a // nt, 0, a % nt), index(b // nt, 0, b % nt)] = B[a, b]
    return Alpha, Beta, ns, nt, index


def block_variables(ns, nt, index):
    var = [0] * (2 * ns * nt)
    for it in range(ns):
        for d in range(nt):
            var[index(it, 1, d)] = 1
    return var


# ---- data and references: one function for the whole mesh and for a slab

def fields(case, seed=5):
    """whole-mesh random fields in [-1, 1]: (U, P, B) for a spatial case, (blocks, lin, var) in BlockSlice order for a space-time one
    (lin: velocity entries only, not the source)"""
    nc = ncell(case)
    n_u, n_p = sizes(nc, case.dg)
    rng = np.random.default_rng(seed)
    if case.scheme is None:  # (the pressure last: the velocity fields do not depend on the pressure space)
        U, B = rng.uniform(-1, 1, 3 * n_u), rng.uniform(-1, 1, 3 * n_u)
        return U, rng.uniform(-1, 1, n_p), B
    _, _, ns, nt, index = weights(case.scheme, case.variable_major)
    nb = 2 * ns * nt
    blocks, lin = [None] * nb, [None] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[index(it, 0, d)] = rng.uniform(-1, 1, 3 * n_u)
            lin[index(it, 0, d)] = rng.uniform(-1, 1, 3 * n_u)
    for it in range(ns):  # (the pressure after the velocities: the velocity fields do not depend on the pressure space)
        for d in range(nt):
            blocks[index(it, 1, d)] = rng.uniform(-1, 1, n_p)
    return blocks, lin, block_variables(ns, nt, index)


def stokes_oracle(nc, verts, strong, weak, outflow, dg):
    return oracle().StokesOracle(nc, verts, strong, NU, weak_mask=weak & ~outflow, penalty1=PENALTY1, penalty2=PENALTY2, dg_pressure=dg)


def oracle_vmult(nc, verts, strong, weak, outflow, dg, mode, B, U, P):
    """(velocity [3 n_u], pressure): StokesOracle.apply plus the convection term of tests/navier_reference.py for modes 1 / 2"""
    orc = stokes_oracle(nc, verts, strong, weak, outflow, dg)
    ku, kp = nref.vmult(orc, mode, B, U, P, nc, verts, strong, weak & ~outflow, 0)
    return ku.reshape(-1), kp


def oracle_st_vmult(nc, verts, strong, weak, outflow, dg, mode, scheme, variable_major, blocks, lin):
    orc = stokes_oracle(nc, verts, strong, weak, outflow, dg)
    Alpha, Beta, ns, nt, index = weights(scheme, variable_major)
    return nref.st_vmult(orc, mode, Alpha, Beta, ns, nt, blocks, lin, index, nc, verts, strong, weak & ~outflow, 0, variable_major)


@functools.lru_cache(maxsize=None)
def _whole_convection(mesh, masks, mode, lin_is_source):
    """the convection part of a spatial case on the whole mesh: independent of the pressure space, shared among the cases"""
    c = Case(mesh, BOUNDS[mesh][0], masks, False, mode, None, True)
    strong, weak, outflow = global_masks(c)
    U, _, B = fields(c)
    r = nref.convection(mode, U if lin_is_source else B, U, ncell(c), vertices(mesh), strong, weak & ~outflow, 0)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def whole_vmult(mesh, masks, dg, mode, lin_is_source=False):
    """the whole-mesh oracle result of a spatial case (cached: computed once, shared, read-only)"""
    c = Case(mesh, BOUNDS[mesh][0], masks, dg, mode, None, True)
    strong, weak, outflow = global_masks(c)
    U, P, _ = fields(c)
    ku, kp = stokes_oracle(ncell(c), vertices(mesh), strong, weak, outflow, dg).apply(U, P)
    ku = ku.reshape(-1).copy()
    if mode:
        ku += _whole_convection(mesh, masks, mode, lin_is_source)
    ku.setflags(write=False)
    kp.setflags(write=False)
    return ku, kp


@functools.lru_cache(maxsize=None)
def whole_st_vmult(mesh, masks, dg, mode, scheme, variable_major):
    c = Case(mesh, BOUNDS[mesh][0], masks, dg, mode, scheme, variable_major)
    strong, weak, outflow = global_masks(c)
    blocks, lin, _ = fields(c)
    out = oracle_st_vmult(ncell(c), vertices(mesh), strong, weak, outflow, dg, mode, scheme, variable_major, blocks, lin)
    for o in out:
        o.setflags(write=False)
    return tuple(out)


# ---- the Q2 divergence at the operator's Gauss points, cell by cell (StokesMatrixFreeOperator::compute_divergence)

def divergence_cells(u, nc, verts):
    """[n_cells] int_K (div u_h)^2 with the Gauss(3)^3 rule and the trilinear map of the cell's eight vertices, the values of u as
    stored; cells lexicographic.  float64, a loop over the cells with the full 3D tables."""
    xq, wq = nref.gauss01(3)
    pts = np.array([[xq[a], xq[b], xq[c]] for c in range(3) for b in range(3) for a in range(3)])
    wts = np.array([wq[a] * wq[b] * wq[c] for c in range(3) for b in range(3) for a in range(3)])
    _, dphi, _, dN = nref.tables_3d(pts)
    U = np.asarray(u, dtype=np.float64).reshape(3, nref.n_velocity(nc))
    out = np.zeros(nc[0] * nc[1] * nc[2])
    for cz in range(nc[2]):
        for cy in range(nc[1]):
            for cx in range(nc[0]):
                dofs = nref._cell_dofs(nc, cx, cy, cz)
                V = nref._cell_vertices(nc, verts, cx, cy, cz)
                J = np.einsum("vd,qve->qde", V, dN)
                grad = np.einsum("qne,qej->qnj", dphi, np.linalg.inv(J))
                div = np.einsum("in,qni->q", U[:, dofs], grad)
                out[cx + nc[0] * (cy + nc[1] * cz)] = np.sum(div * div * np.linalg.det(J) * wts)
    return out
