"""The Stokes / Navier-Stokes operator at velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), stfem_stokes_create_space) on z-slabs of a
partitioned mesh: the case table and the cutting / assembling helpers shared by tests/test_stokes_q3_slab_assembly_cpu.py (the
references on the slabs, cut and summed, equal the references on the whole mesh) and tests/test_gpu_stokes_q3_slabs.py (the kernels on
the slabs against the references on the whole mesh).  The degree-3 counterpart of tests/stokes_slab_cases.py, whose degree-independent
parts (Case, Slab, the slab masks and vertices, the time schemes, rel) are imported.  Plain numpy and the CPU oracle; no GPU, not a
test module.

The contract: a slab is the cell layers [z0, z1) of the global mesh with its own operator; the faces 4 / 5 it shares with a
neighbour are taken out of the strong mask, the weak set and the outflow set (they are no boundary); the operator leaves PARTIAL sums
in the interface planes of every velocity component and of the FE_Q(2) pressure, and the sum over the slabs (the add-exchange) is the
whole-mesh result.  FE_DGP(2) pressure DoFs are cell-local: the slabs' blocks are concatenated.  The CIP term of a slab has no
interface faces (stfem_stokes_set_cip_neighbours refuses degree 3): the slabs' sum lacks exactly those faces.

Layouts: velocity 3 * n_u, component-major, every component lexicographic on the (3 ncell + 1)^3 lattice (x fastest), slab rows
3 z0 : 3 z1 + 1; FE_Q(2) pressure lexicographic on the (2 ncell + 1)^3 lattice, slab rows 2 z0 : 2 z1 + 1; FE_DGP(2) pressure 10 per
cell, cells lexicographic (z slowest); vertices [(ncell + 1)^3][3], x fastest.

Expected values: the linear operator is oracle.StokesOracle at pu = 3, the convection modes tests/navier_q3_reference.py, the
divergence tests/stokes_pressure_q3_reference.py, the CIP term tests/cip_q3_reference.py - all on the WHOLE mesh."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_q3_reference as c3  # noqa: E402
import navier_q3_reference as q3  # noqa: E402
import navier_reference as nref  # noqa: E402
import stokes_pressure_q3_reference as p3  # noqa: E402
from stokes_slab_cases import (NU, PENALTY1, PENALTY2, SCHEMES, Case, Slab, block_index, block_variables, face_mask,  # noqa: E402,F401
                               faces_of, oracle, rel, slab_masks, slab_vertices, weights)

DEGREE = 3
# With NU = 0.3 and a linearisation velocity in [-1, 1] the convection term is 0.03 .. 0.08 of the velocity result of a spatial case and
# less beside the mass part of a time step: a result without the term would nearly pass.  The cases with a convection mode therefore
# run with the viscosity NU_MODES and a linearisation velocity LIN_SCALE * uniform(-1, 1), so that the term is at least a tenth of every
# velocity block (tests/test_stokes_q3_slab_assembly_cpu.py asserts it on the reference values; the threshold and the remedy of
# tests/test_gpu_navier_q3.py).  With 0.03 and 4 the lowest share is 0.31 over the spatial cases (lin = source included, which the
# scale does not reach) and 0.24 over the velocity blocks of the space-time cases; with 0.03 and 1 the latter is 0.06.
NU_MODES, LIN_SCALE = 0.03, 4.0
VELOCITY_STEP, PRESSURE_STEP, DGP_PER_CELL = 3, 2, 10  # DoF planes per cell layer; FE_DGP(2) DoFs of a cell
FORM, JACOBIAN = q3.FORM, q3.JACOBIAN

# ncell, distortion of the interior vertices (0: an axis-aligned box, created WITHOUT vertices from the slab's lower / upper: the
# constant-Jacobian instantiation), upper corner.  The smallest meshes that still hold two interfaces and a one-layer slab
MESHES = {
    "pert": ((3, 2, 4), 0.15, (1.0, 1.0, 1.0)),
    "box": ((2, 3, 3), 0.0, (1.25, 1.0, 0.75)),
}
VERTEX_SEED = 77
# (strong mask, weak faces, outflow faces), face 2 d + s: the four of the degree-2 table and two without any weak face
MASKS = {
    "strong": (63, (), ()),
    "zweak": (0b001111, (4, 5), ()),             # x / y strong, z faces weak: face 4 on the first slab only, face 5 on the last
    "allweak": (0, (0, 1, 2, 3, 4, 5), ()),      # nothing strong: weak x / y faces cut by every interface
    "mixed": (0b010100, (0, 1, 5), (3,)),        # weak 0, 1, 5, outflow 3, faces 2 and 4 strong
    "znatural": (0b001111, (), ()),              # x / y strong, the z faces natural: no slab has a constrained z plane
    "free": (0, (), ()),                         # nothing strong, nothing weak
}
# A degree-3 context with weak faces refuses a convection mode (the inflow term of the faces is not built there: stokes_refuse_inflow_q3),
# so the modes run on the masks without a weak face only
MODE_MASKS = ("strong", "znatural", "free")
# slab bounds in cell layers: two slabs; three with one-layer slabs at both ends and a middle slab holding two interfaces; a one-layer
# middle slab, whose first and last velocity planes are both interface planes; a one-layer first slab
BOUNDS = {"pert": ((0, 2, 4), (0, 1, 3, 4), (0, 2, 3, 4)), "box": ((0, 1, 3),)}


def case_id(c):
    return "-".join([c.mesh, "".join(str(b) for b in c.bounds), c.masks, "dgp" if c.dg else "q2", "mode%d" % c.mode] +
                    ([c.scheme, "vm" if c.variable_major else "tm"] if c.scheme else []))


def _table():
    everywhere = [(mesh, bounds) for mesh in MESHES for bounds in BOUNDS[mesh]]
    vmult = [Case(mesh, bounds, masks, dg, 0, None, True) for mesh, bounds in everywhere for masks in MASKS for dg in (False, True)]
    vmult += [Case(mesh, bounds, masks, False, mode, None, True)
              for mesh, bounds in everywhere for masks in ("strong", "znatural") for mode in (FORM, JACOBIAN)]
    vmult += [Case("pert", (0, 1, 3, 4), "free", True, FORM, None, True), Case("box", (0, 1, 3), "free", True, JACOBIAN, None, True)]
    st = [Case(mesh, bounds, masks, dg, 0, scheme, vm)
          for mesh, bounds, masks in (("pert", (0, 1, 3, 4), "mixed"), ("box", (0, 1, 3), "zweak"))
          for scheme, vm in (("cg2", True), ("cg2", False), ("dg2x2", True)) for dg in (False, True)]
    st += [Case("pert", (0, 1, 3, 4), "znatural", dg, JACOBIAN, scheme, True) for scheme in ("cg2", "dg2x2") for dg in (False, True)]
    return vmult, st


VMULT_CASES, ST_CASES = _table()
CASES = VMULT_CASES + ST_CASES
assert all(c.masks in MODE_MASKS for c in CASES if c.mode)
# the device exchange runs on four of the space-time cases: both pressure spaces, both meshes, both orderings, one in jacobian mode
EXCHANGE_CASES = [Case("pert", (0, 1, 3, 4), "mixed", False, 0, "cg2", True), Case("pert", (0, 1, 3, 4), "mixed", True, 0, "dg2x2", True),
                  Case("box", (0, 1, 3), "zweak", False, 0, "cg2", False), Case("pert", (0, 1, 3, 4), "znatural", False, JACOBIAN, "dg2x2", True)]
assert all(c in ST_CASES for c in EXCHANGE_CASES)
# the CIP term without the interface faces: nothing strong, so every DoF of the two cell layers at an interface receives the faces' part
CIP_CASES = [Case("pert", bounds, "free", False, 0, None, True) for bounds in ((0, 2, 4), (0, 1, 3, 4))]
CIP_DELTA0 = c3.delta0_of("pert", 0)


# ---- meshes and slabs

def ncell(case):
    return MESHES[case.mesh][0]


def is_box(case):
    return MESHES[case.mesh][1] == 0.0


@functools.lru_cache(maxsize=None)
def vertices(mesh):
    """the generator of the degree-2 table: a structured grid, the interior vertices moved by up to distort * h per direction"""
    nc, distort, upper = MESHES[mesh]
    v = nref.perturbed_vertices(nc, distort, VERTEX_SEED, (0, 0, 0), upper)
    v.setflags(write=False)
    return v


def global_masks(case):
    strong, weak, outflow = MASKS[case.masks]
    return strong, face_mask(weak), face_mask(outflow)


def slabs(case):
    """the slabs of a case with the mask rule of slab_masks: faces 4 / 5 are cleared from the strong, weak and outflow sets wherever a
    neighbour exists"""
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


# ---- cutting and assembling

def sizes(nc, dg):
    return q3.n_velocity(DEGREE, nc), p3.n_pressure(DEGREE - 1, nc, dg)


def _shape(variable, nc):
    """(components, DoF planes per cell layer, DoFs of a plane) of a continuous block"""
    comps, step = (3, VELOCITY_STEP) if variable == 0 else (1, PRESSURE_STEP)
    return comps, step, (step * nc[0] + 1) * (step * nc[1] + 1)


def cut_velocity(x, nc, z0, z1):
    """[3][3 z0 : 3 z1 + 1][plane]"""
    comps, step, plane = _shape(0, nc)
    return np.asarray(x).reshape(comps, step * nc[2] + 1, plane)[:, step * z0:step * z1 + 1].reshape(-1).copy()


def cut_q2(x, nc, z0, z1):
    """[2 z0 : 2 z1 + 1][plane]"""
    _, step, plane = _shape(1, nc)
    return np.asarray(x).reshape(step * nc[2] + 1, plane)[step * z0:step * z1 + 1].reshape(-1).copy()


def cut_dgp(x, nc, z0, z1):
    """cells [z0 : z1), z slowest, ten DoFs each"""
    return np.asarray(x).reshape(nc[2], nc[0] * nc[1] * DGP_PER_CELL)[z0:z1].reshape(-1).copy()


def cut(x, variable, dg, nc, z0, z1):
    if variable == 0:
        return cut_velocity(x, nc, z0, z1)
    return cut_dgp(x, nc, z0, z1) if dg else cut_q2(x, nc, z0, z1)


def assemble(parts, variable, dg, nc, bounds):
    """the sum of the slabs' results into a whole-mesh array: interface planes receive both sides' partial sums (the add-exchange);
    FE_DGP(2) pressure blocks are concatenated"""
    assert len(parts) == len(bounds) - 1
    if variable == 1 and dg:
        return np.concatenate([np.asarray(p).reshape(-1) for p in parts])
    comps, step, plane = _shape(variable, nc)
    total = np.zeros((comps, step * nc[2] + 1, plane))
    for r, p in enumerate(parts):
        z0, z1 = bounds[r], bounds[r + 1]
        total[:, step * z0:step * z1 + 1] += np.asarray(p).reshape(comps, step * (z1 - z0) + 1, plane)
    return total.reshape(-1)


def interface_planes(x, variable, dg, nc, bounds):
    """the entries of a whole-mesh array in the interface planes alone (None: FE_DGP(2) pressure has none)"""
    if variable == 1 and dg:
        return None
    comps, step, plane = _shape(variable, nc)
    return np.asarray(x).reshape(comps, step * nc[2] + 1, plane)[:, [step * z for z in bounds[1:-1]]].reshape(-1).copy()


def slab_interface_planes(x, variable, dg, slab):
    """the entries of a slab array in its own interface planes (first and / or last DoF plane)"""
    if variable == 1 and dg:
        return None
    nc = slab.ncell
    comps, step, plane = _shape(variable, nc)
    which = ([0] if slab.has_lower else []) + ([step * nc[2]] if slab.has_upper else [])
    return np.asarray(x).reshape(comps, step * nc[2] + 1, plane)[:, which].reshape(-1).copy()


def constrained3(nc, strong):
    """[3 n_u] bool: the strongly constrained velocity DoFs"""
    return np.tile(q3.constrained(DEGREE, nc, strong), 3)


def interface_layers(nc, bounds):
    """[3 n_u] bool: the velocity DoFs of the two cell layers that touch an interface - where the CIP term of the whole mesh and the sum
    of the slabs' terms may differ (the interface faces couple exactly the DoFs of their two cells)"""
    comps, step, plane = _shape(0, nc)
    m = np.zeros((comps, step * nc[2] + 1, plane), dtype=bool)
    for z in bounds[1:-1]:
        m[:, step * (z - 1):step * (z + 1) + 1] = True
    return m.reshape(-1)


# ---- data and references: one function for the whole mesh and for a slab

def fields(case, seed=5):
    """whole-mesh random fields in [-1, 1]: (U, P, B) for a spatial case, (blocks, lin, var) in BlockSlice order for a space-time one
    (lin: velocity entries only, not the source)"""
    nc = ncell(case)
    n_u, n_p = sizes(nc, case.dg)
    rng = np.random.default_rng(seed)
    if case.scheme is None:  # (the pressure last: the velocity fields do not depend on the pressure space)
        U, B = rng.uniform(-1, 1, 3 * n_u), LIN_SCALE * rng.uniform(-1, 1, 3 * n_u)
        return U, rng.uniform(-1, 1, n_p), B
    _, _, ns, nt, index = weights(case.scheme, case.variable_major)
    nb = 2 * ns * nt
    blocks, lin = [None] * nb, [None] * nb
    for it in range(ns):
        for d in range(nt):
            blocks[index(it, 0, d)] = rng.uniform(-1, 1, 3 * n_u)
            lin[index(it, 0, d)] = LIN_SCALE * rng.uniform(-1, 1, 3 * n_u)
    for it in range(ns):  # (the pressure after the velocities: the velocity fields do not depend on the pressure space)
        for d in range(nt):
            blocks[index(it, 1, d)] = rng.uniform(-1, 1, n_p)
    return blocks, lin, block_variables(ns, nt, index)


def viscosity(mode):
    return NU_MODES if mode else NU


def stokes_oracle(nc, verts, strong, weak, outflow, dg, mode=0):
    return oracle().StokesOracle(nc, verts, strong, viscosity(mode), pu=DEGREE, weak_mask=weak & ~outflow, penalty1=PENALTY1, penalty2=PENALTY2,
                                 dg_pressure=dg)


def convection(mode, B, U, nc, verts, strong, weak, outflow):
    assert not weak & ~outflow  # (no restatement of the inflow term at degree 3: the library refuses the combination)
    return q3.convection(DEGREE, mode, B, U, nc, verts, strong)


def oracle_vmult(nc, verts, strong, weak, outflow, dg, mode, B, U, P):
    """(velocity [3 n_u], pressure): StokesOracle.apply plus the convection term of tests/navier_q3_reference.py for modes 1 / 2"""
    ku, kp = stokes_oracle(nc, verts, strong, weak, outflow, dg, mode).apply(U, P)
    ku = ku.reshape(-1).copy()
    if mode:
        ku += convection(mode, B, U, nc, verts, strong, weak, outflow)
    return ku, kp


def oracle_st_vmult(nc, verts, strong, weak, outflow, dg, mode, scheme, variable_major, blocks, lin):
    Alpha, Beta, ns, nt, index = weights(scheme, variable_major)
    dst = stokes_oracle(nc, verts, strong, weak, outflow, dg, mode).st_vmult(Alpha, Beta, ns, nt, blocks, variable_major)
    if mode:
        assert not weak & ~outflow
        add = q3.st_convection(DEGREE, mode, Alpha, ns, nt, blocks, lin, index, nc, verts, strong)
        dst = [d if a is None else d + a for d, a in zip(dst, add)]
    return dst


def _spatial(mesh, masks, dg=False, mode=0):
    return Case(mesh, BOUNDS[mesh][0], masks, dg, mode, None, True)


@functools.lru_cache(maxsize=None)
def whole_convection(mesh, masks, mode, lin_is_source=False):
    """the convection part of a spatial case on the whole mesh: independent of the pressure space, shared among the cases"""
    c = _spatial(mesh, masks)
    U, _, B = fields(c)
    r = convection(mode, U if lin_is_source else B, U, ncell(c), vertices(mesh), *global_masks(c))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def whole_linear(mesh, masks, dg, faces=True, mode=0):
    """the linear operator of a spatial case on the whole mesh, with the viscosity of `mode`; faces=False: its cell part alone (the same
    strong mask, no weak face)"""
    c = _spatial(mesh, masks, dg)
    strong, weak, outflow = global_masks(c)
    U, P, _ = fields(c)
    ku, kp = stokes_oracle(ncell(c), vertices(mesh), strong, weak if faces else 0, outflow, dg, mode).apply(U, P)
    ku = ku.reshape(-1).copy()
    ku.setflags(write=False)
    kp.setflags(write=False)
    return ku, kp


@functools.lru_cache(maxsize=None)
def whole_vmult(mesh, masks, dg, mode, lin_is_source=False):
    """the whole-mesh result of a spatial case (cached: computed once, shared, read-only)"""
    ku, kp = whole_linear(mesh, masks, dg, True, mode)
    if mode:
        ku = ku + whole_convection(mesh, masks, mode, lin_is_source)
        ku.setflags(write=False)
    return ku, kp


@functools.lru_cache(maxsize=None)
def whole_mass(mesh, masks):
    """M u of the spatial case's velocity: the vector mass with the strong mask (no viscosity in it)"""
    c = _spatial(mesh, masks)
    strong, weak, outflow = global_masks(c)
    U, P, _ = fields(c)
    mu, _ = stokes_oracle(ncell(c), vertices(mesh), strong, weak, outflow, False).apply(U, P, 0.0, 1.0)
    mu = mu.reshape(-1).copy()
    mu.setflags(write=False)
    return mu


@functools.lru_cache(maxsize=None)
def whole_st_vmult(mesh, masks, dg, mode, scheme, variable_major):
    c = Case(mesh, BOUNDS[mesh][0], masks, dg, mode, scheme, variable_major)
    strong, weak, outflow = global_masks(c)
    blocks, lin, _ = fields(c)
    out = oracle_st_vmult(ncell(c), vertices(mesh), strong, weak, outflow, dg, mode, scheme, variable_major, blocks, lin)
    for o in out:
        o.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def whole_divergence(mesh):
    """([n_cells] int_K (div u_h)^2, sqrt of their sum) of the spatial case's velocity, read plain"""
    U, _, _ = fields(_spatial(mesh, "strong"))
    cells, total = p3.divergence_cells(DEGREE, U, MESHES[mesh][0], vertices(mesh))
    cells.setflags(write=False)
    return cells, total


def cip(delta0, W, U, nc, verts, strong):
    return c3.cip(DEGREE, delta0, W, U, nc, verts, strong)


@functools.lru_cache(maxsize=None)
def whole_cip(mesh, masks):
    """delta0 C(u; u) of the spatial case's velocity on the whole mesh, CIP_DELTA0"""
    c = _spatial(mesh, masks)
    U, _, _ = fields(c)
    r = cip(CIP_DELTA0, U, U, ncell(c), vertices(mesh), global_masks(c)[0])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def slab_cips(case):
    """the same term on every slab's own mesh - what a slab's operator computes: no interface face"""
    U, _, _ = fields(case)
    out = []
    for s in slabs(case):
        r = cip(CIP_DELTA0, *(cut_velocity(U, ncell(case), s.z0, s.z1),) * 2, s.ncell, s.vertices, s.strong)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


# ---- the entry points besides vmult / st_vmult
# st_vmult_slice_add, st_Tvmult and mass_vmult: two meshes with weak faces, both pressure spaces; slice_add also in jacobian mode
OTHER_CASES = [Case("pert", (0, 1, 3, 4), "mixed", dg, 0, None, True) for dg in (False, True)] + \
              [Case("box", (0, 1, 3), "allweak", dg, 0, None, True) for dg in (False, True)]
SLICE_ADD_CASES = OTHER_CASES + [Case("pert", (0, 1, 3, 4), "znatural", False, JACOBIAN, None, True)]
# the Nitsche functional: the middle slab of the z-weak mask holds no weak face at all
NITSCHE_CASES = [Case("pert", (0, 1, 3, 4), masks, dg, 0, None, True) for masks in ("mixed", "allweak", "zweak") for dg in (False, True)] + \
                [Case("box", (0, 1, 3), "zweak", False, 0, None, True)]
DIVERGENCE_CASES = [Case("pert", (0, 1, 3, 4), "mixed", False, 0, None, True), Case("box", (0, 1, 3), "allweak", False, 0, None, True)]


def dirichlet(pts):
    """the Dirichlet function of the Nitsche functional at the face points [n][3]"""
    return np.stack([np.sin(pts[:, 0] + 2 * pts[:, 1]), pts[:, 2] ** 2 - pts[:, 0], np.cos(pts[:, 1] * pts[:, 2])], axis=1)


def oracle_nitsche(nc, verts, strong, weak, outflow, dg):
    """(face points, velocity [3 n_u], pressure) of the functional of dirichlet() on a mesh"""
    orc = stokes_oracle(nc, verts, strong, weak, outflow, dg)
    pts = orc.face_points()
    if not len(pts):  # no weak face: no Dirichlet function, nothing is added
        return pts, np.zeros(3 * orc.n_u), np.zeros(orc.n_p)
    ru, rp = orc.nitsche_rhs(dirichlet(pts))
    return pts, ru.reshape(-1), rp


@functools.lru_cache(maxsize=None)
def whole_nitsche(mesh, masks, dg):
    c = _spatial(mesh, masks, dg)
    out = oracle_nitsche(ncell(c), vertices(mesh), *global_masks(c), dg)
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def whole_st_Tvmult(mesh, masks, dg):
    """SystemMatrixStokes::Tvmult as the reference has it, cG(2), one step (with two steps the row sums of the second step's velocity
    rows vanish analytically and the block is a rounding residue, which no relative bound can be held against)"""
    c = Case(mesh, BOUNDS[mesh][0], masks, dg, 0, "cg2", True)
    blocks, _, _ = fields(c)
    Alpha, Beta, ns, nt, _ = weights("cg2")
    out = stokes_oracle(ncell(c), vertices(mesh), *global_masks(c), dg).st_Tvmult(Alpha, Beta, ns, nt, blocks)
    for o in out:
        o.setflags(write=False)
    return tuple(out)
