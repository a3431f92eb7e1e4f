#!/usr/bin/env python3
"""What the CIP interior-face term costs (profiles/stokes_q3_cip.txt): time per linear vmult of the Stokes operator at velocity degree
3 and 2 on N^3 cells without the term and with it (delta0 = 1), on the perturbed mesh of tools/navier_q3_bench.py (distortion 0.1,
seed 7: the general kernels) and on the unit box (the CART kernels).  Degree 2 runs the cell kernel (STFEM_STOKES_CELL=1).

    python tools/stokes_q3_cip_bench.py vmult [N [degrees]]  median (min .. max) of REPEATS windows of REPS calls after WARMUP calls,
                                                             each window closed by a download (a device synchronise); degrees: 32, 3 or 2
    python tools/stokes_q3_cip_bench.py trace [N [degree]]   ten calls of the vmult with the term on the perturbed mesh, for
                                                             rocprofv3 --kernel-trace --stats -- python ... (kernel times, its own run)
    python tools/stokes_q3_cip_bench.py digest               sha256 of degree-2 CIP results on seeded inputs - cip_add, the integrated
                                                             entries with both weights, cip_add_slab and the bound ghosts, on a box and on
                                                             a perturbed mesh, one and several sources: two builds compare equal
STFEM_LIB=<an earlier build's library> measures what that build has: degree 2 alone, through the entries of stfem.h."""
import ctypes
import hashlib
import importlib
import os
import sys
import time

import numpy as np

os.environ["STFEM_STOKES_CELL"] = "1"  # (read when a context is created)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")
HAVE = hasattr(ctypes.CDLL(os.environ.get("STFEM_LIB", stfem.LIB_PATH)), "stfem_stokes_set_cip_space")
if not HAVE:
    stfem.CIP_SPACE_SIGNATURES.clear()  # (an earlier build: bind what it exports)

WARMUP, REPS, REPEATS = 5, 50, 7


def operator(degree, N, box, delta0):
    nc = (N, N, N)
    verts = None if box else stfem.mesh_vertices(nc, distort=0.1, seed=7)
    if degree == 2:
        return stfem.StokesMatrixFreeOperator(nc, vertices=verts, viscosity=0.01, dirichlet_mask=0, delta0=delta0)
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=verts, viscosity=0.01, dirichlet_mask=0)
    op.set_cip_space(delta0)
    return op


def vectors(op):
    rng = np.random.default_rng(0)
    u, p = op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)), op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure))
    return u, p, op.initialize_dof_vector(0), op.initialize_dof_vector(1)


def timed(f, sync):
    for _ in range(WARMUP):
        f()
    sync()
    windows = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            f()
        sync()
        windows.append((time.perf_counter() - t0) / REPS)
    return float(np.median(windows)), float(np.min(windows)), float(np.max(windows))


def vmult(N, degrees):
    print(f"median (min .. max) of {REPEATS} windows of {REPS} calls after {WARMUP} warm-up calls, nothing strongly constrained, "
          f"library {'with' if HAVE else 'without'} the _space entries")
    for box in (False, True):
        for degree in (3, 2):
            if degree not in degrees or (degree == 3 and not HAVE):
                continue
            base = None
            for delta0 in (0.0, 1.0):
                op = operator(degree, N, box, delta0)
                u, p, du, dp = vectors(op)
                t = timed(lambda: op.vmult(du, dp, u, p), dp.download)
                base = base or t[0]
                line = f"{N}^3 {'box      ' if box else 'perturbed'} Q{degree} {'with CIP' if delta0 else 'no CIP  '}: vmult {t[0] * 1e3:7.3f} ms ({t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f})"
                if delta0:
                    line += f"  CIP adds {(t[0] - base) * 1e3:6.3f} ms = {(t[0] - base) / base:5.1%} of the vmult without"
                    if HAVE:
                        line += f", plan {op.last_cip_plan()}"
                print(line, flush=True)
                del op, u, p, du, dp


def trace(N, degree):
    op = operator(degree, N, False, 1.0)
    u, p, du, dp = vectors(op)
    for _ in range(10):
        op.vmult(du, dp, u, p)
    dp.download()


def digest():
    """degree 2 through the entries of stfem.h alone, so that a build without the _space entries computes the same"""
    h = hashlib.sha256()
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 16, 1)
    Gamma, Zeta = np.array([0.7, -1.3, 0.4, 0.9]), np.array([0.2, 0.5, 0.0, 0.0])
    for nc, upper, distort in (((4, 3, 2), (1.0, 1.5, 0.6), 0.0), ((3, 2, 4), (1, 1, 1), 0.15), ((7, 6, 5), (1, 1, 1), 0.1)):
        verts = stfem.mesh_vertices(nc, upper=upper, distort=distort, seed=77) if distort else None
        for mask in (0b111011, 0):
            op = stfem.StokesMatrixFreeOperator(nc, vertices=verts, upper=upper, dirichlet_mask=mask, viscosity=0.3)
            rng = np.random.default_rng(3)
            U = [op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)) for _ in range(4)]
            P = [op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure)) for _ in range(2)]
            du = [op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)) for _ in range(2)]
            dp = [op.initialize_dof_vector(1) for _ in range(2)]

            def mark():
                for v in du + dp:
                    h.update(v.download().tobytes())

            op.cip_add(du[0], U[0], U[0], 0.8)   # weight = source
            op.cip_add(du[1], U[0], U[1], 1.7)   # a weight of its own
            mark()
            for weight in (stfem.CIP_WEIGHT_SOURCE, stfem.CIP_WEIGHT_LINEARISATION):
                op.set_cip(1.3, weight)
                op.vmult(du[0], dp[0], U[0], P[0])
                op.vmult(du[1], dp[1], U[1], P[1], lin=U[2], mode=2)
                mark()
                op.st_vmult(Alpha, Beta, 1, 2, du + dp, U[:2] + P)                       # several sources
                mark()
                op.st_vmult(Alpha, Beta, 1, 2, du + dp, U[:2] + P, lin=U[2:4] + [None, None], mode=1)
                mark()
                op.st_vmult_slice_add(Gamma, Zeta, 1, 2, du + dp, U[0], P[0], lin=U[3], mode=2)
                mark()
            # a slab with neighbours on both sides: the ghost planes are the operator's own packed planes, the ghost vertex planes its
            # outer planes moved outwards
            op.set_cip(0.0)
            lower = upper_v = None
            if verts is not None:
                v4 = np.asarray(verts).reshape(nc[2] + 1, nc[1] + 1, nc[0] + 1, 3)
                lower, upper_v = v4[0] - np.array([0, 0, 0.3]), v4[-1] + np.array([0, 0, 0.3])
            op.set_cip_neighbours(48, lower, upper_v)
            ghosts = [[op.cip_ghost_vector(), op.cip_ghost_vector()] for _ in range(2)]
            for s in range(2):
                op.cip_pack(U[s], 1, ghosts[s][0])  # the planes under the top interface stand in for the slab below
                op.cip_pack(U[s], 0, ghosts[s][1])
                op.cip_bind_ghosts(U[s], ghosts[s][0], ghosts[s][1])
            op.cip_add_slab(du[0], U[0], U[1], 0.9, ghosts[0][0], ghosts[0][1])
            mark()
            op.set_cip(1.1)
            op.st_vmult(Alpha, Beta, 1, 2, du + dp, U[:2] + P)  # the bound ghosts, several sources
            mark()
            for s in range(2):
                op.cip_bind_ghosts(U[s], None, None)
            del ghosts
    print("digest", h.hexdigest())


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "vmult"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    third = sys.argv[3] if len(sys.argv) > 3 else ("32" if what == "vmult" else "3")
    {"vmult": lambda n: vmult(n, [int(ch) for ch in third]), "trace": lambda n: trace(n, int(third)), "digest": lambda _: digest()}[what](size)
