#!/usr/bin/env python3
"""What the weak (Nitsche) faces cost (profiles/stokes_q3_weak_faces.txt): time per vmult of the Stokes operator at velocity degree 3
and 2 on N^3 perturbed cells (the mesh of tools/navier_q3_bench.py: distortion 0.1, seed 7) without weak faces and with all six, and
one per-cell Vanka set-up at degree 3 on M^3 cells without and with them.  Degree 2 runs the cell kernel (STFEM_STOKES_CELL=1).

    python tools/stokes_q3_weak_faces_bench.py vmult [N]     median (min .. max) of REPEATS windows of REPS calls after WARMUP calls,
                                                             each window closed by a download (a device synchronise)
    python tools/stokes_q3_weak_faces_bench.py trace [N [degree]]   ten calls of the vmult with faces (degree 3 by default), for
                                                             rocprofv3 --kernel-trace --stats -- python ... (kernel times, its own run)
    python tools/stokes_q3_weak_faces_bench.py setup [M]     StokesPreconditionVanka.for_space, cG(1), FE_Q(2): create, synchronised
    python tools/stokes_q3_weak_faces_bench.py digest        sha256 of degree-2 results with weak faces on seeded inputs (operator,
                                                             Nitsche functional, per-cell Vanka apply, linear and jacobian): two builds compare equal
A package without set_weak_boundaries_space (an earlier build) measures what it has: degree 3 without faces, degree 2 both."""
import hashlib
import importlib
import os
import sys
import time

import numpy as np

os.environ["STFEM_STOKES_CELL"] = "1"  # (read when a context is created)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

WARMUP, REPS, REPEATS = 5, 50, 7
ALL = list(range(6))


def operator(degree, N, faces, dg=False, mask=0):
    nc = (N, N, N)
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=7)
    if degree == 2:
        return stfem.StokesMatrixFreeOperator(nc, vertices=verts, viscosity=0.01, dirichlet_mask=mask, dg_pressure=dg,
                                              weak_boundary_ids=ALL if faces else ())
    op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, vertices=verts, viscosity=0.01, dirichlet_mask=mask, dg_pressure=dg)
    if faces:
        op.set_weak_boundaries_space(ALL)
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


def vmult(N):
    have = hasattr(stfem.StokesMatrixFreeOperator, "set_weak_boundaries_space")
    print(f"median (min .. max) of {REPEATS} windows of {REPS} calls after {WARMUP} warm-up calls, nothing strongly constrained")
    for rnd in range(2):  # the whole list twice: the second round shows the spread between repeats of the same command
        for degree in (3, 2):
            base = None
            for faces in (False, True):
                if degree == 3 and faces and not have:
                    continue
                op = operator(degree, N, faces)
                u, p, du, dp = vectors(op)
                t = timed(lambda: op.vmult(du, dp, u, p), dp.download)
                base = base or t[0]
                line = f"round {rnd} {N}^3 perturbed Q{degree} {'six weak faces' if faces else 'no weak faces '}: vmult {t[0] * 1e3:7.3f} ms ({t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f})"
                if faces:
                    line += f"  faces add {(t[0] - base) * 1e3:6.3f} ms = {(t[0] - base) / base:5.1%} of the vmult without"
                    if hasattr(op, "last_face_plan"):
                        line += f", plan {op.last_face_plan()}"
                print(line, flush=True)


def trace(N, degree):
    op = operator(degree, N, True)
    u, p, du, dp = vectors(op)
    for _ in range(10):
        op.vmult(du, dp, u, p)
    dp.download()


def setup(M):
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 0.05, 1)
    have = hasattr(stfem.StokesMatrixFreeOperator, "set_weak_boundaries_space")
    for rnd in range(2):
        for faces in (False, True):
            if faces and not have:
                continue
            op = operator(3, M, faces, mask=0 if faces else 63)  # (strong walls, or the same walls imposed weakly)
            probe = op.initialize_dof_vector(1)
            probe.download()
            t0 = time.perf_counter()
            V = stfem.StokesPreconditionVanka.for_space(op, [0, 1], Alpha, Beta)
            probe.download()  # (the set-up synchronises after its last batch itself)
            t = time.perf_counter() - t0
            print(f"round {rnd} {M}^3 perturbed Q3/FE_Q2 cG(1) per-cell Vanka set-up {'six weak faces' if faces else 'no weak faces '}: {t:7.3f} s, "
                  f"{V.setup_batches} batches", flush=True)
            del V, op


def digest():
    h = hashlib.sha256()
    for dg in (False, True):
        op = operator(2, 6, True, dg=dg, mask=0b000011)
        u, p, du, dp = vectors(op)
        op.vmult(du, dp, u, p)
        g = np.random.default_rng(5).uniform(-1, 1, (op.face_points().shape[0], 3))
        op.nitsche_rhs(g, du, dp)
        Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 0.05, 1)
        V = stfem.StokesPreconditionVanka.for_space(op, [0, 1], Alpha, Beta)
        V.vmult([u, p], [du, dp])
        for v in (du, dp, u, p):
            h.update(v.download().tobytes())
        J = stfem.StokesPreconditionVanka.for_space(op, [0, 1], Alpha, Beta, lin=[u, None], mode=2)  # the blocks with the inflow term
        J.vmult([du, dp], [u, p])
        for v in (du, dp):
            h.update(v.download().tobytes())
    print("digest", h.hexdigest())


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "vmult"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else {"vmult": 48, "trace": 48, "setup": 32}.get(what, 0)
    degree = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    {"vmult": vmult, "trace": lambda n: trace(n, degree), "setup": setup, "digest": lambda _: digest()}[what](size)
