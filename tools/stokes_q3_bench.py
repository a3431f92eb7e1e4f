#!/usr/bin/env python3
"""Time per vmult and per cG(2) st_vmult of the degree-3 Stokes cell kernel (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2),
StokesMatrixFreeOperator.with_degree(3, ...)) on 32^3 and 48^3 cells, both pressure spaces, on a box and on a perturbed mesh; beside
it the FE_Q(2) cell kernel (STFEM_STOKES_CELL=1 keeps it on boxes too) on the same cell counts.

Every figure is the median over REPEATS windows of REPS back-to-back calls, each window between a device synchronise (a download of
one pressure vector), after WARMUP calls of the same shape.  The roofline fraction is by ALGORITHMIC bytes: 16 B (one read, one
write) per unknown of (u, p) per source/destination pair - vmult: one pair, cG(2) st_vmult: two pairs - over the 8.0 TB/s peak of
HBM3E; the vertices, the second read of shared DoFs by neighbouring cells and the read-add-write of the colour launches are the
kernel's own traffic and count against it.  Run with no other GPU work in the same call:
    python tools/stokes_q3_bench.py [cells per direction ...]"""
import importlib
import os
import sys
import time

import numpy as np

os.environ["STFEM_STOKES_CELL"] = "1"  # (read when a context is created: the FE_Q(2) comparison runs the cell kernel on boxes too)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

PEAK = 8.0e12  # B/s
WARMUP, REPS, REPEATS = 5, 50, 7
Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 64, 1)


def measure(degree, N, dg, perturbed):
    nc = (N, N, N)
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=7) if perturbed else None
    op = stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=verts, viscosity=1.0, dg_pressure=dg)
    rng = np.random.default_rng(0)
    var = [0, 0, 1, 1]
    src = [op.initialize_dof_vector(v, rng.uniform(-1, 1, 3 * op.n_velocity if v == 0 else op.n_pressure)) for v in var]
    dst = [op.initialize_dof_vector(v) for v in var]
    unknowns = 3 * op.n_velocity + op.n_pressure

    def timed(f):
        for _ in range(WARMUP):
            f()
        dst[2].download()
        windows = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                f()
            dst[2].download()  # synchronises (and copies one pressure vector: part of every window alike)
            windows.append((time.perf_counter() - t0) / REPS)
        return float(np.median(windows)), float(np.min(windows)), float(np.max(windows))

    tv = timed(lambda: op.vmult(dst[0], dst[2], src[0], src[2]))
    ts = timed(lambda: op.st_vmult(Alpha, Beta, 1, 2, dst, src))
    plan = op.last_cell_plan() if degree == 3 else None
    return unknowns, tv, ts, plan


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [32, 48]
    print(f"median (min .. max) of {REPEATS} windows of {REPS} calls after {WARMUP} warm-up calls; roofline = 16 B x unknowns x pairs / time / 8.0 TB/s")
    for N in sizes:
        for perturbed in (False, True):
            for dg in (False, True):
                for degree in (3, 2):
                    unknowns, tv, ts, plan = measure(degree, N, dg, perturbed)
                    pair = {3: ("FE_DGP2" if dg else "FE_Q2"), 2: ("FE_DGP1" if dg else "FE_Q1")}[degree]
                    line = (f"{N}^3 cells {'perturbed' if perturbed else 'box      '} Q{degree}/{pair:7s} unknowns {unknowns:9d}: "
                            f"vmult {tv[0] * 1e3:7.3f} ms ({tv[1] * 1e3:.3f} .. {tv[2] * 1e3:.3f}) roofline {16 * unknowns / tv[0] / PEAK:6.1%}, "
                            f"cG(2) st_vmult {ts[0] * 1e3:7.3f} ms ({ts[1] * 1e3:.3f} .. {ts[2] * 1e3:.3f}) roofline {32 * unknowns / ts[0] / PEAK:6.1%}")
                    if plan:
                        line += f", plan {plan}"
                    print(line, flush=True)


if __name__ == "__main__":
    main()
