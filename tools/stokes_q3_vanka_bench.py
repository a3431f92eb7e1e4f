#!/usr/bin/env python3
"""Set-up and apply time of the per-cell Stokes Vanka smoother at velocity degree 3 (StokesPreconditionVanka.for_space over
StokesMatrixFreeOperator.with_degree(3, ...): FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), cG(2): 4 blocks, 438 / 404 rows per cell) on 16^3 and
24^3 box cells, both pressure spaces; beside it, in the same process on the same board, the degree-2 per-cell smoother through the same
entry (FE_Q(2)^3 x FE_Q(1), cG(1): 2 blocks, 89 rows, 32^3 cells - the configuration of profiles/stokes_vanka_percell.txt).

Set-up: host clock around the constructor (it ends in a device synchronise per batch of cell layers) and around two update(None)
calls, which stage the same set-up into the existing storage.  Apply: step = the streaming kernel + the collecting launch; the
median over ROUNDS alternating rounds - every configuration once per round - of one window of back-to-back steps ended by a
blocking download of one pressure vector, after a warm-up window of each.  A window lasts about WINDOW seconds: each configuration
takes as many steps per window as its warm-up window says that needs (at least MIN_REPS), so the small degree-2 configuration is
timed over as long a stretch of host clock as the large ones.  The roofline fraction is by BLOCK bytes: kpad x mpad x 8 B
per cell, read once per step, over the 8.0 TB/s peak of HBM3E; the gather, the rows written to the scratch array and the collecting
launch are the step's own traffic and count against it.  Run with no other GPU work in the same call:
    python tools/stokes_q3_vanka_bench.py [cells per direction at degree 3 ...]"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

PEAK = 8.0e12  # B/s
MIN_REPS, ROUNDS, WINDOW = 20, 5, 0.25  # WINDOW: seconds


class Config:
    def __init__(self, degree, N, dg, r):
        self.degree, self.N, self.dg, self.r = degree, N, dg, r
        nc = (N, N, N)
        self.op = stfem.StokesMatrixFreeOperator.with_degree(degree, nc, viscosity=1.0, dg_pressure=dg)
        Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, r, 1.0 / 64, 1)
        self.var = [0] * r + [1] * r
        npl = {2: (8, 4), 3: (27, 10)}[degree][1 if dg else 0]
        self.m = r * (3 * (degree + 1) ** 3 + npl)
        self.block_bytes = 8 * (4 * ((self.m + 3) // 4)) * (16 * ((self.m + 15) // 16)) * N ** 3  # kpad x mpad doubles per cell
        pair = {3: ("FE_DGP2" if dg else "FE_Q2"), 2: ("FE_DGP1" if dg else "FE_Q1")}[degree]
        self.name = f"Q{degree}/{pair:7s} cG({r}) {self.m:3d} rows {N}^3 cells"
        t0 = time.perf_counter()
        self.V = stfem.StokesPreconditionVanka.for_space(self.op, self.var, Alpha, Beta)
        self.setup = time.perf_counter() - t0
        self.updates = []
        for _ in range(2):
            t0 = time.perf_counter()
            self.V.update(None)
            self.updates.append(time.perf_counter() - t0)
        rng = np.random.default_rng(0)
        sizes = [3 * self.op.n_velocity if v == 0 else self.op.n_pressure for v in self.var]
        self.src = [self.op.initialize_dof_vector(v, rng.uniform(-1, 1, n)) for v, n in zip(self.var, sizes)]
        self.dst = [self.op.initialize_dof_vector(v) for v in self.var]
        self.windows, self.reps = [], MIN_REPS
        print(f"{self.name}: set-up {self.setup:.3f} s, update {self.updates[0]:.3f} {self.updates[1]:.3f} s in {self.V.setup_batches} batch(es), "
              f"{self.block_bytes * 1e-9:.2f} GB of blocks", flush=True)

    def window(self):
        t0 = time.perf_counter()
        for _ in range(self.reps):
            self.V.step(self.dst, 1.0, False, self.src)
        self.dst[-1].download()  # synchronises (and copies one pressure vector: part of every window alike)
        return (time.perf_counter() - t0) / self.reps


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16, 24]
    configs = []
    for N in sizes:
        for dg in (False, True):
            configs.append(Config(3, N, dg, 2))
    configs.append(Config(2, 32, False, 1))  # the degree-2 apply measured beside them
    for c in configs:
        c.window()  # first launches
        c.reps = max(MIN_REPS, int(np.ceil(WINDOW / c.window())))
        c.window()  # warm-up at the window's length
    for _ in range(ROUNDS):
        for c in configs:
            c.windows.append(c.window())
    print(f"step: median (min .. max) of {ROUNDS} alternating rounds, a window of `steps` steps each (about {WINDOW} s); roofline = block bytes / time / 8.0 TB/s")
    for c in configs:
        med, lo, hi = float(np.median(c.windows)), min(c.windows), max(c.windows)
        print(f"{c.name}: {c.reps:4d} steps, step {med * 1e3:7.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), {c.block_bytes / med * 1e-9:6.0f} GB/s of block bytes = "
              f"{c.block_bytes / med / PEAK:.3f} of the roofline", flush=True)


if __name__ == "__main__":
    main()
