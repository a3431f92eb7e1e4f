#!/usr/bin/env python3
"""Set-up and apply time of the per-cell Stokes Vanka smoother of the LINEARISED operator at velocity degree 3
(StokesPreconditionVanka.for_space(..., lin, mode) over StokesMatrixFreeOperator.with_degree(3, ...): FE_Q(3)^3 x FE_Q(2) / FE_DGP(2),
cG(2): 4 blocks, 438 / 404 rows per cell) on 16^3 box cells, both pressure spaces: per pressure space one smoother in mode 0 (the
linear blocks of stfem_stokes_vanka_create_space, through the same entry) and one in mode 2 (jacobian) about two distinct states.

Set-up: host clock around the constructor (it ends in a device synchronise per batch of cell layers) and around two update calls,
which stage the same set-up into the existing storage - update(None) in mode 0, update(lin) in mode 2, where every state costs a launch
of the cell-matrix kernel over the window of cell layers.  Apply: step = the streaming kernel + the collecting launch, which do not
know the mode; the median over ROUNDS alternating rounds - every smoother once per round - of one window of back-to-back steps ended by
a blocking download of one pressure vector, after a warm-up window of each, exactly as tools/stokes_q3_vanka_bench.py takes it, so that
its figures for the same configuration are comparable.  Run with no other GPU work in the same call:
    python tools/stokes_q3_vanka_linearised_bench.py [--setup-only] [cells per direction ...]
--setup-only: the constructors and updates alone (for a kernel-trace run that splits the set-up into its three stages)."""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

PEAK = 8.0e12  # B/s
MIN_REPS, ROUNDS, WINDOW = 20, 5, 0.25  # WINDOW: seconds
R = 2  # cG(2)


class Config:
    def __init__(self, op, N, dg, mode):
        self.op, self.N, self.dg, self.mode = op, N, dg, mode
        Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, R, 1.0 / 64, 1)
        self.var = [0] * R + [1] * R
        self.m = R * (3 * 64 + (10 if dg else 27))
        self.block_bytes = 8 * (4 * ((self.m + 3) // 4)) * (16 * ((self.m + 15) // 16)) * N ** 3  # kpad x mpad doubles per cell
        self.name = f"Q3/{'FE_DGP2' if dg else 'FE_Q2':7s} cG({R}) {self.m:3d} rows {N}^3 cells mode {mode}"
        rng = np.random.default_rng(0)
        sizes = [3 * op.n_velocity if v == 0 else op.n_pressure for v in self.var]
        # two distinct states, one per time dof; the pressure entries stay null
        self.lin = [op.initialize_dof_vector(0, rng.uniform(-1, 1, n)) if v == 0 else None for v, n in zip(self.var, sizes)] if mode else None
        t0 = time.perf_counter()
        self.V = stfem.StokesPreconditionVanka.for_space(op, self.var, Alpha, Beta, lin=self.lin, mode=mode)
        self.setup = time.perf_counter() - t0
        self.updates = []
        for _ in range(2):
            t0 = time.perf_counter()
            self.V.update(self.lin)
            self.updates.append(time.perf_counter() - t0)
        self.src = [op.initialize_dof_vector(v, rng.uniform(-1, 1, n)) for v, n in zip(self.var, sizes)]
        self.dst = [op.initialize_dof_vector(v) for v in self.var]
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
    args = sys.argv[1:]
    setup_only = "--setup-only" in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [16]
    configs = []
    for N in sizes:
        for dg in (False, True):
            op = stfem.StokesMatrixFreeOperator.with_degree(3, (N, N, N), viscosity=1.0, dg_pressure=dg)
            for mode in (0, 2):
                configs.append(Config(op, N, dg, mode))
    if setup_only:
        return
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
