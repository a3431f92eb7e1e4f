#!/usr/bin/env python3
"""What the Navier-Stokes modes add to the Stokes operator of velocity degree 3 (FE_Q(3)^3 x FE_Q(2) / FE_DGP(2), the default) or 2
(FE_Q(2)^3 x FE_Q(1) / FE_DGP(1)), StokesMatrixFreeOperator.with_degree(degree, ...): time per vmult and per cG(2) st_vmult in mode
none / form / jacobian on 48^3 cells, box and perturbed mesh, both pressure spaces.  The yardstick is the linear vmult (mode none) of the same context in the same run; the
added time of a mode is reported as a fraction of it (for st_vmult: of the linear st_vmult beside it, and of the linear vmult).

A window is `calls` back-to-back calls ended by a blocking download of one pressure vector, host clock; `calls` is chosen per variant
from a first window so that a window lasts about WINDOW seconds.  Per configuration: a warm-up window per variant, then ROUNDS rounds
alternating over the six variants; median (min .. max) over the rounds.  Run with no other GPU work in the same call:
    python tools/navier_q3_bench.py [--degree 2|3] [cells per direction ...]"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

WINDOW, ROUNDS, FIRST = 0.3, 5, 10
MODES = (("none", 0), ("form", 1), ("jacobian", 2))
Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 2, 1.0 / 64, 1)


def measure(degree, N, dg, perturbed):
    nc = (N, N, N)
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=7) if perturbed else None
    op = stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=verts, viscosity=0.01, dg_pressure=dg)
    rng = np.random.default_rng(0)
    var = [0, 0, 1, 1]
    src = [op.initialize_dof_vector(v, rng.uniform(-1, 1, 3 * op.n_velocity if v == 0 else op.n_pressure)) for v in var]
    lin = [op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)) for _ in range(2)] + [None, None]
    dst = [op.initialize_dof_vector(v) for v in var]

    def window(f, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        dst[2].download()  # synchronises (and copies one pressure vector: part of every window alike)
        return (time.perf_counter() - t0) / calls

    variants = {}
    for name, mode in MODES:
        kw = dict(lin=lin[0], mode=mode) if mode else {}
        variants["vmult " + name] = lambda kw=kw: op.vmult(dst[0], dst[2], src[0], src[2], **kw)
    for name, mode in MODES:
        kw = dict(lin=lin, mode=mode) if mode else {}
        variants["st_vmult " + name] = lambda kw=kw: op.st_vmult(Alpha, Beta, 1, 2, dst, src, **kw)
    calls = {}
    for name, f in variants.items():
        window(f, FIRST)
        calls[name] = max(FIRST, int(WINDOW / window(f, FIRST)))
        window(f, calls[name])  # warm-up at the window's own length
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, f in variants.items():
            times[name].append(window(f, calls[name]))
    return op, calls, {name: (float(np.median(t)), float(np.min(t)), float(np.max(t))) for name, t in times.items()}


def main():
    args, degree = sys.argv[1:], 3
    if args[:1] == ["--degree"]:
        degree, args = int(args[1]), args[2:]
    sizes = [int(a) for a in args] or [48]
    print(f"median (min .. max) of {ROUNDS} alternating rounds, a window of `calls` calls each (about {WINDOW} s); "
          "added = (mode - none) / linear vmult of the same context")
    for N in sizes:
        for perturbed in (False, True):
            for dg in (False, True):
                op, calls, t = measure(degree, N, dg, perturbed)
                head = f"{N}^3 cells {'perturbed' if perturbed else 'box      '} Q{degree}/{f'FE_DGP{degree - 1}' if dg else f'FE_Q{degree - 1}':7s}"
                yard = t["vmult none"][0]
                for name in t:
                    med, lo, hi = t[name]
                    line = f"{head} {name:17s} {calls[name]:5d} calls: {med * 1e3:7.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})"
                    kind, mode = name.split(" ")
                    if mode != "none":
                        added = med - t[kind + " none"][0]
                        line += f"  added {added * 1e3:6.3f} ms = {added / yard:5.2f} of the linear vmult"
                        if kind == "st_vmult":
                            line += f", {added / t['st_vmult none'][0]:5.2f} of the linear st_vmult"
                    print(line, flush=True)
                try:
                    cell = op.last_cell_plan()
                except stfem.StfemError:  # (degree 2 on a box: the Kronecker path, no cell launch)
                    cell = None
                print(f"{head} plans: cell {cell}, convection {op.last_convection_plan()}", flush=True)


if __name__ == "__main__":
    main()
