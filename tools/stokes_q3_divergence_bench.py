#!/usr/bin/env python3
"""The divergence functional and the pressure helpers of include/stfem_stokes_pressure_space.h on 48^3 cells, box and perturbed mesh:
stfem_stokes_divergence_space at velocity degree 3 with degree 2 beside it, and for scale the linear vmult of the same context in the
same run; then stfem_stokes_pressure_difference_space at nq = 4 (box, both degree-2 pressure spaces) and the FE_DGP(2) transfers
between 24^3 and 48^3 cells.

A window is `calls` back-to-back calls ended by a stream synchronise, host clock; `calls` is chosen per variant from a first window so
that a window lasts about WINDOW seconds.  Per configuration: a warm-up window per variant, then ROUNDS rounds alternating over the
variants; median (min .. max) over the rounds.  The divergence and the pressure difference are synchronous entries: every call of
theirs ends in a blocking copy of its result, so their figure is the time of a call (kernel, finish kernel, copy, synchronise), not
of the kernel alone.  The roofline fraction is by algorithmic bytes over that call time: 3 Nu doubles read and n_cells written for
the divergence, at 8 TB/s.  Run with no other GPU work in the same call:
    python tools/stokes_q3_divergence_bench.py [cells per direction ...]"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stfem = importlib.import_module("dealii-stfem_amd")

WINDOW, ROUNDS, FIRST = 0.3, 5, 10
PEAK = 8.0e12  # bytes / s


def sync():
    stfem._check(stfem.lib().stfem_stream_synchronize(None), "stfem_stream_synchronize")


def run(variants):
    """name -> (calls, median, min, max) seconds per call"""
    def window(f, calls):
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        sync()
        return (time.perf_counter() - t0) / calls

    calls = {}
    for name, f in variants.items():
        window(f, FIRST)
        calls[name] = max(FIRST, int(WINDOW / window(f, FIRST)))
        window(f, calls[name])  # warm-up at the window's own length
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, f in variants.items():
            times[name].append(window(f, calls[name]))
    return {name: (calls[name], float(np.median(t)), float(np.min(t)), float(np.max(t))) for name, t in times.items()}


def show(head, name, r, note=""):
    calls, med, lo, hi = r
    print(f"{head} {name:22s} {calls:5d} calls: {med * 1e3:7.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}){note}", flush=True)


def divergence(N, perturbed):
    nc = (N, N, N)
    verts = stfem.mesh_vertices(nc, distort=0.1, seed=7) if perturbed else None
    rng = np.random.default_rng(0)
    for degree in (3, 2):
        op = stfem.StokesMatrixFreeOperator.with_degree(degree, nc, vertices=verts, viscosity=0.01)
        u, p = op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)), op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure))
        du, dp = op.initialize_dof_vector(0), op.initialize_dof_vector(1)
        res = run({"divergence_space": lambda: op.divergence_space(u), "linear vmult": lambda: op.vmult(du, dp, u, p)})
        head = f"{N}^3 cells {'perturbed' if perturbed else 'box      '} Q{degree}"
        nbytes = 8.0 * (3 * op.n_velocity + op.n_cells)
        t = res["divergence_space"][1]
        show(head, "divergence_space", res["divergence_space"],
             f"  {nbytes / 1e6:.1f} MB = {nbytes / PEAK * 1e6:.1f} us at 8 TB/s: {nbytes / PEAK / t:.3f} of the roofline; "
             f"{t / res['linear vmult'][1]:.2f} of the linear vmult")
        show(head, "linear vmult", res["linear vmult"])
        print(f"{head} divergence plan (workgroups, cells per wave or half-wave): {op.last_divergence_plan()}", flush=True)


def pressure(N):
    nc, half = (N, N, N), (N // 2,) * 3
    rng = np.random.default_rng(1)
    nq = 4
    for dg in (False, True):
        op = stfem.StokesMatrixFreeOperator.with_degree(3, nc, dg_pressure=dg)
        p = op.initialize_dof_vector(1, rng.uniform(-1, 1, op.n_pressure))
        exact = rng.uniform(-1, 1, (op.n_cells, nq ** 3))
        head = f"{N}^3 cells box       Q3/{'FE_DGP2' if dg else 'FE_Q2'}"
        res = run({"pressure_difference_space": lambda: op.pressure_difference(nq, p, exact)})
        show(head, f"pressure_difference nq={nq}", res["pressure_difference_space"],
             f"  (the call uploads {exact.nbytes / 1e6:.1f} MB of exact values from the host)")
    fine, coarse = stfem.StokesMatrixFreeOperator.with_degree(3, nc, dg_pressure=True), stfem.StokesMatrixFreeOperator.with_degree(3, half, dg_pressure=True)
    f, c = fine.initialize_dof_vector(1, rng.uniform(-1, 1, fine.n_pressure)), coarse.initialize_dof_vector(1, rng.uniform(-1, 1, coarse.n_pressure))
    f2, c2 = fine.initialize_dof_vector(1), coarse.initialize_dof_vector(1)
    res = run({"prolongate": lambda: stfem.stokes_dgp_prolongate(fine, coarse, f2, c), "restrict": lambda: stfem.stokes_dgp_restrict(fine, coarse, c2, f)})
    nbytes = 8.0 * (fine.n_pressure + coarse.n_pressure)
    for name in res:
        show(f"{N // 2}^3 -> {N}^3 cells FE_DGP2", "dgp_" + name + "_space", res[name],
             f"  {nbytes / 1e6:.1f} MB: {nbytes / PEAK / res[name][1]:.3f} of the roofline")


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [48]
    print(f"median (min .. max) of {ROUNDS} alternating rounds, a window of `calls` calls each (about {WINDOW} s)")
    for N in sizes:
        for perturbed in (False, True):
            divergence(N, perturbed)
        pressure(N)


if __name__ == "__main__":
    main()
