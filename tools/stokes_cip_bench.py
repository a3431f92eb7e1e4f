#!/usr/bin/env python3
"""What the CIP interior-face launches (stfem_stokes_set_cip, delta0 != 0) add to one Stokes vmult, Q2/Q1 x cG(1), on a box (Kronecker
path + CART kernel) and on a perturbed mesh (cell kernel + general kernel) of N^3 cells (default 64): wall time per call of a
back-to-back sequence that ends in a device synchronise, the same context with delta0 = 0 and delta0 = 1 in alternating rounds of one
process, median and range over the rounds.  For scale beside it: the convection launches of the jacobian mode on the same meshes took
0.25 ms (box) / 0.31 ms (perturbed) in profiles/navier_convection.txt.
Set-up mode: what the CIP term in the per-cell Vanka blocks (StokesPreconditionVanka(..., delta0=1)) adds to one update() of the blocks,
jacobian mode, cG(1), on N^3 cells (default 32): two smoothers of the same context, delta0 = 0 and delta0 = 1, updated in alternating
rounds, each update ended by a device synchronise.  --root DIR loads the package of another checkout (one without the term times
delta0 = 0 alone), to run the two checkouts in alternating processes.
Slab mode: the term by itself (cip_add) on a z-slab of NXY x NXY x NZ cells (default 64 x 64 x 32) without neighbours and, with
cip_add_slab, with a neighbour on both sides; --root as above (a checkout without the slab entry points times cip_add alone).
Usage: stokes_cip_bench.py [N] [rounds] [calls per round]
       stokes_cip_bench.py setup [N] [rounds] [--root DIR]
       stokes_cip_bench.py slab [NXY] [NZ] [rounds] [calls per round] [--root DIR]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT, WHICH = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "this checkout"
if "--root" in sys.argv:
    at = sys.argv.index("--root")
    ROOT = os.path.abspath(sys.argv[at + 1])
    WHICH = "the --root checkout"
    del sys.argv[at:at + 2]
sys.path.insert(0, ROOT)
stfem = importlib.import_module("dealii-stfem_amd")
fmt = lambda v: f"{np.median(v):8.3f} ms (range {min(v):.3f} .. {max(v):.3f})"  # noqa: E731


def setup_mode(n, rounds):
    Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 1.0 / 64, 1)
    deltas = (0.0, 1.0) if "stfem_stokes_vanka_create_linearised_cip" in stfem.SIGNATURES else (0.0,)
    for mesh in ("box", "perturbed"):
        verts = stfem.mesh_vertices((n, n, n), distort=0.1, seed=7) if mesh == "perturbed" else None
        op = stfem.StokesMatrixFreeOperator((n, n, n), vertices=verts, viscosity=1.0)
        rng = np.random.default_rng(0)
        lin = [op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)), None]
        probe = op.initialize_dof_vector(1)
        smoothers = {d: stfem.StokesPreconditionVanka(op, [0, 1], Alpha, Beta, lin=lin, mode=2, per_cell=True, **({"delta0": d} if d else {}))
                     for d in deltas}

        def timed(v):
            probe.download()
            t0 = time.perf_counter()
            v.update(lin)
            probe.download()  # (synchronises)
            return (time.perf_counter() - t0) * 1e3

        times = {d: [] for d in deltas}
        for v in smoothers.values():
            timed(v)
        for _ in range(rounds):
            for d in deltas:
                times[d].append(timed(smoothers[d]))
        print(f"{mesh:9s} {n}^3 cells, jacobian, cG(1), {rounds} rounds, {smoothers[0.0].setup_batches} batch(es), measured ({WHICH}):", flush=True)
        for d in deltas:
            print(f"    update, delta0 = {d:g} : {fmt(times[d])}")
        if len(deltas) > 1:
            print(f"    the CIP term       : {fmt([b - a for a, b in zip(times[0.0], times[1.0])])}", flush=True)
        del smoothers, op, lin, probe


def slab_mode(nxy, nz, rounds, calls):
    """the term by itself on a slab of nxy x nxy x nz cells: cip_add (the faces inside the slab, the instantiations without SLAB) and,
    where this checkout has it, cip_add_slab with a neighbour on both sides (ghost planes packed from the slab's own source, the ghost
    vertex planes the slab's outer planes shifted by one layer), in alternating rounds"""
    nc = (nxy, nxy, nz)
    slab = "stfem_stokes_cip_add_slab" in stfem.SIGNATURES
    for mesh in ("box", "perturbed"):
        upper = (1.0, 1.0, nz / nxy)
        verts = stfem.mesh_vertices(nc, upper=upper, distort=0.1, seed=7) if mesh == "perturbed" else None
        op = stfem.StokesMatrixFreeOperator(nc, vertices=verts, upper=upper, dirichlet_mask=63 & ~48, viscosity=1.0)
        rng = np.random.default_rng(0)
        u, w = (op.initialize_dof_vector(0, rng.uniform(-1, 1, 3 * op.n_velocity)) for _ in range(2))
        dst = op.initialize_dof_vector(0)
        probe = op.initialize_dof_vector(1)
        kinds = {"cip_add, no neighbours": lambda: op.cip_add(dst, u, w, 1.0)}
        if slab:
            V = np.asarray(verts).reshape(nz + 1, -1, 3) if verts is not None else None
            shift = np.array([0.0, 0.0, upper[2] / nz])
            lo, up = op.initialize_dof_vector(0), op.initialize_dof_vector(0)
            op.cip_pack(u, 1, lo)
            op.cip_pack(u, 0, up)

            def with_neighbours(mask):
                op.set_cip_neighbours(mask, None if V is None else V[0] - shift, None if V is None else V[nz] + shift)

            def two_neighbours():
                op.cip_add_slab(dst, u, w, 1.0, lo, up)

            kinds["cip_add_slab, two neighbours"] = two_neighbours

        def timed(name):
            if slab:
                with_neighbours(48 if "slab" in name else 0)
            for _ in range(3):
                kinds[name]()
            probe.download()
            t0 = time.perf_counter()
            for _ in range(calls):
                kinds[name]()
            probe.download()  # (synchronises)
            return (time.perf_counter() - t0) / calls * 1e3

        times = {k: [] for k in kinds}
        for k in kinds:
            timed(k)
        for _ in range(rounds):
            for k in kinds:
                times[k].append(timed(k))
        print(f"{mesh:9s} {nxy} x {nxy} x {nz} cells, {rounds} rounds x {calls} calls, measured ({WHICH}):", flush=True)
        for k in kinds:
            print(f"    {k:29s}: {fmt(times[k])}", flush=True)
        del op, u, w, dst, probe


if len(sys.argv) > 1 and sys.argv[1] == "slab":
    a = [int(v) for v in sys.argv[2:]]
    slab_mode(a[0] if len(a) > 0 else 64, a[1] if len(a) > 1 else 32, a[2] if len(a) > 2 else 9, a[3] if len(a) > 3 else 40)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "setup":
    setup_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 32, int(sys.argv[3]) if len(sys.argv) > 3 else 7)
    sys.exit(0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
CALLS = int(sys.argv[3]) if len(sys.argv) > 3 else 40
Alpha, Beta, _, _ = stfem.get_fe_time_weights_stokes(stfem.CGP, 1, 1.0 / 64, 1)
for mesh in ("box", "perturbed"):
    verts = stfem.mesh_vertices((N, N, N), distort=0.1, seed=7) if mesh == "perturbed" else None
    op = stfem.StokesMatrixFreeOperator((N, N, N), vertices=verts, viscosity=1.0)
    rng = np.random.default_rng(0)
    src = [op.initialize_dof_vector(v, rng.uniform(-1, 1, 3 * op.n_velocity if v == 0 else op.n_pressure)) for v in (0, 1)]
    dst = [op.initialize_dof_vector(v) for v in (0, 1)]

    def timed(delta0):
        op.set_cip(delta0)
        for _ in range(3):
            op.st_vmult(Alpha, Beta, 1, 1, dst, src)
        dst[1].download()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            op.st_vmult(Alpha, Beta, 1, 1, dst, src)
        dst[1].download()  # (synchronises; the pressure vector is the small one)
        return (time.perf_counter() - t0) / CALLS * 1e3

    timed(1.0), timed(0.0)  # code objects, first launches
    without, with_term = [], []
    for _ in range(ROUNDS):
        without.append(timed(0.0))
        with_term.append(timed(1.0))
    diff = [b - a for a, b in zip(without, with_term)]
    print(f"{mesh:9s} {N}^3 cells, {3 * op.n_velocity + op.n_pressure} DoFs, {ROUNDS} rounds x {CALLS} calls, measured:", flush=True)
    print(f"    vmult, delta0 = 0 : {fmt(without)}")
    print(f"    vmult, delta0 = 1 : {fmt(with_term)}")
    print(f"    the CIP launches  : {fmt(diff)}", flush=True)
    del op, src, dst
