"""The partitioned Stokes system of the C++ mirror WITH the CIP term (host/stfem/stokes_solver.h: StokesSpaces::set_partition ->
stfem_stokes_set_cip_neighbours; StokesSystem::vmult -> stfem_stokes_cip_pack, stfem_neighbour_exchange, stfem_stokes_cip_bind_ghosts)
through its caller host/test_host_stokes_cip_sharded, in the manner of tests/test_host_stokes_sharded.py.

On the one-rank communicator with the rank itself as both neighbours the slab is the middle one of a stack of copies of itself: what it
sends up arrives as its own lower ghost planes.  The oracle is the whole-mesh numpy term (tests/cip_reference.py) on THREE stacked
copies of the slab with the sources repeated (their top DoF plane repeats the bottom one, so the stack carries one field): inside the
middle copy its rows are the slab's rows, and in an interface plane they are the sum of the slab's two partial sums, top and bottom.
The add-exchange of the self-loop returns every partial to its sender (tests/test_host_stokes_sharded.py: both interface planes
double), so the caller's interface planes are compared with twice the slab's own partials - the numpy slab rule of
tests/cip_slab_reference.py, which this test first holds against the stacked oracle as just described.  Bound 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_reference as cref  # noqa: E402
import cip_slab_reference as csr  # noqa: E402
import navier_reference as nref  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-stfem_amd", "host")
TOL = 1e-12
NC, UPPER, NU, MASK, DELTA0 = (4, 3, 2), (1.0, 0.75, 1.25), 0.3, 63 & ~48, 1.0
NDZ = 2 * NC[2] + 1


def _doubled(x, v, dg):
    out = np.array(x, dtype=np.float64)
    if not (v == 1 and dg):
        comps, step = (3, 2) if v == 0 else (1, 1)
        p = out.reshape(comps, step * NC[2] + 1, -1)
        p[:, 0] *= 2
        p[:, -1] *= 2
    return out


def _slab_term(u, verts):
    """the slab's own partial sums of C(u; u) with itself as both neighbours"""
    V = verts.reshape(NC[2] + 1, -1, 3)
    hz = np.array([0.0, 0.0, UPPER[2] / NC[2]])
    return csr.cip_slab(DELTA0, u, u, NC, verts, MASK, 48, csr.pack(u, NC, MASK, 1), csr.pack(u, NC, MASK, 0), V[0] - hz, V[-1] + hz)


def _stacked_term(u):
    """the whole-mesh term on three stacked copies, the source repeated: the rows of the middle copy [3][NDZ][plane]"""
    nc3 = (NC[0], NC[1], 3 * NC[2])
    verts3 = nref.perturbed_vertices(nc3, 0.0, 0, (0, 0, 0), (UPPER[0], UPPER[1], 3 * UPPER[2]))
    U = u.reshape(3, NDZ, -1)
    assert np.array_equal(U[:, 0], U[:, -1])
    U3 = np.concatenate([U[:, :-1], U[:, :-1], U], axis=1)
    whole = cref.cip(DELTA0, U3.reshape(-1), U3.reshape(-1), nc3, verts3, MASK).reshape(3, 3 * (NDZ - 1) + 1, -1)
    return whole[:, NDZ - 1:2 * NDZ - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [False, True])
def test_cpp_stokes_caller_runs_partitioned_with_the_cip_term(dg, tmp_path):
    orc_mod = ssc.oracle()
    exe = os.path.join(HOST, "test_host_stokes_cip_sharded")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = tmp_path / "stokes_cip_sharded.bin"
    res = subprocess.run([exe, *map(str, NC), str(int(dg)), repr(DELTA0), str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"ranks=1 blocks=4 carrier={int(dg)} cip_neighbours=48" in res.stdout
    # the mirror's partitioned smoother ran: one block per cell of the slab, a finite non-zero apply
    assert f"vanka_blocks={NC[0] * NC[1] * NC[2]} vanka_finite=1" in res.stdout
    raw = np.fromfile(out, dtype=np.uint8)
    nb = int(raw[:8].view(np.uint64)[0])
    sizes = [int(v) for v in raw[8:8 + 8 * nb].view(np.uint64)]
    off = 8 + 8 * nb
    n_u, n_p = ssc.sizes(NC, dg)
    var = [0, 0, 1, 1]  # BlockSlice(1, 2, 2), variable-major
    assert nb == 4 and sizes == [3 * n_u if v == 0 else n_p for v in var]
    X, Y = [], []
    for dest in (X, Y):
        for n in sizes:
            dest.append(raw[off:off + 8 * n].view(np.float64).copy())
            off += 8 * n
    assert off == raw.size
    verts = nref.perturbed_vertices(NC, 0.0, 0, (0, 0, 0), UPPER)
    orc = orc_mod.StokesOracle(NC, verts, MASK, NU, dg_pressure=dg)
    A, B, _, _ = orc_mod.time_weights(orc_mod.CGP, 2, 1.0 / 32, 1)
    Alpha, Beta = np.zeros((4, 4)), np.zeros((4, 4))
    index = lambda it, v, d: ssc.block_index(2, it, v, d)  # noqa: E731
    for a in range(2):
        for b in range(2):
            Alpha[index(0, 0, a), index(0, 0, b)] = Alpha[index(0, 0, a), index(0, 1, b)] = Alpha[index(0, 1, a), index(0, 0, b)] = A[a, b]
            Beta[index(0, 0, a), index(0, 0, b)] = B[a, b]
    # the slab's partial sums: the linear operator, then per source time dof the term, scattered like the K part (cip_reference.st_vmult)
    plain = nref.st_vmult(orc, 0, Alpha, Beta, 1, 2, X, None, index, NC, verts, MASK)
    want = [np.array(p, dtype=np.float64) for p in plain]
    for d in range(2):
        i = index(0, 0, d)
        term = _slab_term(X[i], verts)
        # the oracle of the issue: three stacked copies, the middle one's rows
        stacked, t = _stacked_term(X[i]), term.reshape(3, NDZ, -1)
        assert np.linalg.norm(stacked) > 0
        assert ssc.rel(t[:, 1:-1], stacked[:, 1:-1]) <= 1e-13
        assert ssc.rel(t[:, 0] + t[:, -1], stacked[:, 0]) <= 1e-13 and ssc.rel(t[:, 0] + t[:, -1], stacked[:, -1]) <= 1e-13
        for jd in range(2):
            j = index(0, 0, jd)
            if abs(Alpha[j, i]) > nref.EPS10:
                want[j] = want[j] + Alpha[j, i] * term
    worst = 0.0
    for j, v in enumerate(var):
        ref = _doubled(want[j], v, dg)
        assert np.linalg.norm(ref) > 0
        err = ssc.rel(Y[j], ref)
        worst = max(worst, err / TOL)
        assert err <= TOL, (j, err)
        if v == 0:
            assert ssc.rel(_doubled(plain[j], v, dg), ref) > 1e-2  # the term is there, interface faces included
    print(f"ratio caller {worst:.3e}")
