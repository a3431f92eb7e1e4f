"""Per-cell two-variable Stokes Vanka blocks on z-slabs (stfem_stokes_vanka_create_linearised_partitioned): for every slab of a cut the
smoother is set up on the slab's EXTENDED context (the slab plus one ghost cell layer per z neighbour, states cut from the whole-mesh
states), built for the slab's own cells and applied on the slab to the cut of a seeded source; the slabs' results, summed on the host
(stokes_slab_cases.assemble), are compared with the apply of the WHOLE-MESH dense numpy reference (tests/stokes_vanka_reference.py,
with the CIP term tests/stokes_vanka_cip_reference.py).  Bound 1e-10, the TOL of tests/test_gpu_stokes_vanka_linearised.py / _cip.py;
tests/test_cip_slab_contract_cpu.py holds cond_max of the new cases below 1e6 (at most 4.2e4) and the term's change of the reference
above 1e-2.  With the term, the face between a ghost cell and the cell beyond it reaches the slab's outer layer (beyond_mask): cuts
(0,2,4), (0,1,4), (0,1,2,4) and (0,1,3,4) of the four-layer meshes have such cells on one side, both or none, per slab.

Run as a program (the batch test starts it in a fresh process): <file> <case> <cut index> <slab index> <out.npy>."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cip_slab_reference as csr  # noqa: E402
import stokes_slab_cases as ssc  # noqa: E402
import stokes_vanka_cip_reference as scr  # noqa: E402
import stokes_vanka_reference as svr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
KNOB = "STFEM_VANKA_SETUP_LAYERS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, SHAPE = -1, -5


@pytest.fixture(scope="module")
def stfem():
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    return mod


def _spec(name):
    return csr.VANKA_SLAB_SPECS[name] if name in csr.VANKA_SLAB_SPECS else scr.CASES[name]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, whole-mesh reference without the term, with it): built once, shared, never modified"""
    if name in scr.CASES:
        return scr.case(name)
    p = svr.problem(_spec(name))
    base = svr.reference(p)
    return p, base, scr.with_cip(base, p, scr.DELTA0, p.lin)


def _x(p):
    return [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]


def _operator(stfem, p, z0, z1):
    """the Stokes context of the cell layers [z0, z1) of the problem's mesh: z faces constrained / weak where they are the global boundary"""
    nc = (p.nc[0], p.nc[1], z1 - z0)
    strong, weak, _ = ssc.slab_masks(p.mask, p.weak, 0, z0 > 0, z1 < p.nc[2])
    verts = ssc.slab_vertices(p.verts, p.nc, z0, z1) if p.pert else None
    return stfem.StokesMatrixFreeOperator(nc, vertices=verts, lower=(0, 0, z0 / p.nc[2]), upper=(1, 1, z1 / p.nc[2]), dirichlet_mask=strong,
                                          viscosity=p.nu, weak_boundary_ids=ssc.faces_of(weak), dg_pressure=p.dg)


def _cut(p, host, z0, z1):
    return [None if x is None else ssc.cut(x, v, p.dg, p.nc, z0, z1) for x, v in zip(host, p.var)]


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) if x is not None else None for v, x in zip(p.var, host)]


class _Slab:
    """one slab of a cut: its context, its extended context, the masks and the smoother"""

    def __init__(self, stfem, p, bounds, r, delta0, lin_host=None):
        self.z0, self.z1 = bounds[r], bounds[r + 1]
        lo, hi = r > 0, r < len(bounds) - 2
        self.e0, self.e1 = self.z0 - lo, self.z1 + hi
        self.neighbours = (16 if lo else 0) | (32 if hi else 0)
        self.beyond = (16 if lo and self.e0 > 0 else 0) | (32 if hi and self.e1 < p.nc[2] else 0)
        self.p, self.delta0 = p, delta0
        self.op, self.ext = _operator(stfem, p, self.z0, self.z1), _operator(stfem, p, self.e0, self.e1)
        self.lin = self.states(p.lin if lin_host is None else lin_host)
        self.V = stfem.StokesPreconditionVanka(self.op, p.var, p.Alpha, p.Beta, lin=self.lin, mode=p.mode, delta0=delta0,
                                               partition=(self.ext, self.neighbours, self.beyond))
        assert self.V.n_classes == p.nc[0] * p.nc[1] * (self.z1 - self.z0)

    def states(self, host):
        """device states on the extended context, cut from whole-mesh states"""
        return _device(self.ext, self.p, _cut(self.p, host, self.e0, self.e1))

    def apply(self, X):
        src = _device(self.op, self.p, _cut(self.p, X, self.z0, self.z1))
        dst = _device(self.op, self.p, [np.full(s.size, 9.0) for s in src])  # overwritten
        self.V.vmult(dst, src)
        return [d.download() for d in dst]


def _assembled(p, bounds, parts):
    return [ssc.assemble([q[b] for q in parts], v, p.dg, p.nc, bounds) for b, v in enumerate(p.var)]


RUNS = [(name, bounds, delta0) for name, cuts in csr.VANKA_SLAB_CUTS.items() for bounds in cuts
        for delta0 in ((scr.DELTA0, 0.0) if name in ("box224_jac_dg1", "pert224_jac") else (scr.DELTA0,))]


@pytest.mark.parametrize("name,bounds,delta0", RUNS, ids=["-".join([n, "".join(map(str, b)), "cip" if d else "plain"]) for n, b, d in RUNS])
def test_slab_smoothers_sum_to_the_whole_mesh_smoother(name, bounds, delta0, stfem, oracle_mod, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    p, base, ref = _case(name)
    X = _x(p)
    slabs = [_Slab(stfem, p, bounds, r, delta0) for r in range(len(bounds) - 1)]
    assert all(s.V.setup_batches == 1 for s in slabs)
    Y = _assembled(p, bounds, [s.apply(X) for s in slabs])
    want, other = (ref if delta0 else base).vmult(X), (base if delta0 else ref).vmult(X)
    overall = ssc.rel(np.concatenate(Y), np.concatenate(want))
    per_block = [ssc.rel(Y[b], want[b]) for b in range(p.nb)]
    print(name, bounds, "delta0 %g" % delta0, "beyond", [s.beyond for s in slabs], "overall %.3e" % overall,
          "largest block %.3e" % max(per_block), "ratio to the bound %.3e" % (max(overall, *per_block) / TOL))
    assert overall <= TOL and max(per_block) <= TOL, per_block
    assert ssc.rel(np.concatenate(Y), np.concatenate(other)) > 1e-3  # (the term is there, or is not)


def test_update_equals_a_fresh_create_bitwise(stfem, oracle_mod):
    name, bounds = "pert224_jac", (0, 1, 3, 4)
    p, _, _ = _case(name)
    other = svr.problem(_spec(name), seed=12).lin  # (what scr.other_states does for its cases)
    X = _x(p)
    for r in range(3):
        s = _Slab(stfem, p, bounds, r, scr.DELTA0)
        Y1 = s.apply(X)
        lin2 = s.states(other)
        s.V.update(lin2)
        Y2 = s.apply(X)
        Y3 = _Slab(stfem, p, bounds, r, scr.DELTA0, other).apply(X)
        assert ssc.rel(np.concatenate(Y2), np.concatenate(Y1)) > 1e-6  # the blocks did change
        assert all(np.array_equal(a, b) for a, b in zip(Y2, Y3))


def test_batched_setup_in_a_fresh_process_equals_one_batch(stfem, oracle_mod, monkeypatch, tmp_path):
    """pert224_jac cut (0,2,4), the upper slab (own layers 1 and 2 of its three-layer extended context: one ghost layer below, cells
    beyond it): one cell layer per batch in a child process against the one-batch set-up here, bit for bit"""
    name, cut, r = "pert224_jac", 0, 1
    monkeypatch.delenv(KNOB, raising=False)
    p, _, _ = _case(name)
    s = _Slab(stfem, p, csr.VANKA_SLAB_CUTS[name][cut], r, scr.DELTA0)
    assert s.V.setup_batches == 1
    one = np.concatenate(s.apply(_x(p)))
    out = tmp_path / "batched.npy"
    env = dict(os.environ, **{KNOB: "1"})
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(cut), str(r), str(out)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.load(out)
    assert int(got[-1]) == 2  # setup_batches > 1: one per own layer
    assert np.array_equal(got[:-1], one)


def test_refusals(stfem, oracle_mod):
    name, bounds = "pert224_jac", (0, 1, 3, 4)
    p, _, _ = _case(name)
    op, ext = _operator(stfem, p, 1, 3), _operator(stfem, p, 0, 4)
    lin = _device(ext, p, _cut(p, p.lin, 0, 4))
    lib = stfem.lib()

    def refused(status, word, partition, lin_=lin, delta0=scr.DELTA0):
        with pytest.raises(stfem.StfemError) as e:
            stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=lin_, mode=p.mode, delta0=delta0, partition=partition)
        assert e.value.status == status and word in lib.stfem_last_error().decode(), lib.stfem_last_error().decode()

    refused(SHAPE, "ghost layer", (ext, 16, 0))                                      # one layer too many for one neighbour
    refused(SHAPE, "ghost layer", (op, 48, 0))                                       # no ghost layers at all
    refused(SHAPE, "ghost layer", (stfem.StokesMatrixFreeOperator((3, 2, 4)), 48, 0))  # other x-y cell counts (a box besides)
    dgp = stfem.StokesMatrixFreeOperator((2, 2, 4), vertices=p.verts, dirichlet_mask=p.mask, viscosity=p.nu, dg_pressure=True)
    refused(SHAPE, "pressure space", (dgp, 48, 0))
    refused(INVALID, "neighbour_mask", (ext, 48 | 2, 0))
    refused(INVALID, "beyond_mask", (_operator(stfem, p, 0, 3), 16, 32))             # a beyond bit without its neighbour bit
    refused(INVALID, "lin_blocks", (ext, 48, 0), lin_=None)                          # the refusals of create_linearised_cip
    refused(INVALID, "lin_blocks[", (ext, 48, 0), lin_=[None] * p.nb)
    refused(INVALID, "delta0", (ext, 48, 0), delta0=float("nan"))
    refused(INVALID, "null", (None, 48, 0))
    V = stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=lin, mode=p.mode, delta0=scr.DELTA0, partition=(ext, 48, 0))
    assert V.n_classes == 2 * 2 * 2


if __name__ == "__main__":
    case_name, cut_index, slab_index, out_path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    mod = importlib.import_module("dealii-stfem_amd")
    mod.lib()
    prob = svr.problem(_spec(case_name))
    slab = _Slab(mod, prob, csr.VANKA_SLAB_CUTS[case_name][cut_index], slab_index, scr.DELTA0)
    y = np.concatenate(slab.apply(_x(prob)))
    np.save(out_path, np.concatenate([y, [float(slab.V.setup_batches)]]))
