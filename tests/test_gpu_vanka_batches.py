"""The per-cell Vanka set-up in several batches of cell layers (vanka_create_per_cell_device in csrc/stfem_vanka.hip, build_blocks in
csrc/stfem_stokes_vanka_cell.hip): a window of cell matrices that starts one layer below the batch (zw0 = z0 - 1 > 0), the offsets
into the metric / the cell numbering (moff, cell0) and the batch's first block (cell0 of the inversion).  The batch size comes from
the free device memory, so a test mesh is always ONE batch; STFEM_VANKA_SETUP_LAYERS=<n> (read at every set-up) caps it, and
setup_batches (stfem_vanka_setup_batches / stfem_stokes_vanka_setup_batches) reports how many batches a set-up took.

Under n < cell layers the smoother must equal the one-batch set-up BITWISE (each block is computed by one workgroup from the same
inputs, whatever batch it is in) and meet the bound of the one-batch tests against the dense restatement: 1e-10 (double) / 5e-4
(float) for the scalar smoother (test_gpu_vanka.py), 1e-10 for the Stokes smoother (test_gpu_stokes_vanka_linearised.py)."""
import functools
import importlib

import numpy as np
import pytest

import stokes_vanka_reference as svr

pytestmark = pytest.mark.gpu
KNOB = "STFEM_VANKA_SETUP_LAYERS"


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


# ------------------------------------------------------------------ scalar smoother
# perturbed meshes with a per-quadrature-point coefficient: every cell's metric records differ, so a wrong offset shows
SCALAR = {
    "q2_234": (2, (2, 3, 4), 0, 2, 63, 0.1),         # cG(2): two blocks
    "q3_225": (3, (2, 2, 5), 1, 1, 63 & ~48, 0.1),   # dG(1), open z faces, five layers
}


@functools.lru_cache(maxsize=None)
def _scalar_case(name, number):
    """(Alpha, Beta, vertices, coefficient, X, dense reference V X); the coefficient and X are fp32-representable for float"""
    from oracle import vanka_oracle
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, ttype, r, mask, distort = SCALAR[name]
    Alpha, Beta, _, _ = stfem.get_fe_time_weights(ttype, r, 0.05, 1)
    verts = stfem.mesh_vertices(nc, distort=distort, seed=11)
    ncells, nq = int(np.prod(nc)), (p + 1) ** 3
    rng = np.random.default_rng(2)
    cl = rng.uniform(0.5, 2.0, ncells * nq)
    X = rng.uniform(-1, 1, (Alpha.shape[0], int(np.prod([p * c + 1 for c in nc]))))
    if number == "float":
        cl, X = cl.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64)
    want = vanka_oracle.VankaOracle(p, nc, verts, mask, Alpha, Beta, coef_lap=cl).vmult(X)
    return Alpha, Beta, verts, cl, X, want


def _scalar_apply(stfem, ctx, Alpha, Beta, X, batches):
    V = stfem.PreconditionVanka(ctx, Alpha, Beta)
    assert V.n_classes == ctx.n_cells  # one block per cell
    assert V.setup_batches == batches  # what the set-up reports (0: on the host)
    nb = Alpha.shape[0]
    src = stfem.BlockVector(ctx, nb).upload(X)
    dst = stfem.BlockVector(ctx, nb).upload(np.full(X.shape, np.nan))  # overwritten
    V.vmult(dst, src)
    return dst.download()


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("number", ["double", "float"])
@pytest.mark.parametrize("name", list(SCALAR))
def test_scalar_setup_in_batches(name, number, layers, monkeypatch):
    stfem = importlib.import_module("dealii-stfem_amd")
    p, nc, ttype, r, mask, distort = SCALAR[name]
    assert nc[2] >= 4 and layers < nc[2]  # more than one batch; (4, 3) and (5, 2), (5, 3): the last batch is shorter
    Alpha, Beta, verts, cl, X, want = _scalar_case(name, number)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, number=number, dirichlet_mask=mask)
    ctx.evaluate_coefficient(cl.reshape(ctx.n_cells, (p + 1) ** 3), which=1)
    monkeypatch.delenv("STFEM_VANKA_HOST_SETUP", raising=False)
    monkeypatch.delenv(KNOB, raising=False)
    one = _scalar_apply(stfem, ctx, Alpha, Beta, X, 1)
    monkeypatch.setenv(KNOB, str(layers))
    got = _scalar_apply(stfem, ctx, Alpha, Beta, X, -(-nc[2] // layers))
    err = rel(got, want)
    print(f"{name} {number} {layers} layers per batch: rel-L2 vs dense reference {err:.3e}, one batch {rel(one, want):.3e}")
    assert np.array_equal(got, one)
    assert err < (1e-10 if number == "double" else 5e-4)


@pytest.mark.parametrize("number", ["double", "float"])
def test_scalar_batched_device_setup_equals_host_setup(number, monkeypatch):
    """one layer per batch against the same steps on the host, block by block (the bound of
    test_gpu_vanka.py::test_vanka_device_setup_equals_host_setup)"""
    stfem = importlib.import_module("dealii-stfem_amd")
    name = "q2_234"
    p, nc, ttype, r, mask, distort = SCALAR[name]
    Alpha, Beta, verts, cl, X, want = _scalar_case(name, number)
    ctx = stfem.MatrixFreeOperator(p, nc, vertices=verts, number=number, dirichlet_mask=mask)
    ctx.evaluate_coefficient(cl.reshape(ctx.n_cells, (p + 1) ** 3), which=1)
    monkeypatch.setenv(KNOB, "1")
    monkeypatch.setenv("STFEM_VANKA_HOST_SETUP", "0")
    dev = _scalar_apply(stfem, ctx, Alpha, Beta, X, nc[2])
    monkeypatch.setenv("STFEM_VANKA_HOST_SETUP", "1")
    host = _scalar_apply(stfem, ctx, Alpha, Beta, X, 0)
    assert rel(dev, host) < (1e-11 if number == "double" else 1e-5)
    assert rel(host, want) < (1e-10 if number == "double" else 5e-4)


# ------------------------------------------------------------------ Stokes smoother (fp64)
# the cases of tests/stokes_vanka_reference.py with three cell layers and one with four: perturbed, jacobian mode, weak x faces,
# FE_DGP pressure, cG(1) (eight cells: its dense reference takes as long as that of box223_form_dgp, a few seconds; cG(2) with
# a state per time dof on 2 x 2 x 4 cells took 14 s)
STOKES = {
    "box333": svr.CASES["box333"],
    "box223_form_dgp": svr.CASES["box223_form_dgp"],
    "pert214_jac_weak_dgp": ((2, 1, 4), True, 2, True, 0, 1, 1, 63 & ~3, 3, True),
}


@functools.lru_cache(maxsize=None)
def _stokes_case(name):
    p = svr.problem(STOKES[name])
    return p, svr.reference(p)


def _operator(stfem, p):
    return stfem.StokesMatrixFreeOperator(p.nc, vertices=p.verts if p.pert else None, dirichlet_mask=p.mask, viscosity=p.nu,
                                          weak_boundary_ids=[f for f in range(6) if p.weak >> f & 1], dg_pressure=p.dg)


def _device(op, p, host):
    return [op.initialize_dof_vector(v, x) if x is not None else None for v, x in zip(p.var, host)]


def _smoother(stfem, op, p, lin_host):
    dlin = _device(op, p, lin_host) if p.mode else None
    return stfem.StokesPreconditionVanka(op, p.var, p.Alpha, p.Beta, lin=dlin, mode=p.mode, per_cell=True), dlin


def _apply(op, p, V, X):
    src = _device(op, p, X)
    dst = _device(op, p, [np.full(n, np.nan) for n in p.sizes])  # overwritten
    V.vmult(dst, src)
    return np.concatenate([d.download() for d in dst])


# (3 layers: 1 and 2 per batch; 4 layers: 1, 2 and 3; (3, 2) and (4, 3): the last batch is shorter)
@pytest.mark.parametrize("name,layers", [(n, k) for n, spec in STOKES.items() for k in (1, 2, 3) if k < spec[0][2]])
def test_stokes_setup_in_batches(name, layers, monkeypatch, oracle_mod):
    stfem = importlib.import_module("dealii-stfem_amd")
    p, ref = _stokes_case(name)
    assert layers < p.nc[2]  # more than one batch
    op = _operator(stfem, p)
    X = [np.random.default_rng(3).uniform(-1, 1, n) for n in p.sizes]
    want = np.concatenate(ref.vmult(X))
    monkeypatch.delenv(KNOB, raising=False)
    V1, keep1 = _smoother(stfem, op, p, p.lin)
    assert V1.setup_batches == 1
    one = _apply(op, p, V1, X)
    monkeypatch.setenv(KNOB, str(layers))
    Vn, keepn = _smoother(stfem, op, p, p.lin)
    batches = -(-p.nc[2] // layers)
    assert batches > 1 and Vn.setup_batches == batches  # the knob took effect
    assert Vn.n_classes == int(np.prod(p.nc))
    got = _apply(op, p, Vn, X)
    err = rel(got, want)
    print(f"{name} {layers} layers per batch: rel-L2 vs dense reference {err:.3e}, one batch {rel(one, want):.3e}")
    assert np.array_equal(got, one)
    assert err < 1e-10
    # update() (fresh = false) runs the same loop: the one-batch smoother updated to new states under the knob against a fresh
    # one-batch create
    q = svr.problem(STOKES[name], seed=12)
    lin2 = _device(op, p, q.lin) if p.mode else None
    V1.update(lin2)
    assert V1.setup_batches == batches
    upd = _apply(op, p, V1, X)
    monkeypatch.delenv(KNOB, raising=False)
    W, keepw = _smoother(stfem, op, p, q.lin)
    fresh = _apply(op, p, W, X)
    assert np.array_equal(upd, fresh)
    if p.mode:
        assert rel(upd, got) > 1e-6  # the blocks did change
    else:
        assert np.array_equal(upd, got)
