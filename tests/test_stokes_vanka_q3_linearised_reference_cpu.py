"""The dense restatement of the degree-3 per-cell smoother of the LINEARISED Stokes operator
(tests/stokes_vanka_q3_linearised_reference.py) checked by properties on the CPU: its convection matrix against the independent
restatement of the operator's modes, its mode-0 blocks against tests/stokes_vanka_q3_reference.py, the condition numbers of its blocks -
the footing of the 1e-10 of tests/test_gpu_stokes_vanka_q3_linearised.py, which carries over from tests/test_gpu_stokes_vanka_q3.py while
they stay below its COND_BOUND = 1.2e6 -, that the convection term is visible in every case, and that the relaxation history of the GPU
test decreases.  No GPU."""
import numpy as np
import pytest

import navier_q3_reference as nq3
import navier_reference as nref
import stokes_vanka_q3_linearised_reference as lq3
import stokes_vanka_q3_reference as q3r


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.mark.parametrize("mask", [0, 63 & ~3, 63])
@pytest.mark.parametrize("mode", [lq3.FORM, lq3.JACOBIAN])
def test_convection_matrix_is_the_convection_term(mode, mask):
    """C(b) u = navier_q3_reference.convection(3, mode, b, u) on a perturbed 2 x 2 x 2 mesh: u read with its constrained entries as 0
    and the constrained rows dropped, as the operator does it; 1e-13 relative"""
    nc = (2, 2, 2)
    verts = nref.perturbed_vertices(nc, lq3.DISTORT, 21)
    n_u = q3r.n_velocity(nc)
    rng = np.random.default_rng(4)
    b, u = rng.uniform(-1, 1, 3 * n_u), rng.uniform(-1, 1, 3 * n_u)
    cu = np.tile(q3r.constrained(nc, mask), 3)
    Cm = lq3.convection_matrix(mode, b, nc, verts, mask)
    got = Cm @ np.where(cu, 0.0, u)
    got[cu] = 0.0
    want = nq3.convection(3, mode, b, u, nc, verts, mask)
    print("mode", mode, "mask", mask, "C(b) u vs convection: %.3e" % rel(got, want), "|C(b) u| = %.3e" % np.linalg.norm(want))
    assert np.linalg.norm(want) > 0 and rel(got, want) < 1e-13


@pytest.mark.parametrize("name", ["pert222_dgp_cg2", "box322_q2"])
def test_mode_0_is_the_linear_reference_exactly(name, oracle_mod):
    p, base = q3r.case(name)
    ref = lq3.reference(p, base, 0, None)
    assert len(ref.blocks) == len(base.blocks) and all(np.array_equal(a, b) for a, b in zip(ref.blocks, base.blocks))


@pytest.mark.parametrize("name", list(lq3.CASES))
def test_blocks_are_regular_and_the_term_is_visible(name, oracle_mod):
    """every case keeps the footing of the GPU tolerance (cond below q3r.COND_BOUND) and shows the term: the apply with the mode differs
    from the mode-0 apply by at least 1e-4 of its norm.  Measured here with b_scale = 1: cond_max 1.3e2 ... 1.0e6, within 1 % of the
    linear blocks'; the difference of the applies is printed."""
    p, mode, lin, ref, base = lq3.case(name)
    assert ref.rows == p.rows and len(ref.blocks) == int(np.prod(p.nc))
    n_states = len({id(b) for b in lin if b is not None})
    assert len(ref.K) == n_states == p.ns * p.nt
    rng = np.random.default_rng(3)
    X = [rng.uniform(-1, 1, n) for n in p.sizes]
    y, y0 = np.concatenate(ref.vmult(X)), np.concatenate(base.vmult(X))
    last = rel(ref.blocks[-1], base.blocks[-1])
    print(name, "mode", mode, "cond_max %.2e (linear %.2e)" % (ref.cond_max, base.cond_max), "apply differs %.2e" % rel(y, y0),
          "last block inverse differs %.2e" % last)
    assert ref.cond_max < lq3.COND_BOUND
    assert rel(y, y0) >= lq3.VISIBLE


@pytest.mark.parametrize("name", ["cell_free_dgp", "cell_free_q2"])
def test_one_unconstrained_cell_is_the_exact_inverse(name, oracle_mod):
    p, mode, lin, ref, _ = lq3.case(name)
    rng = np.random.default_rng(2)
    x = [rng.uniform(-1, 1, n) for n in p.sizes]
    y = ref.vmult(lq3.st_vmult(p, mode, lin, x))
    err = rel(np.concatenate(y), np.concatenate(x))
    print(name, "V A(b) x - x: %.3e" % err)
    assert err < 100 * np.finfo(float).eps * ref.cond_max


def test_relaxation_history_decreases(oracle_mod):
    """x <- x + 0.5 V (f - A(b) x), jacobian about 0.5 uniform(-1, 1), on the perturbed 2 x 2 x 2 mesh with FE_DGP(2), cG(1), nu = 1: the
    residual norms decrease monotonically, and the term moves them off the linear history of q3r.relaxation()"""
    p, mode, lin, ref, f, norms = lq3.relaxation()
    linear = q3r.relaxation()[3]
    print("jacobian:", " ".join("%.6g" % v for v in norms))
    print("linear:  ", " ".join("%.6g" % v for v in linear))
    assert len(norms) == q3r.RELAX_SWEEPS and all(b < a for a, b in zip(norms, norms[1:]))
    assert ref.cond_max < lq3.COND_BOUND
    assert not np.allclose(norms[1:], linear[1:], rtol=1e-6)
