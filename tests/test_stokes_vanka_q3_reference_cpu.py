"""The dense restatement of the degree-3 per-cell Stokes smoother (tests/stokes_vanka_q3_reference.py) checked by properties on the
CPU, and the condition numbers of its blocks, which are the footing of the 1e-10 of tests/test_gpu_stokes_vanka_q3.py: that tolerance
is the one tests/test_gpu_stokes_vanka_linearised.py holds at cond 1.2e5, and it carries over while the blocks stay within a factor of
ten of that, 1.2e6 (this file prints the conditions; the largest is box221_q2_dg0 at 1.0e6, the others 1.3e2 ... 5.5e5)."""
import numpy as np
import pytest

import stokes_vanka_q3_reference as q3r


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.mark.parametrize("name", list(q3r.CASES))
def test_blocks_are_regular(name, oracle_mod):
    """every case keeps the footing of the GPU tolerance: rows as tabulated, one block per cell, cond below ten times 1.2e5"""
    p, ref = q3r.case(name)
    print(name, "rows", ref.rows, "cond_max %.2e" % ref.cond_max)
    assert ref.rows == p.rows == sum(192 if v == 0 else (10 if p.dg else 27) for v in p.var)
    assert len(ref.blocks) == int(np.prod(p.nc))
    assert ref.cond_max < q3r.COND_BOUND


@pytest.mark.parametrize("name", ["cell_free_dgp", "cell_free_q2"])
def test_one_unconstrained_cell_is_the_exact_inverse(name, oracle_mod):
    p, ref = q3r.case(name)
    rng = np.random.default_rng(2)
    x = [rng.uniform(-1, 1, n) for n in p.sizes]
    y = ref.vmult(q3r.st_vmult(p, x))
    err = rel(np.concatenate(y), np.concatenate(x))
    print(name, "V A x - x: %.3e" % err)
    assert err < 100 * np.finfo(float).eps * ref.cond_max


def test_relaxation_history_decreases(oracle_mod):
    """x <- x + omega V (f - A x) on the perturbed 2 x 2 x 2 mesh with FE_DGP(2): the residual norms decrease monotonically at
    omega 0.5 (12.68 7.098 4.305 2.729 1.83 1.291 0.9458 0.7132) and at omega 0.7.  At omega = 1 the
    norms go 12.68 6.477 3.42 1.796 1.158 0.8628 0.709 0.6014 and stall at 0.2524 from sweep 30 on - still without rising in 40
    sweeps, so monotonicity does not tell omega = 1 from the others in eight sweeps; that history is printed, not asserted."""
    p, ref, f, norms = q3r.relaxation()
    print("omega 0.5:", " ".join("%.4g" % v for v in norms))
    assert all(b < a for a, b in zip(norms, norms[1:]))
    assert np.allclose(norms, [12.7, 7.10, 4.31, 2.73, 1.83, 1.29, 0.946, 0.713], rtol=5e-3)  # (recorded to three digits)
    n07 = q3r.relaxation_history(p, ref, f, 0.7)
    print("omega 0.7:", " ".join("%.4g" % v for v in n07))
    assert all(b < a for a, b in zip(n07, n07[1:]))
    n10 = q3r.relaxation_history(p, ref, f, 1.0)
    print("omega 1.0:", " ".join("%.4g" % v for v in n10))
