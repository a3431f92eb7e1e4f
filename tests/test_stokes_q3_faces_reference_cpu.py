"""What the GPU tests of the weak faces at velocity degree 3 stand on (tests/stokes_q3_faces_reference.py), checked without a GPU:
the Vanka restatement with weak_mask = 0 is the existing one, the oracle's faces are consistent with the strong form on an affine
mesh, and the blocks of every Vanka case stay under the conditioning cap behind the 1e-10 of the smoother tests."""
import numpy as np
import pytest

import stokes_q3_faces_reference as fr
import stokes_vanka_q3_reference as q3r


def test_without_weak_faces_the_reference_is_the_existing_one(oracle_mod):
    p, old = q3r.case("pert222_dgp_cg2")
    new = fr.StokesVankaQ3FacesReference(p.nc, p.verts, p.mask, p.nu, p.var, p.Alpha, p.Beta, dg_pressure=p.dg, weak_mask=0)
    assert np.array_equal(new.K, old.K) and np.array_equal(new.M, old.M)
    assert len(new.blocks) == len(old.blocks) and all(np.array_equal(a, b) for a, b in zip(new.blocks, old.blocks))
    assert new.cond_max == old.cond_max and new.rows == old.rows


@pytest.mark.parametrize("dgp", fr.DGP, ids=fr.DGP_IDS)
def test_consistency_identity_of_the_oracle(dgp, oracle_mod):
    """u = (y^2, z^2, x^2), p = x + 2 y z (FE_Q(2)) or 0 (FE_DGP(2)), g = u on all six weak faces of an affinely sheared 2 x 1 x 2 mesh:
    vmult(u, p) - nitsche_rhs(g) = M (- nu Laplace u + grad p) and the pressure rows vanish, to 1e-12 max|vmult| (the oracle: 1.7e-15
    against max|vmult| = 3.0)"""
    orc = fr.identity_oracle(dgp)
    U, P, F, g = fr.identity_fields(dgp)
    ku, kp = orc.apply(U, P)
    ru, rp = orc.nitsche_rhs(g(orc.face_points()))
    mf, _ = orc.apply(F, np.zeros(orc.n_p), 0.0, 1.0)
    scale = max(np.abs(ku).max(), np.abs(kp).max())
    dev_u, dev_p = np.abs(ku - ru - mf).max(), np.abs(kp - rp).max()
    print("FE_DGP" if dgp else "FE_Q", "max|vmult| %.3f deviation u %.2e p %.2e" % (scale, dev_u, dev_p))
    assert scale > 1.0 and np.abs(ru).max() > 0.1 * scale  # the faces carry a real share
    assert max(dev_u, dev_p) <= 1e-12 * scale


@pytest.mark.parametrize("name", list(fr.VANKA_CASES))
def test_conditioning_cap(name, oracle_mod):
    p, ref = fr.case(name)
    print(name, "rows", ref.rows, "cond_max %.3e" % ref.cond_max)
    assert ref.rows == p.rows
    assert ref.cond_max < fr.COND_BOUND


def test_relaxation_with_faces_decreases(oracle_mod):
    _, _, _, norms = fr.relaxation()
    print("history:", " ".join("%.6e" % v for v in norms))
    assert all(b < a for a, b in zip(norms, norms[1:]))
