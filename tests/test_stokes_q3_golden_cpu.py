"""The yardstick of the degree-3 Stokes pair FE_Q(3)^3 x FE_Q(2) / FE_DGP(2): the CPU oracle at pu = 3 against the dense numpy
assembly behind tests/golden/stokes_q3_*.npz (tests/golden/make_golden_stokes_q3.py), both pressure spaces.  rel-L2 <= 1e-12 per
block (fp64; the two differ by a few 1e-15 at these sizes).  No GPU."""
import os

import numpy as np
import pytest

TOL = 1e-12
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["stokes_q3_cart_2x2x2", "stokes_q3_pert_2x3x2", "stokes_q3_free_3x2x2"]


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


@pytest.mark.parametrize("dgp", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_pu3_reproduces_the_dense_assembly(name, dgp):
    from oracle import oracle
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sfx = "_dgp" if dgp else ""
    nc, nt = tuple(int(v) for v in g["ncell"]), int(g["nt"])
    orc = oracle.StokesOracle(nc, g["vertices"], int(g["mask"]), float(g["nu"]), pu=3, dg_pressure=dgp)
    assert orc.n_u == g["U"].shape[2] == np.prod([3 * n + 1 for n in nc])
    assert orc.n_p == g["P" + sfx].shape[1] == (10 * np.prod(nc) if dgp else np.prod([2 * n + 1 for n in nc]))
    for i in range(nt):
        ku, kp = orc.apply(g["U"][i], g["P" + sfx][i])
        mu, _ = orc.apply(g["U"][i], g["P" + sfx][i], 0.0, 1.0)
        assert rel(ku, g["SU" + sfx][i]) < TOL and rel(kp, g["SP" + sfx][i]) < TOL and rel(mu, g["MU"][i]) < TOL
    # SystemMatrixStokes::vmult with the cG(2) weights of the fixture, variable-major blocks
    blocks = [g["U"][d].reshape(-1) for d in range(nt)] + [g["P" + sfx][d] for d in range(nt)]
    dst = orc.st_vmult(g["Alpha"], g["Beta"], 1, nt, blocks, True)
    for d in range(nt):
        assert rel(dst[d], g["DU" + sfx][d]) < TOL and rel(dst[nt + d], g["DP" + sfx][d]) < TOL
