"""The dense restatement of the linearised per-cell Stokes smoother (tests/stokes_vanka_reference.py) checked by properties on the CPU,
and the condition numbers of its blocks, which set the tolerance of tests/test_gpu_stokes_vanka_linearised.py.

Recorded (this file prints them): the largest cond(B_c) is 1.15e5 over the linearised cases (perturbed 3 x 2 x 2, jacobian, weak faces;
the others 1.3e2 ... 2.5e4) against 1.12e5 over the plain Stokes cases of tests/test_gpu_stokes_vanka.py (cG(2), weak faces) - within a
factor of 10, so the GPU test keeps that file's 1e-10."""
import numpy as np
import pytest

import stokes_vanka_reference as svr
import navier_reference as nref


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300)


# the cases of tests/test_gpu_stokes_vanka.py on unit cubes, in the layout of svr.CASES (all mode 0, boxes); its first one, cG(1) on
# 3 x 3 x 3 cells, is svr.CASES["box333"]
STOKES_CASES = {
    "cg2_322_weak": ((3, 2, 2), False, 0, False, 0, 2, 1, 63 & ~3, 3, False),
    "dgp_223": ((2, 2, 3), False, 0, True, 0, 1, 1, 63, 0, True),
    "dg1_222_2steps": ((2, 2, 2), False, 0, True, 1, 1, 2, 63, 0, True),
    "cell": ((1, 1, 1), False, 0, True, 0, 1, 1, 0, 0, True),
}


@pytest.mark.parametrize("name", ["box333", "pert232"])
def test_mode0_blocks_equal_the_stokes_oracle_bitwise(name, oracle_mod):
    from oracle import vanka_oracle
    p, ref = svr.case(name)
    want = vanka_oracle.StokesVankaOracle(p.nc, p.verts, p.mask, p.nu, p.var, p.Alpha, p.Beta, weak_mask=p.weak, dg_pressure=p.dg)
    assert len(ref.blocks) == len(want.blocks) == int(np.prod(p.nc))
    for a, b in zip(ref.blocks, want.blocks):
        assert np.array_equal(a, b)


def test_one_unconstrained_cell_is_the_exact_inverse(oracle_mod):
    p, ref = svr.case("cell_jac_dgp")
    rng = np.random.default_rng(2)
    x = [rng.uniform(-1, 1, n) for n in p.sizes]
    y = ref.vmult(svr.st_vmult(p, x))
    assert rel(np.concatenate(y), np.concatenate(x)) < 100 * np.finfo(float).eps * ref.cond_max


def test_jacobian_columns_are_form_b_u_plus_form_u_b(oracle_mod):
    nc = (2, 1, 2)
    verts = nref.perturbed_vertices(nc, 0.15, 4)
    n = 3 * nref.n_velocity(nc)
    rng = np.random.default_rng(8)
    b = rng.uniform(-1, 1, n)
    weak = 1 | 32
    for j in rng.choice(n, 12, replace=False):
        e = np.zeros(n)
        e[j] = 1.0
        jac = nref.convection(nref.JACOBIAN, b, e, nc, verts, 0, weak)
        # C_form(b, e) + C_form(e, b); the inflow term of the faces is that of C_form(b, .) alone (operators.h:1738-1743)
        both = nref.convection(nref.FORM, b, e, nc, verts, 0, weak) + nref.convection_cells(nref.FORM, e, b, nc, verts, 0).reshape(-1)
        assert np.linalg.norm(jac - both) <= 1e-14 * max(np.linalg.norm(jac), 1.0)


def test_the_relaxation_history_decreases(oracle_mod):
    _, _, _, norms = svr.relaxation()
    print("relaxation history:", " ".join("%.4e" % v for v in norms))
    assert all(b < a for a, b in zip(norms, norms[1:])), norms
    assert norms[-1] < 0.5 * norms[0], norms


def test_condition_numbers_of_the_blocks(oracle_mod):
    """prints the largest cond(B_c) of every case; the linearised cases stay within 10x of the plain Stokes cases' own"""
    lin = {name: svr.case(name)[1].cond_max for name in svr.CASES}
    lin["relaxation"] = svr.relaxation()[1].cond_max
    stokes = {name: svr.reference(svr.problem(spec)).cond_max for name, spec in STOKES_CASES.items()}
    stokes["cg1_333"] = lin["box333"]
    for title, table in (("linearised", lin), ("stokes", stokes)):
        for name, c in table.items():
            print("cond_max %-10s %-24s %.3e" % (title, name, c))
    assert max(lin.values()) <= 10.0 * max(stokes.values())
