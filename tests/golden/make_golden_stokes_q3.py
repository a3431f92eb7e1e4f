#!/usr/bin/env python3
"""Golden fixtures of the Stokes two-field operator at velocity degree 3, from FIRST PRINCIPLES: the dense numpy assembly of
make_golden_stokes.py (full 3D shape-function tables, independent of oracle/*.c and of the HIP library) with pu = 3.

Velocity FE_Q(3)^3, pressure FE_Q(2) and FE_DGP(2) (both in every file), QGauss(4), MappingQ1; the pair the reference builds for
time degree 2 (tests/tp_03stokes.cc:79-86).  Space-time: cG(2), one time step (two time dofs), laid out as
get_fe_time_weights_stokes does.

Fields, like the FE_Q(2) fixtures: ncell, vertices, mask, nu, nt, Alpha, Beta, U [nt, 3, NU], MU [nt, 3, NU] and, per pressure
space, P [nt, NP], SU, SP (the operator), DU, DP (the space-time product); the FE_DGP(2) ones carry the suffix _dgp.

Run:  python tests/golden/make_golden_stokes_q3.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import structured_vertices, time_weights_single  # noqa: E402
from make_golden_stokes import block_index, dense_stokes, stokes_apply  # noqa: E402


def main():
    cases = [
        # name, ncell, lower, upper, jitter, mask, nu, tau
        ("stokes_q3_cart_2x2x2", (2, 2, 2), (0, 0, 0), (1, 1.5, 0.7), 0.0, 63, 1.0, 0.1),
        ("stokes_q3_pert_2x3x2", (2, 3, 2), (0, 0, 0), (1, 1, 1), 0.15, 0b111011, 0.05, 1 / 16),
        ("stokes_q3_free_3x2x2", (3, 2, 2), (-1, -1, -1), (1, 1, 1), 0.1, 0, 2.5, 0.25),
    ]
    for (name, ncell, lo, up, jit, mask, nu, tau) in cases:
        rng = np.random.default_rng(sum(map(ord, name)))
        verts = structured_vertices(ncell, lo, up, jit, seed=37)
        At, Bt = time_weights_single("cg", 2, tau)
        nt = At.shape[0]
        nb = 2 * nt
        Alpha = np.zeros((nb, nb)); Beta = np.zeros((nb, nb))
        for iv in range(2):
            for jv in range(2):
                if not (iv == 1 and jv == 1):
                    for a in range(nt):
                        for b in range(nt):
                            Alpha[block_index(nt, 2, 0, iv, a), block_index(nt, 2, 0, jv, b)] = At[a, b]
        for a in range(nt):
            for b in range(nt):
                Beta[block_index(nt, 2, 0, 0, a), block_index(nt, 2, 0, 0, b)] = Bt[a, b]
        out = dict(ncell=np.array(ncell), vertices=verts, mask=mask, nu=nu, nt=nt, Alpha=Alpha, Beta=Beta)
        U = None
        for dgp, sfx in ((False, ""), (True, "_dgp")):
            K, M, B = dense_stokes(3, ncell, verts, mask, dgp=dgp)
            NU, NP = K.shape[0], B.shape[1]
            if U is None:
                U = rng.uniform(-1, 1, size=(nt, 3, NU))
            P = rng.uniform(-1, 1, size=(nt, NP))
            DU = np.zeros((nt, 3, NU)); DP = np.zeros((nt, NP))
            SU = np.zeros((nt, 3, NU)); SP = np.zeros((nt, NP)); MU = np.zeros((nt, 3, NU))
            for i in range(nt):
                ou, op, mu = stokes_apply(K, M, B, nu, U[i], P[i])
                SU[i], SP[i], MU[i] = ou, op, mu
                col = block_index(nt, 2, 0, 0, i)
                for j in range(nt):
                    DU[j] += Alpha[block_index(nt, 2, 0, 0, j), col] * ou + Beta[block_index(nt, 2, 0, 0, j), col] * mu
                    DP[j] += Alpha[block_index(nt, 2, 0, 1, j), col] * op
            out.update({"U": U, "MU": MU, "P" + sfx: P, "SU" + sfx: SU, "SP" + sfx: SP, "DU" + sfx: DU, "DP" + sfx: DP})
            print(name, "dgp" if dgp else "q2", "NU", NU, "NP", NP, "nt", nt, "|K|", np.abs(K).max(), "|B|", np.abs(B).max())
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


if __name__ == "__main__":
    main()
