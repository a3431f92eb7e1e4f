"""oracle/krylov_oracle.py checked by itself (no GPU): the exact reference against fractions.Fraction on small inputs, and the
double-precision emulation of the kernels' summation order against the bounds of tests/test_gpu_krylov_kernels.py on every input
family that file uses: the reference alone satisfies the bounds before the device is asked to."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import krylov_oracle as K

NUMBERS = ["double", "float"]
U64, U32 = 2.0 ** -53, 2.0 ** -24  # unit roundoffs
# `magnitude` only scales the bounds, so it is a plain double sum of rounded products: one rounding per product and at most
# n - 1 roundings of positive partial sums, relative error <= n u; n <= 128 = 2^7 terms in the tests that check it
MAGNITUDE_RTOL = Fraction(2) ** (7 - 53)


def frac(a):
    return [[Fraction(float(x)) for x in row] for row in np.atleast_2d(a)]


def inner_product_bound(nb, n_own, magnitude):
    """(m + 18) 2^-53 sum |a_i b_i|: the bound of the GPU file (derivation there)"""
    m = nb * -(-n_own // (K.dot_grid(n_own) * K.WORKGROUP))
    return (m + 18) * U64 * magnitude


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("nb,n,n_own", [(1, 1, 0), (1, 8, 0), (3, 37, 0), (3, 37, 20), (2, 64, 65), (2, 64, -3)])
def test_exact_dot_against_fractions(number, nb, n, n_own):
    a = K.seeded_blocks(1, nb, n, number)
    for b in (K.seeded_blocks(2, nb, n, number), K.cancelling_partner(a, 3, number, n_own)):
        no = K.owned(n, n_own)
        exact = sum(x * y for ra, rb in zip(frac(a), frac(b)) for x, y in zip(ra[:no], rb[:no]))
        mag = sum(abs(x * y) for ra, rb in zip(frac(a), frac(b)) for x, y in zip(ra[:no], rb[:no]))
        d = K.dot(a, b, n_own)
        assert abs(Fraction(d.value) - exact) <= Fraction(math.ulp(d.value)) / 2  # correctly rounded
        assert abs(Fraction(d.value) + Fraction(d.residual) - exact) <= mag * Fraction(2) ** -100
        assert abs(Fraction(d.magnitude) - mag) <= mag * MAGNITUDE_RTOL
        assert K.multi_dot([a], b, n_own)[0] == d


def test_cancelling_partner_cancels():
    """How close to the target 1e-12 of the absolute sum the partner can come is set by the number format: the last correction
    changes one entry b_i by a multiple of its spacing, at most 2 u |b_i| with u the unit roundoff, so the product lands within
    2 u |a_i b_i| of the target.  The corrected entry has |a_i| <= 2, |b_i| <= 2 + 0.25, and the absolute sum exceeds 0.1 nb n
    (asserted), so the floor is target + 2 u 4.5 / (0.1 nb n): about 1e-12 in double, but only 6e-8 in float at nb n = 175
    (the generator picks the smallest |a_i| that can take the correction, so it usually lands far below that)."""
    target = 1e-12
    for number, u in (("double", U64), ("float", U32)):
        for nb, n in ((1, 175), (3, 256), (1, 3135)):
            a = K.seeded_blocks(4, nb, n, number)
            d = K.dot(a, K.cancelling_partner(a, 5, number, target=target))
            assert d.magnitude > 0.1 * nb * n
            floor = 1.1 * target + 2 * u * 4.5 / (0.1 * nb * n)
            assert abs(d.value) <= floor * d.magnitude, (number, nb, n, d, floor)


@pytest.mark.parametrize("number", NUMBERS)
def test_exact_elementwise_against_fractions(number):
    nb, n, k = 2, 9, 11
    xs = [K.seeded_blocks(10 + v, nb, n, number) for v in range(k)]
    y = K.seeded_blocks(3, nb, n, number)
    coef = np.random.default_rng(7).uniform(-1, 1, k)
    coef[4] = 0.0
    r = K.multi_axpy(coef, xs, y)
    fy, fx = frac(y), [frac(x) for x in xs]
    for blk in range(nb):
        for i in range(n):
            exact = fy[blk][i] + sum(Fraction(float(c)) * x[blk][i] for c, x in zip(coef, fx))
            mag = abs(fy[blk][i]) + sum(abs(Fraction(float(c)) * x[blk][i]) for c, x in zip(coef, fx))
            assert abs(Fraction(r.value[blk, i]) + Fraction(r.residual[blk, i]) - exact) <= mag * Fraction(2) ** -98
            assert abs(Fraction(r.magnitude[blk, i]) - mag) <= mag * MAGNITUDE_RTOL
    # the projected vector of a Gram-Schmidt pass is the same update with -h
    hs, before, proj = K.orthogonalize_pass(xs, y, n_own=5, h=coef)
    assert np.array_equal(proj.value, K.multi_axpy(-coef, xs, y).value)
    assert before.value == K.dot(y, y, 5).value and [h.value for h in hs] == [K.dot(x, y, 5).value for x in xs]
    # tensorproduct_add: A rounded to Number, exact zeros skip their column
    A = np.random.default_rng(8).uniform(-2, 2, (3, 4))
    A[:, 2] = 0.0
    A[1, :] = 0.0
    b = K.seeded_blocks(20, 4, n, number)
    c = K.seeded_blocks(21, 3, n, number)
    b[2, :] = np.nan
    b[2, ::2] = np.inf
    t = K.tensorproduct_add(c, A, b, number)
    At = K.round_to(number, A)
    fc, fb = frac(c), frac(np.where(np.isfinite(b), b, 0.0))
    for i in range(3):
        for q in range(n):
            exact = fc[i][q] + sum(Fraction(float(At[i, j])) * fb[j][q] for j in range(4))
            mag = abs(fc[i][q]) + sum(abs(Fraction(float(At[i, j])) * fb[j][q]) for j in range(4))
            assert abs(Fraction(t.value[i, q]) + Fraction(t.residual[i, q]) - exact) <= mag * Fraction(2) ** -98
    assert np.array_equal(t.value[1], c[1]) and not t.residual[1].any()


# the vector lengths of the GPU file's contexts up to Q2 26^3: 8, 175, 256, a mid size (Q2 9 x 7 x 5), 148 877
LENGTHS = [8, 175, 256, 3135, 148877]


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_order_dot_within_the_bound(number, n):
    plane = {8: 4, 175: 35, 256: 32, 3135: 285, 148877: 2809}[n]  # the DoF planes of the GPU file's meshes
    for nb in ((1, 3, 8, 9, 12) if n < 10000 else (1, 3)):
        a = K.seeded_blocks(1, nb, n, number)
        b = K.seeded_blocks(2, nb, n, number)
        cases = [("seeded", b, n_own) for n_own in ((0, 1, 255, 256, 257, n - plane, n, n + 1, -3) if n < 10000 or nb == 1 else (0, n - plane))
                 if n_own <= n + 1]
        # the GPU file's cancellation cases: a partner built over the whole vector and one over the owned range (test_dot), and
        # the one of test_multi_dot, built against the right-hand vector over the whole vector and used at every n_own
        cases += [("cancelling", K.cancelling_partner(a, 3, number, n_own), n_own) for n_own in (0, n - plane)]
        against_w = K.cancelling_partner(b, 3, number)
        cases += [("cancelling against w", against_w, n_own) for n_own in (0, n - plane)]
        for family, bb, n_own in cases:
            left = b if family == "cancelling against w" else a
            d = K.dot(left, bb, n_own)
            got = K.dot_kernel_order(left, bb, n_own)
            err = abs((got - d.value) - d.residual)
            assert err <= inner_product_bound(nb, K.owned(n, n_own), d.magnitude), (family, nb, n_own, err, d)


def test_kernel_order_dot_sees_every_entry():
    """the emulation is no rubber stamp: a dropped entry or a float accumulator leaves the bound"""
    n = 148877
    a, b = K.seeded_blocks(1, 1, n, "float"), K.seeded_blocks(2, 1, n, "float")
    d = K.dot(a, b)
    bound = inner_product_bound(1, n, d.magnitude)
    a2 = a.copy()
    a2[0, 140000] = 0.0
    assert abs(K.dot_kernel_order(a2, b) - d.value) > bound
    assert abs(float(np.sum((a * b).astype(np.float32), dtype=np.float32)) - d.value) > bound


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("k", [1, 8, 9, 17])
def test_kernel_order_multi_axpy_within_the_bound(number, k):
    nb, n = 2, 3135
    xs = [K.seeded_blocks(10 + v, nb, n, number) for v in range(k)]
    y = K.seeded_blocks(3, nb, n, number)
    coef = np.random.default_rng(k).uniform(-1, 1, k)
    if k > 1:
        coef[k // 2] = 0.0
    r = K.multi_axpy(coef, xs, y)
    got = K.multi_axpy_kernel_order(coef, xs, y, number)
    bound = (k + 1) * U64 * r.magnitude + (-(-k // 8) * U32 * r.magnitude if number == "float" else 0.0)
    assert (np.abs((got - r.value) - r.residual) <= bound).all()


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (3, 2), (8, 8), (2, 9), (12, 12)])
def test_kernel_order_tensorproduct_add_within_the_bound(number, shape):
    n = 3135
    A = np.random.default_rng(shape[0] * 16 + shape[1]).uniform(-2, 2, shape)
    b, c = K.seeded_blocks(20, shape[1], n, number), K.seeded_blocks(21, shape[0], n, number)
    r = K.tensorproduct_add(c, A, b, number)
    got = K.tensorproduct_add_kernel_order(c, A, b, number)
    bound = (shape[1] + 1) * (U32 if number == "float" else U64) * r.magnitude
    assert (np.abs((got - r.value) - r.residual) <= bound).all()


def test_planes_reference():
    plane, nz, nb = 6, 4, 2
    v = np.arange(nb * plane * nz, dtype=np.float64).reshape(nb, plane * nz)
    buf = K.plane_pack(v, 2, plane)
    assert buf.shape == (nb, plane) and buf[1, 0] == plane * nz + 2 * plane
    w = K.plane_unpack(np.ones_like(v), 1, buf, 1, plane)
    assert np.array_equal(w[:, plane:2 * plane], buf + 1) and (np.delete(w, np.s_[plane:2 * plane], axis=1) == 1).all()
    for mask in range(4):
        d = K.planes_move(v, 0, np.ones_like(v), 1, 3, mask, plane)
        for q in range(3):
            add = (q == 0 and mask & 1) or (q == 2 and mask & 2)
            assert np.array_equal(d[:, (1 + q) * plane:(2 + q) * plane], v[:, q * plane:(q + 1) * plane] + (1 if add else 0))
        assert (d[:, :plane] == 1).all()
        one = K.planes_move(v, 3, np.ones_like(v), 0, 1, mask, plane)
        assert np.array_equal(one[:, :plane], v[:, 3 * plane:] + (1 if mask else 0))
    # one addition in float
    x = np.full((1, plane), 1.0)
    assert np.array_equal(K.plane_unpack(x, 0, np.full((1, plane), 2.0 ** -30), 1, plane, "float"), x)
