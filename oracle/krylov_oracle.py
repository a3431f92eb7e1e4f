"""Plain numpy reference of the Krylov and plane entry points of the C-ABI (stfem_dot, stfem_multi_dot, stfem_multi_axpy,
stfem_orthogonalize, stfem_tensorproduct_add, stfem_plane_pack, stfem_plane_unpack, stfem_planes_move) on (n_blocks, n_dofs)
arrays, with the same n_own, add and add_mask arguments.

Precision of the reference.  Nothing here depends on np.longdouble.
 - Inner products: every product a_i b_i is split into its rounded value and its exact error term (Dekker's product on
   Veltkamp-split factors: value + error == a_i b_i exactly, barring underflow), and all values and error terms are added with
   math.fsum, which returns the correctly rounded sum.  `Exact.value` is therefore the double nearest to the exact inner
   product, and `Exact.residual` (a second fsum over the same terms and -value) is what the rounding left out.
 - Elementwise updates (multi_axpy, orthogonalize_pass, tensorproduct_add): accumulated in double-double arithmetic
   (Knuth's two-sum and Dekker's product), relative error about 2^-100 per operation; `value + residual` is the result.
 - `Exact.magnitude` is the sum of the absolute values of the terms (sum |a_i b_i|, or |y_i| + sum_v |c_v x_v,i|): the
   quantity every rounding-error bound of tests/test_gpu_krylov_kernels.py is proportional to.

The second half emulates, in double precision, the ORDER in which the kernels add (multi_dot_kernel and dot_finish_kernel of
csrc/stfem_vector.hip: per-thread strided sums over the blocks, the 64-lane tree, four waves, per-thread strided sum of the
partials, the 256-wide tree) and the roundings of multi_axpy_kernel and axpy_kernel.  tests/test_krylov_oracle_cpu.py uses it to
show that such a summation satisfies the bounds before the device is asked to; the GPU tests do not use it."""
import collections
import math

import numpy as np

Exact = collections.namedtuple("Exact", "value residual magnitude")

# launch geometry of csrc/stfem_vector.hip (DOT_VECS, DOT_GRID: csrc/stfem_internal.h)
DOT_VECS, DOT_GRID, WORKGROUP, MAX_BLOCKS = 8, 512, 256, 8


def round_to(number, a):
    """a as the device holds it: rounded to float for number == 'float', returned as float64"""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if number == "float" else a


def owned(n, n_own):
    """the C-ABI's rule: n_own <= 0 or n_own > n means all n entries"""
    return n if n_own <= 0 or n_own > n else int(n_own)


# ----------------------------------------------------------------------------------------- the tests' input families

def seeded_blocks(seed, nb, n, number="double"):
    """uniform in [-1, 1] scaled by position (1 + i / n): a dropped, duplicated or shifted entry changes a sum by about 1 / N of
    the absolute sum; rounded to the context's Number, so that the reference sees what the device sees"""
    rng = np.random.default_rng(seed)
    return round_to(number, rng.uniform(-1, 1, (nb, n)) * (1 + np.arange(n) / n))


def cancelling_partner(a, seed, number="double", n_own=0, target=1e-12):
    """b (of a's shape and family) with <a, b> over the owned range close to `target` times sum |a_i b_i|: the component along a
    is taken out of a seeded b, then single entries of b are corrected, each time the one with the smallest |a_i| that can take
    the correction, until the number format allows no better"""
    a = np.atleast_2d(a)
    n = owned(a.shape[1], n_own)
    b = seeded_blocks(seed, a.shape[0], a.shape[1], number)
    b[:, :n] = round_to(number, b[:, :n] - (np.sum(a[:, :n] * b[:, :n]) / np.sum(a[:, :n] ** 2)) * a[:, :n])
    order = [(blk, i) for blk, i in zip(*np.unravel_index(np.argsort(np.abs(a[:, :n]), axis=None), (a.shape[0], n))) if a[blk, i] != 0.0]
    used = set()
    for _ in range(4):
        value, magnitude = _dot_terms(a, b, n)[1:]
        want = target * magnitude
        if abs(value - want) <= 0.1 * want:
            break
        for blk, i in order:
            delta = (value - want) / a[blk, i]
            if (blk, i) not in used and abs(delta) <= 0.25:
                b[blk, i] = round_to(number, b[blk, i] - delta)
                used.add((blk, i))
                break
    return b


# ----------------------------------------------------------------------------------------- error-free building blocks

def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """(p, e): p = fl(a b), p + e == a b exactly"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def two_sum(a, b):
    """(s, t): s = fl(a + b), s + t == a + b exactly"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _dd_add(hi, lo, p, e):
    """(hi, lo) + (p, e) in double-double"""
    s, t = two_sum(hi, p)
    t = t + (lo + e)
    hi = s + t
    return hi, t - (hi - s)


# ----------------------------------------------------------------------------------------- the reference proper

def _dot_terms(a, b, n):
    """(the products and their error terms, their correctly rounded sum, sum |a_i b_i|) over the first n entries of every block"""
    p, e = two_prod(a[:, :n].ravel(), b[:, :n].ravel())
    terms = p.tolist() + e[e != 0.0].tolist()
    return terms, math.fsum(terms), float(np.sum(np.abs(p)))


def dot(a, b, n_own=0):
    """sum over all blocks of sum_{i < n_own} a_i b_i -> Exact"""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape
    terms, value, magnitude = _dot_terms(a, b, owned(a.shape[1], n_own))
    return Exact(value, math.fsum(terms + [-value]), magnitude)


def multi_dot(vs, w, n_own=0):
    """[<v_i, w>] -> list of Exact"""
    return [dot(v, w, n_own) for v in vs]


def multi_axpy(coef, xs, y):
    """y + sum_v coef_v x_v, elementwise -> Exact of arrays"""
    y = np.asarray(y, dtype=np.float64)
    hi, lo, mag = y.copy(), np.zeros_like(y), np.abs(y)
    for c, x in zip(coef, xs):
        p, e = two_prod(np.float64(c), np.asarray(x, dtype=np.float64))
        hi, lo = _dd_add(hi, lo, p, e)
        mag = mag + np.abs(p)
    return Exact(hi, lo, mag)


def orthogonalize_pass(vs, w, n_own=0, h=None):
    """One classical Gram-Schmidt pass: the inner products over the owned range, the update w - sum_i h_i v_i over the whole
    vector.  h: the coefficients to project with (default: the exact inner products, rounded).
    -> (list of Exact h, Exact <w, w> before, Exact of arrays: the projected vector)"""
    hs = multi_dot(vs, w, n_own)
    if h is None:
        h = [x.value for x in hs]
    return hs, dot(w, w, n_own), multi_axpy([-float(x) for x in h], vs, w)


def tensorproduct_add(c, A, b, number="double"):
    """c_i + sum_j A(i, j) b_j with A rounded to the context's Number first, as the library does; A(i, j) == 0 means b_j is not
    read (NaN and Inf in such a block do not spread) -> Exact of arrays"""
    A = round_to(number, A)
    c, b = np.asarray(c, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert A.shape == (c.shape[0], b.shape[0])
    hi, lo, mag = c.copy(), np.zeros_like(c), np.abs(c)
    for i in range(A.shape[0]):
        for j in range(A.shape[1]):
            if A[i, j] != 0.0:
                p, e = two_prod(A[i, j], b[j])
                hi[i], lo[i] = _dd_add(hi[i], lo[i], p, e)
                mag[i] = mag[i] + np.abs(p)
    return Exact(hi, lo, mag)


def _number(number):
    return np.float32 if number == "float" else np.float64


def plane_pack(v, iz, plane):
    """(n_blocks, plane): DoF plane iz of every block"""
    return np.asarray(v)[:, iz * plane:(iz + 1) * plane].copy()


def plane_unpack(v, iz, buf, add, plane, number="double"):
    """v with plane iz of every block replaced by buf (add == 0) or increased by it (one addition in the context's Number)"""
    T = _number(number)
    out = np.array(v, dtype=np.float64)
    sl = slice(iz * plane, (iz + 1) * plane)
    buf = np.asarray(buf, dtype=np.float64).reshape(out.shape[0], plane)
    out[:, sl] = (out[:, sl].astype(T) + buf.astype(T)).astype(np.float64) if add else buf
    return out


def planes_move(src, iz_src, dst, iz_dst, nplanes, add_mask, plane, number="double"):
    """dst with planes [iz_dst, iz_dst + nplanes) taken from src's [iz_src, ...); bit 0 of add_mask: the first plane of the range
    is added to the destination's, bit 1: the last one (a range of one plane is both)"""
    out = np.array(dst, dtype=np.float64)
    for q in range(nplanes):
        add = (q == 0 and add_mask & 1) or (q == nplanes - 1 and add_mask & 2)
        out = plane_unpack(out, iz_dst + q, plane_pack(src, iz_src + q, plane), 1 if add else 0, plane, number)
    return out


# ----------------------------------------------------------------------------------------- the kernels' order, in double

def dot_grid(n_own):
    return min(-(-n_own // WORKGROUP), DOT_GRID)


def _fma(a, b, s):
    """fl(a b + s) up to the rounding of the low-order parts (numpy has no fma; a product of two floats is exact anyway)"""
    p, e = two_prod(a, b)
    r, t = two_sum(p, s)
    return r + (t + e)


def dot_kernel_order(a, b, n_own=0):
    """stfem_dot / one entry of stfem_multi_dot for at most eight blocks, added in the order of multi_dot_kernel and
    dot_finish_kernel; more than eight blocks: eight at a time, the parts added on the host (stfem_dot's split path)"""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
    if a.shape[0] > MAX_BLOCKS:
        total = 0.0
        for j0 in range(0, a.shape[0], MAX_BLOCKS):
            total += dot_kernel_order(a[j0:j0 + MAX_BLOCKS], b[j0:j0 + MAX_BLOCKS], n_own)
        return total
    n = owned(a.shape[1], n_own)
    grid = dot_grid(n)
    stride = grid * WORKGROUP
    s = np.zeros(stride)
    for blk in range(a.shape[0]):  # every thread: its entries of block 0, then of block 1, ...
        for start in range(0, n, stride):
            m = min(stride, n - start)
            s[:m] = _fma(a[blk, start:start + m], b[blk, start:start + m], s[:m])
    s = s.reshape(grid, WORKGROUP // 64, 64)
    off = 32
    while off > 0:  # __shfl_down: lane 0 ends with the tree sum of its wave
        s[:, :, :off] = s[:, :, :off] + s[:, :, off:2 * off]
        off >>= 1
    r = s[:, :, 0]
    partial = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    red = np.zeros(WORKGROUP)
    for start in range(0, grid, WORKGROUP):  # dot_finish_kernel: thread t adds partial[t], partial[t + 256], ...
        m = min(WORKGROUP, grid - start)
        red[:m] = red[:m] + partial[start:start + m]
    w = WORKGROUP // 2
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w >>= 1
    return float(red[0])


def multi_axpy_kernel_order(coef, xs, y, number="double"):
    """multi_axpy_kernel: groups of eight vectors per launch, every launch accumulates in double and rounds to Number once"""
    T = _number(number)
    y = np.asarray(y, dtype=np.float64).astype(T)
    for k0 in range(0, len(xs), DOT_VECS):
        acc = y.astype(np.float64)
        for c, x in zip(coef[k0:k0 + DOT_VECS], xs[k0:k0 + DOT_VECS]):
            acc = _fma(np.float64(c), np.asarray(x, dtype=np.float64), acc)
        y = acc.astype(T)
    return y.astype(np.float64)


def tensorproduct_add_kernel_order(c, A, b, number="double"):
    """axpy_kernel: one fma in Number per non-zero A(i, j), eight columns per launch"""
    T = _number(number)
    A = np.asarray(A, dtype=np.float64).astype(T)
    out = np.asarray(c, dtype=np.float64).astype(T)
    bT = np.asarray(b, dtype=np.float64).astype(T)
    for i in range(A.shape[0]):
        for j in range(A.shape[1]):
            if A[i, j] != 0:
                if T is np.float32:  # the product of two floats is exact in double, one rounding to float: an fma
                    out[i] = (A[i, j].astype(np.float64) * bT[j].astype(np.float64) + out[i].astype(np.float64)).astype(T)
                else:
                    out[i] = _fma(A[i, j], bT[j], out[i])
    return out.astype(np.float64)
