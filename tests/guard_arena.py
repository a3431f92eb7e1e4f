"""A guarded arena for caller-owned device arrays (helper module of the guard-band tests, not a conftest).

include/stfem.h lets a caller's blocks lie anywhere at element alignment.  The arena places them as *views* inside ONE
allocation, `guard | view | guard | view | ... | guard`, and classifies every byte of it:

  guard        a quiet NaN with a recognisable payload, in the element type of the neighbouring view; compared as raw
               bytes after the call
  source       must be bit-identical after the call
  destination  must equal the expected result

so a stray store anywhere inside the arena is a failing assertion that names the byte, and a stray load that reaches a result
turns it into a NaN.  Layout, fill, classification and the checker are plain numpy on a host byte array (`Arena`); the device
backend (`DeviceMemory`) only copies bytes up and down through a one-block fp64 BlockVector of a helper degree-1 context.

Placements:
  aligned     every view starts on a 256-byte boundary
  packed      every view starts at an odd element index from a 16-byte boundary: 8 mod 16 for fp64, 4 mod 8 for fp32
  descending  packed, and later views lie at lower addresses
"""
import numpy as np

PLACEMENTS = ("aligned", "packed", "descending")

# quiet NaNs (exponent all ones, top mantissa bit set) with payloads nothing computes
GUARD_BITS = {8: 0x7FF80BADC0DE0BAD, 4: 0x7FC0BADD}
POISON_BITS = {8: 0x7FF8D0D0FEEDD0D0, 4: 0x7FC0D0D0}
_UINT = {8: np.uint64, 4: np.uint32}

GUARD_ELEMENTS = 64  # besides two x-y planes of the largest block


def _pattern(bits, itemsize):
    return np.array([bits], dtype=_UINT[itemsize]).view(np.uint8)


def poison(n, dtype):
    """n elements of the destination poison: a NaN that is neither a guard nor a value a kernel produces"""
    dtype = np.dtype(dtype)
    return np.full(n, POISON_BITS[dtype.itemsize], dtype=_UINT[dtype.itemsize]).view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize])


class ArenaError(AssertionError):
    """A finding of the checker: .kind in {guard, source, poison, nan, value, tolerance}, .region, .index, .xyz"""

    def __init__(self, kind, region, index, xyz, detail):
        self.kind, self.region, self.index, self.xyz = kind, region, index, xyz
        where = f"{region}[{index}]" + (f" (x, y, z) = {xyz}" if xyz is not None else "")
        super().__init__(f"{kind}: {where}: {detail}")


class View:
    def __init__(self, name, data, role, shape):
        self.name, self.role = name, role
        self.data = np.ascontiguousarray(data).reshape(-1)
        assert self.data.dtype in (np.float64, np.float32), self.data.dtype
        assert role in ("source", "destination")
        self.shape = None if shape is None else tuple(int(v) for v in shape)
        assert self.shape is None or len(self.shape) == 3
        self.offset = None

    dtype = property(lambda self: self.data.dtype)
    itemsize = property(lambda self: self.data.dtype.itemsize)
    n = property(lambda self: self.data.size)
    nbytes = property(lambda self: self.data.nbytes)
    plane = property(lambda self: self.shape[0] * self.shape[1] if self.shape else 0)

    def xyz(self, index):
        """(x, y, z) of element `index` in blocks of shape (nx, ny, nz), x fastest; the block number in front where the view holds
        several blocks (the velocity vector: one per component)"""
        if self.shape is None:
            return None
        nx, ny, nz = self.shape
        blk, r = divmod(int(index), nx * ny * nz)
        xyz = (r % nx, (r // nx) % ny, r // (nx * ny))
        return xyz if self.n <= nx * ny * nz else (blk,) + xyz


class Region:
    def __init__(self, kind, name, start, stop, itemsize, view=None, before=None, after=None):
        self.kind, self.name, self.start, self.stop, self.itemsize = kind, name, start, stop, itemsize
        self.view, self.before, self.after = view, before, after  # guards: the views in front of and behind them


class Arena:
    """specs -> seal() -> .bytes (upload these) -> check(bytes after the call, expected destinations)"""

    def __init__(self, placement="aligned", base_mod=0):
        assert placement in PLACEMENTS
        assert base_mod % 8 == 0
        self.placement, self.base_mod = placement, base_mod % 256
        self.views, self.by_name = [], {}
        self.regions = None

    def source(self, name, data, shape=None):
        return self._add(View(name, data, "source", shape))

    def destination(self, name, initial, shape=None):
        """initial: poison(n, dtype) where the call overwrites, seeded values where it accumulates"""
        return self._add(View(name, initial, "destination", shape))

    def _add(self, v):
        assert self.regions is None and v.name not in self.by_name and v.n > 0
        self.views.append(v)
        self.by_name[v.name] = v
        return v.name

    # ------------------------------------------------------------------ layout
    def gap_bytes(self):
        """between views: two x-y planes of the largest block plus 64 elements"""
        return max((2 * v.plane + GUARD_ELEMENTS) * v.itemsize for v in self.views)

    def edge_bytes(self):
        """in front of the first and behind the last view: one whole block (the largest)"""
        return max(v.nbytes for v in self.views)

    def _place(self, pos, itemsize):
        a = self.base_mod + pos
        if self.placement == "aligned":
            return pos + (-a) % 256
        return pos + (-a) % 16 + itemsize  # odd element index from a 16-byte boundary

    def seal(self):
        assert self.views and self.regions is None
        gap, edge = self.gap_bytes(), self.edge_bytes()
        order = self.views[::-1] if self.placement == "descending" else self.views
        pos, regions, prev = edge, [], None
        for v in order:
            start = self._place(pos, v.itemsize)
            regions.append(Region("guard", f"guard before {v.name}", pos - (edge if prev is None else gap), start, v.itemsize,
                                  before=prev, after=v))
            v.offset = start
            regions.append(Region(v.role, v.name, start, start + v.nbytes, v.itemsize, view=v))
            pos, prev = start + v.nbytes + gap, v
        end = pos - gap
        total = end + edge + (-(end + edge)) % 8
        regions.append(Region("guard", f"guard behind {prev.name}", end, total, prev.itemsize, before=prev))
        self.regions, self.total = regions, total
        buf = np.empty(total, dtype=np.uint8)
        for r in regions:
            if r.kind != "guard":
                buf[r.start:r.stop] = r.view.data.view(np.uint8)
                continue
            # the half next to each neighbour carries that neighbour's element type, in phase with its elements
            mid = r.start + (r.stop - r.start) // 2 if (r.before is not None and r.after is not None) else (r.stop if r.after is None else r.start)
            for lo, hi, nb in ((r.start, mid, r.before), (mid, r.stop, r.after)):
                if nb is None or hi <= lo:
                    continue
                pat = _pattern(GUARD_BITS[nb.itemsize], nb.itemsize)
                buf[lo:hi] = pat[(np.arange(lo, hi) - nb.offset) % nb.itemsize]
        self.bytes = buf
        self.before = buf.copy()
        return self

    def kind_of_bytes(self):
        """[total] uint8: 0 unclassified, 1 guard, 2 source, 3 destination"""
        k = np.zeros(self.total, dtype=np.uint8)
        for r in self.regions:
            k[r.start:r.stop] += {"guard": 1, "source": 2, "destination": 3}[r.kind]
        return k

    def offset(self, name):
        return self.by_name[name].offset

    def typed(self, buf, name):
        v = self.by_name[name]
        return buf[v.offset:v.offset + v.nbytes].view(v.dtype)

    # ------------------------------------------------------------------ the checker
    def _guard_detail(self, r, byte):
        parts = []
        if r.before is not None:
            d = (byte - (r.before.offset + r.before.nbytes)) // r.before.itemsize
            parts.append(f"{d} elements past the end of {r.before.name}" + self._in_planes(r.before, d))
        if r.after is not None:
            d = (r.after.offset - byte + r.after.itemsize - 1) // r.after.itemsize
            parts.append(f"{d} elements in front of {r.after.name}" + self._in_planes(r.after, d))
        return "; ".join(parts)

    @staticmethod
    def _in_planes(v, d):
        if not v.shape:
            return ""
        return f" (x-line {v.shape[0]}, plane {v.plane}: {d // v.plane} planes + {(d % v.plane) // v.shape[0]} lines + {d % v.shape[0]})"

    def findings(self, after, expected, rtol=None):
        """The first offending byte of every region, in address order.  expected: name -> array for EVERY destination; rtol: None
        compares bit for bit, a number compares every destination by rel-L2 (still no poison, no NaN where the expectation is
        finite)."""
        after = np.asarray(after, dtype=np.uint8)
        assert after.shape == (self.total,)
        missing = [v.name for v in self.views if v.role == "destination" and v.name not in expected]
        assert not missing, f"no expectation for the destinations {missing}: every byte is classified"
        out = []
        for r in self.regions:
            a, b = after[r.start:r.stop], self.before[r.start:r.stop]
            if r.kind in ("guard", "source"):
                bad = np.flatnonzero(a != b)
                if bad.size:
                    byte = r.start + int(bad[0])
                    if r.kind == "guard":
                        out.append(ArenaError("guard", r.name, int(bad[0]) // r.itemsize, None,
                                              f"byte {byte} of the arena changed ({int(b[bad[0]]):#04x} -> {int(a[bad[0]]):#04x}), "
                                              f"{bad.size} bytes in all; {self._guard_detail(r, byte)}"))
                    else:
                        i = int(bad[0]) // r.itemsize
                        out.append(ArenaError("source", r.name, i, r.view.xyz(i),
                                              f"byte {byte} of the arena changed, {bad.size} bytes in all: "
                                              f"{r.view.data[i]!r} -> {a.view(r.view.dtype)[i]!r}"))
                continue
            v = r.view
            got = a.view(v.dtype)
            want = np.ascontiguousarray(expected[v.name], dtype=v.dtype).reshape(-1)
            assert want.size == v.n, (v.name, want.size, v.n)
            left = np.flatnonzero(bits(got) == POISON_BITS[v.itemsize])
            if left.size and not np.array_equal(bits(got)[left], bits(want)[left]):
                i = int(left[np.flatnonzero(bits(got)[left] != bits(want)[left])[0]])
                out.append(ArenaError("poison", v.name, i, v.xyz(i), f"left at its poison value, expected {want[i]!r}"))
                continue
            leak = np.flatnonzero(np.isnan(got) & np.isfinite(want))
            if leak.size:
                i = int(leak[0])
                out.append(ArenaError("nan", v.name, i, v.xyz(i), f"NaN where {want[i]!r} is expected, {leak.size} entries in all"))
                continue
            if rtol is None:
                bad = np.flatnonzero(bits(got) != bits(want))
                if bad.size:
                    i = int(bad[0])
                    out.append(ArenaError("value", v.name, i, v.xyz(i), f"{got[i]!r} != {want[i]!r}, {bad.size} entries differ in all"))
            else:
                err = np.linalg.norm(got.astype(np.float64) - want) / max(np.linalg.norm(want.astype(np.float64)), 1e-300)
                if not err <= rtol:
                    i = int(np.argmax(np.abs(got.astype(np.float64) - want)))
                    out.append(ArenaError("tolerance", v.name, i, v.xyz(i), f"rel-L2 {err:.3e} > {rtol:.1e}; largest at {got[i]!r} vs {want[i]!r}"))
        return out

    def check(self, after, expected, rtol=None):
        found = self.findings(after, expected, rtol)
        if found:
            raise found[0]


# ------------------------------------------------------------------------------------------ the device backend

_helpers = {}


def _helper_ctx(stfem, nbytes):
    """a degree-1 fp64 context on (N, 1, 1) cells whose block holds nbytes: 4 (N + 1) doubles; N a power of two, contexts kept"""
    n = 64
    while 32 * (n + 1) < nbytes:
        n *= 2
    if n not in _helpers:
        _helpers[n] = stfem.MatrixFreeOperator(1, (n, 1, 1))
    return _helpers[n]


class DeviceMemory:
    """n_blocks allocations of the library (one fp64 BlockVector of a helper context), moved as raw bytes by its own upload /
    download.  fp64 blocks are copied unconverted, so NaN payloads and fp32 views survive."""

    def __init__(self, stfem, nbytes, n_blocks=1):
        self.ctx = _helper_ctx(stfem, nbytes)
        self.vec = stfem.BlockVector(self.ctx, n_blocks)
        self.base = [int(self.vec.block_ptr(b)) for b in range(n_blocks)]
        self.capacity = 8 * self.ctx.n_dofs

    def upload(self, blocks):
        host = np.zeros((len(self.base), self.capacity), dtype=np.uint8)
        for b, raw in enumerate(blocks):
            host[b, :raw.size] = raw
        self.vec.upload(host.view(np.float64))
        return self

    def download(self, sizes):
        host = self.vec.download().view(np.uint8)
        return [host[b, :n].copy() for b, n in enumerate(sizes)]


class Spec:
    """One array of a call.  data: the content before the call (float64 / float32), for a destination poison(n, dtype) or seeded
    values; shape: (nx, ny, nz) of its blocks where known"""

    def __init__(self, name, data, role="source", shape=None):
        self.name, self.data, self.role, self.shape = name, np.ascontiguousarray(data).reshape(-1), role, shape


def run_plain(stfem, specs, call):
    """Every array in an allocation of its own, as the library hands them out.  -> (name -> content after the call, what the
    call returned)"""
    mem = DeviceMemory(stfem, max(s.data.nbytes for s in specs), len(specs))
    mem.upload([s.data.view(np.uint8) for s in specs])
    ret = call({s.name: mem.base[i] for i, s in enumerate(specs)})
    raw = mem.download([s.data.nbytes for s in specs])
    return {s.name: r.view(s.data.dtype) for s, r in zip(specs, raw)}, ret


def run_arena(stfem, specs, call, placement):
    """The same call on views of one guarded allocation.  -> (arena, its bytes after the call, what the call returned)"""
    probe = Arena(placement)
    for s in specs:
        (probe.source if s.role == "source" else probe.destination)(s.name, s.data, s.shape)
    mem = DeviceMemory(stfem, probe.seal().total + 512)
    arena = Arena(placement, base_mod=mem.base[0] % 256)
    for s in specs:
        (arena.source if s.role == "source" else arena.destination)(s.name, s.data, s.shape)
    arena.seal()
    mem.upload([arena.bytes])
    ret = call({s.name: mem.base[0] + arena.offset(s.name) for s in specs})
    return arena, mem.download([arena.total])[0], ret


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


BY_CALLER = "reference checked by the caller"


def guard_case(stfem, placement, specs, call, references, rtol_fallback=None, check=None, returned=None):
    """The three assertions of a guard-band case.
    1. the call on library allocations agrees with `references`: name -> (float64 reference, rel-L2 bound of the existing parity
       test) or a function that asserts on the result, for every destination; its sources are untouched.  BY_CALLER instead of a
       reference: the call has no reference by itself (one slab of a cut), the caller compares the returned plain results after
       combining them.  What the call returns (inner products, norms: host values) is handed to `returned` for the same comparison;
    2. the call on arena views gives those destinations, and returns those values, bit for bit (rtol_fallback: by rel-L2, for a
       kernel that documents a path chosen by alignment);
    3. guards and sources of the arena are bit-identical to before.
    check: called after each of the two runs (diagnostics that prove the path).  -> the destinations of the plain run"""
    dests = [s.name for s in specs if s.role == "destination"]
    assert sorted(dests) == sorted(references), (dests, sorted(references))
    plain, ret = run_plain(stfem, specs, call)
    if check:
        check()
    for s in specs:
        if s.role == "source":
            assert np.array_equal(bits(plain[s.name]), bits(s.data)), f"plain run changed the source {s.name}"
    for name, ref in references.items():
        assert np.all(np.isfinite(plain[name])), f"plain run left NaN in {name}"
        if ref is BY_CALLER:
            continue
        if callable(ref):
            ref(plain[name])
            continue
        ref, tol = np.asarray(ref[0], dtype=np.float64).reshape(-1), ref[1]
        err = rel(plain[name], ref)
        print(f"{name}: rel-L2 vs reference {err:.3e} (bound {tol:.1e})")
        assert err < tol, (name, err, tol)
    if returned:
        returned(ret)
    arena, after, ret_arena = run_arena(stfem, specs, call, placement)
    if check:
        check()
    arena.check(after, {n: plain[n] for n in dests}, rtol=rtol_fallback)
    if ret is not None:
        a, b = np.atleast_1d(np.asarray(ret, dtype=np.float64)), np.atleast_1d(np.asarray(ret_arena, dtype=np.float64))
        assert np.array_equal(bits(a), bits(b)), f"returned values differ between library vectors and arena views: {a} / {b}"
    return plain
