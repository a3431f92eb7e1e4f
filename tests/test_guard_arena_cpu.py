"""The guarded arena of the guard-band tests is itself tested here, on a numpy-backed arena without a GPU: the layout
properties, every planted defect the checker has to flag, and the coverage table of the C entry points."""
import importlib
import os
import re

import numpy as np
import pytest

import guard_arena as ga
from guard_coverage import COVERED, EXEMPT, EXEMPT_REASONS

HERE = os.path.dirname(os.path.abspath(__file__))


def make_arena(placement, base_mod=0):
    """fp64 and fp32 sources and destinations of different sizes, blocks with and without a shape"""
    rng = np.random.default_rng(3)
    a = ga.Arena(placement, base_mod)
    a.source("x0", rng.uniform(-1, 1, 7 * 5 * 3), shape=(7, 5, 3))
    a.source("x1", rng.uniform(-1, 1, 7 * 5 * 3), shape=(7, 5, 3))
    a.source("xf", rng.uniform(-1, 1, 343).astype(np.float32), shape=(7, 7, 7))
    a.destination("y0", ga.poison(7 * 5 * 3, np.float64), shape=(7, 5, 3))
    a.destination("yf", ga.poison(343, np.float32), shape=(7, 7, 7))
    a.destination("acc", rng.uniform(-1, 1, 33))
    a.source("u", rng.uniform(-1, 1, 3 * 45), shape=(5, 3, 3))  # three components in one view
    return a.seal()


def expectations(a):
    rng = np.random.default_rng(4)
    return {"y0": rng.uniform(-1, 1, 105), "yf": rng.uniform(-1, 1, 343).astype(np.float32), "acc": rng.uniform(-1, 1, 33)}


def finished(a, exp):
    """the arena's bytes as a correct call leaves them"""
    after = a.bytes.copy()
    for name, want in exp.items():
        a.typed(after, name)[:] = want
    return after


@pytest.mark.parametrize("base_mod", [0, 8, 136, 248])
@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_layout_properties(placement, base_mod):
    a = make_arena(placement, base_mod)
    kinds = a.kind_of_bytes()
    assert kinds.size == a.total and np.all(np.isin(kinds, (1, 2, 3)))  # every byte classified, no overlap
    regions = a.regions
    assert regions[0].start == 0 and regions[-1].stop == a.total
    assert all(r.stop == s.start and r.stop > r.start for r, s in zip(regions, regions[1:]))
    assert [r.kind == "guard" for r in regions] == [i % 2 == 0 for i in range(len(regions))]  # guard | view | ... | guard
    for v in a.views:
        addr = base_mod + v.offset
        if placement == "aligned":
            assert addr % 256 == 0
        else:  # exactly element alignment: an odd element index from a 16-byte boundary
            assert addr % v.itemsize == 0 and addr % (2 * v.itemsize) == v.itemsize
            assert addr % 16 == v.itemsize
    offs = [v.offset for v in a.views]
    assert offs == sorted(offs, reverse=(placement == "descending"))
    # widths: two x-y planes of the largest block plus 64 elements between views, a whole block at both ends
    gap = max((2 * v.plane + 64) * v.itemsize for v in a.views)
    edge = max(v.nbytes for v in a.views)
    assert gap == (2 * 49 + 64) * 4 or gap == (2 * 35 + 64) * 8
    widths = [r.stop - r.start for r in regions if r.kind == "guard"]
    assert widths[0] >= edge and widths[-1] >= edge and all(w >= gap for w in widths[1:-1])


@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_guards_are_nans_of_the_neighbouring_type(placement):
    a = make_arena(placement)
    for r in a.regions:
        if r.kind != "guard":
            continue
        for nb, lo, hi in ((r.before, r.start, r.start + 64), (r.after, r.stop - 64, r.stop)):
            if nb is None:
                continue
            lo += (nb.offset - lo) % nb.itemsize  # in phase with the neighbour's elements
            vals = a.bytes[lo:lo + ((hi - lo) // nb.itemsize) * nb.itemsize].view(nb.dtype)
            assert vals.size >= 7 and np.all(np.isnan(vals))
            assert np.all(ga.bits(vals) == ga.GUARD_BITS[nb.itemsize])


@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_a_correct_call_passes(placement):
    a = make_arena(placement)
    exp = expectations(a)
    assert a.findings(finished(a, exp), exp) == []
    a.check(finished(a, exp), exp)
    with pytest.raises(AssertionError, match="no expectation"):
        a.findings(finished(a, exp), {"y0": exp["y0"]})


@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_single_changed_byte_in_every_guard(placement):
    a = make_arena(placement)
    exp = expectations(a)
    for r in a.regions:
        if r.kind != "guard":
            continue
        for byte in (r.start, (r.start + r.stop) // 2, r.stop - 1):
            after = finished(a, exp)
            after[byte] ^= 0x01
            with pytest.raises(ga.ArenaError) as e:
                a.check(after, exp)
            assert e.value.kind == "guard" and e.value.region == r.name
            assert f"byte {byte} of the arena" in str(e.value)


def test_guard_finding_names_the_distance_in_lines_and_planes():
    a = make_arena("packed")
    exp = expectations(a)
    v = a.by_name["x0"]
    after = finished(a, exp)
    stray = v.offset + v.nbytes + 8 * (35 + 7 + 2)  # one plane, one x-line and two elements past the end of x0
    after[stray:stray + 8] = np.array([1.0]).view(np.uint8)
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp)
    assert "44 elements past the end of x0" in str(e.value) and "1 planes + 1 lines + 2" in str(e.value)


@pytest.mark.parametrize("placement", ga.PLACEMENTS)
def test_single_changed_byte_in_a_source(placement):
    a = make_arena(placement)
    exp = expectations(a)
    for name, index, xyz in (("x1", 7 * 5 + 7 * 2 + 3, (3, 2, 1)), ("xf", 342, (6, 6, 6)), ("u", 2 * 45 + 15 + 4, (2, 4, 0, 1))):
        v = a.by_name[name]
        after = finished(a, exp)
        after[v.offset + index * v.itemsize + 1] ^= 0x80
        with pytest.raises(ga.ArenaError) as e:
            a.check(after, exp)
        assert (e.value.kind, e.value.region, e.value.index, e.value.xyz) == ("source", name, index, xyz)


def test_destination_left_at_poison():
    a = make_arena("packed")
    exp = expectations(a)
    after = finished(a, exp)
    a.typed(after, "y0")[104] = ga.poison(1, np.float64)[0]  # the last entry was never written
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp)
    assert (e.value.kind, e.value.region, e.value.index, e.value.xyz) == ("poison", "y0", 104, (6, 4, 2))
    after = finished(a, exp)
    a.typed(after, "yf")[:] = ga.poison(343, np.float32)  # a call that did nothing
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp, rtol=1e-5)
    assert (e.value.kind, e.value.region, e.value.index) == ("poison", "yf", 0)


def test_nan_in_a_destination_whose_expectation_is_finite():
    a = make_arena("aligned")
    exp = expectations(a)
    for rtol in (None, 1e-12):
        after = finished(a, exp)
        a.typed(after, "acc")[17] = np.nan  # a guard value was read into a result
        with pytest.raises(ga.ArenaError) as e:
            a.check(after, exp, rtol=rtol)
        assert (e.value.kind, e.value.region, e.value.index, e.value.xyz) == ("nan", "acc", 17, None)
    # the guard NaN itself, copied into a destination
    after = finished(a, exp)
    ga.bits(a.typed(after, "yf"))[5] = ga.GUARD_BITS[4]
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp)
    assert (e.value.kind, e.value.index, e.value.xyz) == ("nan", 5, (5, 0, 0))


def test_bitwise_and_tolerance_comparison_of_destinations():
    a = make_arena("packed")
    exp = expectations(a)
    after = finished(a, exp)
    y = a.typed(after, "y0")
    y[50] = np.nextafter(y[50], 2.0)  # one ulp
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp)
    assert (e.value.kind, e.value.region, e.value.index) == ("value", "y0", 50)
    a.check(after, exp, rtol=1e-12)
    y[50] += 1e-6
    with pytest.raises(ga.ArenaError) as e:
        a.check(after, exp, rtol=1e-12)
    assert (e.value.kind, e.value.region, e.value.index) == ("tolerance", "y0", 50)
    # an expected NaN (a source that holds one on purpose) is not a leak
    exp["acc"][3] = np.nan
    a.check(finished(a, exp), exp)


def test_findings_come_in_address_order_one_per_region():
    a = make_arena("aligned")
    exp = expectations(a)
    after = finished(a, exp)
    after[0] ^= 1
    after[a.total - 1] ^= 1
    after[a.offset("x1")] ^= 1
    found = a.findings(after, exp)
    assert [f.kind for f in found] == ["guard", "source", "guard"]


# ------------------------------------------------------------------------------------------ the coverage table

def case_ids():
    ids = set()
    for mod in ("test_gpu_guard_bands", "test_gpu_guard_bands_stokes"):
        with open(os.path.join(HERE, mod + ".py")) as f:
            ids.update(f"{mod}::{name}" for name in re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
    return ids


def test_every_entry_point_is_covered_or_exempt():
    stfem = importlib.import_module("dealii-stfem_amd")
    names = set(stfem.SIGNATURES)
    both = set(COVERED) & set(EXEMPT)
    assert not both, f"listed twice: {sorted(both)}"
    assert not (set(COVERED) | set(EXEMPT)) - names, sorted((set(COVERED) | set(EXEMPT)) - names)
    assert not names - set(COVERED) - set(EXEMPT), f"neither covered nor exempt: {sorted(names - set(COVERED) - set(EXEMPT))}"
    assert set(EXEMPT.values()) <= set(EXEMPT_REASONS), set(EXEMPT.values()) - set(EXEMPT_REASONS)
    assert len(EXEMPT_REASONS) == 4


def test_covered_entry_points_name_a_case_that_calls_them():
    """A sanity check of the table, not a proof: the named case exists, and the entry point is called by name somewhere in that
    case's file or in a wrapper of the package.  That the named case is the one that reaches it is for the reader of the table."""
    ids = case_ids()
    package = os.path.join(os.path.dirname(HERE), "dealii-stfem_amd")
    wrappers = "".join(open(os.path.join(package, f)).read() for f in ("__init__.py", "distributed.py"))
    tests = {mod: open(os.path.join(HERE, mod + ".py")).read() for mod in ("test_gpu_guard_bands", "test_gpu_guard_bands_stokes")}
    for name, case in COVERED.items():
        assert case in ids, (name, case)
        # the entry point is called by its own name in the case's file, or through a wrapper of the package
        assert f".{name}(" in tests[case.split("::")[0]] or f".{name}(" in wrappers, name


def test_exemptions_fit_their_reason():
    """The multi-rank exemptions are the families the scope names and no other; no other exempt name carries a verb of the entry points
    that move a caller's device data."""
    multi = re.compile(r"^stfem_(comm_\w+|halo_\w+|neighbour_exchange|ghost_update)$")
    for name, reason in EXEMPT.items():
        assert (reason == "multi-rank exchange") == bool(multi.match(name)), (name, reason)
    moving = re.compile(r"(vmult|_step$|_add$|_pack$|_unpack$|_move$|_prolongate$|_restrict$|_interpolate$|axpy|axpby|_dot|orthogonalize|convert|"
                        r"upload|download|integrate_|divergence$|drag_lift$|nitsche_rhs|pressure_difference|diagonal|bind_ghosts|vanka_update)")
    for name, reason in EXEMPT.items():
        if reason != "multi-rank exchange":
            assert not moving.search(name), f"{name} moves device data of the caller: it cannot be exempt as '{reason}'"
