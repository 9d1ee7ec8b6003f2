"""Any-angle paths on the navigation layer: line of sight and smoothed traces (include/vtmc_navsight.h, csrc/terrain_navsight.hip).

The rule (NAVSIGHT in include/vtmc_navsight.h) is integers only, so the device is compared with navsight_twin.py for EQUALITY: hits as
bytes, rows and lengths as int32.  The twin is itself pinned to answers worked out by hand.  Fields, boxes and helpers are
nav_support.py's; fields of costs are navfield_twin.py's; the contract every layer's header keeps is tests/test_abi_layers.py's."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import navfield_twin
import naverode_twin
import navsight_twin as twin
from host_check import run_host_check
import nav_support as nav
from nav_support import flat_grid, nav_of
from terrain_twin import no_result

ROOT = nav.ROOT
f32 = np.float32
DIMS, SCALE, ORIGIN = nav.DIMS, nav.SCALE, nav.ORIGIN
ANY, UNREACHED = _lib.NAVSIGHT_ANY_COST, _lib.NAVFIELD_UNREACHED
NAV_PARAMS = (1, 2.5)            # (agent_height, max_step) of the nav builds under the fields
CLIMB, DROP = 1.0, 0.25
LOOKS = (1, 2, 63, 64, 65, 128, 256)      # the edges of the ballot's chunks of 64
EXTRAS = (0, 4096, ANY)
LENS = (1, 2, 7, 256)


def raw(look, extra=ANY, flags=0, reserved=0):
    return _lib.NavSightParamsStruct(look, extra, flags, reserved)


def at(r, x, z, floor=0):
    """The index of a span of grid column (x, z), counted from the bottom."""
    spans, first = nav.column(r, x, z)
    assert floor < len(spans)
    return first + floor


def goal_of(spans):
    """One goal: the middle member of the largest region."""
    region, _ = nav.largest_region(spans)
    inside = np.nonzero(spans["region"] == region)[0]
    return int(inside[len(inside) // 2])


class Case:
    """A nav result with the field of one goal in its largest region, and the twin's walker over both."""

    def __init__(self, navr, climb=CLIMB, drop=DROP):
        self.nav, self.spans = navr, navr[0]
        self.goal = goal_of(self.spans)
        self.cells = navfield_twin.field(self.spans, [(self.goal, 0)], climb, drop)
        self.walker = twin.Walker(navr, navfield_twin.edge_costs(self.spans, climb, drop))
        self.reached = np.nonzero(self.cells["cost"] != UNREACHED)[0].astype(np.int32)
        self.params = vt.NavFieldParams(climb, drop)

    def pairs(self, seed=20261020, count=4096):
        """A fixed seeded set of pairs, a few of them with a -1, and every linked pair."""
        n = len(self.spans)
        rng = np.random.default_rng(seed)
        a, b = rng.integers(0, n, count), rng.integers(0, n, count)
        a[::97], b[5::89] = -1, -1
        s, k = np.nonzero(self.spans["link"] >= 0)
        return np.concatenate([a, s]).astype(np.int32), np.concatenate([b, self.spans["link"][s, k]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def crafted_case(field, box):
    return Case(nav.twin_of(field, box, *NAV_PARAMS))


# -- CPU: the header, the binding, the documents, the host half -----------------------------------------------------------------------------
def test_header_declares_the_layer():
    S = _header.LAYERS["navsight"]
    assert S.constants == {"VTMC_NAVSIGHT_MAX_LOOK": 256, "VTMC_NAVSIGHT_ANY_COST": 0xffffffff}
    assert (_lib.NAVSIGHT_MAX_LOOK, _lib.NAVSIGHT_ANY_COST) == (256, 0xffffffff)
    assert list(S.prototypes) == ["vtmc_nav_sight", "vtmc_navfield_trace_smooth"] == _lib.LAYER_SYMBOLS["navsight"]
    assert set(S.structs) == {"vtmc_navsight_params", "vtmc_navsight_hit"}
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    assert S.prototypes["vtmc_nav_sight"].argtypes == [VP, VP, VP, I32, VP]
    assert S.prototypes["vtmc_navfield_trace_smooth"].argtypes == [VP, VP, I32, I32, VP, VP, VP]
    P = _lib.NavSightParamsStruct
    assert ctypes.sizeof(P) == 16 and (P.max_look.offset, P.max_extra_cost.offset, P.flags.offset, P.reserved.offset) == (0, 4, 8, 12)
    H = _lib.NAVSIGHT_HIT_DTYPE
    assert H.itemsize == 8 and H.names == ("last", "steps") and [H.fields[f][1] for f in H.names] == [0, 4] and vt.NAVSIGHT_HIT_DTYPE is H
    rule = open(S.path).read()
    for word in ("NAVSIGHT", "Column", "Walk", "Visible", "Sight", "Smoothed trace", "ex == ez", "NOT symmetric", "the LAST chain entry", "in 64 bits"):
        assert word in rule, word
    # the layers under it, and the document that named the gap, point here
    for path in (_header.LAYERS["nav"].path, _header.LAYERS["navfield"].path, os.path.join(ROOT, "PATHFINDING.md")):
        assert "vtmc_navsight.h" in open(path).read() and "PATHSMOOTHING.md" in open(path).read(), path


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert hasattr(L, "vtmc_debug_navsight_ms")
    p, spans, hits = raw(64), np.zeros(4, np.int32), np.zeros(4, vt.NAVSIGHT_HIT_DTYPE)
    assert L.vtmc_nav_sight(None, spans.ctypes.data, spans.ctypes.data, 4, hits.ctypes.data) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_trace_smooth(None, spans.ctypes.data, 4, 1, ctypes.byref(p), spans.ctypes.data, spans.ctypes.data) == _lib.ERR_INVALID_ARG
    assert L.vtmc_debug_navsight_ms(None, None) == _lib.ERR_INVALID_ARG


def test_navsight_params():
    p = vt.NavSightParams().to_struct()
    assert (p.max_look, p.max_extra_cost, p.flags, p.reserved) == (64, ANY, 0, 0)
    p = vt.NavSightParams(256, 0).to_struct()
    assert (p.max_look, p.max_extra_cost) == (256, 0) and vt.NavSightParams(1, 4096).to_struct().max_extra_cost == 4096
    assert vt.NavSightParams(0).to_struct().max_look == 0 and vt.NavSightParams(257).to_struct().max_look == 257   # the library's to refuse
    for bad in (dict(max_look=1.5), dict(max_look=True), dict(max_look=2 ** 31), dict(max_extra_cost=-1), dict(max_extra_cost=ANY), dict(max_extra_cost=0.5)):
        with pytest.raises(ValueError):
            vt.NavSightParams(**bad)


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/navsight_host_check.cpp: the host half (csrc/terrain_navsight.h), the walk the kernels call among it, as a stand-alone program
    under ASan and UBSan, on the CPU; it compares the walk with a second formulation of its own."""
    run_host_check("navsight_host_check", tmp_path)


def test_document_states_the_layer():
    text = open(os.path.join(ROOT, "PATHSMOOTHING.md")).read()
    for word in ("VtmcNavSightParams", "VtmcNavSightHit", "column centres", "greedy", "One box only", "snapshot", "not symmetric"):
        assert word in text, word


# -- CPU: the twin against answers stated by hand ---------------------------------------------------------------------------------------------
def test_twin_flat_floor():
    """A 9 x 7 floor: every pair is visible in nx + nz steps; the diagonal takes the corner branch at every step."""
    r = nav_of(flat_grid(9, 7))
    w = twin.Walker(r)
    assert w.n == 63
    for a in range(63):
        for b in range(63):
            assert w.walk(a, b) == (b, abs(a % 9 - b % 9) + abs(a // 9 - b // 9), 0), (a, b)
    a, b = at(r, 0, 0), at(r, 6, 6)
    assert w.walk(a, b) == (b, 12, 0)
    trail = w.passed(a, b)   # per corner the two side spans and the far one: no single step between them
    assert trail == [a] + [at(r, x, z) for i in range(6) for x, z in ((i + 1, i), (i, i + 1), (i + 1, i + 1))]
    assert w.passed(at(r, 0, 3), at(r, 8, 3)) == [at(r, x, 3) for x in range(9)] and w.passed(at(r, 4, 6), at(r, 4, 0)) == [at(r, 4, z) for z in range(6, -1, -1)]
    hits = w.sight([a, -1, b, 5], [b, 3, -1, 5])
    assert hits.dtype == vt.NAVSIGHT_HIT_DTYPE and hits.tolist() == [(b, 12), (-1, 0), (-1, 0), (5, 0)]


def test_twin_one_unlinkable_pillar():
    """The same floor with one column at (3, 3) whose floor stands 4 above it."""
    g = flat_grid(9, 7, 10)
    g[3, 0:7, 3] = nav.SOLID
    r = nav_of(g)
    w = twin.Walker(r)
    assert w.n == 63 and (r[0]["link"][at(r, 3, 3)] == -1).all()
    assert w.walk(at(r, 0, 0), at(r, 6, 6))[:2] == (at(r, 2, 2), 4)      # two corners, then the third one's far span is the pillar
    assert w.walk(at(r, 2, 3), at(r, 4, 3))[:2] == (at(r, 2, 3), 0)
    # (0, 2) -> (6, 4): nx = 6, nz = 2, so ex = 2, 6, 10, 14, 18, 22 and ez = 6, 18.  By hand: x to (1, 2); ex == ez == 6, the corner over
    # (2, 2) and (1, 3) to (2, 3); then ex = 10 < ez = 18, an x step into (3, 3), the pillar: the walk ends on (2, 3) after 3 steps.
    a, b = at(r, 0, 2), at(r, 6, 4)
    assert w.walk(a, b)[:2] == (at(r, 2, 3), 3)
    assert w.passed(a, b) == [at(r, x, z) for x, z in ((0, 2), (1, 2), (2, 2), (1, 3), (2, 3))]
    # the same segment one row lower passes the pillar by: (0, 1) (1, 1) [(2, 1) (1, 2)] (2, 2) (3, 2) (4, 2) [(5, 2) (4, 3)] (5, 3) (6, 3)
    a, b = at(r, 0, 1), at(r, 6, 3)
    assert w.walk(a, b)[:2] == (b, 8)
    assert w.passed(a, b) == [at(r, x, z) for x, z in ((0, 1), (1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (4, 3), (5, 3), (6, 3))]
    # and on the flat floor without the pillar the first one passes: through the centre of (3, 3)
    flat = twin.Walker(nav_of(flat_grid(9, 7)))
    assert flat.walk(at(r, 0, 2), at(r, 6, 4))[:2] == (at(r, 6, 4), 8)


def test_twin_corner_needs_both_sides():
    """Only (1, 0) is missing: (0, 0) -> (1, 1) passes through the corner of four columns and is not visible, although (0, 1) links on."""
    g = flat_grid(5, 4)
    g[1, :, 0] = nav.SOLID   # solid to the top: no floor
    r = nav_of(g)
    w = twin.Walker(r)
    a, b, side = at(r, 0, 0), at(r, 1, 1), at(r, 0, 1)
    assert w.n == 19 and len(nav.column(r, 1, 0)[0]) == 0
    assert r[0]["link"][a].tolist() == [-1, -1, -1, side] and r[0]["link"][side][1] == b
    assert w.walk(a, b)[:2] == (a, 0) and w.walk(side, b)[:2] == (b, 1) and w.walk(a, side)[:2] == (side, 1)
    assert w.walk(b, a)[:2] == (b, 0)   # nor backwards
    assert w.walk(at(r, 0, 1), at(r, 2, 3))[:2] == (at(r, 2, 3), 4)   # a diagonal elsewhere passes


def test_twin_stacked_floors_and_one_way_links():
    """Reaching the target's column on another floor is not visibility; links are followed forwards."""
    g = flat_grid(9, 5, 14)
    g[5, 6:8, 2] = nav.SOLID   # a slab over the floor of (5, 2): two spans, and the floor's neighbours link to the lower one
    r = nav_of(g)
    w = twin.Walker(r)
    low, up = at(r, 5, 2, 0), at(r, 5, 2, 1)
    assert w.n == 46 and r[0]["height"][[low, up]].tolist() == [2.5, 7.5]
    assert w.walk(at(r, 0, 2), low)[:2] == (low, 5) and w.walk(at(r, 0, 2), up)[:2] == (low, 5)
    assert w.walk(at(r, 1, 0), up)[:2] == (low, 6) and not w.visible(at(r, 5, 4), up) and w.visible(at(r, 5, 4), low)
    # crafted_field's D: the upper span of (27, 3), at 7.5, steps down to the pillar (26, 3) at 5.5, whose own +x link goes to the span below
    c = nav.twin_of("crafted", "far", *NAV_PARAMS)
    cw = twin.Walker(c)
    top, pillar = at(c, 27, 3, 1), at(c, 26, 3)
    assert c[0]["height"][[top, pillar]].tolist() == [7.5, 5.5] and c[0]["link"][top][0] == pillar and c[0]["link"][pillar][1] == at(c, 27, 3, 0)
    assert cw.walk(top, pillar)[:2] == (pillar, 1) and cw.walk(pillar, top)[:2] == (at(c, 27, 3, 0), 1)   # down, and not back
    assert c[0]["link"][pillar][0] == -1 and cw.walk(top, at(c, 24, 3))[:2] == (pillar, 1)   # the pillar stands 3 above the floor: the walk ends on it
    # crafted_field's E: the floor under the slab of (32, 3) climbs to (33, 3) at 5.0, which answers to the slab's top
    under, beside = at(c, 32, 3, 0), at(c, 33, 3)
    assert cw.walk(under, beside)[:2] == (beside, 1) and cw.walk(beside, under)[:2] == (at(c, 32, 3, 1), 1)


def test_twin_crafted_bridge():
    """crafted_field's G: the bridge one column wide between the plateaus, over the flat floor."""
    c = nav.twin_of("crafted", "far", *NAV_PARAMS)
    w = twin.Walker(c)
    west, east = at(c, 54, 10), at(c, 63, 10)
    bridge = [at(c, x, 10, 1) for x in range(55, 63)]
    assert w.walk(west, east)[:2] == (east, 9) and w.walk(east, west)[:2] == (west, 9)           # end to end along its axis
    assert w.passed(west, east) == [west] + bridge + [east]
    assert w.walk(at(c, 52, 10), at(c, 66, 10))[:2] == (at(c, 66, 10), 14)
    beside = at(c, 54, 9)   # on the plateau, beside the bridge's foot: the first step leaves the plateau, 6 down
    assert w.walk(beside, bridge[1])[:2] == (beside, 0) and w.walk(beside, east)[0] != east
    under = at(c, 54, 14)   # on the flat floor: the walk arrives under the bridge
    assert c[0]["height"][under] == 2.5 and w.walk(under, bridge[3])[0] == at(c, 58, 10, 0)


def smoothed(case, look, extra, max_len=256):
    return case.walker.smooth(case.cells, case.reached, max_len, look, extra)


def test_twin_smoothing_on_the_crafted_field():
    case = crafted_case("crafted", "far")
    w, D, nxt = case.walker, case.cells["cost"].astype(np.int64), case.cells["next"]
    assert len(case.spans) == 2548 and len(case.reached) == 2478
    plain, plain_len = navfield_twin.trace(case.cells, case.reached, 256)
    assert plain_len.sum() == 80260 and plain_len.max() == 73
    totals = {}
    for extra in (0, ANY):
        for look in (16, 64, 256):
            rows, lens = smoothed(case, look, extra)
            totals[look, extra] = int(lens.sum())
            for i, s0 in enumerate(case.reached):
                row = rows[i, :lens[i]].tolist()
                assert row[0] == s0 and row[-1] == plain[i, plain_len[i] - 1] and (rows[i, lens[i]:] == -1).all()
                assert [s for s in plain[i, :plain_len[i]].tolist() if s in set(row)] == row           # waypoints are spans of the trace, in its order
                for a, b in zip(row, row[1:]):
                    last, steps, cost = w.walk(a, b)
                    assert last == b
                    if extra == 0:
                        assert D[a] - D[b] == cost                                                     # every stretch is a cheapest walk
    assert totals == {(16, 0): 8809, (64, 0): 5702, (256, 0): 5674, (16, ANY): 8785, (64, ANY): 5643, (256, ANY): 5615}
    assert all(totals[256, e] <= totals[64, e] <= totals[16, e] < 80260 for e in (0, ANY)) and totals[64, 0] != totals[64, ANY]
    # max_look 1 is the plain trace; a cut row is the uncut one's beginning
    rows, lens = smoothed(case, 1, ANY)
    assert np.array_equal(rows, plain) and np.array_equal(lens, plain_len)
    rows, lens = smoothed(case, 2, 0)
    cut, cut_len = smoothed(case, 2, 0, 7)
    assert np.array_equal(cut, rows[:, :7]) and np.array_equal(cut_len, np.minimum(lens, 7))
    was_cut = nxt[cut[np.arange(len(cut)), cut_len - 1]] != -1
    assert (was_cut == (lens > 7)).all() and was_cut.any() and (lens == 7).any()   # a row that is cut, and one that fits exactly
    # an invalid and an unreached start
    unreached = int(np.nonzero(case.cells["cost"] == UNREACHED)[0][0])
    rows, lens = w.smooth(case.cells, [-1, unreached, int(case.reached[0])], 4, 64)
    assert lens.tolist()[:2] == [0, 0] and (rows[:2] == -1).all() and lens[2] >= 1


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
def check_sight(ex, case, what):
    a, b = case.pairs()
    got, want = ex.nav_sight(a, b), case.walker.sight(a, b)
    assert got.dtype == vt.NAVSIGHT_HIT_DTYPE and got.tobytes() == want.tobytes(), what
    return got


def check_smooth(ex, case, starts, max_len, look, extra, what):
    rows, lens = ex.nav_trace_smooth(starts, max_len, raw(look, extra))
    want_rows, want_lens = case.walker.smooth(case.cells, starts, max_len, look, extra)
    assert lens.dtype == np.int32 and np.array_equal(lens, want_lens) and rows.dtype == np.int32 and rows.tobytes() == want_rows.tobytes(), (what, max_len, look, extra)
    return rows, lens


@pytest.fixture(scope="module")
def crafted_ex():
    with nav.terrain(nav.crafted_field()) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("box", ["far", "interior"])
def test_gpu_crafted_field_equals_the_twin(crafted_ex, box):
    ex, case = crafted_ex, crafted_case("crafted", box)
    nav.assert_same(ex.terrain_nav(*nav.BOXES[box], nav.raw_params(*NAV_PARAMS)), case.nav, box)
    hits = check_sight(ex, case, box)           # before any field: a nav result is all it needs
    a, b = case.pairs()
    seen = hits["last"] == b
    assert 1000 < seen[:4096].sum() < 3500 and ((a >= 0) & (b >= 0) & ~seen & (hits["steps"] > 0)).sum() > 100 and seen[4096:].all() and (hits["steps"][4096:] == 1).all() and (hits["last"][a < 0] == -1).all()
    cells = ex.nav_field([(case.goal, 0)], case.params)
    assert cells.tobytes() == case.cells.tobytes()
    cut = fits = 0
    for extra in EXTRAS:
        for look in LOOKS:
            for max_len in LENS:
                rows, lens = check_smooth(ex, case, case.reached, max_len, look, extra, box)
                last = rows[np.arange(len(rows)), lens - 1]
                cut += int(((lens == max_len) & (cells["next"][last] != -1)).sum())
                fits += int(((lens == max_len) & (cells["next"][last] == -1)).sum()) if max_len > 1 else 0
    assert cut > 0 and fits > 0   # rows cut exactly at max_len, and rows that end exactly there
    check_sight(ex, case, box)    # ... and a field changes no hit


@pytest.mark.gpu
def test_gpu_outside_box_gives_empty_results(crafted_ex):
    ex = crafted_ex
    L, h = ex._L, ex._h
    assert len(ex.terrain_nav(*nav.BOXES["outside"], nav.raw_params(*NAV_PARAMS))[0]) == 0
    assert len(ex.nav_sight([], [])) == 0 and ex.nav_sight([-1, -1], [-1, -1]).tolist() == [(-1, 0), (-1, 0)]
    hits, zero = np.full(2, 7, np.int32), np.zeros(1, np.int32)
    assert L.vtmc_nav_sight(h, zero.ctypes.data, zero.ctypes.data, 1, hits.ctypes.data) == _lib.ERR_INVALID_ARG and (hits == 7).all()   # there is no span 0
    no_result(lambda: ex.nav_trace_smooth([-1], 4, raw(64)))   # no span to put a goal on: no field


@pytest.mark.gpu
def test_gpu_start_counts(crafted_ex):
    """1, 3, 4, 5 and 257 starts: partial workgroups of four waves; -1 and unreached starts among them."""
    ex, case = crafted_ex, crafted_case("crafted", "far")
    ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
    ex.nav_field([(case.goal, 0)], case.params)
    unreached = np.nonzero(case.cells["cost"] == UNREACHED)[0]
    assert len(unreached) > 10
    pool = np.concatenate([[-1, unreached[0]], case.reached[::9], [-1], unreached[1:8]]).astype(np.int32)
    rng = np.random.default_rng(7)
    rng.shuffle(pool)
    assert len(pool) >= 257
    for count in (1, 3, 4, 5, 257):
        for first in (0, 11):
            starts = pool[first:first + count]
            rows, lens = check_smooth(ex, case, starts, 40, 64, 0, count)
            assert rows.shape == (count, 40)
    rows, lens = check_smooth(ex, case, pool[:257], 40, 256, ANY, 257)
    assert (lens[pool[:257] < 0] == 0).all() and (lens == 0).sum() >= 3 and lens.max() >= 3
    for count in (1, 63, 64, 65, 257):   # partial waves of the sight kernel
        a, b = case.pairs()
        assert ex.nav_sight(a[:count], b[:count]).tobytes() == case.walker.sight(a[:count], b[:count]).tobytes()


@pytest.mark.gpu
def test_gpu_turned_field_equals_the_twin():
    """The same field with x and z exchanged: 74 samples along z, so kz is the long axis of the walks."""
    dims = (DIMS[2], DIMS[1], DIMS[0])
    box, case = "far", crafted_case("turned", "far")
    with nav.terrain(nav.turned_field(), dims) as ex:
        nav.assert_same(ex.terrain_nav(*nav.BOXES[box], nav.raw_params(*NAV_PARAMS)), case.nav, box)
        hits = check_sight(ex, case, box)
        assert ex.nav_field([(case.goal, 0)], case.params).tobytes() == case.cells.tobytes()
        for extra in EXTRAS:
            for look in (2, 64, 65, 256):
                check_smooth(ex, case, case.reached, 256, look, extra, box)
    # the turn changes no answer's kind: as many visible pairs among the linked ones, and walks whose long axis is z
    a, b = case.pairs()
    assert (hits["last"][4096:] == b[4096:]).all() and hits["steps"].max() > 34


@pytest.mark.gpu
def test_gpu_after_an_erosion_paths_keep_the_radius():
    """vtmc_nav_erode at radius 2, then sight and smoothing on the eroded spans: equal to the twin, and every span a walk between two
    consecutive waypoints stands on is at least the radius away from every border of the un-eroded result."""
    radius = 2
    base = nav.twin_of("crafted", "far", *NAV_PARAMS)
    with nav.terrain(nav.crafted_field()) as ex:
        nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS)), base, "far")
        p = _lib.NavErodeParamsStruct(radius, 0, (ctypes.c_int32 * 2)(0, 0))
        D = ex.nav_distance(p)
        eroded = ex.nav_erode(p)
        want = naverode_twin.erode(base, radius)
        nav.assert_same(eroded[:4], want[:4], "eroded")
        origin = eroded[4]
        case = Case(want[:4])
        check_sight(ex, case, "eroded")
        assert ex.nav_field([(case.goal, 0)], case.params).tobytes() == case.cells.tobytes()
        results = {(look, extra): check_smooth(ex, case, case.reached, 256, look, extra, "eroded") for look in (64, 256) for extra in (0, ANY)}
    assert np.array_equal(D, naverode_twin.distance(base, radius)[0]) and (D < 2 * radius).any()
    plain_total = int(navfield_twin.trace(case.cells, case.reached, 256)[1].sum())
    stood = walks = 0
    for (look, extra), (rows, lens) in results.items():
        assert lens.sum() * 5 < plain_total
        for i in range(len(rows)):
            row = rows[i, :lens[i]].tolist()
            for a, b in zip(row, row[1:]):
                trail = case.walker.passed(a, b)
                assert trail[-1] == b and (D[origin[trail]] >= 2 * radius).all(), (look, extra, a, b)
                stood, walks = stood + len(trail), walks + 1
    print("eroded: %d spans, %d traced, waypoints %s; %d walks over %d spans" % (len(case.spans), plain_total, {k: int(v[1].sum()) for k, v in results.items()}, walks, stood))
    assert walks > 1000 and stood > 5 * walks


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nav.RANDOM_BOXES))
def test_gpu_random_field_equals_the_twin(name):
    """The seeded noise world of the nav tests: stacked floors and several regions, on hills whose climbs the field prices, so that the cost
    bound decides (its links happen to be symmetric: the one-way ones are the crafted field's)."""
    with nav.terrain() as ex:
        plane = vt.PlaneModifier(ORIGIN[1] + 8 * SCALE, (-1e6, -1e6), (1e6, 1e6))
        noise = vt.NoiseModifier(7, 3, 0.11, 2.0, 0.5, "fbm", amplitude=2.5, ramp_scale=0.0, lower=(-1e6,) * 3, upper=(1e6,) * 3)
        ex.terrain_update([plane, noise])
        navr = ex.terrain_nav(*nav.RANDOM_BOXES[name], nav.raw_params(2, 1.0))
        case = Case(navr, 2.5, 0.5)
        hits = check_sight(ex, case, name)
        assert ex.nav_field([(case.goal, 0)], case.params).tobytes() == case.cells.tobytes()
        totals = {(look, extra): int(check_smooth(ex, case, case.reached, 256, look, extra, name)[1].sum()) for look in (1, 63, 256) for extra in EXTRAS}
    link = navr[0]["link"]
    s, k = np.nonzero(link >= 0)
    one_way = int((link[link[s, k], k ^ 1] != s).sum())
    print("%s: %d spans, %d reached, %d one-way links, waypoints %s" % (name, len(navr[0]), len(case.reached), one_way, totals))
    assert np.diff(navr[1]).max() >= 2 and len(case.reached) > 500   # stacked floors; one-way links are the crafted field's to cover
    assert totals[256, ANY] < totals[1, ANY] == totals[1, 0] and totals[256, 0] != totals[256, ANY]
    a, b = case.pairs()
    assert ((hits["last"] != b) & (hits["steps"] > 0)).any()


LARGE_STARTS = 512   # starts of the large run: evenly spaced reached spans; the twin smooths them in a few seconds (it prints how long it took)


@pytest.mark.gpu
def test_gpu_large_field_equals_the_twin():
    """The 256^3 world of test_terrain_naverode's large test, some 80 000 spans, one goal in the largest region, max_look 256, twice over:
    the same bytes both times, and the twin's.  The twin smooths the device's cells, which test_terrain_navfield.py compares with Dijkstra."""
    n = 256
    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(n + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        navr = ex.terrain_nav(everything["lower"], everything["upper"], nav.raw_params(4, 1.0, 1 << 24))
        spans = navr[0]
        assert len(spans) > 50000
        goal = goal_of(spans)
        cells = ex.nav_field([(goal, 0)], vt.NavFieldParams(1.0, 0.0))
        reached = np.nonzero(cells["cost"] != UNREACHED)[0]
        starts = reached[::max(len(reached) // LARGE_STARTS, 1)][:LARGE_STARTS].astype(np.int32)
        rng = np.random.default_rng(99)
        a, b = rng.integers(0, len(spans), 4096).astype(np.int32), rng.integers(0, len(spans), 4096).astype(np.int32)
        near = np.clip(a + rng.integers(-40, 41, 4096), 0, len(spans) - 1).astype(np.int32)   # neighbours along a row: many of them visible
        runs = [(ex.nav_trace_smooth(starts, 512, raw(256, 0)), ex.nav_trace_smooth(starts, 512, raw(256)), ex.nav_sight(a, b), ex.nav_sight(a, near)) for _ in range(2)]
        ms = (ctypes.c_float * 2)()
        ex._check(ex._L.vtmc_debug_navsight_ms(ex._h, ms))
        plain_len = ex.nav_trace(starts, 512)[1]
    for x, y in zip(runs[0], runs[1]):
        assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in (zip(x, y) if isinstance(x, tuple) else [(x, y)]))
    t0 = time.time()
    walker = twin.Walker(navr, navfield_twin.edge_costs(spans, 1.0, 0.0))
    want_bound, want_any = walker.smooth(cells, starts, 512, 256, 0), walker.smooth(cells, starts, 512, 256, ANY)
    want_hits, want_near = walker.sight(a, b), walker.sight(a, near)
    took = time.time() - t0
    (bound, any_cost, hits, hits_near) = runs[0]
    print("%d spans, %d reached, %d starts: %d traced spans, %d / %d waypoints (bound 0 / any); %d of 4096 near pairs visible; twin %.1f s; device ms %s"
          % (len(spans), len(reached), len(starts), plain_len.sum(), bound[1].sum(), any_cost[1].sum(), (hits_near["last"] == near).sum(), took, [round(v, 4) for v in ms]))
    assert np.array_equal(bound[1], want_bound[1]) and bound[0].tobytes() == want_bound[0].tobytes()
    assert np.array_equal(any_cost[1], want_any[1]) and any_cost[0].tobytes() == want_any[0].tobytes()
    assert hits.tobytes() == want_hits.tobytes() and hits_near.tobytes() == want_near.tobytes()
    assert len(starts) == LARGE_STARTS and plain_len.max() > 100 and any_cost[1].sum() * 3 < plain_len.sum() and (hits_near["last"] == near).sum() > 100
    assert all(np.isfinite(v) and v >= 0 for v in ms)


@pytest.mark.gpu
def test_gpu_nothing_else_moves():
    """Everything else the context holds, the nav result, the field, the distance and the origin, byte for byte before and after both calls."""
    with nav.terrain() as ex:
        L, h = ex._L, ex._h
        ex.terrain_set_history(16 << 20)
        ex.terrain_update([vt.PlaneModifier(ORIGIN[1] + 6 * SCALE, (-1e6, -1e6), (1e6, 1e6))])
        ex.terrain_update([vt.SphereModifier(nav.world_of((20, 6, 16)), 2.0, False)])
        ex.material_init(1)
        ex.material_vertices(), ex.ao_vertices(vt.AmbientOcclusion(2.0)), ex.scatter_surface(vt.ScatterParams(1.0, seed=3))
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(2, 1.0))
        navr = ex.nav_erode(_lib.NavErodeParamsStruct(1, 0, (ctypes.c_int32 * 2)(0, 0)))[:4]
        ex.nav_distance(_lib.NavErodeParamsStruct(3, 0, (ctypes.c_int32 * 2)(0, 0)))
        case = Case(navr)
        ex.nav_field([(case.goal, 0)], case.params)

        def everything():
            spans, offsets, first, ext = ex.nav_read()
            return nav.held(ex, L, h) + [spans.tobytes(), offsets.tobytes(), first, ext, ex.device_nav(), ex.navfield_read().tobytes(), ex.navfield_info(),
                                         ex.device_navfield(), ex.nav_distance_read().tobytes(), ex.device_nav_distance(), ex.nav_erode_origin().tobytes()]
        before = everything()
        check_sight(ex, case, "held")
        assert everything() == before
        rows, lens = check_smooth(ex, case, case.reached, 64, 64, 0, "held")
        assert lens.max() > 2 and everything() == before
        check_smooth(ex, case, case.reached[:5], 3, 256, ANY, "held")
        assert everything() == before


@pytest.mark.gpu
def test_gpu_errors():
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        spans4 = np.zeros(4, np.int32)
        hits, rows, lens = np.full(8, 7, np.int32), np.full(16, 7, np.int32), np.full(4, 7, np.int32)
        p64 = raw(64)

        def sight(a=spans4, b=spans4, n=4, out=hits):
            return L.vtmc_nav_sight(h, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None, n, out.ctypes.data if out is not None else None)

        def smooth(starts=spans4, n=4, max_len=4, p=p64, paths=rows, lengths=lens):
            return L.vtmc_navfield_trace_smooth(h, starts.ctypes.data if starts is not None else None, n, max_len, ctypes.byref(p) if p is not None else None,
                                                paths.ctypes.data if paths is not None else None, lengths.ctypes.data if lengths is not None else None)

        def untouched():
            return (hits == 7).all() and (rows == 7).all() and (lens == 7).all()

        def clock():
            return L.vtmc_debug_navsight_ms(h, (ctypes.c_float * 2)())
        # before a terrain, and with a terrain before a nav build: every call, also one with nothing to do
        for stage in range(2):
            for call in (sight, smooth, lambda: sight(n=0), lambda: smooth(n=0), clock):
                assert call() == _lib.ERR_NO_RESULT and L.vtmc_last_error(h).decode() != "", stage
            assert untouched()
            if stage == 0:
                ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
                ex.terrain_write_samples(nav.crafted_field())
        case = crafted_case("crafted", "far")
        total = len(case.spans)
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        # a nav result, no field: the sight answers, the smoothed trace does not; the clock refuses before a call that launched a kernel
        assert smooth() == _lib.ERR_NO_RESULT and smooth(n=0) == _lib.ERR_NO_RESULT and "navfield_build" in L.vtmc_last_error(h).decode() and untouched()
        assert clock() == _lib.ERR_NO_RESULT and sight(n=0) == _lib.OK and clock() == _lib.ERR_NO_RESULT and untouched()
        assert sight() == _lib.OK and hits.tolist() == [0, 0] * 4 and clock() == _lib.OK
        hits[:] = 7
        ex.nav_field([(case.goal, 0)], case.params)
        kept = check_smooth(ex, case, case.reached[:50], 16, 64, 0, "kept")
        # every INVALID_ARG writes nothing
        bad_span = [np.array([0, v, 0, 0], np.int32) for v in (-2, total, 2 ** 31 - 1, -2 ** 31)]
        sights = [lambda: sight(n=-1), lambda: sight(a=None), lambda: sight(b=None), lambda: sight(out=None)] + \
            [lambda v=v: sight(a=v) for v in bad_span] + [lambda v=v: sight(b=v) for v in bad_span]
        for i, call in enumerate(sights):
            assert call() == _lib.ERR_INVALID_ARG and "nav_sight" in L.vtmc_last_error(h).decode() and untouched(), i
        smooths = [lambda: smooth(n=-1), lambda: smooth(starts=None), lambda: smooth(paths=None), lambda: smooth(lengths=None), lambda: smooth(p=None),
                   lambda: smooth(max_len=0), lambda: smooth(max_len=-1)] + [lambda v=v: smooth(starts=v) for v in bad_span] + \
            [lambda q=q: smooth(p=q) for q in (raw(0), raw(-1), raw(257), raw(2 ** 31 - 1), raw(-2 ** 31), raw(64, 0, 1), raw(64, ANY, 0x80000000), raw(64, 0, 0, 1),
                                              raw(64, ANY, 0, 0xffffffff))]
        for i, call in enumerate(smooths):
            assert call() == _lib.ERR_INVALID_ARG and "navfield_trace_smooth" in L.vtmc_last_error(h).decode() and untouched(), i
        assert clock() == _lib.OK   # a refused call leaves the last call's clock
        # nothing to do is a success that touches nothing, whatever the pointers
        assert sight(n=0) == _lib.OK and L.vtmc_nav_sight(h, None, None, 0, None) == _lib.OK and untouched()
        assert smooth(n=0) == _lib.OK and L.vtmc_navfield_trace_smooth(h, None, 0, 1, ctypes.byref(p64), None, None) == _lib.OK and untouched()
        again = ex.nav_trace_smooth(case.reached[:50], 16, raw(64, 0))
        assert np.array_equal(again[0], kept[0]) and np.array_equal(again[1], kept[1])
        # whatever drops the field: a nav build, an erode, an init
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        assert smooth() == _lib.ERR_NO_RESULT and sight() == _lib.OK
        ex.nav_field([(case.goal, 0)], case.params)
        assert smooth() == _lib.OK
        ex.nav_erode(_lib.NavErodeParamsStruct(1, 0, (ctypes.c_int32 * 2)(0, 0)))
        assert smooth() == _lib.ERR_NO_RESULT and sight() == _lib.OK
        ex.nav_field([(0, 0)], case.params)
        assert smooth() == _lib.OK
        ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
        hits[:], rows[:], lens[:] = 7, 7, 7
        assert smooth() == _lib.ERR_NO_RESULT and sight() == _lib.ERR_NO_RESULT and clock() == _lib.ERR_NO_RESULT and untouched()


@pytest.mark.gpu
def test_gpu_stage_clock():
    case = crafted_case("crafted", "far")
    ms = (ctypes.c_float * 2)(-1.0, -1.0)
    with nav.terrain(nav.crafted_field()) as fresh:
        fresh.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        assert fresh._L.vtmc_debug_navsight_ms(fresh._h, ms) == _lib.ERR_NO_RESULT and "navsight" in fresh._L.vtmc_last_error(fresh._h).decode()
        fresh.nav_sight([0, 1], [5, 6])
        assert fresh._L.vtmc_debug_navsight_ms(fresh._h, ms) == _lib.OK and all(np.isfinite(v) and v >= 0 for v in ms)
        fresh.nav_field([(case.goal, 0)], case.params)
        fresh.nav_trace_smooth(case.reached, 64, raw(256, 0))
        assert fresh._L.vtmc_debug_navsight_ms(fresh._h, ms) == _lib.OK and all(np.isfinite(v) and v >= 0 for v in ms) and ms[1] > 0
        assert fresh._L.vtmc_debug_navsight_ms(fresh._h, None) == _lib.ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's NavSight and SmoothPaths against the Python path on the same world (host/host_selftest.cpp
    --gpu-navsight)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-navsight", tmp_path)
    hits = np.fromfile(tmp_path / "navsight_hits.bin", vt.NAVSIGHT_HIT_DTYPE)
    files = {k: np.fromfile(tmp_path / ("navsight_%s.i32" % k), np.int32) for k in ("bound_paths", "bound_lengths", "any_paths", "any_lengths")}
    with vt.Extractor(0) as ex:
        spans = nav.mirror_world(ex)[0]
        n = len(spans)
        a = np.repeat(np.arange(n, dtype=np.int32), 5)
        b = np.concatenate([((7 * np.arange(n, dtype=np.int64) + 3) % n).astype(np.int32)[:, None], spans["link"]], axis=1).reshape(-1)
        want_hits = ex.nav_sight(a, b)
        at_goals = ex.nav_locate([(0.0, 6.3, 4.0), (12.0, 6.3, 15.0)], 1.0, 1.0)
        ex.nav_field([(at_goals[0], 0), (at_goals[1], 3000)], vt.NavFieldParams(2.0, 0.5))
        starts = list(range(n)) + [-1]
        bound, any_cost = ex.nav_trace_smooth(starts, 64, vt.NavSightParams(64, 0)), ex.nav_trace_smooth(starts, 64, vt.NavSightParams())
        plain = ex.nav_trace(starts, 64)
    assert n > 100 and hits.tobytes() == want_hits.tobytes() and (want_hits["last"] == b).sum() > n
    assert np.array_equal(files["bound_paths"].reshape(-1, 64), bound[0]) and np.array_equal(files["bound_lengths"], bound[1])
    assert np.array_equal(files["any_paths"].reshape(-1, 64), any_cost[0]) and np.array_equal(files["any_lengths"], any_cost[1])
    assert any_cost[1].sum() < plain[1].sum() and bound[1].max() > 2
