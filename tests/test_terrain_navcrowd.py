"""A crowd stepped along the flow field on the device: one agent per span (include/vtmc_navcrowd.h, csrc/terrain_navcrowd.hip).

The rule (NAVCROWD in include/vtmc_navcrowd.h) is integers only, so the device is compared with navcrowd_twin.py for EQUALITY: agents and
occupancy as bytes, the info as a tuple.  The twin is itself held to the rule's properties on the crafted field.  Fields, boxes and helpers
are nav_support.py's; fields of costs are navfield_twin.py's; the contract every layer's header keeps is tests/test_abi_layers.py's."""
import ctypes
import functools
import os

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import nav_twin
import navfield_twin
import naverode_twin
import navcrowd_twin as twin
from host_check import run_host_check
import nav_support as nav
from nav_support import flat_grid, nav_of, speeds_of
from terrain_twin import no_result

ROOT = nav.ROOT
f32 = np.float32
DIMS, SCALE, ORIGIN = nav.DIMS, nav.SCALE, nav.ORIGIN
ANY, LEAVE, UNREACHED = _lib.NAVCROWD_ANY_DETOUR, _lib.NAVCROWD_LEAVE_ON_ARRIVAL, _lib.NAVFIELD_UNREACHED
WALKING, ARRIVED, STRANDED, GONE, UNPLACED = twin.WALKING, twin.ARRIVED, twin.STRANDED, twin.GONE, twin.UNPLACED
NAV_PARAMS = (1, 0.5)            # (agent_height, max_step) of the nav builds under the crowds
STEEP_PARAMS = (1, 2.5)          # ... where the one-way link of the crafted field's E is wanted
CLIMB, DROP = 1.0, 0.5


def raw(detour=ANY, flags=0, reserved=(0, 0)):
    return _lib.NavCrowdParamsStruct(detour, flags, (ctypes.c_uint32 * 2)(*reserved))


def spread_goals(spans, count=3):
    """`count` goals spread over the largest region: its members at the odd 2 * count-ths."""
    region, _ = nav.largest_region(spans)
    inside = np.nonzero(spans["region"] == region)[0]
    return [(int(inside[len(inside) * f // (2 * count)]), 0) for f in range(1, 2 * count, 2)]


class Case:
    """A nav result with the field of some goals in its largest region, both the twin's."""

    def __init__(self, navr, goals=None, climb=CLIMB, drop=DROP):
        self.nav, self.spans = navr, navr[0]
        self.climb, self.drop = climb, drop
        self.route(goals if goals is not None else spread_goals(self.spans))

    def route(self, goals):
        self.goals = [(int(s), int(c)) for s, c in goals]
        self.cells = navfield_twin.field(self.spans, self.goals, self.climb, self.drop)
        self.costs = navfield_twin.edge_costs(self.spans, self.climb, self.drop)
        self.reached = np.nonzero(self.cells["cost"] != UNREACHED)[0].astype(np.int32)
        self.params = vt.NavFieldParams(self.climb, self.drop)

    def crowd(self):
        return twin.Crowd(self.spans["link"], self.cells, self.costs)

    def field_on(self, ex):
        assert ex.nav_field(self.goals, self.params).tobytes() == self.cells.tobytes()


@functools.lru_cache(maxsize=None)
def crafted_case(field, box):
    return Case(nav.twin_of(field, box, *NAV_PARAMS))


def at(r, x, z, floor=0):
    spans, first = nav.column(r, x, z)
    assert floor < len(spans)
    return first + floor


# -- CPU: the header, the binding, the documents, the host half -----------------------------------------------------------------------------
def test_header_declares_the_layer():
    S = _header.LAYERS["navcrowd"]
    assert S.constants == {"VTMC_NAVCROWD_MAX_AGENTS": 1 << 24, "VTMC_NAVCROWD_MAX_TICKS": 4096, "VTMC_NAVCROWD_MAX_SPEED": 1 << 20, "VTMC_NAVCROWD_BUDGET_CAP": 1 << 21,
                           "VTMC_NAVCROWD_ANY_DETOUR": 0xffffffff, "VTMC_NAVCROWD_LEAVE_ON_ARRIVAL": 1, "VTMC_NAVCROWD_WALKING": 0, "VTMC_NAVCROWD_ARRIVED": 1,
                           "VTMC_NAVCROWD_STRANDED": 2, "VTMC_NAVCROWD_GONE": 3, "VTMC_NAVCROWD_UNPLACED": 4}
    assert (_lib.NAVCROWD_MAX_AGENTS, _lib.NAVCROWD_MAX_TICKS, _lib.NAVCROWD_BUDGET_CAP, _lib.NAVCROWD_ANY_DETOUR) == (1 << 24, 4096, 1 << 21, 0xffffffff)
    assert _lib.NAVCROWD_BUDGET_CAP > _lib.NAVFIELD_UNIT + (1 << 20)      # above every edge cost
    names = ["vtmc_navcrowd_spawn", "vtmc_navcrowd_step", "vtmc_navcrowd_read", "vtmc_navcrowd_info", "vtmc_navcrowd_device_results"]
    assert list(S.prototypes) == names == _lib.LAYER_SYMBOLS["navcrowd"]
    assert set(S.structs) == {"vtmc_navcrowd_agent", "vtmc_navcrowd_params"}
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    assert [S.prototypes[n].argtypes for n in names] == [[VP, VP, VP, I32, VP], [VP, VP, I32], [VP, VP, I32, VP], [VP] * 6, [VP] * 4]
    P = _lib.NavCrowdParamsStruct
    assert ctypes.sizeof(P) == 16 and (P.max_detour.offset, P.flags.offset, P.reserved.offset) == (0, 4, 8) and P.reserved.size == 8
    A = _lib.NAVCROWD_AGENT_DTYPE
    assert A.itemsize == 16 and A.names == ("span", "budget", "speed", "state") and [A.fields[f][1] for f in A.names] == [0, 4, 8, 12]
    assert A["span"] == np.dtype("<i4") and all(A[f] == np.dtype("<u4") for f in A.names[1:]) and vt.NAVCROWD_AGENT_DTYPE is A
    rule = open(S.path).read()
    for word in ("NAVCROWD", "Agent", "Occupancy", "Spawn", "Tick", "Info", "SMALLEST", "in 64 bits", "start of the tick", "CLAIMS", "does not try a later one",
                 "no livelock", "KEEPS it", "OUT OF SCOPE"):
        assert word in rule, word
    assert '("navcrowd", "vtmc_navcrowd.h", "navfield", "CROWD.md")' in open(os.path.join(ROOT, "volumetricterrain_amd", "build.py")).read()


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert hasattr(L, "vtmc_debug_navcrowd_ms")
    p, spans, speeds, agents = raw(), np.zeros(4, np.int32), np.ones(4, np.uint32), np.zeros(4, vt.NAVCROWD_AGENT_DTYPE)
    assert L.vtmc_navcrowd_spawn(None, spans.ctypes.data, speeds.ctypes.data, 4, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navcrowd_step(None, ctypes.byref(p), 1) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navcrowd_read(None, agents.ctypes.data, 4, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navcrowd_info(None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navcrowd_device_results(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_debug_navcrowd_ms(None, None) == _lib.ERR_INVALID_ARG


def test_navcrowd_params():
    p = vt.NavCrowdParams().to_struct()
    assert (p.max_detour, p.flags, list(p.reserved)) == (ANY, 0, [0, 0])
    p = vt.NavCrowdParams(2048, True).to_struct()
    assert (p.max_detour, p.flags) == (2048, LEAVE) and vt.NavCrowdParams(0).to_struct().max_detour == 0
    for bad in (dict(max_detour=-1), dict(max_detour=ANY), dict(max_detour=0.5), dict(max_detour=True)):
        with pytest.raises(ValueError):
            vt.NavCrowdParams(**bad)


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/navcrowd_host_check.cpp: the host half (csrc/terrain_navcrowd.h), the choice the claim kernel calls among it, as a stand-alone
    program under ASan and UBSan, on the CPU; it compares the choice with a second formulation on random small graphs."""
    run_host_check("navcrowd_host_check", tmp_path)


def test_document_states_the_layer():
    text = open(os.path.join(ROOT, "CROWD.md")).read()
    for word in ("VtmcNavCrowdParams", "VtmcNavCrowdAgent", "One agent per span", "One box only", "re-route", "every other tick", "What it costs", "smallest index"):
        assert word in text, word
    for path in (_header.LAYERS["navfield"].path, os.path.join(ROOT, "PATHFINDING.md")):   # where the gap was named
        assert "CROWD.md" in open(path).read(), path


# -- CPU: the twin against the rule's properties -------------------------------------------------------------------------------------------
def contended(case, every):
    starts = case.reached[::every]
    crowd = case.crowd()
    assert crowd.spawn(starts, speeds_of(len(starts))) == len(starts)
    return crowd, starts


def test_twin_invariants_on_the_crafted_field():
    """After every tick no two occupying agents share a span and the occupancy is the agents'; every move follows a link and strictly
    lowers D."""
    case = crafted_case("crafted", "far")
    assert len(case.spans) == 2548 and len(case.reached) == 2462
    D = case.cells["cost"].astype(np.int64)
    for every, detour, flags in ((3, ANY, LEAVE), (2, 2048, 0)):
        crowd, starts = contended(case, every)
        for tick in range(48):
            crowd.step(detour, flags, 1)
            agents, occ = crowd.read()
            on = np.isin(agents["state"], twin.OCCUPYING)
            assert len(np.unique(agents["span"][on])) == on.sum() and (agents["span"][agents["state"] == UNPLACED] == -1).all()
            want = np.full(len(occ), -1, np.int32)
            want[agents["span"][on]] = np.nonzero(on)[0]
            assert np.array_equal(occ, want) and (agents["budget"] <= _lib.NAVCROWD_BUDGET_CAP).all()
            assert crowd.info() == (len(starts), int(on.sum()), int(np.isin(agents["state"], (ARRIVED, GONE)).sum()), tick + 1, crowd.moved_last)
        assert len(crowd.trail) == crowd.moves > 500 and crowd.lost > 50 and crowd.sidesteps > 50
        for _, i, s, t in crowd.trail:
            assert t in case.spans["link"][s] and D[t] < D[s]
        if detour != ANY:
            costs = {(s, int(t)): int(c) for s, _ in enumerate(case.spans) for t, c in zip(case.spans["link"][s], case.costs[s]) if t >= 0}
            assert all(D[t] + costs[s, t] <= D[s] + detour for _, _, s, t in crowd.trail)


def test_twin_lone_agent_reproduces_the_trace():
    """A lone agent whose speed is at least the largest edge cost moves every tick: its spans are navfield_twin.trace's, one per tick."""
    case = crafted_case("crafted", "far")
    fastest = int(case.costs.max())
    paths, lengths = navfield_twin.trace(case.cells, case.reached[::41], 256)
    assert fastest > 1024 and lengths.max() < 256 and lengths.max() > 20
    for row, length in zip(paths, lengths):
        crowd = case.crowd()
        assert crowd.spawn([row[0]], fastest) == 1
        for k in range(1, length):
            crowd.step(0, 0, 1)
            assert crowd.read()[0][0]["span"] == row[k] and crowd.moved_last == 1
        assert crowd.step(0, 0, 1) == (1, 1, 1, int(length), 0) and crowd.read()[0][0]["state"] == ARRIVED


def test_twin_speed_512_on_flat_ground_moves_every_other_tick():
    r = nav_of(flat_grid(12, 1))
    case = Case(r, [(11, 0)], 0.0, 0.0)
    crowd = case.crowd()
    crowd.spawn([0], 512)
    seen = [(int(crowd.step(ANY, 0, 1)[4]), int(crowd.read()[0][0]["span"]), int(crowd.read()[0][0]["budget"])) for _ in range(8)]
    assert seen == [(0, 0, 512), (1, 1, 0), (0, 1, 512), (1, 2, 0), (0, 2, 512), (1, 3, 0), (0, 3, 512), (1, 4, 0)]


def test_twin_of_two_claimants_the_smaller_index_wins():
    """Three spans in a row and the goal in the middle: both ends claim it; then a queue, which moves every other tick."""
    r = nav_of(flat_grid(3, 1))
    case = Case(r, [(1, 0)], 0.0, 0.0)
    for order, winner in (([2, 0], 0), ([0, 2], 0)):
        crowd = case.crowd()
        crowd.spawn(order, 1024)
        crowd.step(ANY, 0, 1)
        agents, occ = crowd.read()
        assert agents["span"].tolist() == [1, order[1]] and occ.tolist()[1] == winner and crowd.lost == 1 and crowd.moved_last == 1
        assert agents["budget"].tolist() == [0, 1024]
        crowd.step(ANY, 0, 3)
        assert crowd.read()[0]["state"].tolist() == [ARRIVED, WALKING] and crowd.read()[0]["budget"][1] == 4096 and crowd.moved_last == 0
    queue = Case(nav_of(flat_grid(8, 1)), [(7, 0)], 0.0, 0.0).crowd()
    queue.spawn([1, 0, -1, 0], 2048)
    assert queue.read()[0]["state"].tolist() == [WALKING, WALKING, UNPLACED, UNPLACED]
    where = []
    for _ in range(4):
        queue.step(ANY, LEAVE, 1)
        where.append(queue.read()[0]["span"][:2].tolist())
    assert where == [[2, 0], [3, 1], [4, 2], [5, 3]]   # a span vacated in a tick is free only from the next one: the follower starts a tick late


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
def same(ex, crowd, what=""):
    """The device's crowd against the twin's: agents and occupancy as bytes, and the info."""
    agents, occ = ex.navcrowd_read()
    want_agents, want_occ = crowd.read()
    assert agents.dtype == vt.NAVCROWD_AGENT_DTYPE and occ.dtype == np.int32
    assert agents.tobytes() == want_agents.tobytes(), (what, np.nonzero(agents != want_agents)[0][:8])
    assert occ.tobytes() == want_occ.tobytes(), what
    assert ex.navcrowd_info() == crowd.info(), what
    return agents, occ


def both(ex, crowd, starts, speeds, what=""):
    assert ex.navcrowd_spawn(starts, speeds) == crowd.spawn(starts, speeds)
    return same(ex, crowd, what)


def step_both(ex, crowd, detour, flags, ticks, what=""):
    assert ex.navcrowd_step(raw(detour, flags), ticks) == crowd.step(detour, flags, ticks), what
    return same(ex, crowd, what)


def crafted_terrain(field):
    if field == "turned":
        return nav.terrain(nav.turned_field(), (DIMS[2], DIMS[1], DIMS[0]))
    return nav.terrain(nav.crafted_field())


@pytest.fixture(scope="module")
def crafted_ex():
    with nav.terrain(nav.crafted_field()) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("field,box", [("crafted", "far"), ("crafted", "interior"), ("turned", "far")])
def test_gpu_contended_crowd_equals_the_twin(field, box):
    """Three goals spread over the largest region, agents on every third reached span, any detour, leaving on arrival, 64 ticks in one call;
    the same as 1 + 2 + 61 ticks; then every second span, a detour of 2048 and 130 ticks.  The twin's counters say that the crowd was
    contended: on the crafted field and the far box 8465 moves, 1925 lost claims, 2033 sidesteps and 94 arrivals of 821 agents, then
    10161, 3619, 3234 and 195 of 1231."""
    case = crafted_case(field, box)
    with crafted_terrain(field) as ex:
        nav.assert_same(ex.terrain_nav(*nav.BOXES[box], nav.raw_params(*NAV_PARAMS)), case.nav, box)
        case.field_on(ex)
        for every, detour, ticks in ((3, ANY, 64), (2, 2048, 130)):
            starts = case.reached[::every]
            speeds = speeds_of(len(starts))
            crowd = case.crowd()
            both(ex, crowd, starts, speeds, "spawn")
            once = step_both(ex, crowd, detour, LEAVE, ticks, "one call")
            arrived = crowd.info()[2]
            print("%s %s: %d agents, %d moves, %d lost claims, %d sidesteps, %d arrivals" % (field, box, len(starts), crowd.moves, crowd.lost, crowd.sidesteps, arrived))
            assert crowd.moves >= 1000 and crowd.lost >= 100 and crowd.sidesteps >= 100 and arrived >= 50
            if (field, box) == ("crafted", "far"):
                assert (len(starts), crowd.moves, crowd.lost, crowd.sidesteps, arrived) in ((821, 8465, 1925, 2033, 94), (1231, 10161, 3619, 3234, 195))
            if every == 3:
                split = case.crowd()
                both(ex, split, starts, speeds, "spawn again")
                for part in (1, 2, 61):
                    step_both(ex, split, detour, LEAVE, part, "split %d" % part)
                again = ex.navcrowd_read()
                assert again[0].tobytes() == once[0].tobytes() and again[1].tobytes() == once[1].tobytes()


@pytest.mark.gpu
def test_gpu_jam(crafted_ex):
    """One goal and nobody leaves: after 300 ticks the crowd is packed round the goal and nothing moves, on both sides."""
    ex, base = crafted_ex, crafted_case("crafted", "far")
    case = Case(base.nav, spread_goals(base.spans, 1))
    ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
    case.field_on(ex)
    starts = case.reached[::3]
    crowd = case.crowd()
    both(ex, crowd, starts, speeds_of(len(starts)))
    agents, occ = step_both(ex, crowd, ANY, 0, 300, "jam")
    info = ex.navcrowd_info()
    assert info[4] == 0 == crowd.moved_last and info[1] == len(starts) and info[2] == 1 and info[3] == 300 and crowd.moves > 1000
    goal = case.goals[0][0]
    assert occ[goal] >= 0 and agents["state"][occ[goal]] == ARRIVED and all(occ[t] >= 0 for t in case.spans["link"][goal] if t >= 0)
    still = step_both(ex, crowd, ANY, 0, 2, "still jammed")
    assert still[1].tobytes() == occ.tobytes() and ex.navcrowd_info()[4] == 0


@pytest.mark.gpu
def test_gpu_spawn(crafted_ex):
    """Duplicate spans and -1 entries: of those that ask for one span the smallest index stands on it."""
    ex, case = crafted_ex, crafted_case("crafted", "far")
    ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
    rng = np.random.default_rng(11)
    starts = rng.integers(0, 600, 1500).astype(np.int32)       # 1500 agents ask for 600 spans: every span several times over
    starts[::17] = -1
    speeds = rng.integers(1, (1 << 20) + 1, 1500)
    speeds[:2] = 1, 1 << 20
    crowd = case.crowd()
    placed = ex.navcrowd_spawn(starts, speeds)                  # before any field: a nav result is all it needs
    assert placed == crowd.spawn(starts, speeds)
    agents, occ = same(ex, crowd, "spawn")
    asked = starts >= 0
    first = {}
    for i in np.nonzero(asked)[0]:
        first.setdefault(int(starts[i]), int(i))
    assert placed == len(first) < asked.sum() and sorted(np.nonzero(agents["state"] == WALKING)[0].tolist()) == sorted(first.values())
    assert (agents["state"][~asked] == UNPLACED).all() and (agents["span"][agents["state"] == UNPLACED] == -1).all()
    assert (agents["speed"] == speeds).all() and (agents["budget"] == 0).all() and ex.navcrowd_info() == (1500, placed, 0, 0, 0)
    assert {int(s): int(i) for s, i in enumerate(occ) if i >= 0} == first
    # a crowd of -1s stands nowhere; a second spawn replaces the first
    assert ex.navcrowd_spawn([-1, -1, -1], 7) == 0 and ex.navcrowd_info() == (3, 0, 0, 0, 0) and (ex.navcrowd_read()[1] == -1).all()
    case.field_on(ex)
    assert ex.navcrowd_step(raw(), 5) == (3, 0, 0, 5, 0)


CORRIDOR = (300, 3)   # columns of the corridor's nav box, on a flat terrain of 304 x 8 x 8 cells


@functools.lru_cache(maxsize=None)
def corridor_grid():
    g = flat_grid(306, 10, 10)
    g.setflags(write=False)
    return g


@pytest.mark.gpu
def test_gpu_agent_counts_on_a_corridor():
    """1, 63, 65 and 821 agents in a corridor of 300 x 3 columns, packed at one end and the goal at the other: partial waves, and a queue
    that crosses workgroup boundaries."""
    lower, upper = nav.world_of((1, 0, 1)), nav.world_of((CORRIDOR[0], 9, CORRIDOR[1]))
    with nav.terrain(corridor_grid(), (304, 8, 8)) as ex:
        got = ex.terrain_nav(lower, upper, nav.raw_params(*NAV_PARAMS))
        assert got[2] == (1, 0, 1) and got[3] == (CORRIDOR[0], 10, CORRIDOR[1]) and len(got[0]) == 900
        navr = nav_twin.build(corridor_grid(), got[2], got[3], *NAV_PARAMS)
        nav.assert_same(got, navr, "corridor")
        case = Case(navr, [(at(navr, 300, 2), 0)], 0.0, 0.0)
        case.field_on(ex)
        assert len(case.reached) == 900
        order = np.argsort(-case.cells["cost"].astype(np.int64), kind="stable").astype(np.int32)   # farthest from the goal first
        for count in (1, 63, 65, 821):
            crowd = case.crowd()
            both(ex, crowd, order[:count], speeds_of(count), count)
            for detour, ticks in ((ANY, 1), (0, 7), (ANY, 40)):
                step_both(ex, crowd, detour, LEAVE if count == 65 else 0, ticks, count)
            assert crowd.moves > 0 and (count == 1 or crowd.lost > 0)


def ramp_grid():
    """A corridor of 40 x 9 columns with a ridge across its middle rows, 0.5 up per column to 2 above the floor and down again."""
    g = flat_grid(42, 11, 14).copy()
    for j, x in enumerate(range(12, 19)):
        rise = min(j + 1, 7 - j) * 0.5           # 0.5 1 1.5 2 1.5 1 0.5
        h = 2.5 + rise
        for z in range(3, 8):
            nav.floor(g, x, z, int(h - 0.25), 0.5 if h % 1 else 1.0)
    return g


@pytest.mark.gpu
def test_gpu_costs_that_differ():
    """A ridge that costs four per unit climbed: with max_detour 0 nobody steps anywhere but along a cheapest way, with any detour a blocked
    agent goes over the ridge.  The twin gives different agents for the two, and the device equals both."""
    g = np.full((42, 18, 18), nav.AIR, f32)
    g[:, :14, :11] = ramp_grid()
    lower, upper = nav.world_of((1, 0, 1)), nav.world_of((40, 13, 9))
    with nav.terrain(g, (40, 16, 16)) as ex:
        got = ex.terrain_nav(lower, upper, nav.raw_params(*NAV_PARAMS))
        navr = nav_twin.build(g, got[2], got[3], *NAV_PARAMS)
        nav.assert_same(got, navr, "ramp")
        case = Case(navr, [(at(navr, 40, 5), 0)], 4.0, 0.0)
        case.field_on(ex)
        assert got[3] == (40, 14, 9) and len(case.reached) == 360 and len(np.unique(case.costs)) >= 3 and int(case.costs.max()) == 1024 + 2048
        starts = np.array([at(navr, x, z) for x in range(1, 11) for z in range(1, 10)], np.int32)   # a block of 90 in front of the ridge
        results = {}
        for detour in (0, ANY):
            crowd = case.crowd()
            both(ex, crowd, starts, speeds_of(len(starts)), detour)
            results[detour] = step_both(ex, crowd, detour, 0, 40, detour)[0]
            assert crowd.moves > 200
        assert results[0].tobytes() != results[ANY].tobytes()


def stacked_case():
    """The crafted field's C and E under a nav build that links steps of 2.5, the goal sets and the starts of the test below: the six spans
    of the two columns first, then a checkerboard of the spans round them."""
    case = Case(nav.twin_of("crafted", "far", *STEEP_PARAMS))
    r = case.nav
    floors = [at(r, 20, 3, f) for f in range(3)]
    under, top, beside = at(r, 32, 3, 0), at(r, 32, 3, 1), at(r, 33, 3)
    special = floors + [under, top, beside]
    near = [first + f for x in range(17, 37) for z in range(1, 7) if (x + z) % 2 == 0 for column, first in [nav.column(r, x, z)] for f in range(len(column))]
    starts = np.array(special + [s for s in near if s not in special], np.int32)
    return case, floors, (under, top, beside), starts, ([(at(r, 40, 3), 0)], [(under, 0)], [(floors[0], 0), (floors[1], 500)])


def check_stacked(case, crowd, floors, one_way, goals):
    """What the twin's run says about the two columns, whatever made the same bytes."""
    under, top, beside = one_way
    link = case.spans["link"]
    agents = crowd.read()[0]
    assert crowd.moves > 50 and agents["state"][[1, 2]].tolist() == [ARRIVED if floors[1] in dict(goals) else STRANDED, STRANDED]
    assert agents["span"][[1, 2]].tolist() == floors[1:]                   # the slabs link nowhere: who stands on them stays
    for _, i, s, t in crowd.trail:
        assert t in link[s] and (s, t) != (beside, under)                  # forwards only
    # the ground floor of column (20, 3) is walked while both slabs over it are occupied: the floors of one column do not contend
    if floors[0] in dict(goals):   # ... or stood round, where the agent on it has arrived
        assert agents["state"][0] == ARRIVED and (crowd.read()[1][link[floors[0]]] >= 0).all()
    else:
        assert any(t == floors[0] or s == floors[0] for _, _, s, t in crowd.trail)


def test_twin_stacked_floors_and_the_one_way_link():
    case, floors, one_way, starts, goal_sets = stacked_case()
    under, top, beside = one_way
    link = case.spans["link"]
    assert under in link[at(case.nav, 31, 3)] and beside in link[under] and under not in link[beside] and top in link[beside]
    assert (link[floors[1:]] == -1).all() and case.spans["height"][floors].tolist() == [2.5, 7.5, 12.5]
    for goals in goal_sets:
        case.route(goals)
        crowd = case.crowd()
        assert crowd.spawn(starts, speeds_of(len(starts))) == len(starts)
        crowd.step(ANY, 0, 24)
        check_stacked(case, crowd, floors, one_way, goals)


@pytest.mark.gpu
def test_gpu_stacked_floors_and_the_one_way_link():
    """The crafted field's C (three floors in column (20, 3)) and E (the floor under the slab of (32, 3) climbs to (33, 3), which answers
    to the slab's top): agents on the floors of one column never contend, and nobody walks a link backwards."""
    case, floors, one_way, starts, goal_sets = stacked_case()
    with nav.terrain(nav.crafted_field()) as ex:
        nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*STEEP_PARAMS)), case.nav, "far")
        for goals in goal_sets:
            case.route(goals)
            case.field_on(ex)
            crowd = case.crowd()
            both(ex, crowd, starts, speeds_of(len(starts)), goals)
            for _ in range(3):
                step_both(ex, crowd, ANY, 0, 8, goals)
            check_stacked(case, crowd, floors, one_way, goals)


@pytest.mark.gpu
def test_gpu_reroute_and_life_cycle():
    """20 ticks, a new field with other goals, 20 more: the crowd survived and equals the twin.  Then an erosion: the crowd is gone, and
    spawn and step on the eroded spans equal the twin.  Then a nav build: nothing answers."""
    base = crafted_case("crafted", "far")
    case = Case(base.nav)
    with nav.terrain(nav.crafted_field()) as ex:
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        case.field_on(ex)
        starts = case.reached[::3]
        crowd = case.crowd()
        both(ex, crowd, starts, speeds_of(len(starts)))
        step_both(ex, crowd, ANY, 0, 20, "before")
        before = crowd.info()
        case.route(spread_goals(case.spans, 2))
        case.field_on(ex)                      # vtmc_navfield_build keeps the crowd
        crowd.set_field(case.cells, case.costs)
        same(ex, crowd, "kept")
        step_both(ex, crowd, ANY, 0, 20, "after")
        assert before[2] > 0 and crowd.info()[3] == 40 and crowd.moved_last > 0
        # an edit keeps it, as it keeps the spans
        ex.terrain_update([vt.SphereModifier(nav.world_of((40, 3, 16)), 2.5, False)])
        same(ex, crowd, "edited")
        # an erosion drops it
        p = _lib.NavErodeParamsStruct(2, 0, (ctypes.c_int32 * 2)(0, 0))
        eroded = ex.nav_erode(p)
        no_result(ex.navcrowd_info)
        no_result(ex.navcrowd_read)
        no_result(lambda: ex.navcrowd_step(raw(), 1))
        want = naverode_twin.erode(base.nav, 2)
        nav.assert_same(eroded[:4], want[:4], "eroded")
        small = Case(want[:4])
        starts = small.reached[::2]
        crowd = small.crowd()
        both(ex, crowd, starts, speeds_of(len(starts)), "eroded")      # spawn needs no field
        no_result(lambda: ex.navcrowd_step(raw(), 1))
        small.field_on(ex)
        step_both(ex, crowd, 2048, LEAVE, 30, "eroded")
        assert crowd.moves > 300
        # a nav build drops it; so does a build that fails after it invalidated the nav result, and an init
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        for call in (ex.navcrowd_info, ex.navcrowd_read, ex.device_navcrowd, lambda: ex.navcrowd_step(raw(), 1)):
            no_result(call)
        assert ex.navcrowd_spawn([0, 1], 1024) == 2
        with pytest.raises(vt.VtmcError):
            ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 0.5, 10))     # too many spans
        no_result(ex.navcrowd_info)
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
        assert ex.navcrowd_spawn([0, 1], 1024) == 2
        ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
        no_result(ex.navcrowd_info)


@pytest.mark.gpu
def test_gpu_nothing_else_moves():
    """Everything else the context holds, the nav result, the field, the distance and the origin, byte for byte before and after spawn
    and step."""
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
        case.field_on(ex)

        def everything():
            spans, offsets, first, ext = ex.nav_read()
            return nav.held(ex, L, h) + [spans.tobytes(), offsets.tobytes(), first, ext, ex.device_nav(), ex.navfield_read().tobytes(), ex.navfield_info(),
                                         ex.device_navfield(), ex.nav_distance_read().tobytes(), ex.device_nav_distance(), ex.nav_erode_origin().tobytes()]
        before = everything()
        starts = case.reached[::2]
        crowd = case.crowd()
        both(ex, crowd, starts, speeds_of(len(starts)))
        assert everything() == before
        step_both(ex, crowd, ANY, LEAVE, 25)
        assert crowd.moves > 100 and everything() == before
        step_both(ex, crowd, 0, 0, 1)
        assert everything() == before


@pytest.mark.gpu
def test_gpu_refusals_keep_the_crowd(crafted_ex):
    ex, case = crafted_ex, crafted_case("crafted", "far")
    L, h = ex._L, ex._h
    total = len(case.spans)
    ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
    ok_spans, ok_speeds, fine = np.array([5, -1, 5, 9], np.int32), np.array([1, 2, 3, 1 << 20], np.uint32), raw()
    agents4 = np.zeros(4, vt.NAVCROWD_AGENT_DTYPE)

    def spawn(spans=ok_spans, speeds=ok_speeds, n=4):
        placed = ctypes.c_int32(-7)
        rc = L.vtmc_navcrowd_spawn(h, spans.ctypes.data if spans is not None else None, speeds.ctypes.data if speeds is not None else None, n, ctypes.byref(placed))
        return rc, placed.value

    def step(p=fine, ticks=1):
        return L.vtmc_navcrowd_step(h, ctypes.byref(p) if p is not None else None, ticks)
    # no crowd yet: everything but spawn answers NO_RESULT
    for call in (step, lambda: step(ticks=0), lambda: L.vtmc_navcrowd_read(h, agents4.ctypes.data, 4, None), lambda: L.vtmc_navcrowd_info(h, None, None, None, None, None),
                 lambda: L.vtmc_navcrowd_device_results(h, None, None, None), lambda: L.vtmc_debug_navcrowd_ms(h, (ctypes.c_float * 1)())):
        assert call() == _lib.ERR_NO_RESULT and L.vtmc_last_error(h).decode() != ""
    crowd = case.crowd()
    starts = case.reached[::5]
    both(ex, crowd, starts, speeds_of(len(starts)))
    kept = ex.navcrowd_read()

    def untouched():
        now = ex.navcrowd_read()
        return now[0].tobytes() == kept[0].tobytes() and now[1].tobytes() == kept[1].tobytes() and ex.navcrowd_info() == crowd.info()
    # no field: step refuses, also with nothing to do
    assert step() == _lib.ERR_NO_RESULT and step(ticks=0) == _lib.ERR_NO_RESULT and "navfield_build" in L.vtmc_last_error(h).decode() and untouched()
    case.field_on(ex)
    bad_span = [np.array([5, v, 5, 9], np.int32) for v in (-2, total, 2 ** 31 - 1, -2 ** 31)]
    bad_speed = [np.array([1, v, 3, 4], np.uint32) for v in (0, (1 << 20) + 1, 0xffffffff)]
    spawns = [lambda: spawn(spans=None), lambda: spawn(speeds=None), lambda: spawn(n=0), lambda: spawn(n=-1), lambda: spawn(n=(1 << 24) + 1), lambda: spawn(n=-2 ** 31)] + \
        [lambda v=v: spawn(spans=v) for v in bad_span] + [lambda v=v: spawn(speeds=v) for v in bad_speed]
    for i, call in enumerate(spawns):
        assert call()[0] == _lib.ERR_INVALID_ARG and "navcrowd_spawn" in L.vtmc_last_error(h).decode() and untouched(), i
    steps = [lambda: step(p=None), lambda: step(ticks=-1), lambda: step(ticks=4097), lambda: step(ticks=2 ** 31 - 1)] + \
        [lambda q=q: step(p=q) for q in (raw(ANY, 2), raw(0, 3), raw(0, 0x80000000), raw(0, 0xffffffff), raw(ANY, 0, (1, 0)), raw(ANY, LEAVE, (0, 1)), raw(0, 0, (0, 0xffffffff)))]
    for i, call in enumerate(steps):
        assert call() == _lib.ERR_INVALID_ARG and "navcrowd_step" in L.vtmc_last_error(h).decode() and untouched(), i
    # reads: capacity, null
    n = len(starts)
    buf, occ = np.zeros(n, vt.NAVCROWD_AGENT_DTYPE), np.zeros(total, np.int32)
    assert L.vtmc_navcrowd_read(h, buf.ctypes.data, n - 1, occ.ctypes.data) == _lib.ERR_CAPACITY and str(n) in L.vtmc_last_error(h).decode()
    assert L.vtmc_navcrowd_read(h, None, n, occ.ctypes.data) == _lib.ERR_INVALID_ARG and not buf.tobytes().strip(b"\0") and not occ.any()
    assert L.vtmc_navcrowd_read(h, buf.ctypes.data, n, None) == _lib.OK and buf.tobytes() == kept[0].tobytes()
    assert L.vtmc_navcrowd_info(h, None, None, None, None, None) == _lib.OK and L.vtmc_navcrowd_device_results(h, None, None, None) == _lib.OK
    # nothing to do is a success that touches nothing; and the crowd still steps as the twin's
    assert step(ticks=0) == _lib.OK and untouched()
    step_both(ex, crowd, ANY, LEAVE, 4096 // 64, "after the refusals")
    assert spawn() == (_lib.OK, 2) and ex.navcrowd_read()[0]["state"].tolist() == [WALKING, UNPLACED, UNPLACED, WALKING]


@pytest.mark.gpu
def test_gpu_device_results(crafted_ex):
    """The device pointers hold the bytes the read gives, before and after a step."""
    ex, case = crafted_ex, crafted_case("crafted", "far")
    ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS))
    case.field_on(ex)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    starts = case.reached[::4]
    crowd = case.crowd()
    both(ex, crowd, starts, speeds_of(len(starts)))
    for ticks in (0, 1, 30):
        if ticks:
            step_both(ex, crowd, ANY, LEAVE, ticks)
        agents, occ = ex.navcrowd_read()
        a, o, count = ex.device_navcrowd()
        d_agents, d_occ = np.zeros(count, vt.NAVCROWD_AGENT_DTYPE), np.zeros(len(case.spans), np.int32)
        assert count == len(starts) and a and o
        assert hip.hipMemcpy(d_agents.ctypes.data, a, d_agents.nbytes, 2) == 0 and hip.hipMemcpy(d_occ.ctypes.data, o, d_occ.nbytes, 2) == 0
        assert d_agents.tobytes() == agents.tobytes() and d_occ.tobytes() == occ.tobytes()
    ms = (ctypes.c_float * 1)(-1.0)
    assert ex._L.vtmc_debug_navcrowd_ms(ex._h, ms) == _lib.OK and np.isfinite(ms[0]) and ms[0] > 0


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's SpawnCrowd, StepCrowd and ReadCrowd against the Python path on the same world (host/host_selftest.cpp
    --gpu-navcrowd)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-navcrowd", tmp_path)
    files = {k: np.fromfile(tmp_path / ("navcrowd_%s.bin" % k), vt.NAVCROWD_AGENT_DTYPE) for k in ("spawned", "stepped", "rerouted")}
    occs = {k: np.fromfile(tmp_path / ("navcrowd_%s_occupancy.i32" % k), np.int32) for k in ("spawned", "stepped", "rerouted")}
    info = np.fromfile(tmp_path / "navcrowd_info.i32", np.int32).reshape(3, 5)
    with vt.Extractor(0) as ex:
        spans = nav.mirror_world(ex)[0]
        n = len(spans)
        at_goals = ex.nav_locate([(0.0, 6.3, 4.0), (12.0, 6.3, 15.0)], 1.0, 1.0)
        ex.nav_field([(at_goals[0], 0), (at_goals[1], 3000)], vt.NavFieldParams(2.0, 0.5))
        starts = [s if s % 7 else -1 for s in range(0, n, 2)] + [2, 2]
        speeds = [400 + (131 * i) % 1200 for i in range(len(starts))]
        want, got_info = {}, []
        placed = ex.navcrowd_spawn(starts, speeds)
        want["spawned"] = ex.navcrowd_read()
        got_info.append(ex.navcrowd_info())
        got_info.append(ex.navcrowd_step(vt.NavCrowdParams(None, True), 24))
        want["stepped"] = ex.navcrowd_read()
        ex.nav_field([(at_goals[1], 0)], vt.NavFieldParams(2.0, 0.5))
        got_info.append(ex.navcrowd_step(vt.NavCrowdParams(1024, False), 16))
        want["rerouted"] = ex.navcrowd_read()
    assert n > 100 and 0 < placed < len(starts) and info.tolist() == [list(i) for i in got_info] and got_info[1][2] > 0 and got_info[2][3] == 40
    for k in files:
        assert files[k].tobytes() == want[k][0].tobytes() and occs[k].tobytes() == want[k][1].tobytes(), k
    assert want["stepped"][0].tobytes() != want["spawned"][0].tobytes() != want["rerouted"][0].tobytes()
