"""Flow fields on the navigation layer: locate, cost field, traced paths (include/vtmc_navfield.h, csrc/terrain_navfield.hip).

The rule (NAVFIELD in include/vtmc_navfield.h) is integers, and float32 of one operation per step for the edge costs and the locate, so
the device is compared with navfield_twin.py for EQUALITY: cells, located spans, paths and lengths as raw bytes.  The twin finds the costs
with another algorithm (Dijkstra over the reversed links; the device relaxes by pulling along the links), and is itself pinned to answers
worked out by hand.  Fields, boxes and helpers are nav_support.py's; the contract every layer's header keeps is tests/test_abi_layers.py's."""
import ctypes
import functools
import os

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import nav_twin
import navfield_twin as twin
from host_check import run_host_check
import nav_support as nav
from nav_support import largest_region, raw_field_params, same_cells, world
from terrain_twin import no_result

ROOT = nav.ROOT
f32 = np.float32
DIMS, SCALE, ORIGIN = nav.DIMS, nav.SCALE, nav.ORIGIN
UNIT, UNREACHED = _lib.NAVFIELD_UNIT, _lib.NAVFIELD_UNREACHED
NO_CUT, CUT = 0x7fffffff, 40 * 1024          # the cut: 40 level steps, on a floor 74 columns long
NAV_PARAMS = ((1, 2.5), (3, 0.5))             # (agent_height, max_step) of the nav builds under the fields
COSTS = ((0.0, 0.0), (1.0, 0.25), (1024.0, 0.0))
GOAL_COSTS = (0, 5000, 0)                     # floor, plateau, platform


def span_at(result, x, z, height):
    """The index of the span of grid column (x, z) with that height."""
    spans, first = nav.column(result, x, z)
    (j,) = np.nonzero(spans["height"] == f32(height))[0]
    return first + int(j)


def crafted_goals(result, turned=False):
    """One goal on the flat floor, one on a plateau, one on the floating platform (crafted_field's G)."""
    at = (lambda x, z, h: span_at(result, z, x, h)) if turned else (lambda x, z, h: span_at(result, x, z, h))
    return list(zip((at(8, 20, 2.5), at(53, 10, 8.5), at(45, 4, 10.5)), GOAL_COSTS))


def choices(spans, cells, climb, drop):
    """Per span, how many k explain its cost."""
    cost, link, D = twin.edge_costs(spans, climb, drop), spans["link"].astype(np.int64), cells["cost"].astype(np.int64)
    reached = D != UNREACHED
    ok = (link >= 0) & reached[np.maximum(link, 0)] & (D[np.maximum(link, 0)] + cost == D[:, None]) & reached[:, None]
    return ok.sum(axis=1)


# -- CPU: the header, the binding, the documents, the host half -----------------------------------------------------------------------------
def test_header_declares_the_layer():
    F = _header.LAYERS["navfield"]
    assert F.constants == {"VTMC_NAVFIELD_UNIT": 1024, "VTMC_NAVFIELD_UNREACHED": 0xffffffff, "VTMC_NAVFIELD_MAX_GOALS": 1 << 20}
    assert (_lib.NAVFIELD_UNIT, _lib.NAVFIELD_UNREACHED, _lib.NAVFIELD_MAX_GOALS) == (1024, 2 ** 32 - 1, 2 ** 20)
    assert list(F.prototypes) == ["vtmc_nav_locate", "vtmc_navfield_build", "vtmc_navfield_read", "vtmc_navfield_info", "vtmc_navfield_device_results",
                                  "vtmc_navfield_trace"] == _lib.LAYER_SYMBOLS["navfield"]
    assert set(F.structs) == {"vtmc_navfield_params", "vtmc_navfield_goal", "vtmc_navfield_cell"}
    VP, I32, FL = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert F.prototypes["vtmc_nav_locate"].argtypes == [VP, VP, I32, FL, FL, VP] and F.prototypes["vtmc_navfield_build"].argtypes == [VP, VP, I32, VP, VP]
    assert F.prototypes["vtmc_navfield_trace"].argtypes == [VP, VP, I32, I32, VP, VP] and F.prototypes["vtmc_navfield_read"].argtypes == [VP, VP, I32]
    # struct sizes: 16, 8 and 8
    assert ctypes.sizeof(_lib.NavFieldParamsStruct) == 16 and _lib.NavFieldParamsStruct.flags.offset == 12 and _lib.NavFieldParamsStruct.max_cost.offset == 8
    c, g = vt.NAVFIELD_CELL_DTYPE, vt.NAVFIELD_GOAL_DTYPE
    assert c.itemsize == 8 and c.names == ("cost", "next") and [c.fields[n][1] for n in c.names] == [0, 4] and c["cost"] == np.uint32 and c["next"] == np.int32
    assert g.itemsize == 8 and g.names == ("span", "cost") and [g.fields[n][1] for n in g.names] == [0, 4] and g["span"] == np.int32 and g["cost"] == np.uint32
    rule = open(F.path).read()
    for word in ("NAVFIELD", "Edge cost", "Goals", "Cost", "Next", "Cell", "Locate", "Trace", "no agent radius", "no any-angle smoothing", "no field across"):
        assert word in rule, word
    # the navigation layer's own header and document point here and gained nothing
    assert "vtmc_navfield.h" in open(_header.LAYERS["nav"].path).read() and "PATHFINDING.md" in open(os.path.join(ROOT, "NAVIGATION.md")).read()


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert hasattr(L, "vtmc_debug_navfield_ms")
    pos, out, n = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int32 * 4)(), ctypes.c_int32()
    goal, p = np.zeros(1, vt.NAVFIELD_GOAL_DTYPE), raw_field_params()
    assert L.vtmc_nav_locate(None, ctypes.byref(pos), 1, 0.5, 0.5, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_build(None, goal.ctypes.data, 1, ctypes.byref(p), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_read(None, ctypes.byref(out), 1) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_info(None, ctypes.byref(n), None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_device_results(None, None, ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_navfield_trace(None, ctypes.byref(out), 1, 2, ctypes.byref(out), ctypes.byref(n)) == _lib.ERR_INVALID_ARG


def test_document_states_the_layer():
    text = open(os.path.join(ROOT, "PATHFINDING.md")).read()
    for word in ("VtmcNavFieldParams", "VtmcNavFieldGoal", "VtmcNavFieldCell", "agent radius", "any-angle", "two boxes"):
        assert word in text, word


def test_navfield_params_validate():
    p = vt.NavFieldParams(1.5, 0.25, max_cost=4096).to_struct()
    assert (p.climb_cost, p.drop_cost, p.max_cost, p.flags) == (1.5, 0.25, 4096, 0)
    assert vt.NavFieldParams(0, 1024).to_struct().max_cost == 0x7fffffff and vt.NavFieldParams(0, 1024).to_struct().drop_cost == 1024.0
    for bad in (dict(climb_cost=-1.0, drop_cost=0.0), dict(climb_cost=np.nan, drop_cost=0.0), dict(climb_cost=np.inf, drop_cost=0.0),
                dict(climb_cost=1024.5, drop_cost=0.0), dict(climb_cost=0.0, drop_cost=-0.5), dict(climb_cost=0.0, drop_cost=np.nan),
                dict(climb_cost=0.0, drop_cost=2000.0), dict(climb_cost=1.0, drop_cost=1.0, max_cost=0), dict(climb_cost=1.0, drop_cost=1.0, max_cost=2 ** 31),
                dict(climb_cost=1.0, drop_cost=1.0, max_cost=1.5), dict(climb_cost=1.0, drop_cost=1.0, max_cost=True)):
        with pytest.raises(ValueError):
            vt.NavFieldParams(**bad)


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/navfield_host_check.cpp: the host half (csrc/terrain_navfield.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("navfield_host_check", tmp_path)


# -- CPU: the twin against answers stated by hand ---------------------------------------------------------------------------------------------
def two_spans(h0, h1):
    """Two spans side by side along x, linked both ways."""
    s = np.zeros(2, vt.NAV_SPAN_DTYPE)
    s["height"], s["link"] = (h0, h1), -1
    s["link"][0][1], s["link"][1][0] = 1, 0
    return s


def test_twin_reproduces_hand_stated_answers():
    """Pins the twin to answers worked out on paper, so that it is not pinned to itself alone."""
    # a flat floor of 9 x 7 columns, climb = drop = 0: 1024 x the Manhattan distance; next is the smallest k that lowers it (-x, +x, -z, +z)
    g = np.full((9, 6, 7), nav.AIR, f32)
    g[:, 0:3, :] = nav.SOLID
    flat = nav_twin.build(g, (0, 0, 0), (9, 6, 7), 1, 0.5)
    assert len(flat[0]) == 63 and (flat[0]["height"] == 2.5).all()
    gx, gz = 3, 4
    cells = twin.field(flat[0], [(gx + 9 * gz, 0)], 0.0, 0.0)
    for z in range(7):
        for x in range(9):
            want_next = (x - 1, z) if x > gx else (x + 1, z) if x < gx else (x, z - 1) if z > gz else (x, z + 1) if z < gz else None
            c = cells[x + 9 * z]
            assert c["cost"] == 1024 * (abs(x - gx) + abs(z - gz)) and c["next"] == (-1 if want_next is None else want_next[0] + 9 * want_next[1]), (x, z)
    assert (choices(flat[0], cells, 0.0, 0.0) == 2).sum() == 63 - 9 - 7 + 1   # off the goal's row and column two k explain the cost
    # ... and max_cost cuts by distance; a second goal record on the same span with a smaller cost wins; a dearer goal elsewhere loses where it is farther
    cut = twin.field(flat[0], [(gx + 9 * gz, 0)], 0.0, 0.0, 2048)
    assert (cut["cost"] != UNREACHED).sum() == 1 + 4 + 8 and cut["cost"].max() == UNREACHED and (cut["next"][cut["cost"] == UNREACHED] == -1).all()
    two = twin.field(flat[0], [(0, 9000), (0, 100), (8, 5000)], 0.0, 0.0)
    assert two["cost"][0] == 100 and two["next"][0] == -1 and two["cost"][1] == 1124 and two["cost"][8] == 5000 and two["next"][8] == -1
    assert two["cost"][6] == 100 + 6 * 1024 and two["next"][6] == 5    # 6244 by way of span 0, against 5000 + 2048
    assert two["cost"][7] == 5000 + 1024 and two["next"][7] == 8       # 6024 by way of span 8, against 100 + 7168
    # edge costs by hand: a step of 0.5 at climb 1 costs 1024 + 512; 0.5 + ulp too (truncation); 2.5 at climb 1024 saturates; down uses drop_cost
    ulp = f32(2.0 ** -22)
    assert twin.edge_cost(2.5, 3.0, 1.0, 9.0) == 1024 + 512 and twin.edge_cost(f32(2.5), f32(3.0) + ulp, 1.0, 9.0) == 1024 + 512
    assert twin.edge_cost(2.5, 5.0, 1024.0, 0.0) == 1024 + 2 ** 20 and twin.edge_cost(5.0, 2.5, 1024.0, 0.0) == 1024
    assert twin.edge_cost(3.0, 2.5, 9.0, 0.25) == 1024 + 128 and twin.edge_cost(2.5, 2.5, 1024.0, 1024.0) == 1024
    assert twin.edge_cost(2.5, 3.5, 1023.0, 0.0) == 1024 + 1023 * 1024 and twin.edge_cost(2.5, 3.5, 1024.0, 0.0) == 1024 + 2 ** 20   # just under, and at, 2^20
    for h1, climb, drop, up, down in ((3.0, 1.0, 0.25, 1536, 1152), (f32(3.0) + ulp, 1.0, 0.25, 1536, 1152), (5.0, 1024.0, 0.0, 1024 + 2 ** 20, 1024)):
        s = two_spans(2.5, h1)
        assert twin.edge_costs(s, climb, drop).tolist() == [[0, up, 0, 0], [down, 0, 0, 0]]
        climbing, dropping = twin.field(s, [(1, 0)], climb, drop), twin.field(s, [(0, 7)], climb, drop)
        assert climbing["cost"].tolist() == [up, 0] and climbing["next"].tolist() == [1, -1]
        assert dropping["cost"].tolist() == [7, 7 + down] and dropping["next"].tolist() == [-1, 0]
    # the one-directional link E of crafted_field(): the floor under the slab of (32, 3) links to the span of (33, 3), which answers the slab's top
    far = nav.twin_of("crafted", "far", 1, 2.5)
    under, beside = span_at(far, 32, 3, 2.5), span_at(far, 33, 3, 5.0)
    assert far[0]["link"][under][1] == beside and far[0]["link"][beside][0] == under + 1
    there, back = twin.field(far[0], [(beside, 0)], 0.0, 0.0), twin.field(far[0], [(under, 0)], 0.0, 0.0)
    assert there["cost"][under] == 1024 and there["next"][under] == beside
    assert back["cost"][beside] == 3 * 1024 and back["next"][beside] not in (under, under + 1)   # round by a neighbour row, three steps
    # locate and trace on the flat floor: column by rounding, span by |e|; a path is the nexts in order
    got = twin.locate(flat, (10.0, 20.0, 30.0), 2.0, [(10.0 + 2.0 * 3, 20.0 + 2.0 * 2.75, 30.0 + 2.0 * 4), (10.0 + 2.0 * 3.5, 25.0, 38.0), (10.0 + 2.0 * 3.49, 25.0, 38.0),
                                                     (10.0 - 2.0, 25.0, 38.0), (16.0, 26.1, 38.0), (np.nan, 25.0, 38.0), (16.0, 25.0, np.inf)], 0.25, 0.25)
    assert got.tolist() == [3 + 9 * 4, 4 + 9 * 4, 3 + 9 * 4, -1, -1, -1, -1]
    paths, lengths = twin.trace(cells, [0, gx + 9 * gz, -1], 5)
    assert lengths.tolist() == [5, 1, 0] and paths.tolist() == [[0, 1, 2, 3, 3 + 9], [gx + 9 * gz, -1, -1, -1, -1], [-1] * 5]
    assert twin.trace(cut, [0], 5)[1].tolist() == [0] and twin.trace(cells, [0], 16)[1].tolist() == [8]


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted_want(field, box, navp, costs, max_cost):
    """The twin's cells of a crafted configuration, and the spans and goals they stand on."""
    result = nav.twin_of(field, box, *navp)
    goals = crafted_goals(result, turned=field == "turned")
    cells = twin.field(result[0], goals, *costs, max_cost)
    cells.setflags(write=False)
    return result, goals, cells


@pytest.fixture(scope="module")
def crafted_results():
    out = {}
    with nav.terrain(nav.crafted_field()) as ex:
        for box in ("far", "interior"):
            for navp in NAV_PARAMS:
                got = ex.terrain_nav(*nav.BOXES[box], nav.raw_params(*navp))
                goals = crafted_goals(got)
                for costs in COSTS:
                    for max_cost in (NO_CUT, CUT):
                        out[box, navp, costs, max_cost] = (ex.nav_field(goals, raw_field_params(*costs, max_cost)), ex.navfield_info())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("box", ["far", "interior"])
@pytest.mark.parametrize("navp", NAV_PARAMS)
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("max_cost", [NO_CUT, CUT])
def test_gpu_crafted_field_equals_the_twin(crafted_results, box, navp, costs, max_cost):
    (spans, offsets, first, ext), goals, want = crafted_want("crafted", box, navp, costs, max_cost)
    assert len(spans) == (2548 if (box, navp[0]) == ("far", 1) else len(spans))
    reached = want["cost"] != UNREACHED
    # the inputs are not vacuous: reached and unreached spans, the NaN-height span among the latter, a choice between two k, and a cut that cuts
    assert reached.any() and not reached.all()
    nan = np.isnan(spans["height"])
    assert nan.sum() == 1 and not reached[nan].any()
    assert (choices(spans, want, *costs) >= 2).any()
    whole = crafted_want("crafted", box, navp, costs, NO_CUT)[2]
    if max_cost == CUT:
        assert reached.sum() < (whole["cost"] != UNREACHED).sum() and np.array_equal(want["cost"][reached], whole["cost"][reached])
    got, (n, n_reached, rounds) = crafted_results[box, navp, costs, max_cost]
    assert (n, n_reached) == (len(spans), int(reached.sum())) and 1 <= rounds <= n + 1
    assert same_cells(got, want), np.nonzero((got["cost"] != want["cost"]) | (got["next"] != want["next"]))[0][:10]


@pytest.mark.gpu
def test_gpu_turned_field_equals_the_twin():
    """The same field with x and z exchanged: every feature's neighbour lies along z, and a row of the floor is 34 columns, not 74."""
    dims = (DIMS[2], DIMS[1], DIMS[0])
    (spans, _, _, _), goals, want = crafted_want("turned", "far", (1, 2.5), (1.0, 0.25), NO_CUT)
    with nav.terrain(nav.turned_field(), dims) as ex:
        got = ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 2.5))
        assert crafted_goals(got, turned=True) == goals
        assert same_cells(ex.nav_field(goals, vt.NavFieldParams(1.0, 0.25)), want)


@functools.lru_cache(maxsize=None)
def serpentine_field():
    """The flat floor cut into corridors along x by walls on every odd z row, each with one gap at alternating ends: one long way."""
    g = np.full(tuple(d + 2 for d in DIMS), nav.AIR, f32)
    g[:, 0:3, :] = nav.SOLID
    for z in range(1, DIMS[2] + 2, 2):
        g[:, :, z] = nav.SOLID
        gap = DIMS[0] + 1 if z % 4 == 1 else 0
        g[gap, 3:, z] = nav.AIR
    g.setflags(write=False)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("turned", [False, True])
def test_gpu_serpentine_converges_in_few_rounds(turned):
    """One way of more than a thousand hops.  A design that settles a run of 256 or more spans per launch needs L / 256 rounds and change;
    one hop per launch would need L.  The bound, rounds * 4 <= L, is a condition on the design, not a measurement."""
    g = serpentine_field()
    dims = DIMS
    if turned:
        g, dims = np.ascontiguousarray(g.transpose(2, 1, 0)), (DIMS[2], DIMS[1], DIMS[0])
    shape = tuple(d + 2 for d in dims)
    want_nav = nav_twin.build(g, (0, 0, 0), shape, 1, 0.5)
    assert len(want_nav[0]) == 17 * 74 + 17 and want_nav[1][1] == 1   # 17 corridors and 17 gaps; column (0, 0) holds the goal, span 0
    want = twin.field(want_nav[0], [(0, 0)], 0.0, 1.0)
    assert (want["cost"] != UNREACHED).all()
    L = int(want["cost"].max()) // UNIT
    assert L > 1000 and L == 17 * 73 + 2 * 16 + 1   # 17 corridors, two hops through each of the 16 walls between them, and the last gap: a dead end
    with nav.terrain(g, dims) as ex:
        got_nav = ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 0.5))
        nav.assert_same(got_nav, want_nav, "serpentine")
        got = ex.nav_field([0], vt.NavFieldParams(0.0, 1.0))
        n, n_reached, rounds = ex.navfield_info()
    print("serpentine%s: %d hops in %d rounds" % (" turned" if turned else "", L, rounds))
    assert same_cells(got, want) and n_reached == n == len(want)
    assert rounds * 4 <= L


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["whole", "b"])
def test_gpu_random_field_equals_the_twin(name):
    """The noise-over-a-plane world of test_terrain_nav.random_world: three goals of distinct costs in its largest region."""
    w, e, h = DIMS
    with nav.terrain() as ex:
        plane = vt.PlaneModifier(ORIGIN[1] + 8 * SCALE, (-1e6, -1e6), (1e6, 1e6))
        noise = vt.NoiseModifier(7, 3, 0.11, 2.0, 0.5, "fbm", amplitude=2.5, ramp_scale=0.0, lower=(-1e6,) * 3, upper=(1e6,) * 3)
        ex.terrain_update([plane, noise])
        spans = ex.terrain_nav(*nav.RANDOM_BOXES[name], nav.raw_params(2, 1.0))[0]
        region, regions = largest_region(spans)
        inside = np.nonzero(spans["region"] == region)[0]
        goals = [(int(inside[0]), 300), (int(inside[len(inside) // 2]), 0), (int(inside[-1]), 12345)]
        got = ex.nav_field(goals, vt.NavFieldParams(2.5, 0.5))
        n, n_reached, rounds = ex.navfield_info()
    want = twin.field(spans, goals, 2.5, 0.5)
    reached = want["cost"] != UNREACHED
    print("%s: %d spans, %d regions, %d reached, %d rounds" % (name, n, len(regions), n_reached, rounds))
    assert len(regions) >= 2 and any(not reached[spans["region"] == r].any() for r in regions)   # a region nobody can leave for a goal
    assert reached[spans["region"] == region].any() and n_reached == reached.sum()
    assert same_cells(got, want)


@pytest.mark.gpu
def test_gpu_locate():
    """Dyadic coordinates, so every float32 step of the rule is exact and the cases are what they say."""
    box = "interior"
    navr = nav.twin_of("crafted", box, 1, 2.5)
    spans, offsets, first, ext = navr
    assert first == (5, 1, 3) and ext == (67, 13, 23)
    u = 2.0 ** -20   # one ulp of a grid coordinate in [8, 16), where the x and z cases lie
    groups = {}
    # column centres of the whole box, a margin of one column outside each face included, at the flat floor's height
    groups["centres"] = ([(x, 2.5, z) for z in range(first[2] - 1, first[2] + ext[2] + 1) for x in range(first[0] - 1, first[0] + ext[0] + 1)], 0.25, 0.25)
    # exactly at i + 0.5 (the upper column's) and the next world coordinate under it (one ulp of the grid coordinate, or two), in x and in z,
    # inside the box and at its four faces
    groups["halves"] = ([(10.5, 2.5, 12.0), (10.5 - u, 2.5, 12.0), (10.0, 2.5, 12.5), (10.0, 2.5, 12.5 - 2 * u), (4.5, 2.5, 12.0), (4.5 - u / 2, 2.5, 12.0),
                         (71.5, 2.5, 12.0), (71.5 - 8 * u, 2.5, 12.0), (10.0, 2.5, 2.5), (10.0, 2.5, 2.5 - u / 2), (10.0, 2.5, 25.5), (10.0, 2.5, 25.5 - 2 * u)], 0.25, 0.25)
    # the stacked column C (20, 3): floors at 2.5, 7.5 and 12.5; the midpoint of two goes to the lower, one ulp over it to the upper
    groups["stacked"] = ([(20.0, gy, 3.0) for gy in (2.5, 7.5, 12.5, 5.0, 5.0 - 2.0 ** -21, 5.0 + 2.0 ** -21, 10.0, 10.0 + 2.0 ** -20, 10.0 - 2.0 ** -20, 0.0, 15.0)], 2.5, 2.5)
    # below and above exactly met, and one ulp short (of the limit, with e = 1 exactly)
    edge = [(9.0, 3.5, 12.0), (9.0, 1.5, 12.0)]
    groups["met"] = (edge, 1.0, 1.0)
    groups["above short"] = (edge, 1.0, 1.0 - 2.0 ** -24)
    groups["below short"] = (edge, 1.0 - 2.0 ** -24, 1.0)
    groups["zero"] = ([(9.0, 2.5, 12.0), (9.0, 2.5 + 2.0 ** -21, 12.0)], 0.0, 0.0)
    # an empty column (70, 3) is solid to the top; the NaN-height span of (20, 16) is never the answer
    groups["empty"] = ([(70.0, 2.5, 3.0), (70.0, 14.0, 3.0), (20.0, 2.5, 16.0), (20.0, 3.0, 16.0)], 8.0, 8.0)
    floor_at = lambda x, z: span_at(navr, x, z, 2.5)
    hand = {"halves": [floor_at(11, 12), floor_at(10, 12), floor_at(10, 13), floor_at(10, 12), floor_at(5, 12), -1, -1, floor_at(71, 12), floor_at(10, 3), -1, -1,
                       floor_at(10, 25)],
            "stacked": [span_at(navr, 20, 3, h) for h in (2.5, 7.5, 12.5, 2.5, 2.5, 7.5, 7.5, 12.5, 7.5, 2.5, 12.5)],
            "met": [floor_at(9, 12)] * 2, "above short": [-1, floor_at(9, 12)], "below short": [floor_at(9, 12), -1], "zero": [floor_at(9, 12), -1],
            "empty": [-1, -1, -1, -1]}
    with nav.terrain(nav.crafted_field()) as ex:
        nav.assert_same(ex.terrain_nav(*nav.BOXES[box], nav.raw_params(1, 2.5)), navr, box)
        for name, (points, below, above) in groups.items():
            want = twin.locate(navr, ORIGIN, SCALE, world(points), below, above)
            if name in hand:
                assert want.tolist() == hand[name], name
            got = ex.nav_locate(world(points), below * SCALE, above * SCALE)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
        centres = twin.locate(navr, ORIGIN, SCALE, world(groups["centres"][0]), 0.25, 0.25).reshape(ext[2] + 2, ext[0] + 2)
        assert (centres[0] == -1).all() and (centres[-1] == -1).all() and (centres[:, 0] == -1).all() and (centres[:, -1] == -1).all()
        assert (centres[1:-1, 1:-1] >= 0).sum() > 1400   # the floor lies open in nearly every column
        # coordinates that are no numbers, or none a grid has
        bad = np.array([(np.nan, 2.25, 8.0), (1.0, np.nan, 8.0), (1.0, 2.25, np.nan), (np.inf, 2.25, 8.0), (1.0, -np.inf, 8.0), (1.0, 2.25, np.inf),
                        (3e38, 2.25, 8.0), (-3e38, 2.25, -3e38), (1.0, 3e38, 8.0), (1.0, 2.25, 8.0)], f32)
        want = twin.locate(navr, ORIGIN, SCALE, bad, 0.25, 0.25)
        assert (want[:-1] == -1).all() and want[-1] == floor_at(8, 12)
        assert np.array_equal(ex.nav_locate(bad, 0.25 * SCALE, 0.25 * SCALE), want)
        assert len(ex.nav_locate(np.zeros((0, 3), f32), 1.0, 1.0)) == 0   # n == 0: a success


@pytest.mark.gpu
def test_gpu_trace(crafted_results):
    """From every span of the first crafted configuration, and from -1: whole paths, then rows cut at 3."""
    key = ("far", NAV_PARAMS[0], COSTS[0], NO_CUT)
    (spans, offsets, first, ext), goals, want = crafted_want("crafted", *key)
    n = len(spans)
    starts = np.concatenate([[-1], np.arange(n), [-1]]).astype(np.int32)
    assert (want["cost"][starts[1:-1]] == UNREACHED).any()
    with nav.terrain(nav.crafted_field()) as ex:
        L, h = ex._L, ex._h
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        kept = ex.nav_field(goals, raw_field_params(*COSTS[0]))
        assert same_cells(kept, want)
        for max_len in (4096, 3):
            paths, lengths = ex.nav_trace(starts, max_len)
            want_paths, want_lengths = twin.trace(want, starts, max_len)
            assert paths.dtype == lengths.dtype == np.int32 and np.array_equal(lengths, want_lengths) and np.array_equal(paths, want_paths), max_len
        assert (want_lengths == 3).any() and (want_lengths == 0).sum() > 2 and (want_lengths == 1).sum() == 3   # cut rows, misses and unreached starts, the goals
        # a start beyond the spans refuses the whole call and keeps the field
        for bad in (n, -2, 2 ** 31 - 1):
            s, p, l = np.array([0, bad, 1], np.int32), np.full((3, 4), 7, np.int32), np.full(3, 7, np.int32)
            assert L.vtmc_navfield_trace(h, s.ctypes.data, 3, 4, p.ctypes.data, l.ctypes.data) == _lib.ERR_INVALID_ARG and "navfield_trace" in L.vtmc_last_error(h).decode()
            assert (p == 7).all() and (l == 7).all() and same_cells(ex.navfield_read(), kept)
        paths, lengths = ex.nav_trace(starts, 4096)
    # every whole path ends on a goal, and its edge costs and the goal's add up to the start's cost
    cost, goal = twin.edge_costs(spans, *COSTS[0]), dict(goals)
    link = spans["link"]
    walked = 0
    for row, length, start in zip(paths, lengths, starts):
        if length == 0:
            assert (row == -1).all() and (start < 0 or want["cost"][start] == UNREACHED)
            continue
        assert length < 4096 and row[0] == start and (row[length:] == -1).all() and int(row[length - 1]) in goal
        total = goal[int(row[length - 1])]
        for a, b in zip(row[:length - 1], row[1:length]):
            (k,) = np.nonzero(link[a] == b)[0][:1]
            total += int(cost[a][k])
        assert total == want["cost"][start], start
        walked += 1
    assert walked == (want["cost"] != UNREACHED).sum()


@pytest.mark.gpu
def test_gpu_large_field_equals_dijkstra():
    """The 256^3 noise terrain of test_terrain_nav's large test, some 80 000 spans in 20 runs of the relaxation: the cells equal the twin's Dijkstra and are the
    same from build to build; a thousand agents are located and traced."""
    n = 256
    rng = np.random.default_rng(20260101)
    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(n + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        navr = ex.terrain_nav(everything["lower"], everything["upper"], nav.raw_params(4, 1.0, 1 << 24))
        spans, offsets, first, ext = navr
        total = len(spans)
        assert total > 50000
        region, _ = largest_region(spans)
        inside = np.nonzero(spans["region"] == region)[0]
        goals = [(int(inside[len(inside) * k // 5]), 1000 * (k - 1)) for k in (1, 2, 3, 4)]
        builds = [ex.nav_field(goals, vt.NavFieldParams(1.0, 0.0)) for _ in range(3)]
        _, n_reached, rounds = ex.navfield_info()
        # agents: near a span, up to 0.45 of a column off its centre and up to 1.5 above or below its floor
        pick = rng.integers(0, total, 1000)
        col = np.searchsorted(offsets, pick, side="right") - 1
        agents = np.stack([first[0] + col % ext[0] + rng.uniform(-0.45, 0.45, 1000), spans["height"][pick] + rng.uniform(-1.5, 1.5, 1000),
                           first[2] + col // ext[0] + rng.uniform(-0.45, 0.45, 1000)], axis=1).astype(f32)
        located = ex.nav_locate(agents, 1.0, 1.25)
        paths, lengths = ex.nav_trace(located, 512)
    print("%d spans, %d reached, %d rounds" % (total, n_reached, rounds))
    want = twin.field(spans, goals, 1.0, 0.0)
    assert same_cells(builds[0], want) and n_reached == (want["cost"] != UNREACHED).sum() > 10000
    assert same_cells(builds[1], builds[0]) and same_cells(builds[2], builds[0])
    want_located = twin.locate(navr, (0.0, 0.0, 0.0), 1.0, agents, 1.0, 1.25)
    assert (want_located >= 0).sum() > 500 and (want_located < 0).any() and np.array_equal(located, want_located)
    want_paths, want_lengths = twin.trace(want, want_located, 512)
    assert np.array_equal(lengths, want_lengths) and np.array_equal(paths, want_paths) and want_lengths.max() > 50


@pytest.mark.gpu
def test_gpu_life_cycle_and_errors(tmp_path):
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        pos, out, n = np.zeros((2, 3), f32), np.zeros(8, np.int32), ctypes.c_int32(7)
        goal = np.zeros(1, vt.NAVFIELD_GOAL_DTYPE)

        def build(goals=goal, count=None, p=raw_field_params(), reached=n):
            return L.vtmc_navfield_build(h, goals.ctypes.data if goals is not None else None, len(goals) if count is None else count,
                                         ctypes.byref(p) if p is not None else None, ctypes.byref(reached) if reached is not None else None)

        def no_field():
            no_result(ex.navfield_read), no_result(ex.device_navfield), no_result(ex.navfield_info), no_result(lambda: ex.nav_trace([0], 4))
            assert L.vtmc_navfield_read(h, out.ctypes.data, 8) == _lib.ERR_NO_RESULT and L.vtmc_navfield_trace(h, None, 0, 1, None, None) == _lib.ERR_NO_RESULT

        def no_nav():
            assert build() == _lib.ERR_NO_RESULT and n.value == 0 and "terrain_nav_build" in L.vtmc_last_error(h).decode()
            assert L.vtmc_nav_locate(h, pos.ctypes.data, 2, 1.0, 1.0, out.ctypes.data) == _lib.ERR_NO_RESULT
            no_field()
        no_nav()                                                                                        # no terrain
        ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
        ex.terrain_set_history(16 << 20)
        no_nav()                                                                                        # a terrain, no nav result
        ex.terrain_write_samples(nav.crafted_field())
        key = ("far", NAV_PARAMS[0], COSTS[1], NO_CUT)
        navr, goals, want = crafted_want("crafted", *key)
        total = len(want)
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        no_field()                                                                                      # a nav result, no field
        assert len(ex.nav_locate(pos, 1.0, 1.0)) == 2
        kept = ex.nav_field(goals, raw_field_params(*COSTS[1]))
        assert same_cells(kept, want)
        # every INVALID_ARG keeps the previous field byte for byte
        nan, inf = float("nan"), float("inf")
        bad_params = [raw_field_params(c, 0.0) for c in (nan, inf, -inf, -1.0, 1024.5)] + [raw_field_params(0.0, d) for d in (nan, inf, -0.5, 1025.0)] + \
            [raw_field_params(1.0, 1.0, 0), raw_field_params(1.0, 1.0, 0x80000000), raw_field_params(1.0, 1.0, 0xffffffff), raw_field_params(1.0, 1.0, NO_CUT, 1)]

        def goal_of(span, cost=0):
            g = np.zeros(2, vt.NAVFIELD_GOAL_DTYPE)
            g["span"], g["cost"] = (0, span), (0, cost)
            return g
        calls = [lambda p=p: build(p=p) for p in bad_params] + [
            lambda: build(goals=None, count=1), lambda: build(p=None), lambda: build(count=0), lambda: build(count=-1), lambda: build(count=_lib.NAVFIELD_MAX_GOALS + 1),
            lambda: build(goals=goal_of(-1)), lambda: build(goals=goal_of(total)), lambda: build(goals=goal_of(2 ** 31 - 1)),
            lambda: build(goals=goal_of(5, 5001), p=raw_field_params(1.0, 1.0, 5000)), lambda: build(goals=goal_of(5, 0x80000000))]
        for i, call in enumerate(calls):
            n.value = 7
            assert call() == _lib.ERR_INVALID_ARG and n.value == 0 and "navfield_build" in L.vtmc_last_error(h).decode(), i
            assert same_cells(ex.navfield_read(), kept), i
        locates = [(pos.ctypes.data, -1, 1.0, 1.0, out.ctypes.data), (None, 2, 1.0, 1.0, out.ctypes.data), (pos.ctypes.data, 2, 1.0, 1.0, None),
                   (pos.ctypes.data, 2, nan, 1.0, out.ctypes.data), (pos.ctypes.data, 2, 1.0, inf, out.ctypes.data), (pos.ctypes.data, 2, -0.5, 1.0, out.ctypes.data),
                   (pos.ctypes.data, 2, 1.0, -1.0, out.ctypes.data)]
        for i, args in enumerate(locates):
            assert L.vtmc_nav_locate(h, *args) == _lib.ERR_INVALID_ARG and "nav_locate" in L.vtmc_last_error(h).decode(), i
        traces = [(out.ctypes.data, -1, 4, out.ctypes.data, out.ctypes.data), (out.ctypes.data, 1, 0, out.ctypes.data, out.ctypes.data),
                  (None, 1, 4, out.ctypes.data, out.ctypes.data), (out.ctypes.data, 1, 4, None, out.ctypes.data), (out.ctypes.data, 1, 4, out.ctypes.data, None)]
        for i, args in enumerate(traces):
            assert L.vtmc_navfield_trace(h, *args) == _lib.ERR_INVALID_ARG and "navfield_trace" in L.vtmc_last_error(h).decode(), i
        assert same_cells(ex.navfield_read(), kept)
        assert L.vtmc_nav_locate(h, None, 0, 1.0, 1.0, None) == _lib.OK and L.vtmc_navfield_trace(h, None, 0, 1, None, None) == _lib.OK   # nothing to do
        records = np.zeros(len(goals), vt.NAVFIELD_GOAL_DTYPE)
        records["span"], records["cost"] = zip(*goals)
        assert build(goals=records, p=raw_field_params(*COSTS[1]), reached=None) == _lib.OK            # n_reached may be null
        assert same_cells(ex.navfield_read(), kept) and ex.navfield_info()[:2] == (total, int((want["cost"] != UNREACHED).sum()))
        # CAPACITY on a short read; the device pointer's contents equal the read's
        buf = np.zeros(total, vt.NAVFIELD_CELL_DTYPE)
        assert L.vtmc_navfield_read(h, buf.ctypes.data, total - 1) == _lib.ERR_CAPACITY and str(total) in L.vtmc_last_error(h).decode()
        assert L.vtmc_navfield_read(h, None, total) == _lib.ERR_INVALID_ARG and L.vtmc_navfield_read(h, buf.ctypes.data, total) == _lib.OK and same_cells(buf, kept)
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        p, count = ex.device_navfield()
        d_cells = np.zeros(total, vt.NAVFIELD_CELL_DTYPE)
        assert count == total and p and hip.hipMemcpy(d_cells.ctypes.data, p, d_cells.nbytes, 2) == 0 and d_cells.tobytes() == buf.tobytes()
        # an edit does not drop the field, nor the spans: both are snapshots; nor does the undo
        spans_before = ex.nav_read()
        ex.terrain_update([vt.SphereModifier(nav.world_of((40, 3, 16)), 2.5, False)])
        assert same_cells(ex.navfield_read(), kept) and nav_twin.nan_aware_equal(ex.nav_read()[0], spans_before[0])
        assert ex.terrain_undo()[0] > 0
        assert same_cells(ex.navfield_read(), kept) and nav_twin.nan_aware_equal(ex.nav_read()[0], spans_before[0])
        # the next nav build drops it, also one that fails after it has invalidated the nav result
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        no_field()
        ex.nav_field(goals, raw_field_params())
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 2.5, total - 1))
        assert e.value.code == _lib.ERR_TOO_LARGE
        no_nav()
        # a nav build refused for its arguments keeps both
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        ex.nav_field(goals, raw_field_params(*COSTS[1]))
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(0, 2.5))
        assert e.value.code == _lib.ERR_INVALID_ARG and same_cells(ex.navfield_read(), kept)
        # a field over an empty nav result has no span to put a goal on
        ex.terrain_nav(*nav.BOXES["outside"], nav.raw_params())
        assert build() == _lib.ERR_INVALID_ARG and (ex.nav_locate(pos, 1.0, 1.0) == -1).all()
        no_field()
        # terrain_load and terrain_init drop it
        path = tmp_path / "t.vtt"
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        ex.nav_field(goals, raw_field_params())
        ex.terrain_save(path)
        ex.terrain_load(path, extract=False)
        no_nav()
        ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(*NAV_PARAMS[0]))
        ex.nav_field(goals, raw_field_params())
        ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
        no_nav()


@pytest.mark.gpu
def test_gpu_nothing_else_moves():
    """Everything else the context holds, and the nav result itself, byte for byte before and after build, locate, trace and read."""
    with nav.terrain() as ex:
        L, h = ex._L, ex._h
        ex.terrain_set_history(16 << 20)
        ex.terrain_update([vt.PlaneModifier(ORIGIN[1] + 6 * SCALE, (-1e6, -1e6), (1e6, 1e6))])
        ex.terrain_update([vt.SphereModifier(nav.world_of((20, 6, 16)), 2.0, False)])
        ex.material_init(1)
        ex.material_vertices(), ex.ao_vertices(vt.AmbientOcclusion(2.0)), ex.scatter_surface(vt.ScatterParams(1.0, seed=3))
        navr = ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(2, 1.0))

        def everything():
            spans, offsets, first, ext = ex.nav_read()
            return nav.held(ex, L, h) + [spans.tobytes(), offsets.tobytes(), first, ext, ex.device_nav()]
        before = everything()
        cells = ex.nav_field([(0, 0), (len(navr[0]) - 1, 77)], vt.NavFieldParams(1.0, 1.0))
        assert everything() == before
        assert same_cells(cells, twin.field(navr[0], [(0, 0), (len(navr[0]) - 1, 77)], 1.0, 1.0))
        pts = world([(3.0, 6.5, 4.0), (40.0, 6.0, 20.0), (20.0, 4.0, 16.0), (-5.0, 6.0, 4.0)])
        located = ex.nav_locate(pts, 1.0, 1.0)
        assert np.array_equal(located, twin.locate(navr, ORIGIN, SCALE, pts, 2.0, 2.0)) and (located >= 0).any()
        assert everything() == before
        paths, lengths = ex.nav_trace(located, 256)
        assert lengths.max() > 1 and everything() == before
        assert same_cells(ex.navfield_read(), cells) and ex.device_navfield()[1] == len(cells) and everything() == before


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's LocateOnNav, BuildNavField and TracePaths against the Python path on the same world
    (host/host_selftest.cpp --gpu-navfield)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-navfield", tmp_path)
    cells = np.fromfile(tmp_path / "navfield_cells.bin", vt.NAVFIELD_CELL_DTYPE)
    paths, lengths = np.fromfile(tmp_path / "navfield_paths.i32", np.int32), np.fromfile(tmp_path / "navfield_lengths.i32", np.int32)
    located = np.fromfile(tmp_path / "navfield_located.i32", np.int32)
    with vt.Extractor(0) as ex:
        spans = nav.mirror_world(ex)[0]
        at = ex.nav_locate([(0.0, 6.3, 4.0), (12.0, 6.3, 15.0), (500.0, 6.3, 4.0)], 1.0, 1.0)
        want = ex.nav_field([(at[0], 0), (at[1], 3000)], vt.NavFieldParams(2.0, 0.5))
        want_paths, want_lengths = ex.nav_trace(list(range(len(spans))) + [-1], 64)
    assert len(spans) > 100 and np.array_equal(located, at) and at[0] >= 0 and at[1] >= 0 and at[2] == -1
    assert same_cells(cells, want) and np.array_equal(lengths, want_lengths) and np.array_equal(paths.reshape(-1, 64), want_paths) and want_lengths.max() > 3
