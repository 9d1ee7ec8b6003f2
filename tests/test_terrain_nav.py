"""The navigation layer: walkable spans, links and regions of a box of the resident terrain (vtmc_terrain_nav_build, include/vtmc_nav.h).

The rule (NAVIGATION in include/vtmc_nav.h) is one float32 operation per step and integers otherwise, so the device is compared with
nav_twin.py for EQUALITY: spans as raw bytes, column_offsets as int32.  There is no tolerance anywhere except in the mesh check.  Fields
are placed with terrain_write_samples, so every bit is chosen.  The fields, boxes and helpers are nav_support.py's; the contract every
layer's header keeps is tests/test_abi_layers.py's."""
import ctypes

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import nav_twin as twin
from host_check import run_host_check
from nav_support import (BOXES, DIMS, ORIGIN, RANDOM_BOXES, SCALE, SEED, assert_same, box_of, column, crafted_field, f32, held, mirror_world, raw_params, terrain,
                         turned_field, twin_of, world_of)
from terrain_twin import bits, no_result, sample_range

OPEN = _lib.NAV_OPEN
AGENT_HEIGHTS, MAX_STEPS = (1, 3), (0.0, 0.5, 1.0, 2.5)


# -- CPU: the header, the mirror, the host half ---------------------------------------------------------------------------------------------
def test_header_declares_the_layer():
    N = _header.LAYERS["nav"]
    assert N.constants == {"VTMC_NAV_OPEN": 0x7fffffff, "VTMC_NAV_MAX_AGENT_HEIGHT": 256} and _lib.NAV_OPEN == 2 ** 31 - 1
    assert list(N.prototypes) == ["vtmc_terrain_nav_build", "vtmc_nav_read", "vtmc_nav_info", "vtmc_nav_device_results"] == _lib.LAYER_SYMBOLS["nav"]
    assert set(N.structs) == {"vtmc_nav_params", "vtmc_nav_span"}
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    assert N.prototypes["vtmc_terrain_nav_build"].argtypes == [VP] * 5 and N.prototypes["vtmc_nav_read"].argtypes == [VP, VP, I32, VP]
    assert ctypes.sizeof(_lib.NavParamsStruct) == 16 and _lib.NavParamsStruct.flags.offset == 12
    d = vt.NAV_SPAN_DTYPE
    assert d.itemsize == 32 and d.names == ("height", "y", "clearance", "link", "region")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 28] and d["link"].shape == (4,)
    rule = open(N.path).read()
    for word in ("NAVIGATION", "Floor", "Clearance", "Span", "Link", "Region", "no agent-radius erosion", "no slope test by normal"):
        assert word in rule, word


def test_library_exports_the_entry_points_and_refuses_null():
    L = vt.load()
    assert hasattr(L, "vtmc_debug_nav_ms")
    lo, up, p, n = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), raw_params(), ctypes.c_int32()
    assert L.vtmc_terrain_nav_build(None, ctypes.byref(lo), ctypes.byref(up), ctypes.byref(p), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_read(None, None, 0, None) == _lib.ERR_INVALID_ARG and L.vtmc_nav_info(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_device_results(None, None, None, None) == _lib.ERR_INVALID_ARG


def test_nav_params_take_world_units():
    p = vt.NavParams(1.7, 0.4, max_spans=500).to_struct(0.5)
    assert (p.agent_height, p.max_spans, p.flags) == (4, 500, 0) and f32(p.max_step) == f32(0.4) / f32(0.5)
    assert vt.NavParams(2.0, 0.0).to_struct(0.5).agent_height == 4 and vt.NavParams(2.0, 0.0).to_struct(0.5).max_step == 0.0
    assert vt.NavParams(1e-3, 1.0).to_struct(1.0).agent_height == 1
    for bad in (dict(agent_height=0.0, max_step=1.0), dict(agent_height=np.nan, max_step=1.0), dict(agent_height=1.0, max_step=-1.0),
                dict(agent_height=1.0, max_step=np.inf), dict(agent_height=1.0, max_step=1.0, max_spans=0),
                dict(agent_height=1.0, max_step=1.0, max_spans=2 ** 31)):
        with pytest.raises(ValueError):
            vt.NavParams(**bad)


def test_world_positions():
    spans = np.zeros(3, vt.NAV_SPAN_DTYPE)
    spans["height"] = (2.5, 7.5, 3.0)
    offsets = np.array([0, 2, 2, 2, 3], np.int32)   # a 2 x 2 box of columns at (5, 3): column 0 holds two spans, column 3 one
    w = vt.nav_world_positions(spans, offsets, (5, 1, 3), (2, 13, 2), ORIGIN, SCALE)
    assert np.array_equal(w, [[-3.0 + 5 * 0.5, 1.0 + 2.5 * 0.5, 2.0 + 3 * 0.5], [-0.5, 1.0 + 7.5 * 0.5, 3.5], [-3.0 + 6 * 0.5, 2.5, 2.0 + 4 * 0.5]])


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/nav_host_check.cpp: the host half (csrc/terrain_nav.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("nav_host_check", tmp_path)


# -- CPU: the twin against answers stated by hand ---------------------------------------------------------------------------------------------
def test_twin_reproduces_hand_stated_answers():
    """Pins the twin to answers worked out on paper from crafted_field(), so that it is not pinned to itself alone."""
    columns = 74 * 34
    # One span per column on the flat floor, then per feature: B the roofs' tops (+1 at x = 12, 13, 14; at 15 the roof sits on the floor),
    # C +2, D +1 in each of the three two-span columns, E +1, F +1 twice, G the platform's 4 x 3 and the bridge's 8 columns over the floor,
    # H the column solid to the top -1, I the NaN above the floor -1 and three roofs +3.
    total = columns + 3 + 2 + 3 + 1 + 2 + (12 + 8) - 1 - 1 + 3
    assert total == 2548
    far = twin_of("crafted", "far", 1, 2.5)
    assert len(far[0]) == total == far[1][-1] and far[2] == (0, 0, 0) and far[3] == (74, 18, 34)
    # agent_height 3 loses the cave floors under 2 and 1 open samples and the ledge under 1
    assert len(twin_of("crafted", "far", 3, 2.5)[0]) == total - 3

    def triples(result, x, z):
        s = column(result, x, z)[0]
        return [(float(h), int(y), int(c)) for h, y, c in zip(s["height"], s["y"], s["clearance"])]
    assert triples(far, 20, 3) == [(2.5, 2, 3), (7.5, 7, 3), (12.5, 12, OPEN)]                 # C
    assert triples(far, 12, 3) == [(2.5, 2, 3), (8.5, 8, OPEN)] and triples(far, 15, 3) == [(8.5, 8, OPEN)]   # B
    assert triples(far, 14, 3) == [(2.5, 2, 1), (8.5, 8, OPEN)]
    assert triples(twin_of("crafted", "far", 3, 2.5), 13, 3) == [(8.5, 8, OPEN)]
    assert triples(far, 6, 3) == [(4.0 + 2.0 ** -21, 4, OPEN)]                                  # A
    assert triples(far, 70, 3) == [] and triples(far, 70, 6) == [(13.5, 13, OPEN)]              # H
    assert triples(far, 10, 16) == [] and triples(far, 11, 16) == [(3.0, 2, OPEN)] == triples(far, 12, 16)   # I
    assert triples(far, 13, 16) == [(2.5, 2, 4), (7.5, 7, OPEN)] == triples(far, 14, 16) == triples(far, 15, 16)
    s, i = column(far, 20, 16)                                                                   # J
    assert len(s) == 1 and np.isnan(s["height"][0]) and (s["link"] == -1).all() and s["region"][0] == i
    assert all(i not in column(far, x, z)[0]["link"] for x, z in ((19, 16), (21, 16), (20, 15), (20, 17)))
    # the interior box: its top plane is sample 13, so the column solid up to 13 has no floor, and the platform's floor is open at 3 samples
    inner = twin_of("crafted", "interior", 1, 2.5)
    assert inner[2] == (5, 1, 3) and inner[3] == (67, 13, 23) and triples(inner, 70, 6) == []
    assert triples(inner, 45, 4) == [(2.5, 2, 7), (10.5, 10, OPEN)]
    assert twin_of("crafted", "outside", 1, 2.5)[1].tolist() == [0] and twin_of("crafted", "outside", 1, 2.5)[3] == (0, 0, 0)

    # links.  A: the steps of exactly max_step link, the steps one ulp larger do not
    def link(result, x, z, j, k):
        return int(column(result, x, z)[0]["link"][j][k])
    for step, z, xs in ((0.5, 3, (3, 4, 5, 6)), (1.0, 6, (3, 4, 5)), (2.5, 9, (3, 4, 5))):
        r = twin_of("crafted", "far", 1, step)
        firsts = [column(r, x, z)[1] for x in xs]
        assert [link(r, x, z, 0, 1) for x in xs[:-1]] == firsts[1:-1] + [-1], step
        assert [link(r, x, z, 0, 0) for x in xs[1:]] == firsts[:-2] + [-1], step
    r0 = twin_of("crafted", "far", 1, 0.0)
    assert link(r0, 3, 12, 0, 1) == -1 and link(r0, 2, 12, 0, 1) == column(r0, 3, 12)[1] and link(r0, 4, 12, 0, 0) == -1
    # D: the tie goes to the lower span; otherwise the nearer one wins, under or over
    low = [column(far, 27, z)[1] for z in (3, 6, 9)]
    assert [link(far, 26, z, 0, 1) for z in (3, 6, 9)] == [low[0], low[1], low[2] + 1]
    assert link(twin_of("crafted", "far", 3, 2.5), 26, 3, 0, 1) == column(twin_of("crafted", "far", 3, 2.5), 27, 3)[1] + 1   # the lower one's opening is too low
    # E: one direction only
    under = column(far, 32, 3)[1]
    assert link(far, 32, 3, 0, 1) == column(far, 33, 3)[1] and link(far, 33, 3, 0, 0) == under + 1 and link(far, 32, 3, 1, 1) == column(far, 33, 3)[1]
    # F: |d| = 1 passes, the common opening does not
    r1 = twin_of("crafted", "far", 1, 1.0)   # at max_step 1: at 2.5 the ledge's neighbour reaches the top of the ledge's roof, 2 above it
    assert link(r1, 38, 3, 0, 1) == -1 and link(r1, 39, 3, 0, 0) == -1 and link(r1, 38, 3, 0, 0) == column(r1, 37, 3)[1]
    assert link(far, 39, 3, 0, 0) == column(far, 38, 3)[1] + 1
    r3 = twin_of("crafted", "far", 3, 2.5)
    assert link(r3, 38, 6, 0, 1) == -1 and link(r3, 39, 6, 0, 0) == -1 and link(far, 38, 6, 0, 1) == column(far, 39, 6)[1]

    # regions at max_step 0.5.  G: the platform is one region of its own; the plateaus are one region through the bridge, not the floor's
    r = twin_of("crafted", "far", 1, 0.5)

    def region(x, z, j=0):
        return int(column(r, x, z)[0]["region"][j])
    assert region(0, 0) == 0 == region(73, 33) == region(45, 4, 0) == region(58, 10, 0)
    platform = {region(x, z, 1) for x in range(44, 48) for z in range(3, 6)}
    assert platform == {column(r, 44, 3)[1] + 1}
    plateaus = {region(x, z) for x in (52, 53, 54, 63, 64, 65, 66) for z in range(8, 13)} | {region(x, 10, 1) for x in range(55, 63)}
    assert plateaus == {column(r, 52, 8)[1]}
    assert (r[0]["region"] <= np.arange(len(r[0]))).all() and (r[0]["region"][r[0]["region"]] == r[0]["region"]).all()


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted_results():
    out = {}
    with terrain(crafted_field()) as ex:
        for box in BOXES:
            for ah in AGENT_HEIGHTS:
                for step in MAX_STEPS:
                    out[box, ah, step] = ex.terrain_nav(*BOXES[box], raw_params(ah, step))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("agent_height", AGENT_HEIGHTS)
@pytest.mark.parametrize("max_step", MAX_STEPS)
def test_gpu_crafted_field_equals_the_twin(crafted_results, box, agent_height, max_step):
    want = twin_of("crafted", box, agent_height, max_step)
    if box == "far":
        assert np.isnan(want[0]["height"]).sum() == 1
    if box == "outside":
        assert len(want[0]) == 0
    assert_same(crafted_results[box, agent_height, max_step], want, (box, agent_height, max_step))


@pytest.mark.gpu
def test_gpu_turned_field_equals_the_twin():
    """The same field with x and z exchanged: 74 samples along z, and every feature's neighbour lies along z."""
    dims = (DIMS[2], DIMS[1], DIMS[0])
    with terrain(turned_field(), dims) as ex:
        for ah, step in ((1, 2.5), (3, 0.5)):
            assert_same(ex.terrain_nav(*BOXES["far"], raw_params(ah, step)), twin_of("turned", "far", ah, step), (ah, step))


@pytest.fixture(scope="module")
def random_world():
    """A seeded smooth field: the library's noise modifier over a plane at half height, read back for the twin; the full extract with it."""
    w, e, h = DIMS
    with terrain() as ex:
        plane = vt.PlaneModifier(ORIGIN[1] + 8 * SCALE, (-1e6, -1e6), (1e6, 1e6))
        noise = vt.NoiseModifier(7, 3, 0.11, 2.0, 0.5, "fbm", amplitude=2.5, ramp_scale=0.0, lower=(-1e6,) * 3, upper=(1e6,) * 3)
        n_dirty, T = ex.terrain_update([plane, noise])
        assert n_dirty == (w // 8) * (e // 8) * (h // 8) and T > 0
        grid = ex.terrain_read_samples()
        tris, dirty = ex.read_triangles(with_offsets=False), ex.terrain_dirty_blocks()
        results = {name: ex.terrain_nav(*b, raw_params(2, 1.0)) for name, b in RANDOM_BOXES.items()}
    return grid, tris, dirty, results


def sample_box(bounds):
    m = type("M", (), {"lower": [f32(v) for v in bounds[0]], "upper": [f32(v) for v in bounds[1]]})
    low, up, first, ext = sample_range(m, tuple(d + 2 for d in DIMS), SCALE, ORIGIN)
    return tuple(first), tuple(ext)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RANDOM_BOXES))
def test_gpu_random_field_equals_the_twin(random_world, name):
    grid, tris, dirty, results = random_world
    want = twin.build(grid, *sample_box(RANDOM_BOXES[name]), 2, 1.0)
    if name == "whole":
        counts = np.diff(want[1])
        print("%d spans, %d regions, up to %d spans in a column" % (len(want[0]), len(np.unique(want[0]["region"])), counts.max()))
        assert counts.max() >= 2 and len(np.unique(want[0]["region"])) >= 2 and (want[0]["link"] >= 0).any()   # the field is no plane
    assert_same(results[name], want, name)


@pytest.mark.gpu
def test_gpu_sub_box_is_consistent_with_the_whole(random_world):
    """Box "a" spans the full y range: its columns' floors equal the whole grid's, and so do the links of its interior columns once the
    span indices are mapped."""
    whole, sub = random_world[3]["whole"], random_world[3]["a"]
    (fx, fy, fz), (dx, dy, dz) = sub[2], sub[3]
    assert fy == 0 and dy == DIMS[1] + 2
    to_whole = np.full(len(sub[0]), -1, np.int64)
    for iz in range(dz):
        for ix in range(dx):
            s, i = column(sub, fx + ix, fz + iz)
            w, j = column(whole, fx + ix, fz + iz)
            assert len(s) == len(w)
            for f in ("height", "y", "clearance"):
                assert np.array_equal(bits(s[f]), bits(w[f])), (ix, iz, f)
            to_whole[i:i + len(s)] = np.arange(j, j + len(w))
    checked = 0
    for iz in range(1, dz - 1):
        for ix in range(1, dx - 1):
            s, i = column(sub, fx + ix, fz + iz)
            w, j = column(whole, fx + ix, fz + iz)
            mapped = np.where(s["link"] >= 0, to_whole[np.maximum(s["link"], 0)], -1)
            assert np.array_equal(mapped, w["link"]), (ix, iz)
            checked += len(s)
    assert checked > 500   # not vacuous: the field holds 1770 spans, the interior of box "a" about half of them


@pytest.mark.gpu
def test_gpu_spans_are_vertices_of_the_mesh(random_world):
    """Every span on a lattice edge that belongs to a cell is a vertex of the full extract: (x, height, z) within 1e-5 grid units, the
    project's position tolerance.  A vertex is 8 * block + block-local position; it is looked up by the lattice edge it rounds to."""
    grid, tris, dirty, results = random_world
    spans, offsets, first, ext = results["whole"]
    w, e, h = DIMS
    v = np.concatenate([tris[f].astype(np.float64) + 8.0 * dirty[tris["block"]] for f in ("p0", "p1", "p2")])
    on_y_edge = (v[:, 0] == np.round(v[:, 0])) & (v[:, 2] == np.round(v[:, 2]))
    v = v[on_y_edge]
    by_edge = {}
    for x, y, z in v:
        for cell in (np.floor(y), np.ceil(y) - 1):   # a vertex on a lattice corner belongs to the edge under it too
            by_edge.setdefault((int(x), int(cell), int(z)), []).append(y)
    col = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    xs, zs = first[0] + col % ext[0], first[2] + col // ext[0]
    keep = (xs <= w) & (zs <= h) & (spans["y"] + 1 <= e)
    assert keep.sum() > 500   # not vacuous: most of the field's 1770 spans lie on a cell's edge
    worst = 0.0
    for x, z, s in zip(xs[keep], zs[keep], spans[keep]):
        ys = by_edge.get((int(x), int(s["y"]), int(z)))
        assert ys, (x, z, s)
        worst = max(worst, min(abs(y - float(s["height"])) for y in ys))
    print("worst |vertex - span height| = %.3g grid units over %d spans" % (worst, keep.sum()))
    assert worst <= 1e-5


@pytest.mark.gpu
def test_gpu_nothing_else_moves_and_a_build_sees_the_edit():
    with terrain() as ex:
        L, h = ex._L, ex._h
        ex.terrain_set_history(16 << 20)
        ex.terrain_update([vt.PlaneModifier(ORIGIN[1] + 6 * SCALE, (-1e6, -1e6), (1e6, 1e6))])
        ex.terrain_update([vt.SphereModifier(world_of((20, 6, 16)), 2.0, False)])
        ex.material_init(1)
        ex.material_vertices(), ex.ao_vertices(vt.AmbientOcclusion(2.0)), ex.scatter_surface(vt.ScatterParams(1.0, seed=3))
        before = held(ex, L, h)
        first = ex.terrain_nav(*BOXES["far"], raw_params(2, 1.0))
        assert_same(first, twin.build(ex.terrain_read_samples(), (0, 0, 0), (74, 18, 34), 2, 1.0), "before the edit")
        assert held(ex, L, h) == before
        assert_same(ex.terrain_nav(*BOXES["interior"], vt.NavParams(2 * SCALE, 1.0 * SCALE)), twin.build(ex.terrain_read_samples(), *box_of("interior"), 2, 1.0), "world units")
        assert held(ex, L, h) == before
        # the result is a snapshot: an edit does not invalidate it; the next build sees the edit
        snapshot = ex.nav_read()
        ex.terrain_update([vt.SphereModifier(world_of((40, 6, 16)), 2.5, True)])
        again = ex.nav_read()
        assert twin.same_bytes(again[0], snapshot[0]) and np.array_equal(again[1], snapshot[1])
        second = ex.terrain_nav(*BOXES["far"], raw_params(2, 1.0))
        assert_same(second, twin.build(ex.terrain_read_samples(), (0, 0, 0), (74, 18, 34), 2, 1.0), "after the edit")
        assert not twin.same_bytes(second[0], first[0])
        assert ex.terrain_undo()[0] > 0
        assert_same(ex.terrain_nav(*BOXES["far"], raw_params(2, 1.0)), first, "after the undo")


@pytest.mark.gpu
def test_gpu_errors_and_limits(tmp_path):
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        lo, up = (ctypes.c_float * 3)(*BOXES["far"][0]), (ctypes.c_float * 3)(*BOXES["far"][1])
        n = ctypes.c_int32(7)

        def build(p, lower=lo, upper=up, count=n):
            return L.vtmc_terrain_nav_build(h, ctypes.byref(lower) if lower is not None else None, ctypes.byref(upper) if upper is not None else None,
                                            ctypes.byref(p) if p is not None else None, ctypes.byref(count) if count is not None else None)

        def nothing_held():
            no_result(ex.nav_read)
            no_result(ex.device_nav)
            assert L.vtmc_nav_info(h, None, None, None) == _lib.ERR_NO_RESULT and L.vtmc_nav_read(h, None, 0, None) == _lib.ERR_NO_RESULT
        assert build(raw_params()) == _lib.ERR_NO_RESULT and n.value == 0 and "terrain_init" in L.vtmc_last_error(h).decode()   # no terrain
        nothing_held()
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        nothing_held()                                                                                  # a terrain, no build
        ex.terrain_write_samples(crafted_field())
        want = twin_of("crafted", "far", 1, 0.5)
        kept = ex.terrain_nav(*BOXES["far"], raw_params(1, 0.5))
        assert_same(kept, want, "far")
        # every INVALID_ARG keeps the previous result
        nan_lo = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
        bad = [raw_params(0), raw_params(257), raw_params(-1), raw_params(1, -0.5), raw_params(1, float("nan")), raw_params(1, float("inf")),
               raw_params(1, 0.5, 0), raw_params(1, 0.5, -5), raw_params(1, 0.5, 1 << 20, 1)]
        calls = [lambda p=p: build(p) for p in bad] + [lambda: build(None), lambda: build(raw_params(), lower=None), lambda: build(raw_params(), upper=None),
                                                       lambda: build(raw_params(), lower=nan_lo), lambda: build(raw_params(), upper=nan_lo)]
        for i, call in enumerate(calls):
            n.value = 7
            assert call() == _lib.ERR_INVALID_ARG and n.value == 0, i
            assert "terrain_nav_build" in L.vtmc_last_error(h).decode()
            got = ex.nav_read()
            assert twin.nan_aware_equal(got[0], kept[0]) and np.array_equal(got[1], kept[1]) and got[2:] == kept[2:], i
        assert build(raw_params(), count=None) == _lib.OK                                               # n_spans may be null
        # terrain_load drops the result as terrain_init does
        path = tmp_path / "t.vtt"
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        nothing_held()
        ex.terrain_nav(*BOXES["interior"], raw_params())
        ex.terrain_save(path)
        ex.terrain_load(path, extract=False)
        nothing_held()


@pytest.mark.gpu
def test_gpu_limits_and_device_pointers():
    with terrain(crafted_field()) as ex:
        L, h = ex._L, ex._h
        want = twin_of("crafted", "far", 1, 0.5)
        total = len(want[0])
        got = ex.terrain_nav(*BOXES["far"], raw_params(1, 0.5, total))                                 # max_spans == the total: fits
        assert_same(got, want, "exact max_spans")
        # CAPACITY on a short read; a read of the exact size without the offsets
        buf = np.zeros(total, vt.NAV_SPAN_DTYPE)
        assert L.vtmc_nav_read(h, buf.ctypes.data, total - 1, None) == _lib.ERR_CAPACITY and str(total) in L.vtmc_last_error(h).decode()
        assert L.vtmc_nav_read(h, buf.ctypes.data, total, None) == _lib.OK and twin.nan_aware_equal(buf, want[0])
        lo3, d3, n = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32()
        assert L.vtmc_nav_info(h, ctypes.byref(lo3), ctypes.byref(d3), ctypes.byref(n)) == _lib.OK
        assert (tuple(lo3), tuple(d3), n.value) == ((0, 0, 0), (74, 18, 34), total)
        # the device pointers' contents equal vtmc_nav_read's
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        p, o, count = ex.device_nav()
        assert count == total and p and o
        d_spans, d_offs = np.zeros(total, vt.NAV_SPAN_DTYPE), np.zeros(74 * 34 + 1, np.int32)
        assert hip.hipMemcpy(d_spans.ctypes.data, p, d_spans.nbytes, 2) == 0 and hip.hipMemcpy(d_offs.ctypes.data, o, d_offs.nbytes, 2) == 0
        assert d_spans.tobytes() == buf.tobytes() and np.array_equal(d_offs, want[1])
        # TOO_LARGE carries the total and leaves no result
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_nav(*BOXES["far"], raw_params(1, 0.5, total - 1))
        assert e.value.code == _lib.ERR_TOO_LARGE and str(total) in str(e.value)
        no_result(ex.nav_read)
        no_result(ex.device_nav)
        assert L.vtmc_nav_info(h, None, None, None) == _lib.ERR_NO_RESULT
        # an empty box is a success with 0 spans, also after a failure
        got = ex.terrain_nav(*BOXES["outside"], raw_params())
        assert len(got[0]) == 0 and got[1].tolist() == [0] and got[3] == (0, 0, 0) and ex.device_nav()[2] == 0
        # terrain_init drops the result
        ex.terrain_nav(*BOXES["far"], raw_params())
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        no_result(ex.nav_read)
        assert len(ex.terrain_nav(*BOXES["far"], raw_params())[1]) == 74 * 34 + 1


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's BuildNav against the Python path on the same world (host/host_selftest.cpp --gpu-nav)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-nav", tmp_path)
    spans = np.fromfile(tmp_path / "nav_spans.bin", vt.NAV_SPAN_DTYPE)
    offsets, box = np.fromfile(tmp_path / "nav_offsets.i32", np.int32), np.fromfile(tmp_path / "nav_box.i32", np.int32)
    with vt.Extractor(0) as ex:
        want = mirror_world(ex)
    assert len(want[0]) > 100 and tuple(box[:3]) == want[2] and tuple(box[3:]) == want[3]
    assert twin.same_bytes(spans, want[0]) and np.array_equal(offsets, want[1])


@pytest.mark.gpu
def test_gpu_large_field_regions_are_the_components():
    """256^3 cells of the benchmark's terrain: 66 564 columns (65 groups of the scan) and some 80 000 spans, where the union pass runs under
    real contention.  The regions must be the components of the device's own links, and the same from build to build."""
    n = 256
    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(n + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        builds = [ex.terrain_nav(everything["lower"], everything["upper"], raw_params(4, 1.0, 1 << 24)) for _ in range(3)]
    spans, offsets, first, ext = builds[0]
    assert ext == (n + 2,) * 3 and len(offsets) == (n + 2) ** 2 + 1 and offsets[-1] == len(spans) > 50000
    assert (np.diff(offsets) >= 0).all() and np.diff(offsets).max() >= 2
    want = twin.regions(spans["link"])
    print("%d spans, %d regions" % (len(spans), len(np.unique(want))))
    assert np.array_equal(spans["region"], want)
    for other in builds[1:]:
        assert twin.same_bytes(other[0], spans) and np.array_equal(other[1], offsets)
