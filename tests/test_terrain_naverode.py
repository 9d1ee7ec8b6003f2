"""An agent radius on the navigation layer: border distance and span erosion (include/vtmc_naverode.h, csrc/terrain_naverode.hip).

The rule (NAVERODE in include/vtmc_naverode.h) is integers only, so the device is compared with naverode_twin.py for EQUALITY: distances
and origins as int32, spans as the nav tests compare them.  The twin holds the distance in two formulations (Jacobi rounds; settling over
the reversed steps) and is itself pinned to answers worked out by hand.  Fields, boxes and helpers are nav_support.py's; the contract every layer's header keeps is
tests/test_abi_layers.py's."""
import ctypes
import functools
import os

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import nav_twin
import navfield_twin
import naverode_twin as twin
from host_check import run_host_check
import nav_support as nav
from nav_support import flat_grid, nav_of, world
from terrain_twin import no_result

ROOT = nav.ROOT
f32 = np.float32
DIMS, SCALE, ORIGIN = nav.DIMS, nav.SCALE, nav.ORIGIN
OPEN_FACES = _lib.NAVERODE_OPEN_BOX_FACES
NAV_PARAMS = ((1, 2.5), (3, 0.5), (1, 0.5))   # (agent_height, max_step) of the nav builds under the erosion
RADII = (0, 1, 2, 3, 5)
GPU_RADII = (0, 1, 2, 5)


def raw(radius, flags=0, reserved=(0, 0)):
    return _lib.NavErodeParamsStruct(radius, flags, (ctypes.c_int32 * 2)(*reserved))


def by_column(nav_result, values):
    """values of a nav result with one span in every column, as [ix, iz]."""
    ext = nav_result[3]
    assert (np.diff(nav_result[1]) == 1).all()
    return np.asarray(values).reshape(ext[2], ext[0]).T


def assert_eroded(got, want, what):
    nav.assert_same(got[:4], want[:4], what)
    assert got[4].dtype == np.int32 and np.array_equal(got[4], want[4]), what


# -- CPU: the header, the binding, the documents, the host half -----------------------------------------------------------------------------
def test_header_declares_the_layer():
    E = _header.LAYERS["naverode"]
    assert E.constants == {"VTMC_NAVERODE_UNIT": 2, "VTMC_NAVERODE_MAX_RADIUS": 255, "VTMC_NAVERODE_OPEN_BOX_FACES": 1}
    assert (_lib.NAVERODE_UNIT, _lib.NAVERODE_MAX_RADIUS, _lib.NAVERODE_OPEN_BOX_FACES) == (2, 255, 1)
    assert list(E.prototypes) == ["vtmc_nav_distance_build", "vtmc_nav_distance_read", "vtmc_nav_distance_device_results", "vtmc_nav_erode",
                                  "vtmc_nav_erode_origin"] == _lib.LAYER_SYMBOLS["naverode"]
    assert set(E.structs) == {"vtmc_naverode_params"}
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    assert E.prototypes["vtmc_nav_distance_build"].argtypes == [VP, VP, VP] == E.prototypes["vtmc_nav_erode"].argtypes
    assert E.prototypes["vtmc_nav_distance_read"].argtypes == [VP, VP, I32] == E.prototypes["vtmc_nav_erode_origin"].argtypes
    assert E.prototypes["vtmc_nav_distance_device_results"].argtypes == [VP, VP, VP]
    S = _lib.NavErodeParamsStruct
    assert ctypes.sizeof(S) == 16 and (S.radius.offset, S.flags.offset, S.reserved.offset) == (0, 4, 8)
    rule = open(E.path).read()
    for word in ("NAVERODE", "Border", "Steps", "Distance", "Erosion", "radius - 1 Jacobi rounds", "origin[new] = old index"):
        assert word in rule, word
    # the layers under it point here
    for path in (_header.LAYERS["nav"].path, _header.LAYERS["navfield"].path):
        assert "vtmc_naverode.h" in open(path).read(), path


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert hasattr(L, "vtmc_debug_naverode_ms")
    p, n, out = raw(1), ctypes.c_int32(), (ctypes.c_int32 * 4)()
    assert L.vtmc_nav_distance_build(None, ctypes.byref(p), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_distance_read(None, ctypes.byref(out), 4) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_distance_device_results(None, None, ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_erode(None, ctypes.byref(p), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_nav_erode_origin(None, ctypes.byref(out), 4) == _lib.ERR_INVALID_ARG
    assert L.vtmc_debug_naverode_ms(None, None) == _lib.ERR_INVALID_ARG


def test_naverode_params_take_world_units():
    p = vt.NavErodeParams(0.6).to_struct(0.5)
    assert (p.radius, p.flags, tuple(p.reserved)) == (2, 0, (0, 0))
    assert vt.NavErodeParams(1.0, open_box_faces=True).to_struct(0.5).radius == 2 and vt.NavErodeParams(1.0, True).to_struct(0.5).flags == OPEN_FACES
    assert vt.NavErodeParams(0.0).to_struct(0.5).radius == 0 and vt.NavErodeParams(-0.0).to_struct(2.0).radius == 0
    assert vt.NavErodeParams(1e-3).to_struct(1.0).radius == 1 and vt.NavErodeParams(0.7).to_struct(0.1).radius == int(np.ceil(f32(0.7) / f32(0.1)))
    assert vt.NavErodeParams(1000.0).to_struct(0.5).radius == 2000   # beyond NAVERODE_MAX_RADIUS: the library's to refuse
    for bad in (np.nan, -1.0, -1e-30, np.inf, -np.inf):
        with pytest.raises(ValueError):
            vt.NavErodeParams(bad)


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/naverode_host_check.cpp: the host half (csrc/terrain_naverode.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("naverode_host_check", tmp_path)


def test_document_states_the_layer():
    text = open(os.path.join(ROOT, "NAVEROSION.md")).read()
    for word in ("VtmcNavErodeParams", "chamfer", "whole columns", "snapshot", "OPEN_BOX_FACES"):
        assert word in text, word


# -- CPU: the twin against answers stated by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dz", [(9, 7), (7, 12), (1, 5), (2, 2)])
def test_twin_flat_floor(dx, dz):
    """Shut faces: D = min(2 * min(ix, dx-1-ix, iz, dz-1-iz), 2 * radius).  Open faces: no border at all."""
    r = nav_of(flat_grid(dx, dz))
    assert len(r[0]) == dx * dz
    ix, iz = np.meshgrid(np.arange(dx), np.arange(dz), indexing="ij")
    to_face = np.minimum(np.minimum(ix, dx - 1 - ix), np.minimum(iz, dz - 1 - iz))
    for radius in RADII:
        D, rounds = twin.distance(r, radius)
        assert D.dtype == np.int32 and np.array_equal(by_column(r, D), np.minimum(2 * to_face, 2 * radius)), radius
        assert rounds <= max(radius - 1, 0) and np.array_equal(twin.distance_dijkstra(r, radius), D)
        assert twin.border(r).sum() == (to_face == 0).sum()
        assert not twin.border(r, OPEN_FACES).any() and (twin.distance(r, radius, OPEN_FACES)[0] == 2 * radius).all()
        kept = twin.erode(r, radius)
        assert np.array_equal(kept[4], np.nonzero((by_column(r, D) >= 2 * radius).T.reshape(-1))[0])
        assert len(twin.erode(r, radius, OPEN_FACES)[0]) == dx * dz


def test_twin_one_unlinkable_pillar():
    """A flat floor with open faces and one column whose floor stands 4 above it: at offsets (1,0), (1,1), (2,0), (2,1), (3,0), (2,2) from
    the pillar D is 0, 2, 2, 3, 4, 5, clamped to 2 * radius; the pillar's own top is a border."""
    g = flat_grid(13, 13, 10)
    g[6, 0:7, 6] = nav.SOLID
    r = nav_of(g)
    assert len(r[0]) == 169 and twin.border(r, OPEN_FACES).sum() == 5
    hand = {(1, 0): 0, (1, 1): 2, (2, 0): 2, (2, 1): 3, (3, 0): 4, (2, 2): 5}
    for radius in RADII:
        D = by_column(r, twin.distance(r, radius, OPEN_FACES)[0])
        assert D[6, 6] == 0
        for (a, b), d in hand.items():
            for ox, oz in ((a, b), (-a, b), (a, -b), (-a, -b), (b, a), (-b, a), (b, -a), (-b, -a)):   # the rule's eight symmetries
                assert D[6 + ox, 6 + oz] == min(d, 2 * radius), (radius, ox, oz)
        assert D[0, 0] == 2 * radius and np.array_equal(twin.distance_dijkstra(r, radius, OPEN_FACES), twin.distance(r, radius, OPEN_FACES)[0])


def test_twin_crafted_bridge():
    """crafted_field's G and J: radius 1 removes the one-column bridge, the two plateaus it joined become two regions, and the span with a NaN
    height goes."""
    r = nav.twin_of("crafted", "far", 1, 0.5)
    plateau = lambda x, z: nav.column(r, x, z)[1]       # the plateaus are solid from the bottom: one span per column
    bridge = lambda x: nav.column(r, x, 10)[1] + 1      # the bridge hangs over the flat floor
    assert r[0]["region"][plateau(53, 10)] == r[0]["region"][plateau(64, 10)] == r[0]["region"][bridge(58)]
    nan_span = nav.column(r, 20, 16)[1]
    assert np.isnan(r[0]["height"][nan_span]) and twin.border(r)[nan_span] and twin.border(r, OPEN_FACES)[nan_span]
    spans, offsets, first, ext, origin = twin.erode(r, 1)
    where = {int(o): i for i, o in enumerate(origin)}
    assert all(bridge(x) not in where for x in range(55, 63)) and nan_span not in where
    a, b = where[plateau(53, 10)], where[plateau(64, 10)]
    assert spans["region"][a] != spans["region"][b] and spans["region"][a] == where[plateau(53, 9)] and spans["link"][where[plateau(54, 10)]][1] == -1
    assert offsets[-1] == len(spans) == len(origin) and (np.diff(origin) > 0).all() and (first, ext) == (r[2], r[3])
    for f in ("height", "y", "clearance"):
        assert spans[f].tobytes() == r[0][f][origin].tobytes()


def test_twin_formulations_agree_and_the_turn_changes_nothing():
    for box in ("far", "interior"):
        for ah, step in NAV_PARAMS:
            for radius in RADII:
                for flags in (0, OPEN_FACES):
                    hist = []
                    for field in ("crafted", "turned"):
                        r = nav.twin_of(field, "far", ah, step) if box == "far" else turned_interior(field, ah, step)
                        D, rounds = twin.distance(r, radius, flags)
                        assert rounds <= max(radius - 1, 0), (field, box, ah, step, radius, flags)
                        assert np.array_equal(twin.distance_dijkstra(r, radius, flags), D), (field, box, ah, step, radius, flags)
                        hist.append(np.bincount(D, minlength=2 * radius + 1))
                    assert np.array_equal(hist[0], hist[1]), (box, ah, step, radius, flags)
    # the inputs are not vacuous: the interior box, shut faces, agent 1, step 2.5
    r = nav.twin_of("crafted", "interior", 1, 2.5)
    assert len(r[0]) == 1572 and twin.border(r).sum() == 289
    assert [len(twin.erode(r, radius)[0]) for radius in (1, 2, 3, 5)] == [1283, 989, 755, 367]
    assert twin.border(r, OPEN_FACES).sum() < 289


@functools.lru_cache(maxsize=None)
def turned_interior(field, agent_height, max_step):
    """The interior box of the crafted field, and the same box of the turned field: x and z of its bounds exchanged."""
    if field == "crafted":
        return nav.twin_of("crafted", "interior", agent_height, max_step)
    first, ext = nav.box_of("interior")
    return nav_twin.build(nav.turned_field(), first[::-1], ext[::-1], agent_height, max_step)


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
def distance_of(ex, p):
    """(distances, n_border) of a raw parameter struct on the nav result held."""
    n = ctypes.c_int32(-7)
    ex._check(ex._L.vtmc_nav_distance_build(ex._h, ctypes.byref(p), ctypes.byref(n)))
    return ex.nav_distance_read(), n.value


def run_cases(ex, boxes, params):
    out = {}
    for box in boxes:
        for ah, step in params:
            for radius in GPU_RADII:
                for flags in (0, OPEN_FACES):
                    before = ex.terrain_nav(*boxes[box], nav.raw_params(ah, step))
                    dist, n_border = distance_of(ex, raw(radius, flags))
                    out[box, ah, step, radius, flags] = (before, dist, n_border, ex.nav_erode(raw(radius, flags)))
    return out


@pytest.fixture(scope="module")
def crafted_results():
    with nav.terrain(nav.crafted_field()) as ex:
        return run_cases(ex, nav.BOXES, NAV_PARAMS[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(nav.BOXES))
@pytest.mark.parametrize("radius", GPU_RADII)
@pytest.mark.parametrize("flags", (0, OPEN_FACES))
def test_gpu_crafted_field_equals_the_twin(crafted_results, box, radius, flags):
    for ah, step in NAV_PARAMS[:2]:
        what = (box, ah, step, radius, flags)
        want_nav = nav.twin_of("crafted", box, ah, step)
        before, dist, n_border, eroded = crafted_results[what]
        nav.assert_same(before, want_nav, what)
        want_d = twin.distance(want_nav, radius, flags)[0]
        assert dist.dtype == np.int32 and np.array_equal(dist, want_d) and n_border == twin.border(want_nav, flags).sum(), what
        assert_eroded(eroded, twin.erode(want_nav, radius, flags), what)
        if radius == 0:
            nav.assert_same(eroded[:4], want_nav, what)
            assert np.array_equal(eroded[4], np.arange(len(want_nav[0])))
        if box == "outside":
            assert len(dist) == 0 and n_border == 0 and len(eroded[0]) == 0 and len(eroded[4]) == 0 and eroded[1].tolist() == [0]
        elif radius == 2 and flags == 0:
            assert 0 < len(eroded[0]) < len(want_nav[0]) and (want_d == 3).any()   # spans are removed, and a two-hop step decides somewhere


@pytest.mark.gpu
def test_gpu_turned_field_equals_the_twin():
    """The same field with x and z exchanged: 74 samples along z, and every feature's neighbour lies along z."""
    dims = (DIMS[2], DIMS[1], DIMS[0])
    with nav.terrain(nav.turned_field(), dims) as ex:
        for ah, step in NAV_PARAMS[:2]:
            want_nav = nav.twin_of("turned", "far", ah, step)
            for radius, flags in ((1, 0), (2, OPEN_FACES), (5, 0)):
                nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(ah, step)), want_nav, (ah, step))
                dist, n_border = distance_of(ex, raw(radius, flags))
                assert np.array_equal(dist, twin.distance(want_nav, radius, flags)[0]) and n_border == twin.border(want_nav, flags).sum()
                assert_eroded(ex.nav_erode(raw(radius, flags)), twin.erode(want_nav, radius, flags), (ah, step, radius, flags))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, OPEN_FACES))
def test_gpu_random_field_equals_the_twin(flags):
    """The seeded noise world of the nav tests: stacked floors, several regions, links that are not symmetric."""
    with nav.terrain() as ex:
        plane = vt.PlaneModifier(ORIGIN[1] + 8 * SCALE, (-1e6, -1e6), (1e6, 1e6))
        noise = vt.NoiseModifier(7, 3, 0.11, 2.0, 0.5, "fbm", amplitude=2.5, ramp_scale=0.0, lower=(-1e6,) * 3, upper=(1e6,) * 3)
        ex.terrain_update([plane, noise])
        for name, box in nav.RANDOM_BOXES.items():
            before = ex.terrain_nav(*box, nav.raw_params(2, 1.0))
            dist, n_border = distance_of(ex, raw(2, flags))
            assert np.array_equal(dist, twin.distance(before, 2, flags)[0]) and n_border == twin.border(before, flags).sum(), name
            want = twin.erode(before, 2, flags)
            assert 0 < len(want[0]) < len(before[0]) and 0 < n_border < len(before[0]), name
            assert_eroded(ex.nav_erode(raw(2, flags)), want, name)


@pytest.mark.gpu
def test_gpu_large_field_equals_the_twin():
    """256^3 cells of the nav tests' large world: 66 564 columns (65 groups of the scan) and some 80 000 spans, far more than one workgroup
    of anything; the relabelling runs under real contention.  Radius 3, three times over: the same bytes."""
    n = 256
    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(n + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        runs = []
        for _ in range(3):
            before = ex.terrain_nav(everything["lower"], everything["upper"], nav.raw_params(4, 1.0, 1 << 24))
            dist, n_border = distance_of(ex, raw(3))
            runs.append((before, dist, n_border, ex.nav_erode(raw(3))))
        ms = (ctypes.c_float * 5)()
        ex._check(ex._L.vtmc_debug_naverode_ms(ex._h, ms))
    before, dist, n_border, eroded = runs[0]
    assert len(before[0]) > 50000 and len(before[1]) == (n + 2) ** 2 + 1
    want_d, rounds = twin.distance(before, 3)
    print("%d spans, %d borders, %d kept in %d regions; twin rounds %d; device ms %s" % (len(before[0]), n_border, len(eroded[0]), len(np.unique(eroded[0]["region"])),
                                                                                          rounds, [round(v, 4) for v in ms]))
    assert np.array_equal(dist, want_d) and n_border == twin.border(before).sum() and np.array_equal(twin.distance_dijkstra(before, 3), want_d)
    assert ms[4] == 2.0 and all(np.isfinite(v) and v >= 0 for v in ms)
    assert_eroded(eroded, twin.erode(before, 3), "large")
    assert 0 < len(eroded[0]) < len(before[0]) and np.array_equal(eroded[0]["region"], nav_twin.regions(eroded[0]["link"]))
    for other in runs[1:]:
        assert nav_twin.same_bytes(other[0][0], before[0]) and np.array_equal(other[1], dist) and other[2] == n_border
        assert nav_twin.same_bytes(other[3][0], eroded[0]) and np.array_equal(other[3][1], eroded[1]) and np.array_equal(other[3][4], eroded[4])


@pytest.mark.gpu
def test_gpu_composition_and_the_layers_above():
    base = nav.twin_of("crafted", "far", 1, 2.5)
    field_params = vt.NavFieldParams(1.0, 0.25)
    with nav.terrain(nav.crafted_field()) as ex:
        L, h = ex._L, ex._h
        # erode by 1 and then by 2: the twin applied twice; origin refers to the first erosion's indices
        nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 2.5)), base, "far")
        once = twin.erode(base, 1)
        assert_eroded(ex.nav_erode(raw(1)), once, "once")
        twice = twin.erode(once[:4], 2)
        got = ex.nav_erode(raw(2))
        assert_eroded(got, twice, "twice")
        assert 0 < len(twice[0]) < len(once[0]) < len(base[0]) and got[4].max() < len(once[0]) and not np.array_equal(once[4][got[4]], got[4])
        assert np.array_equal(ex.nav_erode_origin(), twice[4])
        # a field and a distance built before the erode are gone afterwards
        nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 2.5)), base, "far")
        no_result(ex.nav_erode_origin)   # a nav build drops the origin
        radius = 2
        D = ex.nav_distance(raw(radius))
        assert np.array_equal(D, twin.distance(base, radius)[0])
        ex.nav_field([0], field_params)
        assert len(ex.navfield_read()) == len(base[0])
        eroded = ex.nav_erode(raw(radius))
        want = twin.erode(base, radius)
        assert_eroded(eroded, want, "radius 2")
        no_result(ex.navfield_read)
        no_result(ex.nav_distance_read)
        no_result(ex.device_nav_distance)
        assert L.vtmc_navfield_trace(h, None, 0, 4, None, None) == _lib.ERR_NO_RESULT
        # locate, field and trace on the eroded result equal their twin on the eroded spans
        spans, offsets, first, ext, origin = want
        points = [(x, 2.5, z) for z in range(0, 34, 3) for x in range(0, 74, 5)] + [(58.0, 8.5, 10.0), (53.0, 8.5, 10.0), (64.5, 8.5, 10.0), (20.0, 3.0, 16.0),
                                                                                      (0.0, 2.5, 0.0), (1.0, 2.5, 1.0), (2.0, 2.5, 2.0), (30.0, 2.5, 24.0)]
        want_at = navfield_twin.locate(want[:4], ORIGIN, SCALE, world(points), 1.0, 1.0)
        at = ex.nav_locate(world(points), 1.0 * SCALE, 1.0 * SCALE)
        assert np.array_equal(at, want_at)
        bridge, corner, inner, far = len(points) - 8, len(points) - 4, len(points) - 2, len(points) - 1
        assert at[bridge] == -1 and at[corner] == -1 and at[corner + 1] == -1 and at[inner] >= 0 and at[far] >= 0   # over a removed span: -1
        assert (navfield_twin.locate(base, ORIGIN, SCALE, world(points), 1.0, 1.0)[[bridge, corner, corner + 1]] >= 0).all()
        goals = [(int(at[inner]), 0), (int(at[far]), 500)]
        cells = ex.nav_field(goals, field_params)
        want_cells = navfield_twin.field(spans, goals, 1.0, 0.25)
        assert cells.tobytes() == want_cells.tobytes() and (want_cells["cost"] != _lib.NAVFIELD_UNREACHED).sum() > 1000
        starts = np.concatenate([at, np.arange(len(spans), dtype=np.int32)])
        paths, lengths = ex.nav_trace(starts, 256)
        want_paths, want_lengths = navfield_twin.trace(want_cells, starts, 256)
        assert np.array_equal(paths, want_paths) and np.array_equal(lengths, want_lengths) and lengths.max() > 30
        # no path comes nearer to a border than the radius: every span of every path, in the distances of the un-eroded result
        on_paths = paths[paths >= 0]
        assert len(on_paths) > 10000 and (D[origin[on_paths]] >= 2 * radius).all() and (D < 2 * radius).any()
        # a distance on the eroded result stands until the next nav build
        again = ex.nav_distance(raw(1))
        assert np.array_equal(again, twin.distance(want[:4], 1)[0]) and np.array_equal(ex.nav_erode_origin(), origin)
        ex.terrain_nav(*nav.BOXES["interior"], nav.raw_params(1, 2.5))
        no_result(ex.nav_distance_read)
        no_result(ex.nav_erode_origin)
        no_result(ex.navfield_read)


@pytest.mark.gpu
def test_gpu_nothing_else_moves_and_an_edit_changes_neither_result():
    with nav.terrain() as ex:
        L, h = ex._L, ex._h
        ex.terrain_set_history(16 << 20)
        ex.terrain_update([vt.PlaneModifier(ORIGIN[1] + 6 * SCALE, (-1e6, -1e6), (1e6, 1e6))])
        ex.terrain_update([vt.SphereModifier(nav.world_of((20, 6, 16)), 2.0, False)])
        ex.material_init(1)
        ex.material_vertices(), ex.ao_vertices(vt.AmbientOcclusion(2.0)), ex.scatter_surface(vt.ScatterParams(1.0, seed=3))
        before = nav.held(ex, L, h)
        built = ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(2, 1.0))
        D = ex.nav_distance(vt.NavErodeParams(3 * SCALE))   # world units: 3 columns
        assert np.array_equal(D, twin.distance(built, 3)[0]) and (D == 6).any() and (D == 0).any()
        assert nav.held(ex, L, h) == before
        again = ex.nav_read()
        assert nav_twin.same_bytes(again[0], built[0]) and np.array_equal(again[1], built[1])   # a distance build leaves the nav result
        eroded = ex.nav_erode(vt.NavErodeParams(2.4 * SCALE, open_box_faces=True))
        assert_eroded(eroded, twin.erode(built, 3, OPEN_FACES), "world units")
        assert 0 < len(eroded[0]) < len(built[0]) and nav.held(ex, L, h) == before
        # both are snapshots: a later edit changes neither
        D1 = ex.nav_distance(raw(1))
        ex.terrain_update([vt.SphereModifier(nav.world_of((40, 6, 16)), 2.5, True)])
        after = ex.nav_read()
        assert nav_twin.same_bytes(after[0], eroded[0]) and np.array_equal(after[1], eroded[1])
        assert np.array_equal(ex.nav_distance_read(), D1) and np.array_equal(ex.nav_erode_origin(), eroded[4])


@pytest.mark.gpu
def test_gpu_errors():
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        n, buf = ctypes.c_int32(7), np.full(4096, 7, np.int32)

        def calls(p=raw(1)):
            return [lambda: L.vtmc_nav_distance_build(h, ctypes.byref(p) if p is not None else None, ctypes.byref(n)),
                    lambda: L.vtmc_nav_erode(h, ctypes.byref(p) if p is not None else None, ctypes.byref(n))]
        readers = [lambda: L.vtmc_nav_distance_read(h, buf.ctypes.data, len(buf)), lambda: L.vtmc_nav_distance_device_results(h, None, ctypes.byref(n)),
                   lambda: L.vtmc_nav_erode_origin(h, buf.ctypes.data, len(buf))]
        # before a terrain, and with a terrain before a nav build: every call
        for stage in range(2):
            for call in calls() + readers + [lambda: L.vtmc_debug_naverode_ms(h, (ctypes.c_float * 5)())]:
                assert call() == _lib.ERR_NO_RESULT and L.vtmc_last_error(h).decode() != "", stage
            assert (buf == 7).all()
            if stage == 0:
                ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
                ex.terrain_write_samples(nav.crafted_field())
        want_nav = nav.twin_of("crafted", "far", 1, 0.5)
        nav.assert_same(ex.terrain_nav(*nav.BOXES["far"], nav.raw_params(1, 0.5)), want_nav, "far")
        # a nav result, neither a distance nor an origin yet
        for call in readers:
            assert call() == _lib.ERR_NO_RESULT
        assert ex.nav_distance(raw(2)).tobytes() == twin.distance(want_nav, 2)[0].tobytes()
        assert readers[2]() == _lib.ERR_NO_RESULT   # a distance build is no erode
        first = ex.nav_erode(raw(1))
        kept_d = ex.nav_distance(raw(2, OPEN_FACES))
        want_first = twin.erode(want_nav, 1)
        assert_eroded(first, want_first, "first")
        assert np.array_equal(kept_d, twin.distance(want_first[:4], 2, OPEN_FACES)[0])
        total = len(first[0])
        # every INVALID_ARG keeps the nav result, the distance and the origin
        bad = [raw(-1), raw(256), raw(2 ** 31 - 1), raw(-2 ** 31), raw(1, 2), raw(1, 3), raw(1, 0x80000000), raw(1, 0, (1, 0)), raw(1, 0, (0, -1)), None]
        for i, p in enumerate(bad):
            for j, call in enumerate(calls(p)):
                n.value = 7
                assert call() == _lib.ERR_INVALID_ARG and n.value == 0, (i, j)
                assert ("nav_erode" if j else "nav_distance_build") in L.vtmc_last_error(h).decode()
                got = ex.nav_read()
                assert nav_twin.nan_aware_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and got[2:] == first[2:4], (i, j)
                assert np.array_equal(ex.nav_distance_read(), kept_d) and np.array_equal(ex.nav_erode_origin(), first[4]), (i, j)
        # the counts may be null
        p = raw(0)
        assert L.vtmc_nav_distance_build(h, ctypes.byref(p), None) == _lib.OK and L.vtmc_nav_erode(h, ctypes.byref(p), None) == _lib.OK
        assert np.array_equal(ex.nav_erode_origin(), np.arange(total)) and ex.nav_read()[0].tobytes() == first[0].tobytes()
        kept_d = ex.nav_distance(raw(2))
        # CAPACITY on reads one too small; the exact size passes
        out = np.full(total, 7, np.int32)
        for read in (L.vtmc_nav_distance_read, L.vtmc_nav_erode_origin):
            out[:] = 7
            assert read(h, out.ctypes.data, total - 1) == _lib.ERR_CAPACITY and str(total) in L.vtmc_last_error(h).decode() and (out == 7).all()
            assert read(h, None, total) == _lib.ERR_INVALID_ARG
            assert read(h, out.ctypes.data, total) == _lib.OK
        assert np.array_equal(ex.nav_distance_read(), kept_d)
        # terrain_init drops all three
        ex.terrain_init(*DIMS, SCALE, ORIGIN, nav.SEED)
        for call in calls() + readers:
            assert call() == _lib.ERR_NO_RESULT


@pytest.mark.gpu
def test_gpu_device_pointers():
    """The device pointers' contents equal what the reads return; an erode moves the nav result's."""
    with nav.terrain(nav.crafted_field()) as ex:
        built = ex.terrain_nav(*nav.BOXES["interior"], nav.raw_params(1, 2.5))
        D = ex.nav_distance(raw(3))
        p, count = ex.device_nav_distance()
        assert p and count == len(built[0]) == len(D)
        assert np.array_equal(ex.copy_to_host(p, D.nbytes).view(np.int32), D)
        spans_before = ex.device_nav()[0]
        eroded = ex.nav_erode(raw(3))
        no_result(ex.device_nav_distance)
        d_spans, d_offsets, total = ex.device_nav()
        assert total == len(eroded[0]) == 755 and d_spans and d_spans != spans_before
        assert ex.copy_to_host(d_spans, eroded[0].nbytes).tobytes() == eroded[0].tobytes()
        assert np.array_equal(ex.copy_to_host(d_offsets, eroded[1].nbytes).view(np.int32), eroded[1])
        D = ex.nav_distance(raw(1, OPEN_FACES))
        p, count = ex.device_nav_distance()
        assert count == total and np.array_equal(ex.copy_to_host(p, D.nbytes).view(np.int32), D)


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's NavDistance and ErodeNav against the Python path on the same world (host/host_selftest.cpp
    --gpu-naverode)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-naverode", tmp_path)
    dist, origin = np.fromfile(tmp_path / "naverode_distance.i32", np.int32), np.fromfile(tmp_path / "naverode_origin.i32", np.int32)
    spans, offsets = np.fromfile(tmp_path / "naverode_spans.bin", vt.NAV_SPAN_DTYPE), np.fromfile(tmp_path / "naverode_offsets.i32", np.int32)
    with vt.Extractor(0) as ex:
        built = nav.mirror_world(ex)
        want_d = ex.nav_distance(vt.NavErodeParams(1.2))
        want = ex.nav_erode(vt.NavErodeParams(0.8, open_box_faces=True))
    assert len(built[0]) > 100 and 0 < len(want[0]) < len(built[0]) and (want_d > 0).any()
    assert np.array_equal(dist, want_d) and np.array_equal(origin, want[4])
    assert nav_twin.same_bytes(spans, want[0]) and np.array_equal(offsets, want[1])
