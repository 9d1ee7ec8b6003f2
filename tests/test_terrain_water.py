"""Standing water (include/vtmc_water.h, csrc/terrain_water.hip): vtmc_terrain_flood and the readers of its result against the twin
(water_twin.py), a numpy restatement of the rule WATER.  The rule is integers, 32-bit copies and a few single FP32 operations, so every
comparison here is for EQUALITY: records and volumes as raw bytes.  The crafted field, its boxes and its source sets are water_support.py's."""
import ctypes
import os

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib
import water_support as ws
import water_twin as twin
from host_check import run_host_check
from terrain_twin import bits, no_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# case, box -> (source_body, [(level, n_samples, n_surface, lo, hi, at a face, n_sources)], wet, (near, refused, values > 0, wet values == 0))
TABLE = {
    ("separate", "whole"): ([1, 0, 2, -1, -1, 0], [(7.5, 5662, 1377, (50, 3, 4), (134, 13, 38), 0, 2), (7.0, 3612, 629, (4, 7, 4), (40, 12, 36), 0, 1),
                                                   (3.5, 75, 25, (60, 3, 30), (64, 5, 34), 0, 1)], 9349, (7954, 1, 12298, 2122)),
    ("separate", "interior"): ([-1, 0, -1, -1, -1, -1], [(7.5, 4080, 1020, (50, 10, 4), (109, 13, 20), 1, 1)], 4080, (2874, 0, 4636, 1020)),
    ("spill", "whole"): ([0, 0, 1], [(8.75, 13969, 2033, (4, 3, 4), (134, 15, 38), 0, 2), (3.5, 75, 25, (60, 3, 30), (64, 5, 34), 0, 1)], 14044, (8776, 1, 20368, 25)),
    ("spill", "interior"): ([-1, 0, -1], [(8.75, 7670, 1234, (30, 8, 4), (109, 15, 20), 1, 1)], 7670, (4022, 0, 10270, 0)),
    ("sky", "whole"): ([0], [(13.5, 64403, 0, (0, 3, 0), (137, 25, 41), 1, 1)], 64403, (10336, 1, 68942, 5796)),
    ("sky", "interior"): ([-1], [], 0, (0, 0, 0, 0)),
}


# -- CPU: the header, the binding, the documents, the host half -----------------------------------------------------------------------------
def test_header_declares_the_layer():
    S = _header.LAYERS["water"]
    assert S.constants == {"VTMC_WATER_MAX_SOURCES": 4096, "VTMC_WATER_MAX_LEVELS": 8, "VTMC_WATER_AT_FACE": 1}
    assert (_lib.WATER_MAX_SOURCES, _lib.WATER_MAX_LEVELS, _lib.WATER_AT_FACE) == (4096, 8, 1)
    names = ["vtmc_terrain_flood", "vtmc_water_info", "vtmc_water_bodies", "vtmc_water_read", "vtmc_water_device_results", "vtmc_water_probe"]
    assert list(S.prototypes) == names == _lib.LAYER_SYMBOLS["water"]
    assert set(S.structs) == {"vtmc_water_source", "vtmc_water_body"}
    VP, I32, U32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64
    assert [S.prototypes[n].argtypes for n in names] == [[VP, VP, VP, VP, I32, U32, VP, VP], [VP] * 6, [VP, VP, I32], [VP, VP, VP, I64], [VP] * 4, [VP, VP, I32, VP, VP]]
    rule = open(S.path).read()
    for word in ("WATER: the rule", "Box", "Open", "Plane", "Source", "Flood", "JOINS", "nested or disjoint", "Body order", "NEAR", "diagonal contact only", "Probe",
                 "OUT OF SCOPE", "replaces the context's", "labelling did not converge"):
        assert word in rule, word
    assert '("water", "vtmc_water.h", "core", "WATER.md")' in open(os.path.join(ROOT, "volumetricterrain_amd", "build.py")).read()


def test_mirror_layouts():
    s, b = _lib.WATER_SOURCE_DTYPE, _lib.WATER_BODY_DTYPE
    assert s.itemsize == 16 and s.names == ("position", "level") and [s.fields[f][1] for f in s.names] == [0, 12] and s["position"].shape == (3,)
    assert b.itemsize == 64 and b.names == ("seed", "lo", "hi", "level", "n_samples", "n_surface", "flags", "n_sources", "reserved")
    assert [b.fields[f][1] for f in b.names] == [0, 12, 24, 36, 40, 44, 48, 52, 56] and b["level"] == np.dtype("<f4") and b["flags"] == np.dtype("<u4")
    assert vt.WATER_SOURCE_DTYPE is s and vt.WATER_BODY_DTYPE is b
    for method in ("terrain_flood", "water_info", "water_bodies", "water_read", "device_water", "water_probe", "water_extract", "water_world_positions"):
        assert callable(getattr(vt.Extractor, method)), method
    hpp = open(os.path.join(ROOT, "host", "voxel_terrain.hpp")).read()
    assert "Flood(" in hpp and "ProbeWater(" in hpp


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert hasattr(L, "vtmc_debug_water_ms")
    lo, up, src = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), twin.sources_of([(0, 0, 0, 1)])
    assert L.vtmc_terrain_flood(None, ctypes.byref(lo), ctypes.byref(up), src.ctypes.data, 1, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_water_info(None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_water_bodies(None, None, 0) == _lib.ERR_INVALID_ARG
    assert L.vtmc_water_read(None, None, None, 0) == _lib.ERR_INVALID_ARG
    assert L.vtmc_water_device_results(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_water_probe(None, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_debug_water_ms(None, None) == _lib.ERR_INVALID_ARG


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/water_host_check.cpp: the host half (csrc/terrain_water.h) as a stand-alone program under ASan and UBSan, on the CPU: the
    rejections by value, the level -> plane search against a scan over awkward scales and origins, the volume dims, the nearest sample."""
    run_host_check("water_host_check", tmp_path)


def test_documents_state_the_layer():
    text = open(os.path.join(ROOT, "WATER.md")).read()
    for word in ("VtmcWaterSource", "VtmcWaterBody", "dig", "flood", "extract", "probe", "What it costs", "Limits", "replaces the context's extract result", "snapshot"):
        assert word in text, word
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "WATER.md" in open(os.path.join(ROOT, doc)).read(), doc
    assert "include/vtmc_water.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "tile_label.h" in open(os.path.join(ROOT, "DESIGN.md")).read()


# -- CPU: the twin against the rule ---------------------------------------------------------------------------------------------------------
def test_twin_on_a_hand_written_case():
    """6^3 samples, scale 1, origin 0: rock with a basin x, z 1..4, y 1..3 under two planes of sky.  A source on the basin's floor at level 2
    wets planes 1 and 2 (32 samples, 16 of them under open dry samples); one above its level and one in rock are dry."""
    g = np.full((6, 6, 6), f32(0.5), f32)
    g[1:5, 1:4, 1:5] = f32(-0.5)
    g[:, 4:, :] = f32(-0.5)
    r = twin.flood(g, (0, 0, 0), (6, 6, 6), 1.0, (0.0, 0.0, 0.0), [(2, 1, 2, 2.0), (2, 3, 2, 2.0), (0, 2, 0, 2.0), (2.4, 1.4, 2.4, 2.0), (9, 1, 2, 2.0)])
    assert r.source_body.tolist() == [0, -1, -1, 0, -1] and len(r.bodies) == 1 and r.wet == 32 and r.vd == (10, 10, 10)
    b = r.bodies[0]
    assert (b["seed"].tolist(), b["lo"].tolist(), b["hi"].tolist()) == ([1, 1, 1], [1, 1, 1], [4, 2, 4])
    assert (float(b["level"]), int(b["n_samples"]), int(b["n_surface"]), int(b["flags"]), int(b["n_sources"]), b["reserved"].tolist()) == (2.0, 32, 16, 0, 2, [0, 0])
    assert (r.body[1:5, 1:3, 1:5] == 0).all() and (r.body >= 0).sum() == 32
    w = r.water
    assert (w[1:5, 1, 1:5] == 1).all() and (w[1:5, 2, 1:5] == 0).all() and (w[1:5, 3, 1:5] == -1).all()     # wet at depth 1, at the level; the open sample above
    assert (w[:6, 0, :6] == 1).all() and (w[0, 1, :6] == 1).all() and (w[0, 2, :6] == 0).all() and (w[0, 3, :6] == -1).all()   # one sample into the ground
    assert (w[6:] == -1).all() and (w[:, 4:] == -1).all() and int((w > 0).sum()) == 72 and twin.volume_counts(r) == (36 + 20 + 20 + 36, 0, 72, 16)
    # a lower level inside the higher body joins it; a lower level elsewhere makes its own body after it
    g2 = g.copy()
    g2[0, 1:4, 0] = f32(-0.5)                               # a shaft in the corner, cut off from the basin below plane 4
    r2 = twin.flood(g2, (0, 0, 0), (6, 6, 6), 1.0, (0.0, 0.0, 0.0), [(0, 1, 0, 1.0), (2, 1, 2, 2.0), (3, 1, 3, 1.0)])
    assert r2.source_body.tolist() == [1, 0, 0] and [int(b["n_samples"]) for b in r2.bodies] == [32, 1] and int(r2.bodies[0]["n_sources"]) == 2
    assert int(r2.bodies[1]["flags"]) == _lib.WATER_AT_FACE and int(r2.bodies[0]["flags"]) == 0
    empty = twin.flood(g, (0, 0, 0), (0, 6, 6), 1.0, (0.0, 0.0, 0.0), [(2, 1, 2, 2.0)])
    assert empty.source_body.tolist() == [-1] and empty.ext == (0, 0, 0) and empty.vd == (0, 0, 0) and len(empty.bodies) == 0


def test_twin_helpers():
    assert [twin.volume_dim(d) for d in (1, 2, 3, 10, 11, 138, 26, 42, 80, 20, 30, 1026)] == [10, 10, 10, 10, 18, 138, 26, 42, 82, 26, 34, 1026]
    assert [twin.nearest(p, -3.0, 0.5) for p in (-3.0, -2.75, -2.76, -3.26, 1e30, -1e30, np.nan)] == [0, 1, 0, -1, 2 ** 31 - 1, -2 ** 31, None]
    assert [twin.plane_of(h, 0.5, 1.0, 26) for h in (0.99, 1.0, 1.24, 1.5, 13.5, 99.0)] == [-1, 0, 0, 1, 25, 25]
    lv = twin.levels_of(twin.sources_of([(0, 0, 0, 1.0), (0, 0, 0, -0.0), (0, 0, 0, 7.0), (0, 0, 0, 0.0), (0, 0, 0, 1.0)]))
    assert [bits(v) for v in lv] == [bits(f32(7.0)), bits(f32(1.0)), bits(f32(0.0)), bits(f32(-0.0))]


@pytest.mark.parametrize("case,box", list(TABLE))
def test_twin_reproduces_the_table(case, box):
    source_body, bodies, wet, counts = TABLE[(case, box)]
    r = ws.twin_of(case, box)
    assert ws.figures(r) == (source_body, bodies, wet, counts)
    assert r.vd == tuple(twin.volume_dim(d) for d in ws.BOXES[box][1]) and r.water.shape == r.body.shape == r.vd
    if len(r.bodies):
        assert r.water.max() <= 1 and r.water.min() == -1 and (r.water[r.body >= 0] >= 0).all()


# -- GPU ------------------------------------------------------------------------------------------------------------------------------------
terrain, device_volumes = ws.terrain, ws.device_volumes


@pytest.fixture(scope="module")
def crafted_ex():
    with terrain(ws.crafted_field()) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("case,box", list(TABLE))
def test_gpu_flood_equals_the_twin(crafted_ex, case, box):
    """Every row of the table, bytes against the twin, through vtmc_water_read and through the device pointers."""
    ex, want = crafted_ex, ws.twin_of(case, box)
    source_body, n = ex.terrain_flood(twin.sources_of(ws.CASES[case]), *ws.bounds_of(box))
    ws.same_result(ex, want, source_body, n)
    water, body = device_volumes(ex)
    assert np.array_equal(body, want.body) and np.ascontiguousarray(water).tobytes() == np.ascontiguousarray(want.water).tobytes()
    ms = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert ex._L.vtmc_debug_water_ms(ex._h, ms) == _lib.OK and all(np.isfinite(v) and v >= 0 for v in ms)


@pytest.mark.gpu
def test_gpu_no_sources_and_the_empty_box(crafted_ex):
    ex = crafted_ex
    source_body, n = ex.terrain_flood(np.zeros(0, vt.WATER_SOURCE_DTYPE), *ws.bounds_of("interior"))
    want = twin.flood(ws.crafted_field(), *ws.BOXES["interior"], ws.SCALE, ws.ORIGIN, twin.sources_of([]))
    ws.same_result(ex, want, source_body, n)
    water, body = ex.water_read()
    assert n == 0 and len(source_body) == 0 and (water == -1).all() and (body == -1).all() and ex.water_extract() == 0
    source_body, n = ex.terrain_flood(twin.sources_of(ws.CASES["spill"]), (1000.0,) * 3, (1010.0,) * 3)
    assert source_body.tolist() == [-1, -1, -1] and n == 0
    lo, d, vd, nb, wet = ex.water_info()
    assert (d, vd, nb, wet) == ((0, 0, 0), (0, 0, 0), 0, 0) and len(ex.water_bodies()) == 0 and ex.device_water() == (None, None, (0, 0, 0))
    water, body = ex.water_read()
    assert water.size == 0 and body.size == 0 and ex.water_extract() == 0
    assert [a.tolist() for a in ex.water_probe([ws.world_of((20, 9, 10))])] == [[-1], [0.0]]


@pytest.mark.gpu
def test_gpu_life_cycle_and_refusals_keep_the_result(tmp_path):
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        lo_c, up_c = (ctypes.c_float * 3)(*ws.bounds_of("whole")[0]), (ctypes.c_float * 3)(*ws.bounds_of("whole")[1])
        good = twin.sources_of(ws.CASES["separate"])

        def flood(lower=lo_c, upper=up_c, src=good, n=None, flags=0):
            out, nb = np.full(4097, -7, np.int32), ctypes.c_int32(-7)
            count = n if n is not None else (len(src) if src is not None else 1)
            return L.vtmc_terrain_flood(h, lower and ctypes.byref(lower), upper and ctypes.byref(upper), src.ctypes.data if src is not None else None,
                                        count, flags, out.ctypes.data, ctypes.byref(nb))
        assert flood() == _lib.ERR_NO_RESULT and "terrain_init" in L.vtmc_last_error(h).decode()
        ex.terrain_init(*ws.DIMS, ws.SCALE, ws.ORIGIN, ws.SEED)
        ex.terrain_write_samples(ws.crafted_field())
        readers = (ex.water_info, ex.water_bodies, ex.water_read, ex.device_water, ex.water_extract, lambda: ex.water_probe([(0, 0, 0)]))
        for call in readers:
            no_result(call)
        want = ws.twin_of("separate", "whole")
        ws.same_result(ex, want, *ex.terrain_flood(good, *ws.bounds_of("whole")))

        def with_value(field, k, v, i=1):
            s = good.copy()
            if field == "level":
                s["level"][i] = v
            else:
                s["position"][i, k] = v
            return s
        nine = twin.sources_of([ws.source((20, 9, 10), ws.h(j)) for j in range(9)])
        eight = twin.sources_of([ws.source((20, 9, 10), ws.h(9 + j % 8)) for j in range(4096)])
        many = np.zeros(4097, vt.WATER_SOURCE_DTYPE)
        nan_lo = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
        bad = [lambda: flood(lower=None), lambda: flood(upper=None), lambda: flood(src=None), lambda: flood(lower=nan_lo), lambda: flood(upper=nan_lo),
               lambda: flood(flags=1), lambda: flood(flags=0x80000000), lambda: flood(n=-1), lambda: flood(src=many), lambda: flood(src=nine)] + \
            [lambda v=v, k=k: flood(src=with_value("position", k, v)) for v in (np.nan, np.inf, -np.inf) for k in range(3)] + \
            [lambda v=v: flood(src=with_value("level", 0, v, i=5)) for v in (np.nan, np.inf, -np.inf)]
        for i, call in enumerate(bad):
            assert call() == _lib.ERR_INVALID_ARG and "terrain_flood" in L.vtmc_last_error(h).decode(), i
            ws.same_result(ex, want, want.source_body, len(want.bodies))
        recs = np.zeros(3, vt.WATER_BODY_DTYPE)
        assert L.vtmc_water_bodies(h, recs.ctypes.data, 2) == _lib.ERR_CAPACITY and not recs.tobytes().strip(b"\0")
        assert L.vtmc_water_bodies(h, None, 3) == _lib.ERR_INVALID_ARG and L.vtmc_water_bodies(h, recs.ctypes.data, 3) == _lib.OK and recs.tobytes() == want.bodies.tobytes()
        vn = int(np.prod(want.vd))
        assert L.vtmc_water_read(h, None, None, vn - 1) == _lib.ERR_CAPACITY and L.vtmc_water_read(h, None, None, vn) == _lib.OK
        assert L.vtmc_water_info(h, None, None, None, None, None) == _lib.OK and L.vtmc_water_device_results(h, None, None, None) == _lib.OK
        assert L.vtmc_water_probe(h, None, 1, None, None) == _lib.ERR_INVALID_ARG and L.vtmc_water_probe(h, None, -1, None, None) == _lib.ERR_INVALID_ARG
        assert L.vtmc_water_probe(h, None, 0, None, None) == _lib.OK
        # the limits themselves pass: 4096 sources on 8 levels, all on one sample (one seed of the highest level, the others join)
        sb, n = ex.terrain_flood(eight, *ws.bounds_of("whole"))
        assert n == 1 and (sb == 0).all() and int(ex.water_bodies()[0]["n_sources"]) == 4096 and float(ex.water_bodies()[0]["level"]) == ws.h(16)
        # an edit keeps the result: it is a snapshot; save + load and init drop it
        ws.same_result(ex, want, *ex.terrain_flood(good, *ws.bounds_of("whole")))
        ex.terrain_update([vt.SphereModifier(ws.world_of((45, 12, 8)), 2.6, False)])
        ws.same_result(ex, want, want.source_body, len(want.bodies))
        path = str(tmp_path / "t.vtmt")
        ex.terrain_save(path)
        ex.terrain_load(path, extract=False)
        for call in readers:
            no_result(call)
        ex.terrain_flood(good, *ws.bounds_of("whole"))
        ex.terrain_init(*ws.DIMS, ws.SCALE, ws.ORIGIN, ws.SEED)
        for call in readers:
            no_result(call)


@pytest.mark.gpu
def test_gpu_flood_after_an_erode_through_the_rim():
    """A sphere eroded through the sill between the basins, below B's level: B now runs into A, whose source joins."""
    with terrain(ws.crafted_field()) as ex:
        src = twin.sources_of(ws.CASES["separate"])
        before = ex.terrain_flood(src, *ws.bounds_of("whole"))
        assert before[0].tolist() == [1, 0, 2, -1, -1, 0] and before[1] == 3
        ex.terrain_update([vt.SphereModifier(ws.world_of((45, 12, 8)), 2.6, False)])
        grid = ex.terrain_read_samples()
        want = twin.flood(grid, *ws.BOXES["whole"], ws.SCALE, ws.ORIGIN, src)
        ws.same_result(ex, want, *ex.terrain_flood(src, *ws.bounds_of("whole")))
        assert want.source_body.tolist() == [0, 0, 1, -1, -1, 0] and len(want.bodies) == 2 and int(want.bodies[0]["n_sources"]) == 3
        assert int(want.bodies[0]["n_samples"]) > 5662 + 3612 and want.bodies[0]["lo"].tolist()[0] == 4


@pytest.mark.gpu
def test_gpu_nothing_else_moves():
    """Everything else the context holds, byte for byte before and after floods: the grid, the history, the dirty list, the extract result,
    the materials, the occlusion, the scatter, the nav result, the field and the crowd."""
    import nav_support as nav
    with terrain(ws.crafted_field()) as ex:
        L, h = ex._L, ex._h
        ex.terrain_set_history(16 << 20)
        ex.terrain_update([vt.SphereModifier(ws.world_of((45, 12, 8)), 2.6, False)])
        ex.terrain_update([vt.SphereModifier(ws.world_of((90, 17, 12)), 2.0, True)])
        ex.material_init(1)
        ex.material_vertices(), ex.ao_vertices(vt.AmbientOcclusion(2.0)), ex.scatter_surface(vt.ScatterParams(1.0, seed=3))
        spans = ex.terrain_nav(None, None, nav.raw_params(2, 1.0))[0]
        ex.nav_field([0, len(spans) // 2], vt.NavFieldParams(2.0, 0.5))
        ex.navcrowd_spawn(list(range(0, len(spans), 3)), [700] * len(range(0, len(spans), 3)))
        ex.navcrowd_step(vt.NavCrowdParams(None, True), 3)

        def everything():
            s, offsets, first, ext = ex.nav_read()
            agents, occ = ex.navcrowd_read()
            return nav.held(ex, L, h) + [s.tobytes(), offsets.tobytes(), first, ext, ex.device_nav(), ex.navfield_read().tobytes(), ex.navfield_info(),
                                         ex.device_navfield(), agents.tobytes(), occ.tobytes(), ex.navcrowd_info(), ex.device_navcrowd()]
        before = everything()
        for case, box in (("separate", "whole"), ("spill", "interior"), ("sky", "whole")):
            _, n = ex.terrain_flood(twin.sources_of(ws.CASES[case]), *ws.bounds_of(box))
            assert n >= 1 and everything() == before
        ex.water_probe([ws.world_of((20, 9, 10))]), ex.water_read(), ex.water_bodies()
        assert everything() == before
        # the next edit draws what it would have drawn without the floods: the event counter stood still
        ex.terrain_update([vt.SphereModifier(ws.world_of((100, 12, 12)), 3.0, False)])
        after = bits(ex.terrain_read_samples())
    with terrain(ws.crafted_field()) as ex:
        ex.terrain_update([vt.SphereModifier(ws.world_of((45, 12, 8)), 2.6, False)])
        ex.terrain_update([vt.SphereModifier(ws.world_of((90, 17, 12)), 2.0, True)])
        ex.terrain_update([vt.SphereModifier(ws.world_of((100, 12, 12)), 3.0, False)])
        assert np.array_equal(bits(ex.terrain_read_samples()), after)


def random_case(seed):
    """A 64 x 16 x 64 random field, open with probability 0.33 -- just above the cubic lattice's site-percolation threshold, so components
    are long and cross many tiles --, and 32 sources on 8 levels on random open samples, a little off them."""
    rng = np.random.default_rng(seed)
    dims = (64, 16, 64)
    g = ws.random_field(rng, dims)
    levels = ws.h(rng.choice(np.arange(2, 18), 8, replace=False)) + rng.choice([0.0, 0.25, 0.125], 8)
    open_samples = np.argwhere(~(g > 0))
    samples = open_samples[rng.choice(len(open_samples), 32, replace=False)]       # on open samples: above its level, a source is dry all the same
    rows = [tuple(np.asarray(ws.world_of(tuple(int(v) for v in s))) + rng.uniform(-0.2, 0.2, 3)) + (float(levels[i % 8]),) for i, s in enumerate(samples)]
    return dims, g, twin.sources_of(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gpu_random_field_equals_the_twin(seed):
    dims, g, src = random_case(seed)
    shape = tuple(d + 2 for d in dims)
    with terrain(g, dims) as ex:
        for first, ext in (((0, 0, 0), shape), ((3, 1, 5), (60, 15, 58))):
            want = twin.flood(g, first, ext, ws.SCALE, ws.ORIGIN, src)
            lower, upper = ws.world_of(first), ws.world_of(tuple(first[k] + ext[k] - 1 for k in range(3)))
            ws.same_result(ex, want, *ex.terrain_flood(src, lower, upper))
            if first == (0, 0, 0):
                assert len(want.bodies) >= 4 and want.wet > 1000 and (want.source_body >= 0).sum() > len(want.bodies), (len(want.bodies), want.wet)   # some join


@pytest.mark.gpu
def test_gpu_probe_equals_the_twin(crafted_ex):
    ex, want = crafted_ex, ws.twin_of("spill", "interior")
    ex.terrain_flood(twin.sources_of(ws.CASES["spill"]), *ws.bounds_of("interior"))
    rng = np.random.default_rng(7)
    lo, hi = np.asarray(ws.world_of((-2, -2, -2))), np.asarray(ws.world_of((140, 28, 44)))
    p = rng.uniform(lo, hi, (4096, 3)).astype(f32)
    p[:1024] = rng.uniform(ws.world_of((45, 8, 2)), ws.world_of((112, 17, 22)), (1024, 3)).astype(f32)      # many of them in the water
    wx, wy, wz = ws.world_of((60, 12, 10))
    edge = [(wx + 0.25, wy, wz), (wx - 0.25, wy, wz), (wx, wy + 0.25, wz), (wx, wy - 0.25, wz), (wx, wy, wz + 0.25), (wx, 8.75, wz), (wx, 8.875, wz), (wx, 9.0, wz),
            ws.world_of((29, 12, 10)), ws.world_of((30, 12, 10)), (ws.world_of((30, 12, 10))[0] - 0.25, wy, wz), ws.world_of((109, 12, 10)), ws.world_of((110, 12, 10)),
            ws.world_of((20, 9, 10)), (1e30, wy, wz), (-1e30, wy, wz), (wx, 3e38, wz), (np.nan, wy, wz), (wx, np.nan, wz), (wx, wy, np.nan), (np.inf, wy, wz),
            (wx, -np.inf, wz), (wx, wy, np.inf)]
    p = np.concatenate([p, np.asarray(edge, f32)])
    body, depth = ex.water_probe(p)
    want_body, want_depth = twin.probe(want, p, ws.SCALE, ws.ORIGIN)
    assert body.dtype == np.int32 and depth.dtype == f32 and np.array_equal(body, want_body) and depth.tobytes() == want_depth.tobytes()
    assert (body >= 0).sum() > 300 and (body < 0).sum() > 1000 and body[4096:4096 + 5].tolist() == [0, 0, 0, 0, 0] and body[-9:].tolist() == [-1] * 9
    assert (depth[body < 0] == 0).all() and depth[4096] == f32(8.75) - f32(wy)
    only_body = np.full(3, -7, np.int32)
    assert ex._L.vtmc_water_probe(ex._h, p[4096:].ctypes.data, 3, only_body.ctypes.data, None) == _lib.OK and only_body.tolist() == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("case,box", [("spill", "interior"), ("spill", "whole")])
def test_gpu_extraction_of_the_water_volume(crafted_ex, case, box):
    """water_extract of the device volume against the CPU oracle's extract of the twin's volume; every vertex on a vertical lattice edge from
    a wet sample to an open one lies at its body's level; and water_world_positions puts it where the terrain's own lattice is."""
    import oracle
    from extract_checks import assert_tris_match
    ex, want = crafted_ex, ws.twin_of(case, box)
    ex.terrain_flood(twin.sources_of(ws.CASES[case]), *ws.bounds_of(box))
    T = ex.water_extract()
    got, offs = ex.read_triangles()
    want_tris, want_offs, _ = oracle.extract_grid(want.water, threads=4)
    assert T == len(want_tris) > 1000 and np.array_equal(offs, want_offs)
    assert_tris_match(got, want_tris)
    # the vertices on vertical lattice edges, in world space and back on the terrain's lattice
    p = np.concatenate([got[f] for f in ("p0", "p1", "p2")])
    block = np.concatenate([got["block"]] * 3)
    world = ex.water_world_positions(block, p)
    g = (world - np.asarray(ws.ORIGIN)) / ws.SCALE                      # grid units: exact for this origin and scale
    on_column = (g[:, 0] == np.round(g[:, 0])) & (g[:, 2] == np.round(g[:, 2])) & (g[:, 1] != np.round(g[:, 1]))
    gx, gz, gy = g[on_column, 0].astype(int), g[on_column, 2].astype(int), g[on_column, 1]
    j = np.floor(gy).astype(int)
    first, ext = want.first, want.ext
    assert (gx >= first[0]).all() and (gx < first[0] + ext[0]).all() and (j >= first[1]).all() and (j + 1 < first[1] + ext[1]).all()
    below, above = want.body[gx - first[0], j - first[1], gz - first[2]], want.body[gx - first[0], j + 1 - first[1], gz - first[2]]
    open_above = ~(ws.crafted_field()[gx, j + 1, gz] > 0)
    surface = (below >= 0) & (above < 0) & open_above
    assert surface.sum() > 1000, surface.sum()
    level_in_grid_units = (want.bodies["level"][below[surface]].astype(np.float64) - ws.ORIGIN[1]) / ws.SCALE
    assert np.abs(gy[surface] - level_in_grid_units).max() <= 1e-5
    assert np.abs(world[on_column][surface][:, 1] - want.bodies["level"][below[surface]]).max() <= 1e-5 * ws.SCALE
    # an extract of the terrain itself replaces the water's result, and the flood is still there
    ex.extract_grid(np.ascontiguousarray(ws.crafted_field()[:10, :10, :10]))
    assert ex.last_counts()[0] == 1 and ex.water_info()[3] == len(want.bodies)


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's Flood and ProbeWater against the Python path on the same world (host/host_selftest.cpp --gpu-water)."""
    from test_host_mirror import run_host_mirror
    run_host_mirror("--gpu-water", tmp_path)
    import nav_support as nav
    with vt.Extractor(0) as ex:
        nav.mirror_world(ex)
        src = twin.sources_of([(5.0, 5.0, 9.0, 6.0), (5.0, 4.5, 9.5, 5.5), (500.0, 6.0, 10.0, 7.0)])
        sb, n = ex.terrain_flood(src, (-1.0, 1.0, 3.0), (30.0, 15.0, 16.5))
        water, body = ex.water_read()
        pb, pd = ex.water_probe([(5.0, 4.0, 9.0), (27.5, 12.0, 10.0), (5.0, 5.75, 9.0)])
        assert np.fromfile(tmp_path / "water_source_body.i32", np.int32).tolist() == sb.tolist() and n == len(ex.water_bodies())
        assert np.fromfile(tmp_path / "water_bodies.bin", vt.WATER_BODY_DTYPE).tobytes() == ex.water_bodies().tobytes()
        assert np.fromfile(tmp_path / "water_volume.f32", f32).tobytes() == np.ascontiguousarray(water.transpose(2, 1, 0)).tobytes()
        assert np.fromfile(tmp_path / "water_body_volume.i32", np.int32).tobytes() == np.ascontiguousarray(body.transpose(2, 1, 0)).tobytes()
        assert np.fromfile(tmp_path / "water_probe_body.i32", np.int32).tolist() == pb.tolist()
        assert np.fromfile(tmp_path / "water_probe_depth.f32", f32).tobytes() == pd.tobytes()
        assert n == 1 and sb.tolist() == [0, 0, -1] and pb.tolist() == [0, -1, 0]
