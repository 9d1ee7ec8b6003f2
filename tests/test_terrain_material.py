"""The material layer (vtmc_material_*): the control volume of VoxelTerrain.SetControlMap resident on the device, the paint brush on it
and the material weights of every extracted vertex, bit for bit against material_twin.py, a numpy FP32 restatement of include/vtmc.h's
rule.  The twin is fed the positions and blocks the device itself returned, so the position tolerance of the extract plays no part.

The terrain is (64, 24, 48) cells with the WORLD of test_terrain_brushes.py at scale 0.5 and origin (3, -2, 7.5): three different
per-axis factors; scale and origin enter paint only."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import material_twin as twin
from host_check import run_host_check
from terrain_twin import gpu_struct, no_result
from test_terrain_brushes import WORLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (64, 24, 48), 0.5, (3.0, -2.0, 7.5), 4321
N_BLOCKS = (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
EDIT = ("sphere", ((14.0, 9.0, 20.0), 1.75, False))   # a small dig at the plane's surface: a few dirty blocks


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def random_layer(C, seed):
    return np.random.default_rng(seed).integers(0, 256, (C, C, C, 8), dtype=np.uint8)


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_channels_and_the_stroke():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    m = re.search(r"#define\s+VTMC_MATERIAL_CHANNELS\s+(\d+)", text)
    assert m and int(m.group(1)) == 8 == _lib.MATERIAL_CHANNELS
    m = re.search(r"#define\s+VTMC_MATERIAL_MAX_STROKES\s+(\d+)", text)
    assert m and int(m.group(1)) == 4096 == _lib.MATERIAL_MAX_STROKES
    body = re.search(r"typedef struct vtmc_material_stroke \{(.*?)\} vtmc_material_stroke;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S)
    assert body
    fields = [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()]
    assert fields == ["float center[3]", "float radius", "float strength", "int32_t channel"]


def test_mirror_struct_layout():
    S = _lib.MaterialStroke
    assert ctypes.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("center", 0), ("radius", 12), ("strength", 16), ("channel", 20)]
    s = vt.MaterialStroke((1.5, -2.25, 3.0), 4.5, 6, 0.25).to_struct()
    assert tuple(s.center) == (1.5, -2.25, 3.0) and (s.radius, s.strength, s.channel) == (4.5, 0.25, 6)
    assert vt.MaterialStroke((0, 0, 0), 1.0, 0).to_struct().strength == 1.0   # default strength
    for strength in (0.0, 1.0):
        vt.MaterialStroke((0, 0, 0), 1.0, 7, strength)


@pytest.mark.parametrize("args", [
    ((np.nan, 0, 0), 1.0, 0, 1.0), ((0, np.inf, 0), 1.0, 0, 1.0), ((0, 0, 0), 0.0, 0, 1.0), ((0, 0, 0), -1.0, 0, 1.0),
    ((0, 0, 0), np.inf, 0, 1.0), ((0, 0, 0), np.nan, 0, 1.0), ((0, 0, 0), 1.0, 0, -0.1), ((0, 0, 0), 1.0, 0, 1.5),
    ((0, 0, 0), 1.0, 0, np.nan), ((0, 0, 0), 1.0, 0, np.inf), ((0, 0, 0), 1.0, -1, 1.0), ((0, 0, 0), 1.0, 8, 1.0), ((0, 0, 0), 1.0, 1.5, 1.0)])
def test_mirror_rejects_what_the_library_rejects(args):
    with pytest.raises(ValueError):
        vt.MaterialStroke(*args)


# -- CPU: known answers of the twin -----------------------------------------------------------------------------------------------------
def test_twin_uniform_layer_gives_its_bytes_everywhere():
    C = 16
    texel = np.array([13, 0, 255, 7, 100, 31, 1, 254], np.uint8)
    layer = np.broadcast_to(texel, (C, C, C, 8)).copy()
    rng = np.random.default_rng(1)
    blocks = np.stack([rng.integers(0, DIMS[k] // 8, 500) for k in range(3)], axis=1)
    pos = rng.uniform(0, 8, (500, 3)).astype(f32)
    blocks[:6] = [(0, 0, 0), (7, 2, 5), (0, 2, 0), (7, 0, 5), (3, 0, 5), (3, 2, 0)]       # the wrap faces: g = 0 and g = cells
    pos[:6] = [(0, 0, 0), (8, 8, 8), (0, 8, 0), (8, 0, 8), (4.5, 0, 8), (4.5, 8, 0)]
    assert np.array_equal(twin.vertex_weights(layer, DIMS, blocks, pos), np.broadcast_to(texel, (500, 8)))


def test_twin_quantise_rounds_ties_to_even():
    c = np.array([-1, 0, f32(0.5) / f32(255), f32(1.5) / f32(255), f32(2.5) / f32(255), 1, 2], f32)
    assert twin.quantise(c).tolist() == [0, 0, 0, 2, 2, 255, 255]


def test_twin_full_stroke_on_a_texel_centre():
    C = 16
    layer = random_layer(C, 2)
    px, py, pz = twin.texel_centres(C, DIMS, SCALE, ORIGIN)
    i, j, k, r = 5, 9, 3, 3.0
    stroke = ((px[i], py[j], pz[k]), r, 6, 1.0)
    out = twin.paint(layer, [stroke], DIMS, SCALE, ORIGIN)
    assert out[k, j, i].tolist() == [0, 0, 0, 0, 0, 0, 255, 0]
    d = np.sqrt((px[None, None, :].astype(np.float64) - px[i]) ** 2 + (py[None, :, None].astype(np.float64) - py[j]) ** 2 +
                (pz[:, None, None].astype(np.float64) - pz[k]) ** 2)
    far = d >= r
    assert far.any() and (~far).sum() > 1
    assert np.array_equal(out[far], layer[far])
    assert (out[~far] != layer[~far]).any()


def test_twin_ramp_at_a_texel_centre_gives_that_texel():
    C = 16
    layer = np.zeros((C, C, C, 8), np.uint8)
    layer[...] = (np.arange(C) * 16)[None, None, :, None] + np.arange(8)[None, None, None, :]     # linear along x, per channel offset
    # texel i's centre: t = g * (C / W) - 0.5 = i, g = (i + 0.5) * 4 for W = 64: fx == 0
    i = np.arange(C)
    g = (i + 0.5) * (DIMS[0] / C)
    blocks = np.stack([(g // 8).astype(np.int64), np.ones(C, np.int64), np.full(C, 2)], axis=1)
    pos = np.stack([(g % 8).astype(f32), np.full(C, 3.3, f32), np.full(C, 1.7, f32)], axis=1)
    assert np.array_equal(twin.vertex_weights(layer, DIMS, blocks, pos), layer[0, 0, i])


def test_null_context_is_an_error_not_a_crash():
    L = vt.load()
    n, p, c = ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_int32()
    buf = np.zeros(64, np.uint8)
    calls = [L.vtmc_material_init(None, 1), L.vtmc_material_set_control_map(None, buf.ctypes.data, 1), L.vtmc_material_write(None, buf.ctypes.data),
             L.vtmc_material_read(None, buf.ctypes.data, ctypes.byref(c)), L.vtmc_material_paint(None, buf.ctypes.data, 1),
             L.vtmc_material_vertices(None, ctypes.byref(n)), L.vtmc_material_read_vertices(None, buf.ctypes.data, 8),
             L.vtmc_material_device_results(None, ctypes.byref(p), ctypes.byref(n))]
    assert calls == [_lib.ERR_INVALID_ARG] * 8


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/material_host_check.cpp: the host half (csrc/terrain_material.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("material_host_check", tmp_path)


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
def terrain(indexed=False, history=0):
    ex = vt.Extractor(0)
    ex.set_output_mode(indexed)
    ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
    if history:
        ex.terrain_set_history(history)
    return ex


def build_world(ex):
    n_dirty, T = ex.terrain_update([gpu_struct(s) for s in WORLD])
    assert n_dirty == N_BLOCKS and T > 0      # every block: the dense mapping
    return T


def geometry(ex, indexed):
    """(blocks (n, 3), positions (n, 3)) of the vertices of the result the context holds, in the order of the weights; for the indexed
    mode also the global vertex number of every triangle corner."""
    dirty = ex.terrain_dirty_blocks()
    if not indexed:
        tris, _ = ex.read_triangles()
        pos = np.stack([tris["p0"], tris["p1"], tris["p2"]], axis=1).reshape(-1, 3)
        return np.repeat(dirty[tris["block"]], 3, axis=0).reshape(-1, 3), pos, None
    verts, idx, voffs, toffs = ex.read_indexed_mesh()
    vblock = np.repeat(np.arange(len(dirty)), np.diff(voffs))
    tblock = np.repeat(np.arange(len(dirty)), np.diff(toffs))
    return dirty[vblock].reshape(-1, 3), verts["position"].reshape(-1, 3), idx + voffs[tblock][:, None]


def invalid(fn):
    with pytest.raises(vt.VtmcError) as e:
        fn()
    assert e.value.code == _lib.ERR_INVALID_ARG
    return str(e.value)


@pytest.fixture(scope="module")
def results():
    """Both output modes on the same terrain and layer: the weights, geometry and twin answer of the world-building update (every block
    dirty) and of one small edit after it (a block list)."""
    layer = random_layer(16, 7)
    out = {}
    for indexed in (False, True):
        with terrain(indexed) as ex:
            assert ex.material_init(1) == 16
            ex.material_write(layer)
            for name in ("dense", "list"):
                if name == "dense":
                    build_world(ex)
                else:
                    n_dirty, T = ex.terrain_update([gpu_struct(EDIT)])
                    assert 0 < n_dirty < N_BLOCKS and T > 0      # a proper subset: the list mapping
                blocks, pos, corners = geometry(ex, indexed)
                got = ex.vertex_materials()
                out[indexed, name] = dict(blocks=blocks, pos=pos, corners=corners, got=got, want=twin.vertex_weights(layer, DIMS, blocks, pos),
                                          T=ex.last_counts()[1])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("order", [(1, 2), (2, 1)])
def test_gpu_set_control_map_quantises_one_group_and_keeps_the_other(order):
    C = 16
    rng = np.random.default_rng(11)
    with terrain() as ex:
        ex.material_init(1)
        want = twin.initial(C)
        assert np.array_equal(ex.material_read(), want)
        for group in order:
            img = rng.uniform(-0.5, 1.5, (C, C, C, 4)).astype(f32)
            img.reshape(-1)[:7] = [-1, 0, f32(0.5) / f32(255), f32(1.5) / f32(255), f32(2.5) / f32(255), 1, 2]     # the ties
            img.reshape(-1)[7:11] = [np.inf, -np.inf, 1e-40, -0.0]
            ex.set_control_map(img, group)
            want = twin.set_control_map(want, img, group)
            assert np.array_equal(ex.material_read(), want)
        bad = rng.uniform(0, 1, (C, C, C, 4)).astype(f32)
        bad[C - 1, 3, 2, 1] = np.nan
        for group in (1, 2):
            assert "NaN" in invalid(lambda: ex.set_control_map(bad, group))
        for group in (0, 3, -1):
            invalid(lambda: ex.set_control_map(np.zeros((C, C, C, 4), f32), group))
        with pytest.raises(ValueError):
            ex.set_control_map(np.zeros((C, C, 4), f32), 1)
        assert np.array_equal(ex.material_read(), want)


def strokes_for(C):
    """About 40 strokes (center, radius, channel, strength) on the world x 3..35, y -2..10, z 7.5..31.5."""
    rng = np.random.default_rng(100 + C)
    px, py, pz = twin.texel_centres(C, DIMS, SCALE, ORIGIN)
    ts = [float(p[1] - p[0]) for p in (px, py, pz)]
    s = [((12.0, 4.0, 18.0), 5.0, 1, 1.0), ((12.0, 4.0, 18.0), 5.0, 5, 0.5), ((13.5, 4.5, 19.0), 4.0, 2, 0.75),      # overlapping, different channels
         ((1.0, 4.0, 20.0), 4.0, 3, 1.0), ((20.0, 13.0, 33.5), 4.5, 7, 0.9),                                       # centres outside, balls reach in
         ((3.0, -2.0, 7.5), 2.5, 4, 1.0), ((35.0, 10.0, 31.5), 3.0, 6, 1.0),                                        # over corner texels
         ((3.0 + 5 * ts[0], -2.0 + 3 * ts[1], 7.5 + 4 * ts[2]), 0.1, 2, 1.0),                                       # reaches no texel centre
         ((20.0, 5.0, 20.0), 6.0, 0, 0.0), ((20.0, 5.0, 20.0), 6.0, 3, 1.0),                                        # strength 0 and 1
         ((float(px[4]), float(py[6]), float(pz[9])), 1.0, 5, 1.0), ((-40.0, 50.0, 90.0), 3.0, 1, 1.0)]             # on a texel centre; far away
    for _ in range(28):
        c = (rng.uniform(1, 37), rng.uniform(-4, 12), rng.uniform(5, 34))
        s.append((c, float(rng.uniform(0.3, 7.0)), int(rng.integers(0, 8)), float(rng.choice([1.0, rng.uniform(0, 1)]))))
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("fineness", [1, 3])
def test_gpu_paint_matches_the_twin_stroke_by_stroke_and_in_one_call(fineness):
    C = 16 * fineness
    strokes = strokes_for(C)
    assert len(strokes) == 40
    with terrain() as ex:
        assert ex.material_init(fineness) == C
        start = random_layer(C, 5)
        ex.material_write(start)
        want = start
        for i, s in enumerate(strokes):
            ex.paint([vt.MaterialStroke(*s)])
            after = twin.paint(want, [s], DIMS, SCALE, ORIGIN)
            assert np.array_equal(ex.material_read(), after), i
            if i in (7, 8, 11):     # below half a texel between centres; strength 0; far away: the layer keeps its bytes
                assert np.array_equal(after, want), i
            if i in (5, 6):         # over a corner texel: something changed, and nothing on the three opposite faces
                k = 0 if i == 5 else C - 1
                far = C - 1 - k
                changed = (after != want).any(axis=-1)
                assert changed[k, k, k] and not changed[far].any() and not changed[:, far].any() and not changed[:, :, far].any()
            want = after
        assert (want != start).any()
        ex.material_write(start)
        ex.paint([vt.MaterialStroke(*s) for s in strokes])       # the same strokes in one call, one pass per texel
        assert np.array_equal(ex.material_read(), want)
        assert np.array_equal(twin.paint(start, strokes, DIMS, SCALE, ORIGIN), want)
        ex.paint([])
        assert np.array_equal(ex.material_read(), want)


def assert_weights(r):
    got, want = r["got"], r["want"]
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), len(got), bad[:5], got[bad[:5]], want[bad[:5]], r["blocks"][bad[:5]], r["pos"][bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense", "list"])
def test_gpu_soup_vertex_weights(results, name):
    r = results[False, name]
    assert len(r["got"]) == 3 * r["T"] and (3 * r["T"]) % 64 != 0     # partial waves and a partial tile
    if name == "dense":
        gx = (8 * r["blocks"][:, 0]).astype(f32) + r["pos"][:, 0]
        assert (gx == 0).any() and (gx == DIMS[0]).any()               # the wrap on both x faces: texels C-1 and 0
        assert 3 * r["T"] > 2 * 768                                    # more than one tile
    assert_weights(r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense", "list"])
def test_gpu_indexed_vertex_weights_and_their_soup(results, name):
    r, soup = results[True, name], results[False, name]
    assert len(r["got"]) == len(r["pos"]) and r["T"] == soup["T"] and len(r["got"]) % 256 != 0
    assert_weights(r)
    # de-indexed: the corner's bytes are the soup's wherever the two modes agree on the corner's position bit for bit
    corners = r["corners"].reshape(-1)
    same = (bits(r["pos"][corners]) == bits(soup["pos"])).all(axis=1) & (r["blocks"][corners] == soup["blocks"]).all(axis=1)
    print("%s: %d of %d corners bit-identical in both modes" % (name, same.sum(), len(same)))
    assert 2 * same.sum() >= len(same)
    assert np.array_equal(r["got"][corners][same], soup["got"][same])


@pytest.mark.gpu
def test_gpu_vertex_weights_at_fineness_3_soup():
    """C = 48 on 64 x 24 x 48 cells: factors 0.75, 2 and 1."""
    layer = random_layer(48, 9)
    with terrain() as ex:
        ex.material_init(3)
        ex.material_write(layer)
        build_world(ex)
        blocks, pos, _ = geometry(ex, False)
        assert_weights(dict(got=ex.vertex_materials(), want=twin.vertex_weights(layer, DIMS, blocks, pos), blocks=blocks, pos=pos))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
def test_gpu_single_triangle_and_empty_results(indexed):
    layer = random_layer(16, 3)
    with terrain(indexed) as ex:
        ex.material_init(1)
        ex.material_write(layer)
        # only sample (0, 0, 0) turns solid: one triangle in cell (0, 0, 0) of block (0, 0, 0)
        n_dirty, T = ex.terrain_update([vt.SphereModifier(ORIGIN, 0.25, True)])
        assert (n_dirty, T) == (1, 1)
        blocks, pos, _ = geometry(ex, indexed)
        got = ex.vertex_materials()
        assert got.shape == (3, 8)
        assert_weights(dict(got=got, want=twin.vertex_weights(layer, DIMS, blocks, pos), blocks=blocks, pos=pos))
        # an erode in the void: dirty blocks without surface
        n_dirty, T = ex.terrain_update([vt.SphereModifier((20.0, 4.0, 20.0), 2.0, False)])
        assert n_dirty > 0 and T == 0
        assert ex.material_vertices() == 0 and ex.vertex_materials().shape == (0, 8)
        assert ex.material_device_results()[1] == 0


def raw_stroke(center, radius, strength, channel):
    s = _lib.MaterialStroke()
    s.center[:] = center
    s.radius, s.strength, s.channel = radius, strength, channel
    return s


@pytest.mark.gpu
def test_gpu_staleness_and_lifecycle():
    with terrain(history=4 << 20) as ex:
        L, h = ex._L, ex._h
        buf = np.zeros((1 << 16, 8), np.uint8)
        read = lambda cap=len(buf): L.vtmc_material_read_vertices(h, buf.ctypes.data, cap)   # noqa: E731
        no_result(ex.material_read)                      # no layer yet
        no_result(lambda: ex.paint([vt.MaterialStroke((0, 0, 0), 1.0, 0)]))
        no_result(ex.material_vertices)
        for fineness in (0, 9, -1):
            invalid(lambda: ex.material_init(fineness))
        ex.material_init(2)
        no_result(ex.material_vertices)                  # a layer, no result
        assert read() == _lib.ERR_NO_RESULT
        build_world(ex)
        assert read() == _lib.ERR_NO_RESULT              # a result, its weights not computed yet
        ex.paint([vt.MaterialStroke((12.0, 4.0, 18.0), 5.0, 2, 0.8)])
        layer = ex.material_read()
        n = ex.material_vertices()
        assert n > 0 and read() == _lib.OK
        assert read(n - 1) == _lib.ERR_INVALID_ARG and read(n) == _lib.OK       # a capacity below n
        ex.paint([vt.MaterialStroke((20.0, 4.0, 18.0), 2.0, 1, 0.5)])           # paint leaves the result and its weights alone
        layer = ex.material_read()
        assert read() == _lib.OK
        steps = [lambda: ex.terrain_update([gpu_struct(EDIT)]), ex.terrain_undo, ex.terrain_redo]
        for step in steps:                               # any later extract: stale until material_vertices runs again
            step()
            assert read() == _lib.ERR_NO_RESULT
            no_result(ex.material_device_results)
            assert np.array_equal(ex.material_read(), layer)        # undo / redo leave the layer alone
            assert ex.material_vertices() > 0 and read() == _lib.OK
        # every refused paint names its stroke and writes nothing
        good = raw_stroke((12.0, 4.0, 18.0), 3.0, 1.0, 4)
        nan, inf = float("nan"), float("inf")
        for bad in [raw_stroke((nan, 0, 0), 1.0, 1.0, 0), raw_stroke((0, inf, 0), 1.0, 1.0, 0), raw_stroke((0, 0, -inf), 1.0, 1.0, 0),
                    raw_stroke((0, 0, 0), nan, 1.0, 0), raw_stroke((0, 0, 0), inf, 1.0, 0), raw_stroke((0, 0, 0), 0.0, 1.0, 0),
                    raw_stroke((0, 0, 0), -1.0, 1.0, 0), raw_stroke((0, 0, 0), 1.0, nan, 0), raw_stroke((0, 0, 0), 1.0, inf, 0),
                    raw_stroke((0, 0, 0), 1.0, -0.25, 0), raw_stroke((0, 0, 0), 1.0, 1.25, 0), raw_stroke((0, 0, 0), 1.0, 1.0, -1),
                    raw_stroke((0, 0, 0), 1.0, 1.0, 8)]:
            assert "stroke 2" in invalid(lambda: ex.paint([good, good, bad, good]))
            assert np.array_equal(ex.material_read(), layer)
        arr = (_lib.MaterialStroke * 4097)()
        for s in arr:
            s.radius, s.strength = 1.0, 1.0
        for n_strokes in (4097, -1):
            assert L.vtmc_material_paint(h, ctypes.cast(arr, ctypes.c_void_p), n_strokes) == _lib.ERR_INVALID_ARG
        assert L.vtmc_material_paint(h, None, 1) == _lib.ERR_INVALID_ARG
        assert L.vtmc_material_paint(h, None, 0) == _lib.OK
        assert np.array_equal(ex.material_read(), layer)
        # a result that did not come from the terrain is refused
        grid = np.full((10, 10, 10), -1.0, f32)
        grid[3:6, 3:6, 3:6] = 1.0
        assert ex.extract_grid(grid) > 0
        no_result(ex.material_vertices)
        assert read() == _lib.ERR_NO_RESULT
        # vtmc_terrain_init drops the layer
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        no_result(ex.material_read)
        no_result(ex.material_vertices)


@pytest.mark.gpu
def test_gpu_round_trips():
    with terrain() as ex:
        assert ex.material_init(2) == 32 == ex.material_size()
        ex.paint([vt.MaterialStroke((12.0, 4.0, 18.0), 6.0, 3, 0.7), vt.MaterialStroke((25.0, 2.0, 25.0), 8.0, 6, 1.0)])
        layer = ex.material_read()
        assert layer.shape == (32, 32, 32, 8) and (layer != twin.initial(32)).any()
        ex.material_write(layer)
        assert np.array_equal(ex.material_read(), layer)
        other = random_layer(32, 4)
        ex.material_write(other)
        assert np.array_equal(ex.material_read(), other)
        with pytest.raises(ValueError):
            ex.material_write(other[:16])
        build_world(ex)
        got = ex.vertex_materials()
        d_ptr, n = ex.material_device_results()
        assert n == len(got) and d_ptr
        assert np.array_equal(ex.copy_to_host(d_ptr, 8 * n).reshape(n, 8), got)
        assert ex.material_init(1) == 16                 # again: replaces the layer, and the weights of the old one are gone
        assert np.array_equal(ex.material_read(), twin.initial(16))
        no_result(ex.material_device_results)
