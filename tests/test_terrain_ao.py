"""Per-vertex ambient occlusion (vtmc_ao_*): one byte per vertex of a terrain extract, marched through the resident density grid, bit for
bit against ao_twin.py, a numpy FP32 restatement of include/vtmc.h's rule.  The twin is fed the positions, normals and blocks the device
itself returned and the grid of terrain_read_samples, so no tolerance of the extract plays a part: the comparison is equality of bytes,
every vertex.

The terrain is (64, 24, 48) cells with the WORLD of test_terrain_brushes.py at scale 0.5 and origin (3, -2, 7.5), plus one VTMC_MOD_PATH
tunnel that dives from the surface to the bottom of the grid and comes up again: real occlusion, and surface next to all six grid faces.
On the CPU twin of that world (the oracle's extract) the 6-cell result holds 13225 bytes of 255 among 28722, 27 below 128, minimum 98."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import ao_twin as twin
from host_check import run_host_check
import path_twin
from terrain_twin import gpu_struct, no_result
from test_terrain_brushes import WORLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (64, 24, 48), 0.5, (3.0, -2.0, 7.5), 4321
N_BLOCKS = (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
EDIT = ("sphere", ((14.0, 9.0, 20.0), 1.75, False))   # the material tests' small dig at the plane's surface: a few dirty blocks
_PTS = np.array([(6.0, 9.5, 12.0), (14.0, 1.5, 18.0), (26.0, 0.75, 24.0), (32.0, 8.5, 28.0)])
TUNNEL = ("path", dict(segments=np.column_stack([_PTS[:-1], np.full(3, 1.5), _PTS[1:], np.full(3, 1.5)]), addOrErode=False))
# (radius in world units, strength, steps): 6 cells / 8 steps, 2.2 cells / 3 steps, 0.4 cells / 1 step
PARAMS = [(3.0, 1.0, 8), (1.1, 0.6, 3), (0.2, 1.0, 1)]


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_limits_and_the_params():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    m = re.search(r"#define\s+VTMC_AO_MAX_STEPS\s+(\d+)", text)
    assert m and int(m.group(1)) == 8 == _lib.AO_MAX_STEPS == twin.MAX_STEPS
    m = re.search(r"#define\s+VTMC_AO_MAX_RADIUS_CELLS\s+(\d+)", text)
    assert m and int(m.group(1)) == 6 == _lib.AO_MAX_RADIUS_CELLS == twin.MAX_RADIUS_CELLS
    body = re.search(r"typedef struct vtmc_ao_params \{(.*?)\} vtmc_ao_params;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S)
    assert body
    fields = [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()]
    assert fields == ["float radius", "float strength", "int32_t steps", "uint32_t flags"]


def test_mirror_struct_layout():
    S = _lib.AoParams
    assert ctypes.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("radius", 0), ("strength", 4), ("steps", 8), ("flags", 12)]
    s = vt.AmbientOcclusion(2.5, 0.25, 7).to_struct()
    assert (s.radius, s.strength, s.steps, s.flags) == (2.5, 0.25, 7, 0)
    s = vt.AmbientOcclusion(1.0).to_struct()
    assert (s.strength, s.steps) == (1.0, 4)                    # the defaults
    for strength, steps in ((0.0, 1), (1.0, 8)):
        vt.AmbientOcclusion(1e3, strength, steps)               # the radius limit depends on the terrain: the library's to refuse


@pytest.mark.parametrize("args", [(np.nan,), (np.inf,), (0.0,), (-1.0,), (1.0, -0.1), (1.0, 1.5), (1.0, np.nan), (1.0, np.inf),
                                  (1.0, 1.0, 0), (1.0, 1.0, 9), (1.0, 1.0, 2.5)])
def test_mirror_rejects_what_the_library_rejects_by_value(args):
    with pytest.raises(ValueError):
        vt.AmbientOcclusion(*args)


def test_null_context_is_an_error_not_a_crash():
    L = vt.load()
    n, p = ctypes.c_int64(), ctypes.c_void_p()
    buf = np.zeros(64, np.uint8)
    params = _lib.AoParams(1.0, 1.0, 4, 0)
    calls = [L.vtmc_ao_vertices(None, ctypes.byref(params), ctypes.byref(n)), L.vtmc_ao_read_vertices(None, buf.ctypes.data, 64),
             L.vtmc_ao_device_results(None, ctypes.byref(p), ctypes.byref(n))]
    assert calls == [_lib.ERR_INVALID_ARG] * 3


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/ao_host_check.cpp: the host half (csrc/terrain_ao.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("ao_host_check", tmp_path)


# -- CPU: known answers of the twin -----------------------------------------------------------------------------------------------------
H = 10.5                      # the plane's height in samples, between two sample planes
PLANE_SHAPE = (34, 26, 34)


def plane_grid(lid=None):
    """density = H - y at sample plane y; lid: that one sample plane set to 1.5 instead."""
    y = np.arange(PLANE_SHAPE[1]).astype(f32)
    grid = np.broadcast_to((f32(H) - y)[None, :, None], PLANE_SHAPE).astype(f32).copy()
    if lid is not None:
        grid[:, lid, :] = f32(1.5)
    return grid


def plane_vertices(n=40, seed=3):
    """Vertices on the plane y = H with the normal (0, 1, 0), at least 6 samples from the grid's x and z faces."""
    rng = np.random.default_rng(seed)
    blocks = np.stack([rng.integers(1, 3, n), np.ones(n, np.int64), rng.integers(1, 3, n)], axis=1)
    pos = np.stack([rng.uniform(0, 8, n).astype(f32), np.full(n, H - 8, f32), rng.uniform(0, 8, n).astype(f32)], axis=1)
    return blocks, pos, np.broadcast_to(np.array([0, 1, 0], f32), (n, 3)).copy()


def test_twin_open_plane_is_unoccluded():
    blocks, pos, nrm = plane_vertices()
    for radius, steps in ((4.0, 4), (6.0, 8), (0.4, 1)):
        # every direction with c > 0 climbs: q.y > H, where the field H - y is below zero
        assert (twin.vertex_ao(plane_grid(), blocks, pos, nrm, radius, 1.0, 1.0, steps) == 255).all()


def test_twin_solid_lid_known_byte():
    """The plane with the sample plane y = 12 set to 1.5, Rg = 4, S = 4, strength 1, a vertex at y = 10.5 with normal (0, 1, 0).
    h = 1, 2, 3, 4 and fall = 1, 0.75, 0.5, 0.25.  Along y the field is -0.5 at 11, 1.5 at 12, -2.5 at 13, linear in between and the
    same for every x and z, so a fetch depends on q.y alone.  N = (0, 1, 0) gives c = d.y: the nine directions with j = +1.
      (0, 1, 0), c = 1:  q.y = 11.5, 12.5, 13.5, 14.5 -> field 0.5, -0.5, < 0, < 0 -> o = 0.5 * 1 = 0.5
      the four with two components, c = 0.70710678:  q.y = 11.2071, 11.9142, 12.6213, 13.3284 -> field -0.0858, 1.3284 (clamped to 1),
        -0.9853, < 0 -> o = 1 * 0.75 = 0.75
      the four corners, c = 0.57735027:  q.y = 11.0774, 11.6547, 12.2321, 12.8094 -> field -0.3453, 0.8094, 0.5718, -1.7376
        -> o = max(0.8094 * 0.75, 0.5718 * 0.5) = 0.60705
    num = 0.5 + 4 * 0.70710678 * 0.75 + 4 * 0.57735027 * 0.60705 = 4.02324;  den = 1 + 4 * 0.70710678 + 4 * 0.57735027 = 6.13783
    a = 1 - 4.02324 / 6.13783 = 0.34452;  a * 255 = 87.85 -> 88 (0.35 from a rounding boundary: the FP32 roundings do not reach it)."""
    blocks, pos, nrm = plane_vertices()
    assert (twin.vertex_ao(plane_grid(lid=12), blocks, pos, nrm, 4.0, 1.0, 1.0, 4) == 88).all()
    # strength scales the occlusion, not the byte: a = 1 - 0.5 * 0.65548 = 0.67226 -> 171.4 -> 171
    assert (twin.vertex_ao(plane_grid(lid=12), blocks, pos, nrm, 4.0, 1.0, 0.5, 4) == 171).all()


def test_twin_enclosed_vertex():
    """Every fetch returns 1.5 -> r = 1 at step 1, where fall = 1: o = 1 in every direction taken, num == den, a = 1 - strength."""
    grid = np.full(PLANE_SHAPE, 1.5, f32)
    rng = np.random.default_rng(4)
    blocks, pos, _ = plane_vertices(30)
    nrm = rng.normal(size=(30, 3)).astype(f32)
    for strength, want in ((0.0, 255), (0.5, 128), (1.0, 0)):       # 127.5 rounds to the even 128
        assert want == int(np.rint(f32(1 - strength) * f32(255)))
        for steps in (1, 4, 8):
            assert (twin.vertex_ao(grid, blocks, pos, nrm, 5.0, 1.0, strength, steps) == want).all()


def test_twin_bad_normals_are_unoccluded():
    grid = np.full(PLANE_SHAPE, 1.5, f32)
    blocks, pos, _ = plane_vertices(6)
    nan, inf = np.nan, np.inf
    nrm = np.array([(0, 0, 0), (nan, 0, 1), (nan, nan, nan), (0, inf, 0), (-0.0, 0.0, -0.0), (1e-30, 0, 0)], f32)
    got = twin.vertex_ao(grid, blocks, pos, nrm, 3.0, 1.0, 1.0, 4)
    assert got.tolist() == [255, 255, 255, 255, 255, 255]          # the last: l = sqrt(1e-60) underflows to 0
    assert twin.vertex_ao(grid, blocks[:1], pos[:1], np.array([(1e-18, 0, 0)], f32), 3.0, 1.0, 1.0, 4).tolist() == [0]


def test_twin_grid_corners_clamp_as_edge_replication():
    """Vertices at g = 0 and g = dim on each axis at Rg = 6: a march leaves the grid by up to 6 samples.  The twin's clamp must keep every
    index inside (numpy raises on an index out of range) and read what a grid padded with its edge samples holds there.  The padded
    evaluation shifts every coordinate by 8 (one block), so the two may differ in the last bit of a weight; the samples are multiples of
    1/8 and the seed is fixed, and with them every byte agrees."""
    rng = np.random.default_rng(8)
    shape = (18, 10, 26)
    grid = (rng.integers(-16, 17, shape) / 8).astype(f32)
    cells = [s - 2 for s in shape]
    blocks, pos = [], []
    for k in range(3):
        for high in (False, True):
            for _ in range(12):
                b = [int(rng.integers(0, cells[a] // 8)) for a in range(3)]
                p = [float(f32(rng.uniform(0, 8))) for _ in range(3)]
                b[k], p[k] = (cells[k] // 8 - 1, 8.0) if high else (0, 0.0)
                blocks.append(b), pos.append(p)
    for b, p in (((0, 0, 0), (0, 0, 0)), ((1, 0, 2), (8, 8, 8)), ((0, 0, 2), (0, 8, 8)), ((1, 0, 0), (8, 0, 0))):     # the corners themselves
        blocks.append(list(b)), pos.append([float(v) for v in p])
    blocks, pos = np.array(blocks), np.array(pos, f32)
    nrm = rng.normal(size=pos.shape).astype(f32)
    padded = np.pad(grid, 8, mode="edge")
    for steps in (8, 3):
        got = twin.vertex_ao(grid, blocks, pos, nrm, 6.0, 1.0, 1.0, steps)
        assert np.array_equal(got, twin.vertex_ao(padded, blocks + 1, pos, nrm, 6.0, 1.0, 1.0, steps))
        assert len(set(got.tolist())) > 10


def test_twin_direction_table():
    d = twin.directions()
    assert len(d) == 26 and d[0][:3] == (-1, -1, -1) and d[12][:3] == (-1, 0, 0) and d[13][:3] == (1, 0, 0) and d[25][:3] == (1, 1, 1)
    assert [(i + 1) + 3 * (j + 1) + 9 * (k + 1) for i, j, k, _ in d] == [c for c in range(27) if c != 13]
    assert {float(ln) for *_, ln in d} == {1.0, float(f32(0.70710678)), float(f32(0.57735027))}


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
def terrain(indexed=False, history=0):
    ex = vt.Extractor(0)
    ex.set_output_mode(indexed)
    ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
    if history:
        ex.terrain_set_history(history)
    return ex


def build_world(ex):
    n_dirty, T = ex.terrain_update([path_twin.gpu_struct(s) for s in WORLD + [TUNNEL]])
    assert n_dirty == N_BLOCKS and T > 0      # every block: the dense mapping
    return T


def geometry(ex, indexed):
    """(blocks, positions, normals, vertices per block of the dirty list) of the result the context holds, in the order of the bytes."""
    dirty = ex.terrain_dirty_blocks()
    if not indexed:
        tris, offs = ex.read_triangles()
        return twin.soup_vertices(tris, dirty) + (3 * np.diff(offs),)
    verts, _, voffs, _ = ex.read_indexed_mesh()
    return twin.indexed_vertices(verts, voffs, dirty) + (np.diff(voffs),)


def routes(ex, direct_max=-2):
    """(workgroups that staged a tile, workgroups on the direct route) of the last vtmc_ao_vertices; direct_max >= 0 sets the vertex count
    up to which a block goes direct, -1 restores the library's default."""
    c = (ctypes.c_uint32 * 2)()
    assert ex._L.vtmc_debug_ao_routes(ex._h, ctypes.byref(c), direct_max) == _lib.OK
    return c[0], c[1]


def want_of(ex, geo, radius, strength, steps):
    return twin.vertex_ao(ex.terrain_read_samples(), geo[0], geo[1], geo[2], radius, SCALE, strength, steps)


def assert_bytes(got, want, geo):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), len(got), bad[:5], got[bad[:5]], want[bad[:5]], geo[0][bad[:5]], geo[1][bad[:5]], geo[2][bad[:5]])


@pytest.fixture(scope="module")
def results():
    """Both output modes: the bytes, geometry, twin answers and route counts of the world-building update (every block dirty) under the
    three parameter sets, and of one small edit after it (a block list) at 6 cells / 8 steps under two route thresholds."""
    out = {}
    for indexed in (False, True):
        with terrain(indexed) as ex:
            T = build_world(ex)
            geo = geometry(ex, indexed)
            assert len(geo[1]) == (ex.last_vertex_count() if indexed else 3 * T)
            for p in PARAMS:
                got = ex.vertex_ao(*p)
                out[indexed, "dense", p] = dict(got=got, want=want_of(ex, geo, *p), geo=geo, routes=routes(ex))
            assert routes(ex, 1 << 30) == out[indexed, "dense", PARAMS[-1]]["routes"]      # setting the threshold counts nothing
            out[indexed, "dense", "direct"] = dict(got=ex.vertex_ao(*PARAMS[0]), routes=routes(ex, -1))
            n_dirty, T = ex.terrain_update([gpu_struct(EDIT)])
            assert 0 < n_dirty < N_BLOCKS and T > 0      # a proper subset: the list mapping
            geo = geometry(ex, indexed)
            want = want_of(ex, geo, *PARAMS[0])
            per_block = np.sort(geo[3][geo[3] > 0])
            assert len(per_block) >= 2 and per_block[0] < per_block[-1]
            out[indexed, "list", "default"] = dict(got=ex.vertex_ao(*PARAMS[0]), want=want, geo=geo, routes=routes(ex))
            routes(ex, int(per_block[0]))                # the smallest block of the list goes direct, the largest keeps its tile
            out[indexed, "list", "split"] = dict(got=ex.vertex_ao(*PARAMS[0]), want=want, geo=geo, routes=routes(ex, -1), per_block=per_block)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("params", PARAMS)
def test_gpu_full_result_matches_the_twin(results, indexed, params):
    r = results[indexed, "dense", params]
    assert_bytes(r["got"], r["want"], r["geo"])
    nonempty = int((r["geo"][3] > 0).sum())
    tiles, direct = r["routes"]
    print("%s %r: %d vertices, %d blocks with a tile, %d direct" % ("indexed" if indexed else "soup", params, len(r["got"]), tiles, direct))
    assert tiles + direct == nonempty and tiles > 0 and direct > 0          # both routes, and no workgroup for an empty block
    assert direct == int(((r["geo"][3] > 0) & (r["geo"][3] <= 12)).sum())
    if params == PARAMS[0]:     # not vacuous: open ground, real occlusion, and most of the surface shaded
        got = r["got"]
        assert (got == 255).any() and (got < 128).any() and 2 * int((got == 255).sum()) < len(got)
        assert np.array_equal(results[indexed, "dense", "direct"]["got"], got)      # every block on the direct route: the same bytes
        assert results[indexed, "dense", "direct"]["routes"] == (0, nonempty)


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
def test_gpu_sparse_dirty_list_matches_the_twin_on_both_routes(results, indexed):
    r = results[indexed, "list", "default"]
    assert_bytes(r["got"], r["want"], r["geo"])
    assert (r["want"] < 255).any()
    s = results[indexed, "list", "split"]
    assert_bytes(s["got"], s["want"], s["geo"])
    tiles, direct = s["routes"]
    assert tiles > 0 and direct > 0 and tiles + direct == len(s["per_block"]) and direct == int((s["per_block"] <= s["per_block"][0]).sum())
    assert sum(r["routes"]) == len(s["per_block"])


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
def test_gpu_grid_faces(results, indexed):
    """The vertices whose march can leave the grid, face by face: the clamp, and the tile's edge."""
    r = results[indexed, "dense", PARAMS[0]]
    blocks, pos = r["geo"][0], r["geo"][1]
    for k in range(3):
        g = (8 * blocks[:, k]).astype(f32) + pos[:, k]
        for face in (g < 6, g > DIMS[k] - 6):
            assert face.any()
            assert np.array_equal(r["got"][face], r["want"][face])
            assert len(set(r["got"][face].tolist())) > 1


def raw_params(radius, strength, steps, flags=0):
    return _lib.AoParams(radius, strength, steps, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
def test_gpu_lifecycle(indexed):
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.set_output_mode(indexed)
        buf = np.zeros(1 << 17, np.uint8)
        read = lambda cap=len(buf): L.vtmc_ao_read_vertices(h, buf.ctypes.data, cap)   # noqa: E731
        compute = lambda p: L.vtmc_ao_vertices(h, ctypes.byref(p), None)               # noqa: E731
        no_result(lambda: ex.vertex_ao(1.0))                 # no terrain
        assert read() == _lib.ERR_NO_RESULT
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        no_result(lambda: ex.vertex_ao(1.0))                 # a terrain, no result
        no_result(ex.device_ao)
        # an erode in the void: dirty blocks without surface
        n_dirty, T = ex.terrain_update([vt.SphereModifier((20.0, 4.0, 20.0), 2.0, False)])
        assert n_dirty > 0 and T == 0
        assert ex.ao_vertices(vt.AmbientOcclusion(1.0)) == 0 and ex.vertex_ao(1.0).shape == (0,) and ex.device_ao()[1] == 0
        assert read(0) == _lib.OK
        ex.terrain_set_history(4 << 20)
        build_world(ex)
        assert read() == _lib.ERR_NO_RESULT                  # a result, its bytes not computed yet
        got = ex.vertex_ao(*PARAMS[0])
        n = len(got)
        assert n > 0 and read() == _lib.OK and np.array_equal(buf[:n], got)
        assert read(n - 1) == _lib.ERR_INVALID_ARG and read(n) == _lib.OK       # a capacity below n
        assert compute(raw_params(3.0, 1.0, 8)) == _lib.OK                      # exactly 6 cells
        assert L.vtmc_ao_vertices(h, None, None) == _lib.ERR_INVALID_ARG
        nan, inf = float("nan"), float("inf")
        for bad in [raw_params(3.005, 1.0, 8), raw_params(1.0, 1.0, 0), raw_params(1.0, 1.0, 9), raw_params(1.0, 1.0, 4, 1),
                    raw_params(0.0, 1.0, 4), raw_params(-1.0, 1.0, 4), raw_params(nan, 1.0, 4), raw_params(inf, 1.0, 4),
                    raw_params(1.0, -0.25, 4), raw_params(1.0, 1.25, 4), raw_params(1.0, nan, 4)]:
            assert compute(bad) == _lib.ERR_INVALID_ARG
            buf[:n] = 7
            assert read() == _lib.OK and np.array_equal(buf[:n], got)           # refused, the previous values still readable
        d_ptr, dn = ex.device_ao()
        assert dn == n and d_ptr and np.array_equal(ex.copy_to_host(d_ptr, n), got)
        # any later extract: stale until ao_vertices runs again
        ex.terrain_update([gpu_struct(EDIT)])
        assert read() == _lib.ERR_NO_RESULT
        no_result(ex.device_ao)
        edited = ex.vertex_ao(*PARAMS[1])
        assert len(edited) > 0 and read() == _lib.OK
        ex.terrain_undo()
        assert read() == _lib.ERR_NO_RESULT
        geo = geometry(ex, indexed)
        assert_bytes(ex.vertex_ao(*PARAMS[0]), want_of(ex, geo, *PARAMS[0]), geo)     # the restored grid
        # a result that did not come from the terrain is refused
        grid = np.full((10, 10, 10), -1.0, f32)
        grid[3:6, 3:6, 3:6] = 1.0
        assert ex.extract_grid(grid) > 0
        no_result(lambda: ex.vertex_ao(1.0))
        assert read() == _lib.ERR_NO_RESULT


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True])
def test_gpu_independent_of_the_material_layer(results, indexed):
    want = results[indexed, "dense", PARAMS[1]]["got"]        # computed without a layer
    with terrain(indexed) as ex:
        ex.material_init(1)
        build_world(ex)
        weights = ex.vertex_materials()
        assert np.array_equal(ex.vertex_ao(*PARAMS[1]), want)
        out = np.empty_like(weights)
        assert ex._L.vtmc_material_read_vertices(ex._h, out.ctypes.data, len(out)) == _lib.OK and np.array_equal(out, weights)
        assert np.array_equal(ex.vertex_materials(), weights)  # and the reverse: the bytes stay current
        d_ptr, n = ex.device_ao()
        assert n == len(want) and np.array_equal(ex.copy_to_host(d_ptr, n), want)
