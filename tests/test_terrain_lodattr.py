"""Per-vertex materials and occlusion of a level-of-detail extract and of its skirts (vtmc_lod_material_vertices, vtmc_lod_ao_vertices,
vtmc_lodattr_*, include/vtmc_lodattr.h).

The rule LODATTR is restated by lodattr_twin.py, which composes material_twin.py and ao_twin.py without touching them; every comparison
here is for EQUALITY OF BYTES.  On the CPU the twin runs on the CPU oracle's meshes of the twin's tiles (lod_twin.node_tiles ->
oracle.extract_tiles); on the GPU it is fed the device's own records.

The scene is test_terrain_lodskirt's: scene_samples() written as samples, 64 x 32 x 32 cells, roots of level 2, viewer "corner", split 1:
37 nodes of levels 0, 1 and 2.  The control map is a product of three sines, constant along no axis.  test_the_inputs_are_not_vacuous
asserts, through the oracle alone, that these inputs can tell a wrong kernel from a right one.

The occlusion cases are (radius, steps) with ceil(radius / scale) = 1, 2 and 6.  The 20 % floor on bytes that differ from 255 holds at
every level for the cases of reach 2 and 6; a march of at most one cell (reach 1) over the open ground near the viewer darkens 6.8 % of the
level-0 vertices (613 of 9018), and that case states its own floor of 5 %."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import ao_twin
import lod_twin
import lodattr_twin as twin
import lodskirt_twin
import material_twin
from host_check import run_host_check
from lod_support import POISON, bits
from terrain_twin import no_result
from test_terrain_lod import DIMS, MAX_LEVEL, ORIGIN, SCALE, SEED, VIEWERS, full_world, select, world_of
from test_terrain_lodskirt import scene_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DEPTH = 1.0
MATERIAL, AO, MESH, SKIRTS = 0, 1, 0, 1
AO_CASES = {1: (0.5, 8), 2: (1.0, 1), 6: (2.9, 8)}          # reach -> (radius, steps); strength below
STRENGTH = 0.875
FLOOR = {1: 0.05, 2: 0.20, 6: 0.20}                          # the share of bytes != 255 at every level (see the module's docstring)
SYMBOLS = ["vtmc_lod_material_vertices", "vtmc_lod_ao_vertices", "vtmc_lodattr_info", "vtmc_lodattr_read", "vtmc_lodattr_device_results"]


def control_map(C, group):
    k, j, i = np.meshgrid(*(np.arange(C, dtype=np.float64),) * 3, indexing="ij")
    c = np.arange(4, dtype=np.float64)[None, None, None, :]
    v = 0.5 + 0.5 * np.sin(0.37 * i[..., None] + 0.9 * c + group) * np.sin(0.61 * j[..., None] + 0.4 * c) * np.sin(0.83 * k[..., None] + 1.0 + 0.7 * c)
    return v.astype(f32)


def layer_of(fineness):
    C = 16 * fineness
    layer = material_twin.initial(C)
    for group in (1, 2):
        layer = material_twin.set_control_map(layer, control_map(C, group), group)
    for axis in range(3):
        assert (np.diff(layer.astype(np.int64), axis=axis) != 0).any()
    return layer


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_constants_and_symbol_order():
    path = os.path.join(ROOT, "include", "vtmc_lodattr.h")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    for name, value in (("MATERIAL", 0), ("AO", 1), ("MESH", 0), ("SKIRTS", 1)):
        assert re.search(r"#define\s+VTMC_LODATTR_%s\s+%d\b" % (name, value), text) and getattr(_lib, "LODATTR_" + name) == value
    assert (twin.MATERIAL, twin.AO, twin.MESH, twin.SKIRTS) == (0, 1, 0, 1) == (MATERIAL, AO, MESH, SKIRTS)
    assert '#include "vtmc_lodskirt.h"' in text and "typedef struct" not in text             # the params are vtmc.h's vtmc_ao_params
    assert list(_lib.LAYER_SYMBOLS["lodattr"]) == SYMBOLS
    assert ctypes.sizeof(_lib.AoParams) == 16
    whole = " ".join(open(path).read().split())
    for word in ("LODATTR", "(float)o.x + p.x * (float)s", "(float)(o.x / s) + p.x", "n_L = (dim - 2) / s + 2", "NOT CONTINUOUS", "attr(b), attr(a), attr(a)",
                 "attr(b), attr(a), attr(b)", "never evaluated at its own position", "bit for bit"):
        assert word in whole, word
    for doc in ("include/vtmc.h", "LODSEAMS.md", "README.md", "INTEGRATION.md", "LODSHADING.md"):
        assert "vtmc_lodattr.h" in open(os.path.join(ROOT, doc)).read(), doc
    shading = " ".join(open(os.path.join(ROOT, "LODSHADING.md")).read().split())
    for word in ("node's own cells", "not continuous", "What it costs", "vtmc_lod_skirts"):
        assert word in shading, word
    for name in ("lod_vertex_materials", "lod_vertex_ao", "lod_skirt_materials", "lod_skirt_ao", "device_lod_attributes", "lodattr_info"):
        assert callable(getattr(vt.Extractor, name)), name


def test_null_pointers_are_errors_not_crashes():
    L = vt.load()
    p, n = _lib.AoParams(1.0, 1.0, 4, 0), ctypes.c_int64()
    assert L.vtmc_lod_material_vertices(None, ctypes.byref(n), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lod_material_vertices(None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lod_ao_vertices(None, ctypes.byref(p), None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lod_ao_vertices(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodattr_info(None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodattr_read(None, 0, 0, None, 0) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodattr_device_results(None, 1, 1, None, None) == _lib.ERR_INVALID_ARG


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/lodattr_host_check.cpp: csrc/terrain_lodattr.h, the functions the kernels call, as a stand-alone program under ASan and UBSan."""
    run_host_check("lodattr_host_check", tmp_path)


# -- CPU: the twin on the oracle's meshes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle_mod):
    S = scene_samples()
    nodes = select("corner", 1.0)
    records, offs, _ = oracle_mod.extract_tiles(lod_twin.node_tiles(S, nodes))
    skirt, node_offsets, _ = lodskirt_twin.skirts(records, lodskirt_twin.face_masks(DIMS, nodes), DEPTH)
    return dict(S=S, nodes=nodes, records=records, offs=offs, skirt=skirt, node_offsets=node_offsets)


def test_the_inputs_are_not_vacuous(scene, oracle_mod):
    S, nodes, records = scene["S"], scene["nodes"], scene["records"]
    assert len(nodes) == 37 and sorted(set(nodes[:, 3].tolist())) == [0, 1, 2]
    block, pos, nrm = twin.soup_vertices(records)
    level = nodes[block, 3]
    assert (np.bincount(level, minlength=3) > 500).all()                                       # every level has vertices
    for reach, (radius, steps) in AO_CASES.items():
        assert int(np.ceil(f32(radius) / f32(SCALE))) == reach
        ao = twin.vertex_ao(S, nodes, block, pos, nrm, radius, SCALE, STRENGTH, steps)
        share = [float((ao[level == lv] != 255).mean()) for lv in range(3)]
        print("reach %d: share of bytes != 255 per level %s, %d distinct bytes" % (reach, ["%.3f" % s for s in share], len(set(ao.tolist()))))
        assert min(share) >= FLOOR[reach], (reach, share)
    per_node = np.diff(scene["offs"])
    assert per_node.max() > 128                                                                # more than one chunk of soup records
    assert ((per_node > 0) & (3 * per_node <= 12)).any()                                       # the direct route at the default threshold (soup)
    welded = np.array([len(oracle_mod.extract_grid_indexed(np.ascontiguousarray(t.reshape(10, 10, 10).transpose(2, 1, 0)))[0])
                       for t in lod_twin.node_tiles(S, nodes)])
    assert ((welded > 0) & (welded <= 12)).any()                                               # ... and indexed
    g = nodes[block, :3] + pos.astype(np.float64) * (1 << level)[:, None]
    assert (g == 0).any()                                                                      # a vertex on a lower face: tx = -0.5, the Repeat wrap
    # a march at level 2 that reads lattice index n_L - 1: direction +k alone is taken when N_k > 0, and its last step fetches at g_k + Rg
    two = level == 2
    gl = nodes[block[two], :3] // 4 + pos[two].astype(np.float64)
    n_l = np.array([twin.lattice_samples(d + 2, 4) for d in DIMS])
    assert n_l.tolist() == [18, 10, 10]
    for reach, (radius, _) in AO_CASES.items():
        reads_last = ((nrm[two] > 0) & (gl + radius / SCALE > n_l - 2)).any()
        assert reads_last or reach < 6, reach
    assert len(scene["skirt"]) > 100


def test_twin_at_level_0_is_the_plain_twins(oracle_mod):
    """A selection with every node at level 0: the composed twin equals the two full-resolution twins block for block."""
    S = scene_samples()
    nodes = select("inside", 1024.0)
    assert (nodes[:, 3] == 0).all() and len(nodes) == (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
    records, _, _ = oracle_mod.extract_tiles(lod_twin.node_tiles(S, nodes))
    block, pos, nrm = twin.soup_vertices(records)
    assert len(pos) > 5000
    assert np.array_equal(twin.lattice(S, 0), S)
    layer = layer_of(1)
    assert np.array_equal(twin.vertex_materials(layer, DIMS, nodes, block, pos), material_twin.vertex_weights(layer, DIMS, nodes[block, :3] // 8, pos))
    radius, steps = AO_CASES[2]
    assert np.array_equal(twin.vertex_ao(S, nodes, block, pos, nrm, radius, SCALE, STRENGTH, steps),
                          ao_twin.vertex_ao(S, nodes[block, :3] // 8, pos, nrm, radius, SCALE, STRENGTH, steps))


def test_twin_skirt_corners_carry_a_mesh_vertex_of_their_node(scene):
    """Every skirt corner's value is that of a mesh vertex of the same node with bitwise the same position and normal -- for the displaced
    corners, the position and normal of the vertex they were displaced from."""
    S, nodes, records, skirt = scene["S"], scene["nodes"], scene["records"], scene["skirt"]
    layer = layer_of(3)
    radius, steps = AO_CASES[2]
    block, pos, nrm = twin.soup_vertices(records)
    mesh = {MATERIAL: twin.vertex_materials(layer, DIMS, nodes, block, pos), AO: twin.vertex_ao(S, nodes, block, pos, nrm, radius, SCALE, STRENGTH, steps)[:, None]}
    corners = {MATERIAL: twin.skirt_materials(layer, DIMS, nodes, skirt), AO: twin.skirt_ao(S, nodes, skirt, radius, SCALE, STRENGTH, steps)[:, None]}
    key = lambda b, p, n: (int(b),) + tuple(bits(p).tolist()) + tuple(bits(n).tolist())       # noqa: E731
    by_vertex = {key(b, p, n): i for i, (b, p, n) in enumerate(zip(block, pos, nrm))}
    first = skirt[0::2]
    source = {0: ("p0", "n0"), 1: ("p1", "n1")}                                                 # b and a of record 2q
    assert len(corners[AO]) == 3 * len(skirt) == 6 * len(first)
    for q in range(len(first)):
        for c in range(6):
            pk, nk = source[twin.SKIRT_SOURCE[c]]
            i = by_vertex[key(first["block"][q], first[pk][q], first[nk][q])]
            for attr in (MATERIAL, AO):
                assert np.array_equal(corners[attr][6 * q + c], mesh[attr][i]), (q, c, attr)
    assert twin.SKIRT_SOURCE == (0, 1, 1, 0, 1, 0)
    # the displaced corners a', b' themselves were never evaluated: their own positions are no vertex of the mesh
    moved = (first["p2"] != first["p1"]).any(axis=1)
    assert moved.sum() > 50 and not any(key(first["block"][q], first["p2"][q], first["n2"][q]) in by_vertex for q in np.nonzero(moved)[0])


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
HIP = None


def hip():
    global HIP
    if HIP is None:
        HIP = ctypes.CDLL("libamdhip64.so")
        HIP.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        HIP.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return HIP


def poison_values(ex):
    """Overwrites every value buffer the layer holds for the current result with POISON bytes on the device -- as many bytes as the context
    has ever held there, the buffers grow only -- so that a pass which leaves a byte unwritten cannot find an earlier pass's there."""
    seen = ex.__dict__.setdefault("_poisoned_lodattr", {})
    for attr, width in ((MATERIAL, 8), (AO, 1)):
        for target in (MESH, SKIRTS):
            try:
                p, n = ex.device_lod_attributes(attr, target)
            except vt.VtmcError:
                continue
            size = seen[attr, target] = max(seen.get((attr, target), 0), n * width)
            if p and size:
                assert hip().hipMemset(p, POISON, size) == 0
    assert hip().hipDeviceSynchronize() == 0


def routes(ex, direct_max=-2):
    c = (ctypes.c_uint32 * 2)()
    assert ex._L.vtmc_debug_lodattr_routes(ex._h, ctypes.byref(c), direct_max) == _lib.OK
    return c[0], c[1]


def geometry(ex, indexed):
    """(block, positions, normals) of the vertices of the result the context holds, in the order of its values."""
    if indexed:
        verts, _, voffs, _ = ex.read_indexed_mesh()
        return twin.indexed_vertices(verts, voffs)
    return twin.soup_vertices(ex.read_triangles()[0])


@pytest.fixture(scope="module")
def world():
    ex = vt.Extractor(0)
    ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
    S = scene_samples()
    ex.terrain_write_samples(S)
    assert np.array_equal(bits(ex.terrain_read_samples()), bits(S))
    yield dict(ex=ex, S=S)
    ex.close()


@pytest.fixture
def ex(world):
    e = world["ex"]
    yield e
    e.set_output_mode(False)
    routes(e, -1)
    assert e._L.vtmc_debug_lodattr_skirts_in_node(e._h, 1) == _lib.OK                         # the library's choice


def paint_layer(ex, fineness):
    C = ex.material_init(fineness)
    for group in (1, 2):
        ex.set_control_map(control_map(C, group), group)
    layer = ex.material_read()
    assert np.array_equal(layer, layer_of(fineness))
    return layer


def extract(ex, indexed, all_faces=False, name="corner", split=1.0):
    ex.set_output_mode(indexed)
    n_nodes, T = ex.terrain_extract_lod(world_of(VIEWERS[name]), MAX_LEVEL, split)
    nodes = ex.terrain_lod_nodes()
    n_skirt = ex.lod_skirts(DEPTH, all_faces)
    return nodes, T, ex.lodskirt_read()[0], n_skirt


def assert_equal_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d values differ, first at %d: %s != %s" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("indexed,fineness,reach,all_faces", [(False, 1, 1, False), (False, 3, 2, True), (False, 1, 6, False),
                                                              (True, 3, 1, True), (True, 1, 2, False), (True, 3, 6, True)],
                         ids=lambda v: str(v))
def test_gpu_mesh_and_skirts_equal_the_twin(ex, world, indexed, fineness, reach, all_faces):
    """Both attributes, both targets, whole buffers, after poisoning what an earlier case left there.  At reach 6 the 22-sample tile is
    wider than the whole 18 x 10 x 10 lattice of level 2: both clamps act on both sides."""
    S = world["S"]
    radius, steps = AO_CASES[reach]
    layer = paint_layer(ex, fineness)
    nodes, T, skirt, n_skirt = extract(ex, indexed, all_faces)
    assert T > 1000 and n_skirt > 100 and sorted(set(nodes[:, 3].tolist())) == [0, 1, 2]
    block, pos, nrm = geometry(ex, indexed)
    want = {(MATERIAL, MESH): twin.vertex_materials(layer, DIMS, nodes, block, pos), (MATERIAL, SKIRTS): twin.skirt_materials(layer, DIMS, nodes, skirt),
            (AO, MESH): twin.vertex_ao(S, nodes, block, pos, nrm, radius, SCALE, STRENGTH, steps),
            (AO, SKIRTS): twin.skirt_ao(S, nodes, skirt, radius, SCALE, STRENGTH, steps)}
    level = nodes[block, 3]
    print("%s, fineness %d, reach %d, steps %d: %d vertices, %d skirt corners; bytes != 255 per level %s" %
          ("indexed" if indexed else "soup", fineness, reach, steps, len(pos), 3 * n_skirt, [int((want[AO, MESH][level == lv] != 255).sum()) for lv in range(3)]))
    ex.lod_material_vertices(), ex.lod_ao_vertices(vt.AmbientOcclusion(radius, STRENGTH, steps))   # so that there is something to poison
    poison_values(ex)
    assert ex.lod_material_vertices() == (len(pos), 3 * n_skirt) == ex.lodattr_info(MATERIAL)
    assert ex.lod_ao_vertices(vt.AmbientOcclusion(radius, STRENGTH, steps)) == (len(pos), 3 * n_skirt) == ex.lodattr_info(AO)
    staged, direct = routes(ex)
    assert staged > 0 and direct > 0 and staged + direct == int((np.bincount(block, minlength=len(nodes)) > 0).sum())
    for (attr, target), w in want.items():
        assert_equal_bytes(ex.lodattr_read(attr, target), w, (attr, target))
    assert np.array_equal(ex.lod_skirt_materials(), want[MATERIAL, SKIRTS]) and np.array_equal(ex.lod_skirt_ao(), want[AO, SKIRTS])
    # the device pointers hold the same bytes
    for (attr, target), w in want.items():
        p, n = ex.device_lod_attributes(attr, target)
        back = np.zeros_like(w)
        assert n == len(w) and hip().hipMemcpy(back.ctypes.data, p, back.nbytes, 2) == 0 and back.tobytes() == w.tobytes()
    # the extract's result and the skirts are byte for byte what they were
    assert ex.lodskirt_read()[0].tobytes() == skirt.tobytes() and ex.last_counts() == (len(nodes), T)


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
def test_gpu_routes_write_the_same_bytes(ex, world, indexed):
    """direct_max forced to 0 (every node stages a tile) and above every node's count (every node reads the grid): equal to each other
    and to the twin, the counters show the route taken; the same with the skirt quads in a pass of their own."""
    S = world["S"]
    radius, steps = AO_CASES[6]
    nodes, T, skirt, n_skirt = extract(ex, indexed)
    block, pos, nrm = geometry(ex, indexed)
    want = twin.vertex_ao(S, nodes, block, pos, nrm, radius, SCALE, STRENGTH, steps)
    want_skirt = twin.skirt_ao(S, nodes, skirt, radius, SCALE, STRENGTH, steps)
    non_empty = int((np.bincount(block, minlength=len(nodes)) > 0).sum())
    ex.lod_ao_vertices(vt.AmbientOcclusion(radius, STRENGTH, steps))
    for in_node in (1, 0):
        assert ex._L.vtmc_debug_lodattr_skirts_in_node(ex._h, in_node) == _lib.OK
        for direct_max, expect in ((0, (non_empty, 0)), (1 << 30, (0, non_empty))):
            routes(ex, direct_max)
            poison_values(ex)
            assert ex.lod_ao_vertices(vt.AmbientOcclusion(radius, STRENGTH, steps)) == (len(pos), 3 * n_skirt)
            assert routes(ex) == expect, (in_node, direct_max)
            assert_equal_bytes(ex.lodattr_read(AO, MESH), want, ("mesh", in_node, direct_max))
            assert_equal_bytes(ex.lodattr_read(AO, SKIRTS), want_skirt, ("skirts", in_node, direct_max))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
def test_gpu_level_0_is_the_full_resolution_rule(indexed):
    """No twin involved: a level-of-detail result with every node at level 0 against vertex_materials() / vertex_ao() of a second context
    that holds the same samples and a result of every block of its dirty list; matched per block by cell origin, the byte sequences of a
    block are equal."""
    radius, steps = AO_CASES[2]
    with vt.Extractor(0) as flat, vt.Extractor(0) as lod:
        for e in (flat, lod):
            e.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
            e.set_output_mode(indexed)
        flat.terrain_write_samples(scene_samples())
        n_dirty, T = flat.terrain_update(full_world()[-1:])                                    # the noise modifier spans the terrain: every block is dirty
        assert n_dirty == (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8) and T > 1000
        S = flat.terrain_read_samples()
        lod.terrain_write_samples(S)
        assert np.array_equal(bits(lod.terrain_read_samples()), bits(S))
        for e in (flat, lod):
            paint_layer(e, 3)
        n_nodes, T_lod = lod.terrain_extract_lod(world_of(VIEWERS["inside"]), MAX_LEVEL, 1024.0)
        nodes = lod.terrain_lod_nodes()
        assert (nodes[:, 3] == 0).all() and n_nodes == n_dirty and T_lod == T
        assert lod.lod_skirts(DEPTH) == 0
        flat_blocks = flat.terrain_dirty_blocks()
        assert not np.array_equal(nodes[:, :3], 8 * flat_blocks)                               # depth-first against x-fastest: the orders differ
        offs = {e: np.asarray(e.read_indexed_mesh()[2] if indexed else 3 * e.read_triangles()[1], np.int64) for e in (flat, lod)}
        got = {MATERIAL: lod.lod_vertex_materials(), AO: lod.lod_vertex_ao(radius, STRENGTH, steps)}
        assert lod.lodattr_info(AO) == (len(got[AO]), 0) and len(lod.lod_skirt_ao()) == 0 and lod.lod_skirt_materials().shape == (0, 8)
        want = {MATERIAL: flat.vertex_materials(), AO: flat.vertex_ao(radius, STRENGTH, steps)}
        assert len(set(want[AO].tolist())) > 50 and len(np.unique(want[MATERIAL], axis=0)) > 1000
        where = {tuple(o): i for i, o in enumerate((8 * flat_blocks).tolist())}
        for i, node in enumerate(nodes[:, :3].tolist()):
            j = where[tuple(node)]
            for attr in (MATERIAL, AO):
                a, b = got[attr][offs[lod][i]:offs[lod][i + 1]], want[attr][offs[flat][j]:offs[flat][j + 1]]
                assert a.tobytes() == b.tobytes(), (i, j, attr)


@pytest.mark.gpu
def test_gpu_life_cycle_and_refusals(ex):
    L, h = ex._L, ex._h
    viewer = world_of(VIEWERS["corner"])
    ao = lambda radius=1.0, strength=1.0, steps=4, flags=0: L.vtmc_lod_ao_vertices(h, ctypes.byref(_lib.AoParams(radius, strength, steps, flags)), None, None)   # noqa: E731
    readers = [lambda a=a, t=t: ex.lodattr_read(a, t) for a in (MATERIAL, AO) for t in (MESH, SKIRTS)]
    readers += [lambda a=a, t=t: ex.device_lod_attributes(a, t) for a in (MATERIAL, AO) for t in (MESH, SKIRTS)]
    with vt.Extractor(0) as fresh:
        no_result(fresh.lod_material_vertices)                                                 # no terrain, no result
        no_result(lambda: fresh.lod_vertex_ao(1.0))
        fresh.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        fresh.terrain_write_samples(scene_samples())
        fresh.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
        no_result(fresh.lod_material_vertices)                                                 # before material_init
        for a in (MATERIAL, AO):
            no_result(lambda: fresh.lodattr_info(a))                                           # a reader before its compute call
            for t in (MESH, SKIRTS):
                no_result(lambda: fresh.lodattr_read(a, t))
                no_result(lambda: fresh.device_lod_attributes(a, t))
        n = fresh.lod_ao_vertices(vt.AmbientOcclusion(1.0))                                    # occlusion works without material_init ...
        assert n == (3 * fresh.last_counts()[1], 0) == fresh.lodattr_info(AO)                 # ... and without skirts the skirt target is empty
        no_result(fresh.lod_skirt_ao)
        no_result(lambda: fresh.lodattr_info(MATERIAL))                                        # neither attribute stands in for the other
        no_result(fresh.vertex_materials), no_result(lambda: fresh.vertex_ao(1.0)), no_result(fresh.material_vertices)   # the old entry points refuse as before
        fresh.material_init(1)
        assert fresh.lod_material_vertices() == n and len(fresh.lodattr_read(AO, MESH)) == n[0]
        no_result(fresh.vertex_materials), no_result(lambda: fresh.vertex_ao(1.0))
        n_dirty, _ = fresh.terrain_update([vt.SphereModifier((8.0, 6.5, 9.0), 1.75, False)])
        assert n_dirty > 0
        no_result(fresh.lod_material_vertices), no_result(lambda: fresh.lod_vertex_ao(1.0))   # the result is the dirty list's
        for a in (MATERIAL, AO):
            no_result(lambda: fresh.lodattr_info(a)), no_result(lambda: fresh.lodattr_read(a, MESH))
        assert len(fresh.vertex_materials()) == len(fresh.vertex_ao(1.0)) > 0                  # ... and the old entry points answer for it
    paint_layer(ex, 1)
    ex.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
    n_skirt = ex.lod_skirts(DEPTH)
    counts = ex.lod_material_vertices()
    assert counts == ex.lod_ao_vertices(vt.AmbientOcclusion(1.0, 0.75, 3)) == (3 * ex.last_counts()[1], 3 * n_skirt)
    before = [ex.lodattr_read(a, t) for a in (MATERIAL, AO) for t in (MESH, SKIRTS)]
    unchanged = lambda: all(np.array_equal(ex.lodattr_read(a, t), b) for (a, t), b in zip([(a, t) for a in (MATERIAL, AO) for t in (MESH, SKIRTS)], before))   # noqa: E731
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(radius=3.01), dict(strength=-0.1), dict(strength=1.5),
                dict(strength=nan), dict(steps=0), dict(steps=9), dict(flags=1)):
        assert ao(**bad) == _lib.ERR_INVALID_ARG and unchanged(), bad                         # ao_params_fault's faults keep the previous values
    assert L.vtmc_lod_ao_vertices(h, None, None, None) == _lib.ERR_INVALID_ARG and unchanged()
    buf = np.zeros((counts[0], 8), np.uint8)
    for attr, target in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert L.vtmc_lodattr_read(h, attr, target, buf.ctypes.data, counts[0]) == _lib.ERR_INVALID_ARG
        assert L.vtmc_lodattr_device_results(h, attr, target, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodattr_info(h, 2, None, None) == _lib.ERR_INVALID_ARG
    for attr in (AO, MATERIAL):                                                                # the weights last: buf then holds them
        assert L.vtmc_lodattr_read(h, attr, MESH, buf.ctypes.data, counts[0] - 1) == _lib.ERR_INVALID_ARG
        assert L.vtmc_lodattr_read(h, attr, SKIRTS, buf.ctypes.data, counts[1] - 1) == _lib.ERR_INVALID_ARG
        assert L.vtmc_lodattr_read(h, attr, MESH, None, counts[0]) == _lib.ERR_INVALID_ARG
        assert L.vtmc_lodattr_read(h, attr, MESH, buf.ctypes.data, counts[0]) == _lib.OK
    assert np.array_equal(buf, before[0]) and unchanged()
    # the layer's values are its own: the old buffers hold nothing, the old entry points refuse
    no_result(ex.vertex_materials), no_result(lambda: ex.vertex_ao(1.0)), no_result(ex.material_device_results), no_result(ex.device_ao)
    # lod_skirts after a compute call drops only the skirt target, of both attributes
    assert ex.lod_skirts(DEPTH, True) > n_skirt
    for a in (MATERIAL, AO):
        assert ex.lodattr_info(a) == (counts[0], 0) and np.array_equal(ex.lodattr_read(a, MESH), before[2 * a])
        no_result(lambda: ex.lodattr_read(a, SKIRTS)), no_result(lambda: ex.device_lod_attributes(a, SKIRTS))
    # a refused lod_skirts keeps the skirts and so the values of their corners
    assert ex.lod_ao_vertices(vt.AmbientOcclusion(1.0, 0.75, 3))[1] == 3 * ex.lodskirt_info()[2]
    assert L.vtmc_lod_skirts(h, ctypes.byref(_lib.LodSkirtParamsStruct(0.0, 0)), None) == _lib.ERR_INVALID_ARG
    assert len(ex.lod_skirt_ao()) == 3 * ex.lodskirt_info()[2]
    no_result(ex.lod_skirt_materials)                                                          # only the occlusion was computed again
    # any later extract makes all of them stale
    ex.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
    for reader in readers:
        no_result(reader)
    for a in (MATERIAL, AO):
        no_result(lambda: ex.lodattr_info(a))
    assert ex.lod_material_vertices() == (counts[0], 0) and np.array_equal(ex.lodattr_read(MATERIAL, MESH), before[0])
    g = np.full((10, 10, 10), -1.0, f32)
    g[3:6, 3:6, 3:6] = 1.0
    assert ex.extract_grid(g) > 0
    no_result(ex.lod_material_vertices), no_result(lambda: ex.lod_vertex_ao(1.0))
    for reader in readers:
        no_result(reader)


@pytest.mark.gpu
def test_gpu_terrain_events_make_the_values_stale_and_an_empty_result_is_success(tmp_path):
    viewer = world_of(VIEWERS["corner"])
    with vt.Extractor(0) as e:
        e.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        e.terrain_set_history(1 << 24)
        e.terrain_write_samples(scene_samples())
        e.material_init(1)

        def shade():
            e.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
            e.lod_skirts(DEPTH)
            assert e.lod_material_vertices() == e.lod_ao_vertices(vt.AmbientOcclusion(1.0)) and e.lodattr_info(AO)[1] > 0

        def stale():
            for a in (MATERIAL, AO):
                no_result(lambda: e.lodattr_info(a))
                for t in (MESH, SKIRTS):
                    no_result(lambda: e.lodattr_read(a, t))

        shade()
        e.terrain_update([vt.SphereModifier((8.0, 6.5, 9.0), 1.75, False)])
        stale()
        shade()
        e.terrain_undo()
        stale()
        shade()
        e.terrain_redo()
        stale()
        shade()
        path = tmp_path / "world.vtt"
        e.terrain_save(str(path))
        e.terrain_load(str(path))
        stale()
        e.material_init(1)
        shade()
        e.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        stale()
        # all air, the viewer far away: two roots, no triangle -- success with 0 vertices
        e.terrain_write_samples(np.full(tuple(d + 2 for d in DIMS), -1.0, f32))
        e.material_init(1)
        for indexed in (False, True):
            e.set_output_mode(indexed)
            assert e.terrain_extract_lod(world_of(VIEWERS["far"]), MAX_LEVEL, 1.0) == (2, 0)
            assert e.lod_material_vertices() == (0, 0) == e.lod_ao_vertices(vt.AmbientOcclusion(1.0))
            assert e.lod_vertex_materials().shape == (0, 8) and len(e.lod_vertex_ao(1.0)) == 0
            no_result(e.lod_skirt_ao)
            assert e.lod_skirts(DEPTH) == 0
            assert e.lod_ao_vertices(vt.AmbientOcclusion(1.0)) == (0, 0) and len(e.lod_skirt_ao()) == 0   # skirts exist and are empty
