"""Skirt triangles over the seams of a level-of-detail extract (vtmc_lod_skirts / vtmc_lodskirt_*, include/vtmc_lodskirt.h).

The rule LODSKIRT is restated in numpy by lodskirt_twin.py.  On the CPU the twin runs on the CPU oracle's meshes of the twin's tiles
(lod_twin.node_tiles -> oracle.extract_tiles): its masks against a brute-force restatement over lod_twin.level_map, the properties of its
records, and the closure walk -- between the boundary curves of a fine and a coarse node on their shared face every point must lie inside
a skirt triangle.  On the GPU the twin is fed the device's own records, so masks, counts, offsets, `block`, the copied positions and all
normals must be EQUAL and the displaced positions agree within the project's 1e-5.

The scene is set from samples, so twin and device start from the same bits: test_terrain_lod's 64 x 32 x 32 cells with roots of level 2,
S = min(h - y, |p - (20, 10, 16)| - 6) with h = 14 + 5 sin(0.23 x) cos(0.31 z) + 3 sin(0.11 x + 0.4 z), evaluated in float64."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import lod_twin
import lodskirt_twin as twin
from host_check import run_host_check
from lod_support import (assert_skirts_match_the_twin, bits, brute_masks, check_closure, check_skirt_properties, device_records, interior_masks,
                         poison_skirts)
from terrain_twin import no_result
from test_terrain_lod import CASES, DIMS, MAX_LEVEL, ORIGIN, SCALE, SEED, VIEWERS, select, world_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DEPTH = 1.0
FLOATS = ("p0", "p1", "p2", "n0", "n1", "n2")


def scene_samples():
    x, y, z = np.meshgrid(*(np.arange(d + 2, dtype=np.float64) for d in DIMS), indexing="ij")
    h = 14.0 + 5.0 * np.sin(0.23 * x) * np.cos(0.31 * z) + 3.0 * np.sin(0.11 * x + 0.4 * z)
    ball = np.sqrt((x - 20.0) ** 2 + (y - 10.0) ** 2 + (z - 16.0) ** 2) - 6.0
    return np.minimum(h - y, ball).astype(f32)


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_struct_the_flag_and_the_rule():
    path = os.path.join(ROOT, "include", "vtmc_lodskirt.h")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert re.search(r"#define\s+VTMC_LODSKIRT_ALL_FACES\s+1u", text) and _lib.LODSKIRT_ALL_FACES == 1 == twin.ALL_FACES and _lib.LODSKIRT_MAX_DEPTH == 8
    body = re.search(r"typedef struct vtmc_lodskirt_params \{(.*?)\} vtmc_lodskirt_params;", text, re.S)
    assert [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()] == ["float depth", "uint32_t flags"]
    assert list(_lib.LAYER_SYMBOLS["lodskirt"]) == ["vtmc_lod_skirts", "vtmc_lodskirt_info", "vtmc_lodskirt_masks", "vtmc_lodskirt_read", "vtmc_lodskirt_device_results"]
    whole = " ".join(open(path).read().split())
    for word in ("LODSKIRT", "Flagged", "bitwise equal", "correctly rounded", "(b, a, a')", "(b, a', b')", "node_offsets", "VTMC_ERR_TOO_LARGE"):
        assert word in whole, word
    for doc in ("include/vtmc.h", "DESIGN.md", "README.md", "INTEGRATION.md", "LODSEAMS.md"):
        assert "vtmc_lod_skirts" in open(os.path.join(ROOT, doc)).read(), doc


def test_mirror_struct_layout_and_what_it_rejects_by_value():
    P = _lib.LodSkirtParamsStruct
    assert ctypes.sizeof(P) == 8 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("depth", 0), ("flags", 4)]
    s = vt.LodSkirtParams(0.75, True).to_struct()
    assert (s.depth, s.flags) == (0.75, 1)
    s = vt.LodSkirtParams().to_struct()
    assert (s.depth, s.flags) == (1.0, 0)
    vt.LodSkirtParams(8.0)
    for bad in (0.0, -1.0, 8.5, 9.0, np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError):
            vt.LodSkirtParams(bad)


def test_null_pointers_are_errors_not_crashes():
    L = vt.load()
    p, n = _lib.LodSkirtParamsStruct(1.0, 0), ctypes.c_int64()
    assert L.vtmc_lod_skirts(None, ctypes.byref(p), ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lod_skirts(None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodskirt_info(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodskirt_masks(None, None, 0) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodskirt_read(None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_lodskirt_device_results(None, None, None, None) == _lib.ERR_INVALID_ARG


# -- CPU: the masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,split", CASES, ids=["%s-split%g" % c for c in CASES])
def test_twin_masks_equal_the_brute_force(name, split):
    nodes = select(name, split)
    for all_faces in (False, True):
        assert np.array_equal(twin.face_masks(DIMS, nodes, all_faces), brute_masks(DIMS, nodes, all_faces)), (name, split, all_faces)
    assert np.array_equal(twin.face_masks(DIMS, nodes, True), interior_masks(DIMS, nodes))    # ALL_FACES: exactly the interior faces


def test_twin_known_masks():
    for name in VIEWERS:
        if name != "far":
            nodes = select(name, 1024.0)                                                         # every node level 0: no face is flagged
            assert (nodes[:, 3] == 0).all() and not twin.face_masks(DIMS, nodes).any()
            assert np.array_equal(twin.face_masks(DIMS, nodes, True), interior_masks(DIMS, nodes))
    roots = select("far", 1.0)                                                                   # two roots: nothing, and their shared face
    assert twin.face_masks(DIMS, roots).tolist() == [0, 0] and twin.face_masks(DIMS, roots, True).tolist() == [2, 1]
    nodes = select("corner", 1.0)
    masks = twin.face_masks(DIMS, nodes)
    assert masks[-1] == 1 and masks[8] & 2                                                       # the far root towards the near one's children, and back
    assert sorted(set(nodes[masks != 0, 3].tolist())) == [0, 1, 2]


# -- CPU: the twin on the oracle's meshes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle_mod):
    """Viewer (-1, 3, 5) cells, split 1: nodes of levels 0, 1 and 2.  The oracle's records of the twin's tiles and the twin's skirts."""
    S = scene_samples()
    nodes = select("corner", 1.0)
    assert sorted(set(nodes[:, 3].tolist())) == [0, 1, 2]
    records, offs, _ = oracle_mod.extract_tiles(lod_twin.node_tiles(S, nodes))
    masks = twin.face_masks(DIMS, nodes)
    skirt, node_offsets, faces = twin.skirts(records, masks, DEPTH)
    return dict(S=S, nodes=nodes, records=records, offs=offs, masks=masks, skirt=skirt, node_offsets=node_offsets, faces=faces)


def test_twin_properties(scene):
    skirt, faces, records = scene["skirt"], scene["faces"], scene["records"]
    quads, with_edge, inwards = check_skirt_properties(skirt, faces, DEPTH)
    print("twin: %d quads, %d with a source edge, %d second triangles face inwards" % (quads, with_edge, inwards))
    # the records: `block` travels, normals travel with their positions, offsets count the records of the nodes before
    assert np.array_equal(np.diff(scene["node_offsets"]), np.bincount(skirt["block"], minlength=len(scene["nodes"])))
    assert (np.diff(skirt["block"]) >= 0).all() and scene["node_offsets"][-1] == len(skirt)
    assert not np.diff(scene["node_offsets"])[scene["masks"] == 0].any()                         # an unflagged node has no skirt
    first, second = skirt[0::2], skirt[1::2]
    assert first["n1"].tobytes() == first["n2"].tobytes() == second["n1"].tobytes() and first["n0"].tobytes() == second["n0"].tobytes() == second["n2"].tobytes()
    # every quad's source edge is an edge of a triangle of its node with exactly two corners on the face
    tmask = twin.triangle_masks(records, scene["masks"])
    assert np.array_equal(np.bincount(records["block"], weights=[bin(m).count("1") for m in tmask], minlength=len(scene["nodes"])) * 2, np.diff(scene["node_offsets"]))
    # a flat normal moves nothing; a normal along the face axis alone moves nothing either
    P = np.array([[0.0, 3.0, 4.0]], f32)
    assert np.array_equal(twin.displace(P, np.array([[5.0, 0.0, 0.0]], f32), 0, 1.0), P)
    assert np.array_equal(twin.displace(P, np.array([[np.nan, np.nan, np.nan]], f32), 0, 1.0), P)
    assert np.array_equal(twin.displace(P, np.array([[0.0, 3e38, 3e38]], f32), 0, 1.0), P)       # l2 overflows
    assert np.array_equal(twin.displace(P, np.array([[9.0, 0.0, -2.0]], f32), 0, 1.5), np.array([[0.0, 3.0, 5.5]], f32))


def test_twin_skirts_close_the_seams(scene):
    check_closure(scene["nodes"], scene["records"], scene["masks"], scene["skirt"], DEPTH)


def test_host_check_runs_clean_under_the_host_sanitizers_and_agrees_with_the_twin(tmp_path):
    """tools/lodskirt_host_check.cpp: the host half (csrc/terrain_lodskirt.h) as a stand-alone program under ASan and UBSan, on the CPU:
    its own known answers, then the masks of the node lists of every case, with and without ALL_FACES, which must equal the twin's."""
    cases = [(name, split, flags) for name, split in CASES for flags in (0, 1)] + [("inside", 1024.0, 0), ("inside", 1024.0, 1)]
    args = []
    for name, split, flags in cases:
        nodes = select(name, split)
        args += [str(d) for d in DIMS] + [str(flags), str(len(nodes))] + [str(v) for v in nodes.ravel().tolist()]
    run = run_host_check("lodskirt_host_check", tmp_path, args)
    chunks = re.split(r"^case \d+ ", run.stdout, flags=re.M)[1:]
    assert len(chunks) == len(cases)
    for (name, split, flags), chunk in zip(cases, chunks):
        status, _, body = chunk.partition("\n")
        assert status == "ok", (name, split, flags)
        assert np.array_equal(np.array(body.split(), np.int64), twin.face_masks(DIMS, select(name, split), bool(flags))), (name, split, flags)


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
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
    e.set_tuning(emit_fast_math=1)
    assert e._L.vtmc_debug_lodskirt_store(e._h, 0) == _lib.OK


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast_math", "exact"])
def test_gpu_skirts_equal_the_twin(ex, oracle_mod, indexed, exact):
    nodes = select("corner", 1.0)
    ex.set_tuning(emit_fast_math=0 if exact else 1)
    ex.set_output_mode(indexed)
    n_nodes, T = ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
    assert n_nodes == len(nodes) and np.array_equal(ex.terrain_lod_nodes(), nodes) and T > 1000
    before = ex.read_indexed_mesh() if indexed else ex.read_triangles()
    records, got, masks, differ = assert_skirts_match_the_twin(ex, oracle_mod, DIMS, nodes, indexed, DEPTH)
    print("%s, %s: %d triangles, %d skirt records, displaced components whose bits differ from the twin's: %d"
          % ("indexed" if indexed else "soup", "exact" if exact else "fast math", T, len(got), differ))
    quads, with_edge, inwards = check_skirt_properties(got, twin.quad_faces(got), DEPTH)
    print("device: %d quads, %d with a source edge, %d second triangles face inwards" % (quads, with_edge, inwards))
    # the extract's own result is byte for byte what it was
    after = ex.read_indexed_mesh() if indexed else ex.read_triangles()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and ex.last_counts() == (n_nodes, T)
    # the staged store variant writes the same bytes and the same offsets
    direct_offsets = ex.lodskirt_read()[1]
    poison_skirts(ex)                                                    # the staged pass must write every byte, not find them there
    assert ex._L.vtmc_debug_lodskirt_store(ex._h, 1) == _lib.OK
    assert ex.lod_skirts(DEPTH) == len(got)
    staged, staged_offsets = ex.lodskirt_read()
    assert staged.tobytes() == got.tobytes() and np.array_equal(staged_offsets, direct_offsets)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["corner", "inside", "on_a_face"])
@pytest.mark.parametrize("split", [1.0, 2.0])
def test_gpu_viewers_and_splits(ex, oracle_mod, name, split):
    nodes = select(name, split)
    ex.terrain_extract_lod(world_of(VIEWERS[name]), MAX_LEVEL, split)
    _, got, masks, _ = assert_skirts_match_the_twin(ex, oracle_mod, DIMS, nodes, False, 0.75)
    assert (len(got) > 0) == bool(masks.any()) == bool((nodes[:, 3] > 0).any())                # on_a_face at split 2 is all level 0: no skirts
    # a flagged node without a triangle is handled: its range of the offsets is empty
    offs = ex.read_triangles()[1]
    empty_flagged = (masks != 0) & (np.diff(offs) == 0)
    print("%s split %g: %d nodes, %d flagged, %d of them without a triangle, %d skirt records" % (name, split, len(nodes), (masks != 0).sum(), empty_flagged.sum(), len(got)))
    assert not np.diff(ex.lodskirt_read()[1])[empty_flagged].any()


@pytest.mark.gpu
def test_gpu_all_faces_and_flagged_nodes_without_triangles(ex, oracle_mod):
    nodes = select("inside", 2.0)
    ex.terrain_extract_lod(world_of(VIEWERS["inside"]), MAX_LEVEL, 2.0)
    _, plain, masks, _ = assert_skirts_match_the_twin(ex, oracle_mod, DIMS, nodes, False, DEPTH)
    _, every, all_masks, _ = assert_skirts_match_the_twin(ex, oracle_mod, DIMS, nodes, False, DEPTH, all_faces=True)
    assert len(every) > len(plain) and (all_masks & masks == masks).all() and (all_masks != 0).all()
    offs = ex.read_triangles()[1]
    assert ((all_masks != 0) & (np.diff(offs) == 0)).any()                                       # some flagged node has no triangles
    # the same in indexed mode, with the staged stores
    ex.set_output_mode(True)
    ex.terrain_extract_lod(world_of(VIEWERS["inside"]), MAX_LEVEL, 2.0)
    assert ex._L.vtmc_debug_lodskirt_store(ex._h, 1) == _lib.OK
    assert_skirts_match_the_twin(ex, oracle_mod, DIMS, nodes, True, DEPTH, all_faces=True)


@pytest.mark.gpu
def test_gpu_skirts_close_the_seams(ex, oracle_mod):
    nodes = select("corner", 1.0)
    ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
    records = device_records(ex, oracle_mod, False)
    ex.lod_skirts(DEPTH)
    got, _ = ex.lodskirt_read()
    check_closure(nodes, records, ex.lodskirt_masks(), got, DEPTH)
    # the world mapping is the node's own
    pos = ex.lod_world_positions(nodes, got["block"], got["p2"])
    lo = np.array(ORIGIN) + (nodes[got["block"], :3] - DEPTH * (1 << nodes[got["block"], 3])[:, None] - 1e-3) * SCALE
    hi = np.array(ORIGIN) + (nodes[got["block"], :3] + (8 + DEPTH) * (1 << nodes[got["block"], 3])[:, None] + 1e-3) * SCALE
    assert (pos >= lo).all() and (pos <= hi).all()


@pytest.mark.gpu
def test_gpu_all_level_0_and_device_pointers(ex):
    n_nodes, T = ex.terrain_extract_lod(world_of(VIEWERS["inside"]), MAX_LEVEL, 1e6)
    assert T > 0 and (ex.terrain_lod_nodes()[:, 3] == 0).all()
    assert ex.lod_skirts(DEPTH) == 0 and ex.lodskirt_info() == (n_nodes, 0, 0)
    got, offsets = ex.lodskirt_read()
    assert len(got) == 0 and len(offsets) == n_nodes + 1 and not offsets.any() and not ex.lodskirt_masks().any()
    assert ex.device_lodskirts()[2] == 0
    # the device pointers read back equal to lodskirt_read
    ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
    n = ex.lod_skirts(DEPTH)
    got, offsets = ex.lodskirt_read()
    d_tris, d_offsets, d_n = ex.device_lodskirts()
    assert d_n == n == len(got) > 0 and d_tris and d_offsets
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    back, back_offsets = np.zeros_like(got), np.zeros_like(offsets)
    assert hip.hipMemcpy(back.ctypes.data, d_tris, back.nbytes, 2) == 0 and hip.hipMemcpy(back_offsets.ctypes.data, d_offsets, back_offsets.nbytes, 2) == 0
    assert back.tobytes() == got.tobytes() and np.array_equal(back_offsets, offsets)


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's LodSkirts against the Python path on the same world (host/host_selftest.cpp --gpu-lodskirt)."""
    import subprocess
    from test_host_mirror import TIME_LIMIT, build_host
    from test_terrain_lod import base_world
    r = subprocess.run([build_host(), "--gpu-lodskirt", str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT)
    assert r.returncode == 0 and "HOST-LODSKIRT-OK" in r.stdout, (r.returncode, r.stdout[-600:], r.stderr[-600:])
    counts = np.fromfile(tmp_path / "lodskirt_counts.i32", np.int32)
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_update(base_world())
        n_nodes, T = ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
        n = ex.lod_skirts(1.0)
        offsets = ex.lodskirt_read()[1]
    assert np.array_equal(counts, 3 * np.diff(offsets)) and counts.sum() == 3 * n > 0
    assert ("lodskirt: nodes %d triangles %d skirt triangles %d" % (n_nodes, T, n)) in r.stdout


@pytest.mark.gpu
def test_gpu_state_and_errors(ex):
    L, h = ex._L, ex._h
    call = lambda depth, flags: L.vtmc_lod_skirts(h, ctypes.byref(_lib.LodSkirtParamsStruct(depth, flags)), None)   # noqa: E731
    viewer = world_of(VIEWERS["corner"])
    readers = (ex.lodskirt_info, ex.lodskirt_masks, ex.lodskirt_read, ex.device_lodskirts)
    with vt.Extractor(0) as fresh:                                       # before any level-of-detail extract
        no_result(fresh.lod_skirts)
        fresh.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        no_result(fresh.lod_skirts)
        fresh.terrain_write_samples(scene_samples())
        fresh.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
        for reader in (fresh.lodskirt_info, fresh.lodskirt_masks, fresh.lodskirt_read, fresh.device_lodskirts):
            no_result(reader)                                            # a level-of-detail result, no skirts built for it
        assert fresh.lod_skirts(DEPTH) > 0
        fresh.terrain_update([vt.SphereModifier((8.0, 6.5, 9.0), 1.75, False)])
        no_result(fresh.lod_skirts)                                      # the result is the dirty list's
        for reader in (fresh.lodskirt_info, fresh.lodskirt_masks, fresh.lodskirt_read, fresh.device_lodskirts):
            no_result(reader)
    n_nodes, T = ex.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
    tris_before = ex.read_triangles()
    n = ex.lod_skirts(DEPTH)
    before, before_offsets = ex.lodskirt_read()
    masks_before = ex.lodskirt_masks()

    def unchanged():
        got, offsets = ex.lodskirt_read()
        return (ex.lodskirt_info() == (n_nodes, int((masks_before != 0).sum()), n) and got.tobytes() == before.tobytes() and np.array_equal(offsets, before_offsets)
                and np.array_equal(ex.lodskirt_masks(), masks_before))

    nan, inf = float("nan"), float("inf")
    for depth, flags in ((0.0, 0), (9.0, 0), (nan, 0), (1.0, 2), (-1.0, 0), (inf, 0), (8.000001, 0), (1.0, 3), (1.0, 0x80000000)):
        assert call(depth, flags) == _lib.ERR_INVALID_ARG and unchanged(), (depth, flags)
    assert L.vtmc_lod_skirts(h, None, None) == _lib.ERR_INVALID_ARG and unchanged()
    buf = np.zeros(n, vt.TRI_DTYPE)
    assert L.vtmc_lodskirt_read(h, buf.ctypes.data, n - 1, None) == _lib.ERR_CAPACITY
    assert L.vtmc_lodskirt_masks(h, np.zeros(n_nodes, np.uint8).ctypes.data, n_nodes - 1) == _lib.ERR_CAPACITY
    assert L.vtmc_lodskirt_read(h, buf.ctypes.data, n, None) == _lib.OK and buf.tobytes() == before.tobytes()
    assert call(8.0, 1) == _lib.OK and not unchanged()                   # the largest depth, every face
    after = ex.read_triangles()
    assert after[0].tobytes() == tris_before[0].tobytes() and np.array_equal(after[1], tris_before[1]) and ex.last_counts() == (n_nodes, T)
    # a later extract of any kind drops them
    ex.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
    for reader in readers:
        no_result(reader)
    assert ex.lod_skirts(DEPTH) == n and unchanged()
    g = np.full((10, 10, 10), -1.0, f32)
    g[3:6, 3:6, 3:6] = 1.0
    assert ex.extract_grid(g) > 0
    no_result(ex.lod_skirts)
    for reader in readers:
        no_result(reader)
