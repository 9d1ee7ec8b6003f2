"""Level-of-detail extraction of the resident terrain (vtmc_terrain_extract_lod / vtmc_terrain_lod_nodes).

The front end -- the selection of an octree of nodes around a viewer on the host, and the gather of every node's 10x10x10 tile at stride
2^level on the device -- is compared with lod_twin.py, a numpy restatement of include/vtmc.h's rule; the mesh of the gathered tiles is
compared with the CPU oracle run on the twin's tiles (oracle.extract_tiles), so the oracle stays the yardstick: cases and counts exact,
floats within the project's 1e-5, and equal bits with emit_fast_math = 0.

The terrain is 64 x 32 x 32 cells at scale 0.5 with its origin off zero; every viewer, the scale and every split are dyadic rationals, so
each comparison of the selection is exact in double and the node lists must be EQUAL.  Roots are level 2 (32 cells): two of them."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import lod_twin as twin
from host_check import run_host_check
from extract_checks import FLOATS, assert_tris_match
from lod_support import bits, lod_tiles, oracle_indexed_soup
from terrain_twin import assert_triangles, no_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (64, 32, 32), 0.5, (-3.0, 1.0, 2.0), 977
MAX_LEVEL = 2
N_BLOCKS = (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
SPLITS = (1.0, 1.5, 2.0, 4.0)
# viewers in cells: inside the terrain (twice), outside it (twice), exactly on a face shared by nodes of every level, just outside a corner, far away
VIEWERS = {"inside": (10.25, 5.5, 20.75), "inside_high_x": (40.0, 17.5, 3.0), "outside": (-40.0, 10.0, 10.0),
           "outside_far_corner": (100.5, 50.0, -7.0), "on_a_face": (32.0, 8.0, 16.0), "corner": (-1.0, 3.0, 5.0), "far": (1000.0, 1000.0, 1000.0)}
CASES = [(name, split) for name in VIEWERS for split in SPLITS]


def world_of(cells):
    """The world position of a point given in cells: origin + c * scale, exact for these dyadic values (also as float32)."""
    w = tuple(ORIGIN[k] + cells[k] * SCALE for k in range(3))
    assert all(float(f32(v)) == v for v in w)
    return w


def select(name, split, max_level=MAX_LEVEL):
    return twin.select_nodes(DIMS, ORIGIN, SCALE, world_of(VIEWERS[name]), max_level, split)


# the base world is what host/host_selftest.cpp --gpu-lod builds; the GPU tests add one noise modifier
def base_world():
    return [vt.PlaneModifier(6.3, (-100.0, -100.0), (100.0, 100.0)),
            vt.SphereModifier((27.5, 8.0, 10.0), 4.25, True),      # cells (61, 14, 16), 8.5 cells: crosses the terrain's upper x face
            vt.SphereModifier((5.0, 6.0, 9.0), 3.0, False)]


def full_world():
    return base_world() + [vt.NoiseModifier(seed=11, octaves=3, frequency=0.21, amplitude=2.5, ramp_scale=1.0, ramp_center=6.0,
                                            lower=(-3.0, 1.0, 2.0), upper=(29.0, 17.0, 18.0))]


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_structs_and_the_limit():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vtmc.h")).read(), flags=re.S)
    m = re.search(r"#define\s+VTMC_LOD_MAX_LEVEL\s+(\d+)", text)
    assert m and int(m.group(1)) == 7 == _lib.LOD_MAX_LEVEL == twin.MAX_LEVEL
    for name, want in (("vtmc_lod_params", ["float viewer[3]", "float split", "int32_t max_level", "int32_t max_nodes"]),
                       ("vtmc_lod_node", ["int32_t origin[3]", "int32_t level"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
        assert body, name
        assert [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()] == want


def test_the_documents_state_the_rule_the_order_and_the_seams():
    for doc in ("include/vtmc.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "vtmc_terrain_extract_lod" in text, doc
        assert re.search(r"not stitched", text, re.I), doc
    header = " ".join(open(os.path.join(ROOT, "include", "vtmc.h")).read().split())
    assert "depth-first" in header and "Chebyshev" in header and "differ by at most one level" in header


def test_mirror_struct_layout():
    P, N = _lib.LodParams, _lib.LodNode
    assert ctypes.sizeof(P) == 24 and ctypes.sizeof(N) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("viewer", 0), ("split", 12), ("max_level", 16), ("max_nodes", 20)]
    assert [(n, getattr(N, n).offset) for n, _ in N._fields_] == [("origin", 0), ("level", 12)]
    s = vt.LodParams((1.5, -2.0, 3.25), 3, 1.5, 99).to_struct()
    assert (tuple(s.viewer), s.split, s.max_level, s.max_nodes) == ((1.5, -2.0, 3.25), 1.5, 3, 99)
    s = vt.LodParams((0, 0, 0), 0).to_struct()
    assert (s.split, s.max_nodes) == (2.0, 1 << 18)               # the defaults
    vt.LodParams((0, 0, 0), 7, 1.0, 1)                            # whether the roots divide a terrain is the library's to refuse


@pytest.mark.parametrize("args", [((np.nan, 0, 0), 2), ((0, np.inf, 0), 2), ((0, 0), 2), ((0, 0, 0), 2, 0.5), ((0, 0, 0), 2, np.nan),
                                  ((0, 0, 0), 2, np.inf), ((0, 0, 0), -1), ((0, 0, 0), 8), ((0, 0, 0), 1.5), ((0, 0, 0), 2, 2.0, 0),
                                  ((0, 0, 0), 2, 2.0, -5), ((0, 0, 0), 2, 2.0, 2 ** 31)])
def test_mirror_rejects_what_the_library_rejects_by_value(args):
    with pytest.raises(ValueError):
        vt.LodParams(*args)


def test_null_pointers_are_errors_not_crashes():
    L = vt.load()
    n, t = ctypes.c_int32(), ctypes.c_int32()
    p = _lib.LodParams((0.0, 0.0, 0.0), 2.0, 2, 100)
    buf = np.zeros((4, 4), np.int32)
    assert L.vtmc_terrain_extract_lod(None, ctypes.byref(p), ctypes.byref(n), ctypes.byref(t)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_terrain_extract_lod(None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_terrain_lod_nodes(None, buf.ctypes.data, 4, ctypes.byref(n)) == _lib.ERR_INVALID_ARG


# -- CPU: the twin's selection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,split", CASES, ids=["%s-split%g" % c for c in CASES])
def test_twin_selection_tiles_the_terrain_once_with_two_to_one_faces(name, split):
    nodes = select(name, split)
    assert nodes.dtype == np.int32 and nodes.shape[1] == 4 and len(nodes) >= 2
    assert (twin.coverage(DIMS, nodes) == 1).all()                                   # every cell in exactly one node
    assert ((nodes[:, 3] >= 0) & (nodes[:, 3] <= MAX_LEVEL)).all()
    assert (nodes[:, :3] % (8 << nodes[:, 3])[:, None] == 0).all()                   # origins are multiples of 8 * 2^L
    assert twin.max_face_level_step(DIMS, nodes) <= 1                                # checked, not assumed
    assert sum(8 ** int(lv) for lv in nodes[:, 3]) == N_BLOCKS


def test_twin_known_selections():
    # far away: only the roots, x fastest
    for split in SPLITS:
        assert select("far", split).tolist() == [[0, 0, 0, 2], [32, 0, 0, 2]]
    # split large enough: every node level 0, in depth-first order (child bit 0 = x, 1 = y, 2 = z)
    for name in VIEWERS:
        if name != "far":
            nodes = select(name, 1024.0)
            assert len(nodes) == N_BLOCKS and (nodes[:, 3] == 0).all()
            assert nodes[:9, :3].tolist() == [[0, 0, 0], [8, 0, 0], [0, 8, 0], [8, 8, 0], [0, 0, 8], [8, 0, 8], [0, 8, 8], [8, 8, 8], [16, 0, 0]]
            assert nodes[64].tolist() == [32, 0, 0, 0]                               # the second root's first leaf
    # the viewer just outside the corner, split 1: the far root stays whole (d = 33), the near one splits, of its children those at
    # x = 16 stay (d = 17) and those at x = 0 split
    nodes = select("corner", 1.0)
    assert np.bincount(nodes[:, 3]).tolist() == [32, 4, 1]
    assert nodes[8].tolist() == [16, 0, 0, 1] and nodes[-1].tolist() == [32, 0, 0, 2]
    # exactly on a face: d is 0 for the boxes on both sides, so both split; at distance exactly split * n a node stays (strict <)
    nodes = select("on_a_face", 1.0)
    lv = twin.level_map(DIMS, nodes)
    assert lv[3, 1, 2] == 0 and lv[4, 1, 2] == 0
    c16 = twin.select_nodes(DIMS, ORIGIN, SCALE, world_of((-16.0, 3.0, 5.0)), 2, 1.0)    # d = 16 to the level-1 nodes at x = 0: not below 16
    assert np.bincount(c16[:, 3], minlength=3).tolist() == [0, 8, 1]
    assert twin.select_nodes(DIMS, ORIGIN, SCALE, world_of((-15.5, 3.0, 5.0)), 2, 1.0)[:, 3].min() == 0
    # max_level 0 and 1
    assert len(select("inside", 4.0, 0)) == N_BLOCKS
    assert (twin.coverage(DIMS, select("inside", 1.0, 1)) == 1).all()


def test_twin_tiles(oracle_mod):
    """Level 0 is the block's own tile (the oracle's gather); a coarse tile is the point subsample, and its index 9 is the grid's last
    plane again where it lies past it."""
    rng = np.random.default_rng(5)
    S = rng.normal(size=tuple(d + 2 for d in DIMS)).astype(f32)
    nodes = select("inside", 1024.0)
    assert np.array_equal(twin.node_tiles(S, nodes), oracle_mod.gather_tiles(S, nodes[:, :3] // 8))
    roots = select("far", 1.0)
    T = twin.node_tiles(S, roots).reshape(2, 10, 10, 10)            # [node, k, j, i]
    assert np.array_equal(T[0, :9, :9, :], S[0:40:4, 0:33:4, 0:33:4].transpose(2, 1, 0)[:9, :9, :])
    assert np.array_equal(T[1, :9, :9, :9], S[32:65:4, 0:33:4, 0:33:4].transpose(2, 1, 0))
    assert np.array_equal(T[1, :9, :9, 9], S[65, 0:33:4, 0:33:4].T)                  # 32 + 36 = 68 -> 65
    assert np.array_equal(T[0, 9, :9, :], S[0:40:4, 0:33:4, 33].T) and np.array_equal(T[0, :9, 9, :], S[0:40:4, 33, 0:33:4].T)
    loose = twin.node_tiles(S, roots, clamp=False).reshape(2, 10, 10, 10)
    assert np.array_equal(loose[:, :9, :9, :9], T[:, :9, :9, :9]) and not np.array_equal(loose[1, :9, :9, 9], T[1, :9, :9, 9])


def test_twin_world_positions():
    nodes = np.array([[0, 0, 0, 0], [32, 0, 16, 2]], np.int32)
    got = twin.world_positions(ORIGIN, SCALE, nodes, np.array([0, 1, 1]), np.array([[1.5, 0, 8], [0, 0, 0], [8, 2.5, 1]], f32))
    assert got.tolist() == [[-2.25, 1.0, 6.0], [13.0, 1.0, 10.0], [29.0, 6.0, 12.0]]


def test_host_check_runs_clean_under_the_host_sanitizers_and_agrees_with_the_twin(tmp_path):
    """tools/lod_host_check.cpp: the host half (csrc/terrain_lod.h) as a stand-alone program under ASan and UBSan, on the CPU: its own
    known answers, then the node lists of every case above, which must equal the twin's."""
    cases = [(name, split, MAX_LEVEL) for name, split in CASES] + [("inside", 1024.0, 2), ("inside", 4.0, 0), ("on_a_face", 1.0, 1)]
    args = []
    for name, split, level in cases:
        args += [str(d) for d in DIMS] + [float(v).hex() for v in ORIGIN] + [float(SCALE).hex()] + [float(v).hex() for v in world_of(VIEWERS[name])]
        args += [str(level), float(split).hex(), str(1 << 18)]
    args += [str(d) for d in DIMS] + ["0"] * 3 + ["1"] + ["0"] * 3 + ["2", "1", "1"]          # two roots, max_nodes 1
    args += [str(d) for d in DIMS] + ["0"] * 3 + ["1"] + ["0"] * 3 + ["3", "1", "100"]        # a 64-cell root does not divide 32
    args += [str(d) for d in DIMS] + ["0"] * 3 + ["1"] + ["nan", "0", "0"] + ["2", "1", "100"]
    run = run_host_check("lod_host_check", tmp_path, args)   # without arguments first, then with these
    chunks = re.split(r"^case \d+ ", run.stdout, flags=re.M)[1:]
    assert len(chunks) == len(cases) + 3
    for (name, split, level), chunk in zip(cases, chunks):
        status, _, body = chunk.partition("\n")
        assert status == "ok", (name, split, level, status)
        got = np.array([[int(v) for v in line.split()] for line in body.splitlines()], np.int32).reshape(-1, 4)
        assert np.array_equal(got, select(name, split, level)), (name, split, level)
    assert [c.strip() for c in chunks[-3:]] == ["too_large", "dims", "invalid"]


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
def lod_params(viewer_world, max_level=MAX_LEVEL, split=2.0, max_nodes=1 << 18):
    """A raw vtmc_lod_params: what reaches the library unchecked."""
    return _lib.LodParams(tuple(float(v) for v in viewer_world), float(split), int(max_level), int(max_nodes))


@pytest.fixture(scope="module")
def world():
    """The terrain, built once per output mode from the same seed and queue: the context (left in soup mode), its grid, and the
    full-resolution result of the world-building update (every block dirty) in both modes."""
    ex = vt.Extractor(0)
    full = {}
    for indexed in (True, False):
        ex.set_output_mode(indexed)
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        n_dirty, T = ex.terrain_update(full_world())
        assert n_dirty == N_BLOCKS and T > 2000
        full[indexed] = ex.read_indexed_mesh() if indexed else ex.read_triangles()
    S = ex.terrain_read_samples()
    assert (S[65, :, :] > 0).any() and (S[65, :, :] < 0).any()          # the surface crosses the terrain's upper x face
    yield dict(ex=ex, S=S, full=full)
    ex.close()


@pytest.fixture
def ex(world):
    e = world["ex"]
    yield e
    e.set_output_mode(False)
    e.set_tuning(emit_fast_math=1)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
def test_gpu_nodes_equal_the_twin(ex, split):
    for name in VIEWERS:
        want = select(name, split)
        n, T = ex.terrain_extract_lod(world_of(VIEWERS[name]), MAX_LEVEL, split)
        got = ex.terrain_lod_nodes()
        assert n == len(want) and got.dtype == np.int32 and np.array_equal(got, want), (name, split)
        assert ex.last_counts() == (n, T)


@pytest.mark.gpu
def test_gpu_level_0_is_the_ordinary_extract(ex, world):
    """split huge: every node is level 0, in depth-first order; node for node the bytes of the full rebuild's block at the same origin."""
    viewer = world_of(VIEWERS["inside"])
    # soup
    ex.set_output_mode(False)
    n, T = ex.terrain_extract_lod(viewer, MAX_LEVEL, 1e6)
    nodes = ex.terrain_lod_nodes()
    assert n == N_BLOCKS and (nodes[:, 3] == 0).all()
    block = nodes[:, 0] // 8 + (DIMS[0] // 8) * (nodes[:, 1] // 8 + (DIMS[1] // 8) * (nodes[:, 2] // 8))
    assert sorted(block.tolist()) == list(range(N_BLOCKS)) and not np.array_equal(block, np.arange(N_BLOCKS))
    full, foffs = world["full"][False]
    got, offs = ex.read_triangles()
    assert T == len(full) == len(got)
    assert np.array_equal(np.diff(offs), np.diff(foffs)[block])
    nonempty = 0
    for i, b in enumerate(block):
        g, w = got[offs[i]:offs[i + 1]], full[foffs[b]:foffs[b + 1]]
        assert (g["block"] == i).all() and (w["block"] == b).all()
        for f in FLOATS:
            assert np.array_equal(bits(g[f]), bits(w[f])), (i, b, f)
        nonempty += len(g) > 0
    assert nonempty > 20
    # indexed
    ex.set_output_mode(True)
    assert ex.terrain_extract_lod(viewer, MAX_LEVEL, 1e6) == (n, T)
    fv, fi, fvo, fto = world["full"][True]
    gv, gi, gvo, gto = ex.read_indexed_mesh()
    assert np.array_equal(gto, offs) and np.array_equal(np.diff(gvo), np.diff(fvo)[block]) and len(gv) == len(fv)
    for i, b in enumerate(block):
        assert gv[gvo[i]:gvo[i + 1]].tobytes() == fv[fvo[b]:fvo[b + 1]].tobytes(), (i, b)
        assert np.array_equal(gi[gto[i]:gto[i + 1]], fi[fto[b]:fto[b + 1]]), (i, b)


@pytest.fixture(scope="module")
def mixed(world, oracle_mod):
    """The viewer just outside a corner, split 1: nodes of all three levels.  The twin's tiles of the device's grid and the oracle's
    answers for them, computed once."""
    nodes = select("corner", 1.0)
    tiles = twin.node_tiles(world["S"], nodes)
    soup, offs, cases = oracle_mod.extract_tiles(tiles)
    return dict(nodes=nodes, tiles=tiles, soup=soup, offs=offs, cases=cases, welded=oracle_indexed_soup(oracle_mod, tiles))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast_math", "exact"])
def test_gpu_mixed_levels_match_the_oracle(ex, mixed, oracle_mod, indexed, exact):
    nodes, want = mixed["nodes"], mixed["soup"]
    assert sorted(set(nodes[:, 3].tolist())) == [0, 1, 2]                       # all three levels occur
    per_level = [int(np.diff(mixed["offs"])[nodes[:, 3] == lv].sum()) for lv in range(3)]
    assert min(per_level) > 0, per_level                                         # ... and each of them carries surface
    ex.set_tuning(emit_fast_math=0 if exact else 1)
    ex.set_output_mode(indexed)
    n, T = ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
    assert n == len(nodes) and np.array_equal(ex.terrain_lod_nodes(), nodes)
    assert np.array_equal(lod_tiles(ex, n).view(np.uint32), mixed["tiles"].view(np.uint32))       # the gather itself, bit for bit
    assert T == len(want)
    assert np.array_equal(ex.read_cases(), mixed["cases"])
    if not indexed:
        got, offs = ex.read_triangles()
        assert np.array_equal(offs, mixed["offs"])                               # per-node triangle counts
        worst = assert_tris_match(got, want, atol=0.0 if exact else 1e-5)
        print("soup, %s: %d nodes, %d triangles, worst deviation %g" % ("exact" if exact else "fast math", n, T, worst))
    else:
        verts, idx, voffs, toffs = ex.read_indexed_mesh()
        assert np.array_equal(toffs, mixed["offs"])
        got = oracle_mod.deindex(verts, idx, voffs, toffs)
        worst = assert_tris_match(got, want, atol=1e-5)                          # welded vertices against the reference's records: the 1e-5 bar
        print("indexed, %s: %d nodes, %d vertices, worst deviation from the soup %g" % ("exact" if exact else "fast math", n, len(verts), worst))
        if exact:
            assert_tris_match(got, mixed["welded"], atol=0.0)                    # against the oracle's own welded form: equal bits
    # the world mapping: every vertex inside its node's box, and the Python helper against the twin's formula
    p, blk = got["p0"], got["block"]
    pos = ex.lod_world_positions(nodes, blk, p)
    assert pos.dtype == np.float64 and np.array_equal(pos, twin.world_positions(ORIGIN, SCALE, nodes, blk, p))
    lo = np.array(ORIGIN) + nodes[blk, :3] * SCALE
    hi = lo + (8 << nodes[blk, 3])[:, None] * SCALE
    assert (pos >= lo).all() and (pos <= hi).all()
    assert np.array_equal(ex.lod_world_positions(nodes, blk, np.stack([got["p0"], got["p1"], got["p2"]], axis=1))[:, 0], pos)


@pytest.mark.gpu
def test_gpu_index_9_clamps_to_the_last_sample_plane(ex, world, oracle_mod):
    """Only the roots: level 2, stride 4, index 9 at sample o + 36 -- past dim - 1 = 65 along x for the root at x = 32 (68), and past 33
    along y and z for both (36).  The gathered tiles equal the twin's edge-replicated ones; a twin that clamps nothing differs, in the
    tiles and in the normals they give, so the test can fail."""
    S = world["S"]
    roots = select("far", 2.0)
    assert roots.tolist() == [[0, 0, 0, 2], [32, 0, 0, 2]] and 32 + 9 * 4 > S.shape[0] - 1 and 9 * 4 > S.shape[1] - 1
    tiles, loose = twin.node_tiles(S, roots), twin.node_tiles(S, roots, clamp=False)
    ex.set_tuning(emit_fast_math=0)
    n, T = ex.terrain_extract_lod(world_of(VIEWERS["far"]), MAX_LEVEL, 2.0)
    assert n == 2 and T > 0
    got_tiles = lod_tiles(ex, 2)
    assert np.array_equal(got_tiles.view(np.uint32), tiles.view(np.uint32))
    assert not np.array_equal(got_tiles.view(np.uint32), loose.view(np.uint32))
    # the same through the public path: cases and normals
    want, offs, cases = oracle_mod.extract_tiles(tiles)
    wrong, wrong_offs, wrong_cases = oracle_mod.extract_tiles(loose)
    assert np.array_equal(ex.read_cases(), cases) and np.array_equal(cases, wrong_cases) and np.array_equal(offs, wrong_offs)   # index 9 feeds no case
    got, goffs = ex.read_triangles()
    assert np.array_equal(goffs, offs)
    assert_tris_match(got, want, atol=0.0)
    P, N, W = (np.stack([t[f + "0"], t[f + "1"], t[f + "2"]], axis=1) for t, f in ((got, "p"), (got, "n"), (wrong, "n")))
    on_upper_x = (got["block"] == 1)[:, None] & (P[:, :, 0] == 8.0)      # vertices on the root's upper x face: their normals read index 9
    assert on_upper_x.sum() > 10
    assert all(np.array_equal(bits(got[f]), bits(wrong[f])) for f in ("p0", "p1", "p2"))
    assert not np.array_equal(bits(N[on_upper_x]), bits(W[on_upper_x]))
    inner = (P < 7.0).all(axis=(1, 2))                                   # triangles away from the upper faces never see index 9
    assert inner.any() and np.array_equal(bits(N[inner]), bits(W[inner]))


@pytest.mark.gpu
def test_gpu_side_effects(oracle_mod):
    """A level-of-detail extract reads the terrain and replaces the context's result; it changes nothing else, and its result is no
    result of the dirty list: materials and occlusion refuse it."""
    edit = vt.SphereModifier((8.0, 6.5, 9.0), 1.75, False)
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(8 << 20)
        ex.terrain_update(full_world())
        ex.material_init(1)
        n_dirty, T = ex.terrain_update([edit])
        assert 0 < n_dirty < N_BLOCKS and T > 0
        dirty, S, history = ex.terrain_dirty_blocks(), ex.terrain_read_samples(), ex.terrain_history()
        assert history[0] == 2
        gx, gz = np.meshgrid(np.linspace(-2.5, 28.5, 12), np.linspace(2.5, 17.5, 8), indexing="ij")
        origins = np.stack([gx.ravel(), np.full(gx.size, 16.5), gz.ravel()], axis=1).astype(f32)
        directions = np.broadcast_to(np.array([0.05, -1.0, 0.02], f32), origins.shape).copy()
        hits = ex.terrain_raycast(origins, directions)
        assert (hits["triangle"] >= 0).sum() > 50
        assert len(ex.vertex_materials()) == 3 * T and len(ex.vertex_ao(2.0)) == 3 * T
        n, T_lod = ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
        assert n == 37 and T_lod > 0 and ex.last_counts() == (n, T_lod)
        assert np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(S))
        assert ex.terrain_history() == history
        assert ex.terrain_raycast(origins, directions).tobytes() == hits.tobytes()
        no_result(ex.vertex_materials)
        no_result(lambda: ex.vertex_ao(2.0))
        no_result(ex.material_vertices)
        # the event counter did not move: the next update draws what it would have drawn, and extracts its dirty set as usual
        with vt.Extractor(0) as other:
            other.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
            other.terrain_update(full_world())
            other.terrain_update([edit])
            second = vt.SphereModifier((20.0, 7.0, 12.0), 2.0, True)
            want_counts = other.terrain_update([second])
            want_grid, want_tris = other.terrain_read_samples(), other.read_triangles()
        assert ex.terrain_update([second]) == want_counts
        no_result(ex.terrain_lod_nodes)                                  # the result is the dirty list's again
        grid = ex.terrain_read_samples()
        assert np.array_equal(bits(grid), bits(want_grid))
        got = ex.read_triangles()
        assert got[0].tobytes() == want_tris[0].tobytes() and np.array_equal(got[1], want_tris[1])
        assert_triangles(ex, oracle_mod, grid, ex.terrain_dirty_blocks(), want_counts[1])
        assert len(ex.vertex_materials()) == 3 * want_counts[1] and len(ex.vertex_ao(2.0)) == 3 * want_counts[1]
        assert ex.terrain_history()[0] == 3


@pytest.mark.gpu
def test_gpu_errors(ex):
    L, h = ex._L, ex._h
    call = lambda p: L.vtmc_terrain_extract_lod(h, ctypes.byref(p), None, None)   # noqa: E731
    viewer = world_of(VIEWERS["corner"])
    with vt.Extractor(0) as fresh:                                       # before terrain_init
        no_result(lambda: fresh.terrain_extract_lod(viewer, MAX_LEVEL))
        no_result(fresh.terrain_lod_nodes)
        fresh.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        no_result(fresh.terrain_lod_nodes)                               # a terrain, no level-of-detail result
        assert fresh.terrain_extract_lod(viewer, MAX_LEVEL, 1.0) == (37, 0)   # an empty terrain: nodes without a triangle
        assert len(fresh.terrain_lod_nodes()) == 37 and fresh.last_counts() == (37, 0)
    n, T = ex.terrain_extract_lod(viewer, MAX_LEVEL, 1.0)
    want_nodes = select("corner", 1.0)
    assert n == len(want_nodes) == 37
    before, before_offs = ex.read_triangles()

    def unchanged():
        tris, offs = ex.read_triangles()
        return (ex.last_counts() == (n, T) and tris.tobytes() == before.tobytes() and np.array_equal(offs, before_offs)
                and np.array_equal(ex.terrain_lod_nodes(), want_nodes))

    assert call(lod_params(viewer, 3)) == _lib.ERR_DIMS and unchanged()              # a 64-cell root does not divide 32
    assert call(lod_params(viewer, 2, 1.0, len(want_nodes) - 1)) == _lib.ERR_TOO_LARGE and unchanged()
    assert call(lod_params(viewer, 2, 4.0, 2)) == _lib.ERR_TOO_LARGE and unchanged()
    nan, inf = float("nan"), float("inf")
    for bad in [lod_params((nan, 0.0, 0.0)), lod_params((0.0, inf, 0.0)), lod_params((0.0, 0.0, -inf)), lod_params(viewer, 2, 0.5),
                lod_params(viewer, 2, nan), lod_params(viewer, 2, inf), lod_params(viewer, 2, 0.0), lod_params(viewer, -1), lod_params(viewer, 8),
                lod_params(viewer, 2, 2.0, 0), lod_params(viewer, 2, 2.0, -3)]:
        assert call(bad) == _lib.ERR_INVALID_ARG
    assert L.vtmc_terrain_extract_lod(h, None, None, None) == _lib.ERR_INVALID_ARG and unchanged()
    assert call(lod_params(viewer, 2, 1.0, len(want_nodes))) == _lib.OK and unchanged()      # exactly enough
    buf = np.zeros((40, 4), np.int32)
    count = ctypes.c_int32()
    assert L.vtmc_terrain_lod_nodes(h, buf.ctypes.data, 36, ctypes.byref(count)) == _lib.ERR_CAPACITY and count.value == 37
    assert L.vtmc_terrain_lod_nodes(h, buf.ctypes.data, 37, None) == _lib.OK and np.array_equal(buf[:37], want_nodes)
    # another extract since: the node list is no longer the result's
    g = np.full((10, 10, 10), -1.0, f32)
    g[3:6, 3:6, 3:6] = 1.0
    assert ex.extract_grid(g) > 0
    no_result(ex.terrain_lod_nodes)


@pytest.mark.gpu
def test_gpu_host_mirror(tmp_path):
    """The C++ VoxelTerrain mirror's ExtractLod / LodNodes against the Python path on the same world (host/host_selftest.cpp --gpu-lod)."""
    from test_host_mirror import run_host_mirror
    r = run_host_mirror("--gpu-lod", tmp_path)
    nodes = np.fromfile(tmp_path / "lod_nodes.i32", np.int32).reshape(-1, 4)
    counts = np.fromfile(tmp_path / "lod_counts.i32", np.int32)
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_update(base_world())
        n, T = ex.terrain_extract_lod(world_of(VIEWERS["corner"]), MAX_LEVEL, 1.0)
        want_nodes, (_, offs) = ex.terrain_lod_nodes(), ex.read_triangles()
    assert np.array_equal(nodes, want_nodes) and np.array_equal(nodes, select("corner", 1.0))
    assert np.array_equal(counts, 3 * np.diff(offs)) and counts.sum() == 3 * T
    assert ("lod: nodes %d triangles %d " % (n, T)) in r.stdout
