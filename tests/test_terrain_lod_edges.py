"""The level-of-detail extract and its skirts (vtmc_terrain_extract_lod, vtmc_lod_skirts) away from the one world of test_terrain_lod.py
and test_terrain_lodskirt.py: at strides 8 and 16, past one scan group of skirt tiles, with more than 256 records in a tile, with lanes
that hang several quads, with vertices that must stay where they are, and off the dyadic world, where a selection done in float32 decides
differently from the rule's double.

Every world is written from samples -- a float64 formula cast to float32 -- so the twins and the device start from the same bits.  Every
world has CPU tests that state, against the twins and the CPU oracle alone, the CONDITIONS it must meet for its GPU tests to mean anything:
a GPU test is only as good as the world it runs on.  Conditions are asserted as inequalities, not as counts: sin may differ in its last
bit between machines.

  deep_a     128^3 cells, scale 0.3, origin (-3.1, 0.7, 2.3): a heightfield with a cave, roots of level 4 (128 cells), nodes of levels 0..3
  deep_b     256 x 128 x 128 cells, scale 1, origin 0: the same field, nodes of levels 2, 3 and 4; index 9 lies past the last sample
             plane along y and z in the level-4 root (at x = 0) and along x in the level-2 nodes at x = 224
  lattice128 128 x 64 x 64 cells: a product of sines inside a slab, more than 262 144 triangles = more than 1024 skirt tiles
  lattice64  64^3 cells: the same product, every interior face flagged: tiles with more than 256 skirt records
  parity     64 x 32 x 40 cells, S = +1 where x + y + z is odd, else -1: every cell edge is crossed, exactly 1280 full tiles, every
             central difference is 0, so every normal is flat and no skirt vertex may move
  ragged     96 x 64 x 160 cells = 3 x 2 x 5 roots of level 2, scale 0.3, origin (-3.1, 0.7, 2.3): the selection off the dyadic world"""
import functools
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import lod_twin
import lodskirt_twin as skirt_twin
from extract_checks import assert_tris_match
from host_check import run_host_check
from lod_support import (assert_skirts_match_the_twin, bits, brute_masks, check_closure, check_skirt_properties, device_records, interior_masks,
                         lod_tiles, oracle_indexed_soup, poison_skirts)

f32, f64 = np.float32, np.float64
TILE, GROUP = 256, 1024                    # kLodSkirtTile triangles in a skirt tile, kScanThreads tiles in a scan group
OFF_DYADIC = (0.3, (-3.1, 0.7, 2.3))


def grid_xyz(dims):
    return np.meshgrid(*(np.arange(d + 2, dtype=f64) for d in dims), indexing="ij")


def hills_field(dims):
    """S = min(h - y, |p - (70, 50, 40)| - 22), h = 60 + 20 sin(0.05 x + 0.3) cos(0.045 z) + 9 sin(0.11 x + 0.07 z)."""
    x, y, z = grid_xyz(dims)
    h = 60.0 + 20.0 * np.sin(0.05 * x + 0.3) * np.cos(0.045 * z) + 9.0 * np.sin(0.11 * x + 0.07 * z)
    ball = np.sqrt((x - 70.0) ** 2 + (y - 50.0) ** 2 + (z - 40.0) ** 2) - 22.0
    return np.minimum(h - y, ball).astype(f32)


def lattice_field(dims, slab=None):
    """S = sin(0.9 x + 0.3) sin(0.8 y + 0.1) sin(0.7 z + 0.2) + 0.05; with slab = (lo, hi), -1 where z < lo or z > hi."""
    x, y, z = grid_xyz(dims)
    S = np.sin(0.9 * x + 0.3) * np.sin(0.8 * y + 0.1) * np.sin(0.7 * z + 0.2) + 0.05
    if slab:
        S = np.where((z < slab[0]) | (z > slab[1]), -1.0, S)
    return S.astype(f32)


def parity_field(dims):
    x, y, z = grid_xyz(dims)
    return np.where((x + y + z) % 2 == 1, 1.0, -1.0).astype(f32)


def ragged_field(dims):
    """S = min(h - y, |p - (30, 20, 60)| - 13), h = 30 + 11 sin(0.07 x + 0.3) cos(0.05 z) + 5 sin(0.13 x + 0.09 z)."""
    x, y, z = grid_xyz(dims)
    h = 30.0 + 11.0 * np.sin(0.07 * x + 0.3) * np.cos(0.05 * z) + 5.0 * np.sin(0.13 * x + 0.09 * z)
    ball = np.sqrt((x - 30.0) ** 2 + (y - 20.0) ** 2 + (z - 60.0) ** 2) - 13.0
    return np.minimum(h - y, ball).astype(f32)


class World:
    """A terrain and one selection on it.  viewer_cells places the viewer in cells; the world position is rounded to float32 once, here,
    and twin and device are both handed that float32."""

    def __init__(self, name, dims, field, viewer_cells, max_level, split, all_faces=False, placement=(1.0, (0.0, 0.0, 0.0))):
        self.name, self.dims, self.field, self.max_level, self.split, self.all_faces = name, dims, field, max_level, split, all_faces
        self.scale, self.origin = placement
        self.viewer = self.world_of(viewer_cells)

    def world_of(self, cells):
        return tuple(float(f32(self.origin[k] + cells[k] * self.scale)) for k in range(3))

    def select(self, viewer=None, max_level=None, split=None):
        return lod_twin.select_nodes(self.dims, self.origin, self.scale, self.viewer if viewer is None else viewer,
                                     self.max_level if max_level is None else max_level, self.split if split is None else split)


WORLDS = {w.name: w for w in (
    World("deep_a", (128, 128, 128), hills_field, (-1.0, 50.0, 5.0), 4, 1.0, placement=OFF_DYADIC),
    World("deep_b", (256, 128, 128), hills_field, (300.0, 50.0, 5.0), 4, 1.0),
    World("lattice128", (128, 64, 64), functools.partial(lattice_field, slab=(9, 52)), (60.0, 30.0, 30.0), 2, 2.0),
    World("lattice64", (64, 64, 64), lattice_field, (-1.0, 3.0, 5.0), 2, 2.0, all_faces=True),
    World("parity", (64, 32, 40), parity_field, (10.0, 5.0, 20.0), 0, 2.0, all_faces=True),
    World("ragged", (96, 64, 160), ragged_field, (-1.0, 30.0, 5.0), 2, 1.0, placement=OFF_DYADIC),
)}
DEEP_LEVELS = {"deep_a": [0, 1, 2, 3], "deep_b": [2, 3, 4]}
_reference = {}


def reference(oracle_mod, name, depth=1.0):
    """The CPU side of a world, computed once and left unchanged: the samples, the twin's nodes and tiles, the oracle's records, cases and
    per-node offsets of those tiles, the twin's masks and its skirts of the oracle's records; for the deep worlds also the oracle's welded
    mesh of the tiles, de-indexed."""
    if name not in _reference:
        w = WORLDS[name]
        S = w.field(w.dims)
        nodes = w.select()
        tiles = lod_twin.node_tiles(S, nodes)
        soup, offs, cases = oracle_mod.extract_tiles(tiles)
        masks = skirt_twin.face_masks(w.dims, nodes, w.all_faces)
        tmask = skirt_twin.triangle_masks(soup, masks)
        skirt, node_offsets, faces = skirt_twin.skirts(soup, masks, depth)
        for a in (S, nodes, tiles, soup, offs, cases, masks, tmask, skirt, node_offsets, faces):
            a.setflags(write=False)
        _reference[name] = dict(S=S, nodes=nodes, tiles=tiles, soup=soup, offs=offs, cases=cases, masks=masks, tmask=tmask, skirt=skirt,
                                node_offsets=node_offsets, faces=faces)
        if name in DEEP_LEVELS:
            _reference[name]["welded"] = oracle_indexed_soup(oracle_mod, tiles)
            _reference[name]["welded"].setflags(write=False)
    return _reference[name]


def popcount(a):
    return np.unpackbits(np.asarray(a, np.uint8)[:, None], axis=1).sum(axis=1)


def tile_record_totals(tmask):
    """The skirt records of every tile of kLodSkirtTile triangles: 2 per set bit of the triangles' face masks."""
    padded = np.zeros(-(-len(tmask) // TILE) * TILE, np.int64)
    padded[:len(tmask)] = 2 * popcount(tmask)
    return padded.reshape(-1, TILE).sum(axis=1)


# -- CPU: the conditions of the worlds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep_a", "deep_b"])
def test_deep_worlds_meet_their_conditions(oracle_mod, name):
    w, r = WORLDS[name], reference(oracle_mod, name)
    nodes, per_node, per_node_skirts = r["nodes"], np.diff(r["offs"]), np.diff(r["node_offsets"])
    assert (lod_twin.coverage(w.dims, nodes) == 1).all() and lod_twin.max_face_level_step(w.dims, nodes) <= 1
    assert sorted(set(nodes[:, 3].tolist())) == DEEP_LEVELS[name]
    for level in DEEP_LEVELS[name]:                                              # every present level carries triangles and skirt records
        assert per_node[nodes[:, 3] == level].sum() > 0 and per_node_skirts[nodes[:, 3] == level].sum() > 0, level
    if name == "deep_a":
        assert per_node[0] == 0                                                  # starts with an empty node
    else:
        assert per_node[-1] == 0 and r["offs"][-2] == len(r["soup"])             # ends with one: its first triangle is T, the offsets kernel's t >= n_tris
        # index 9 lies past the last sample plane (dim + 1) along every axis for some node, along y and z for the level-4 root (sample
        # 144 past 129), along x for the level-2 nodes at x = 224 (260 past 257): a twin that clamps nothing differs
        past = nodes[:, :3] + 9 * (1 << nodes[:, 3])[:, None] > np.array(w.dims) + 1
        assert past.any(axis=0).all() and past[nodes[:, 3] == 4, 1:].all() and past[nodes[:, 3] == 2, 0].any()
        assert not np.array_equal(bits(lod_twin.node_tiles(r["S"], nodes, clamp=False)), bits(r["tiles"]))
    assert ((r["masks"] != 0) & (per_node == 0)).any()                           # a flagged node without a triangle
    assert np.array_equal(r["masks"], brute_masks(w.dims, nodes)) and not (r["masks"] & ~interior_masks(w.dims, nodes)).any()
    print("%s: %d nodes, levels %s, %d triangles, skirt records per level %s" % (name, len(nodes), np.bincount(nodes[:, 3]).tolist(), len(r["soup"]),
          [int(per_node_skirts[nodes[:, 3] == lv].sum()) for lv in DEEP_LEVELS[name]]))


@pytest.mark.parametrize("name", ["deep_a", "deep_b"])
def test_deep_twin_skirts_close_the_seams(oracle_mod, name):
    """The reference alone: the twin's skirts of the oracle's records have the properties and close the seams between levels 0/1, 1/2 and
    2/3 (deep_a) and 2/3 and 3/4 (deep_b) under the caps of the first scene."""
    r = reference(oracle_mod, name)
    check_skirt_properties(r["skirt"], r["faces"], 1.0)
    walk = check_closure(r["nodes"], r["soup"], r["masks"], r["skirt"], 1.0)
    assert walk["skipped"] == 0, walk
    # seams between every pair of adjacent levels are walked: boundary edges of both levels lie in one face plane
    tri, face, A, _ = skirt_twin.boundary_edges(r["soup"], r["masks"])
    node = r["soup"]["block"][tri]
    plane = skirt_twin.node_cells(r["nodes"], node, A)[np.arange(len(tri)), face >> 1]
    keys = set(zip((face >> 1).tolist(), plane.tolist(), r["nodes"][node, 3].tolist()))
    for level in DEEP_LEVELS[name][:-1]:
        assert any((a, p, level + 1) in keys for a, p, lv in keys if lv == level), level


def test_lattice128_meets_its_conditions(oracle_mod):
    r = reference(oracle_mod, "lattice128")
    T, offs, per_node_skirts = len(r["soup"]), r["offs"], np.diff(r["node_offsets"])
    assert T > TILE * GROUP and T % TILE != 0
    assert len(set(r["nodes"][:, 3].tolist())) == 2
    hanging = np.nonzero(r["tmask"])[0]
    assert (hanging >= TILE * GROUP).any()                                       # a quad hangs from a triangle past the first scan group
    assert (hanging < 2 * TILE).any()                                            # ... and one from tile 0 or 1
    assert ((offs[:-1] >= TILE * GROUP) & (per_node_skirts > 0)).any()           # a node whose first triangle lies past it, with skirts
    assert ((r["masks"] != 0) & (np.diff(offs) == 0)).any()
    print("lattice128: %d nodes, %d triangles = %d tiles, %d skirt records from tiles %d..%d" % (len(r["nodes"]), T, -(-T // TILE), len(r["skirt"]),
          hanging.min() // TILE, hanging.max() // TILE))


@pytest.mark.parametrize("name", ["lattice64", "parity"])
def test_crowded_worlds_meet_their_conditions(oracle_mod, name):
    r = reference(oracle_mod, name)
    totals, several = tile_record_totals(r["tmask"]), int((popcount(r["tmask"]) >= 2).sum())
    assert totals.max() > TILE                                                   # the staged emit's chunk loop runs more than once
    assert several >= 1000                                                       # lanes that advance their slot more than once
    assert totals.sum() == len(r["skirt"])
    print("%s: %d nodes, %d triangles, %d skirt records, largest tile total %d, %d triangles with two or more faces"
          % (name, len(r["nodes"]), len(r["soup"]), len(r["skirt"]), totals.max(), several))


def test_parity_meets_its_conditions(oracle_mod):
    r = reference(oracle_mod, "parity")
    T = len(r["soup"])
    assert T % TILE == 0 and T // TILE > GROUP                                   # the last tile is full, and there are two scan groups
    assert (r["nodes"][:, 3] == 0).all() and len(r["nodes"]) == 160
    for k in ("n0", "n1", "n2"):                                                 # the oracle's normals are flat: the twin moves nothing
        assert not r["soup"][k].any()
    first, second = r["skirt"][0::2], r["skirt"][1::2]
    assert len(first) > 50000
    assert first["p2"].tobytes() == first["p1"].tobytes() == second["p1"].tobytes() and second["p2"].tobytes() == second["p0"].tobytes()
    assert not skirt_twin.face_masks(WORLDS["parity"].dims, r["nodes"]).any()    # without ALL_FACES nothing is flagged


# -- CPU: off the dyadic world -------------------------------------------------------------------------------------------------------------------
SPLITS = (1.0, 1.1, 1.37, 2.0, 2.5, 3.3)


def select_nodes_f32(dims, origin, scale, viewer, max_level, split):
    """lod_twin.select_nodes with every operation in float32: what the near ties must tell from the rule."""
    c = [(f32(viewer[k]) - f32(origin[k])) / f32(scale) for k in range(3)]
    split, n_root, out = f32(split), 8 << max_level, []

    def distance(o, n):
        d = f32(0.0)
        for k in range(3):
            below, above = f32(o[k]) - c[k], c[k] - (f32(o[k]) + f32(n))
            d = below if below > d else d
            d = above if above > d else d
        return d

    def descend(o, level):
        n = 8 << level
        if level > 0 and distance(o, n) < split * f32(n):
            h = n // 2
            for k in range(8):
                descend((o[0] + h * (k & 1), o[1] + h * ((k >> 1) & 1), o[2] + h * ((k >> 2) & 1)), level - 1)
        else:
            out.append((o[0], o[1], o[2], level))

    for rz in range(dims[2] // n_root):
        for ry in range(dims[1] // n_root):
            for rx in range(dims[0] // n_root):
                descend((rx * n_root, ry * n_root, rz * n_root), max_level)
    return np.array(out, np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def random_viewers():
    """(viewer in world space as float32 values, max_level, split): inside the terrain, outside it within a root or two, and far away."""
    w, rng, out = WORLDS["ragged"], np.random.default_rng(20261), []
    for i in range(60):
        kind = i % 3
        lo, hi = ((0.0, 1.0), (-0.6, 1.6), (-30.0, 30.0))[kind]
        cells = [rng.uniform(lo, hi) * d for d in w.dims]
        out.append((w.world_of(cells), int(rng.integers(0, 3)), float(f32(SPLITS[int(rng.integers(0, len(SPLITS)))]))))
    return out


@functools.lru_cache(maxsize=None)
def near_tie_viewers():
    """A viewer at x = origin.x - scale * split * n sees the nodes of n cells at x = 0 at exactly d = split * n: the comparison of the rule
    is a tie in real numbers, and how the quotient (v - o) / scale rounds decides it.  For n = 16 and 32 and three splits, the float32
    values within 40 steps of that x, at a fixed y and z inside the terrain: 486 viewers, all at max_level 2."""
    w, out = WORLDS["ragged"], []
    y, z = w.world_of((0.0, 20.3, 70.9))[1:]
    for split in (1.0, 1.37, 2.5):
        for n in (16, 32):
            x0 = f32(f64(f32(w.origin[0])) - f64(f32(w.scale)) * f64(f32(split)) * n)
            for step in range(-40, 41):
                x = (x0.view(np.int32) + np.int32(step)).view(f32)
                out.append(((float(x), y, z), 2, float(f32(split))))
    return out


@functools.lru_cache(maxsize=None)
def ragged_selections():
    """The twin's node list of every viewer, random ones first."""
    w = WORLDS["ragged"]
    return [w.select(v, level, split) for v, level, split in random_viewers() + near_tie_viewers()]


def test_near_ties_tell_a_float32_selection_from_the_rule():
    w, ties = WORLDS["ragged"], near_tie_viewers()
    want = ragged_selections()[len(random_viewers()):]
    assert len(ties) == 486
    differ = sum(not np.array_equal(select_nodes_f32(w.dims, w.origin, w.scale, v, level, split), nodes) for (v, level, split), nodes in zip(ties, want))
    print("near ties: a float32 selection differs from the rule for %d of %d viewers" % (differ, len(ties)))
    assert differ >= 3
    # ... and the random viewers alone could not: that is why the ties are here
    same = sum(np.array_equal(select_nodes_f32(w.dims, w.origin, w.scale, v, level, split), nodes)
               for (v, level, split), nodes in zip(random_viewers()[:20], ragged_selections()[:20]))
    assert same == 20                                                            # the restatement is the rule wherever nothing is tied


def test_selection_off_the_dyadic_world_host_check_equals_the_twin(tmp_path):
    """tools/lod_host_check.cpp under ASan and UBSan on every random and every near-tie viewer of the 3 x 2 x 5 root lattice: its node
    lists equal the twin's, which tile the terrain once with face level steps of at most 1."""
    w = WORLDS["ragged"]
    cases, want = random_viewers() + near_tie_viewers(), ragged_selections()
    assert {level for _, level, _ in random_viewers()} == {0, 1, 2} and {s for _, _, s in random_viewers()} == {float(f32(s)) for s in SPLITS}
    args = []
    for viewer, level, split in cases:
        args += [str(d) for d in w.dims] + [float(f32(v)).hex() for v in w.origin] + [float(f32(w.scale)).hex()] + [float(v).hex() for v in viewer]
        args += [str(level), float(split).hex(), str(1 << 18)]
    run = run_host_check("lod_host_check", tmp_path, args)
    chunks = re.split(r"^case \d+ ", run.stdout, flags=re.M)[1:]
    assert len(chunks) == len(cases)
    sizes = []
    for (viewer, level, split), nodes, chunk in zip(cases, want, chunks):
        status, _, body = chunk.partition("\n")
        assert status == "ok", (viewer, level, split, status)
        got = np.array(body.split(), np.int32).reshape(-1, 4)
        assert np.array_equal(got, nodes), (viewer, level, split)
        assert (lod_twin.coverage(w.dims, nodes) == 1).all() and lod_twin.max_face_level_step(w.dims, nodes) <= 1, (viewer, level, split)
        sizes.append(len(nodes))
    print("%d viewers, node lists of %d to %d nodes" % (len(cases), min(sizes), max(sizes)))
    assert min(sizes) == 30 and max(sizes) == 1920                              # only the roots; every block its own node


def test_ragged_world_has_three_levels_with_skirts(oracle_mod):
    w, r = WORLDS["ragged"], reference(oracle_mod, "ragged")
    per_node_skirts = np.diff(r["node_offsets"])
    assert sorted(set(r["nodes"][:, 3].tolist())) == [0, 1, 2]
    assert all(per_node_skirts[r["nodes"][:, 3] == level].sum() > 0 for level in range(3))
    assert np.array_equal(r["masks"], brute_masks(w.dims, r["nodes"]))
    assert np.array_equal(skirt_twin.face_masks(w.dims, r["nodes"], True), interior_masks(w.dims, r["nodes"]))


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def devices():
    """A context per world, built on first use: the terrain written from the world's samples and read back bit for bit."""
    made = {}

    def get(name):
        if name not in made:
            w = WORLDS[name]
            ex = vt.Extractor(0)
            made[name] = ex
            ex.terrain_init(*w.dims, w.scale, w.origin, 7)
            S = w.field(w.dims)
            ex.terrain_write_samples(S)
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(S))
        return made[name]

    yield get
    for ex in made.values():
        ex.close()


@pytest.fixture
def device(devices):
    used = []

    def get(name):
        used.append(devices(name))
        return used[-1]

    yield get
    for e in used:
        e.set_output_mode(False)
        e.set_tuning(emit_fast_math=1)
        assert e._L.vtmc_debug_lodskirt_store(e._h, 0) == _lib.OK


def extract(ex, w, nodes):
    n, T = ex.terrain_extract_lod(w.viewer, w.max_level, w.split)
    assert n == len(nodes) and np.array_equal(ex.terrain_lod_nodes(), nodes) and ex.last_counts() == (n, T)
    return T


def skirts_match(ex, oracle_mod, w, nodes, indexed, depth, all_faces=False, staged_too=False):
    """assert_skirts_match_the_twin, after which the device's skirt buffers are poisoned: the record buffer only grows and every pass
    writes into it again, so the next pass on this context -- the staged one here, the next test's otherwise -- must write every byte it
    is compared on.  staged_too: the STAGED store variant then fills the poisoned buffers and must give DIRECT's bytes and offsets."""
    out = assert_skirts_match_the_twin(ex, oracle_mod, w.dims, nodes, indexed, depth, all_faces)
    direct, direct_offsets = out[1], ex.lodskirt_read()[1]
    poison_skirts(ex)
    if staged_too:
        assert ex._L.vtmc_debug_lodskirt_store(ex._h, 1) == _lib.OK
        assert ex.lod_skirts(depth, all_faces) == len(direct)
        staged, staged_offsets = ex.lodskirt_read()
        assert ex._L.vtmc_debug_lodskirt_store(ex._h, 0) == _lib.OK
        assert staged.tobytes() == direct.tobytes() and np.array_equal(staged_offsets, direct_offsets)
        poison_skirts(ex)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast_math", "exact"])
@pytest.mark.parametrize("name", ["deep_a", "deep_b"])
def test_gpu_deep_levels_match_the_oracle_and_the_twin(device, oracle_mod, name, exact, indexed):
    """test_terrain_lod's test_gpu_mixed_levels_match_the_oracle and test_terrain_lodskirt's skirt tests at strides 8 and 16."""
    w, r, ex = WORLDS[name], reference(oracle_mod, name), device(name)
    nodes, want = r["nodes"], r["soup"]
    ex.set_tuning(emit_fast_math=0 if exact else 1)
    ex.set_output_mode(indexed)
    T = extract(ex, w, nodes)
    tiles = lod_tiles(ex, len(nodes))
    assert np.array_equal(bits(tiles), bits(r["tiles"]))                         # the gather at strides 1..16, bit for bit
    if name == "deep_b":
        assert not np.array_equal(bits(tiles), bits(lod_twin.node_tiles(r["S"], nodes, clamp=False)))
    assert T == len(want) and np.array_equal(ex.read_cases(), r["cases"])
    if not indexed:
        got, offs = ex.read_triangles()
        assert np.array_equal(offs, r["offs"])
        worst = assert_tris_match(got, want, atol=0.0 if exact else 1e-5)
    else:
        verts, idx, voffs, toffs = ex.read_indexed_mesh()
        assert np.array_equal(toffs, r["offs"])
        got = oracle_mod.deindex(verts, idx, voffs, toffs)
        worst = assert_tris_match(got, want, atol=1e-5)                          # welded vertices against the reference's records: the 1e-5 bar
        if exact:
            assert_tris_match(got, r["welded"], atol=0.0)                        # against the oracle's own welded form: equal bits
    # the skirts: every face with a node behind it at depth 0.75, then the seams at depth 1
    _, every, _, differ_all = skirts_match(ex, oracle_mod, w, nodes, indexed, 0.75, all_faces=True)
    records, got_skirt, masks, differ = skirts_match(ex, oracle_mod, w, nodes, indexed, 1.0, staged_too=True)
    assert np.array_equal(masks, r["masks"]) and len(every) > len(got_skirt) > 0
    check_skirt_properties(got_skirt, skirt_twin.quad_faces(got_skirt), 1.0)
    walk = check_closure(nodes, records, masks, got_skirt, 1.0)
    print("%s, %s, %s: %d nodes, %d triangles, worst deviation from the oracle %g; %d + %d skirt records, displaced components whose bits "
          "differ from the twin's: %d + %d; largest gap walked %.3f coarse cells"
          % (name, "indexed" if indexed else "soup", "exact" if exact else "fast math", len(nodes), T, worst, len(got_skirt), len(every), differ, differ_all,
             walk["max_gap"]))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
def test_gpu_skirts_past_one_scan_group(device, oracle_mod, indexed):
    """More than 1024 skirt tiles, the last one ragged: the emit and the offsets kernel add a group offset that is not 0, to records and to
    node_offsets alike.  No closure walk here: it is a Python loop."""
    w, r, ex = WORLDS["lattice128"], reference(oracle_mod, "lattice128"), device("lattice128")
    ex.set_output_mode(indexed)
    T = extract(ex, w, r["nodes"])
    assert T == len(r["soup"]) > TILE * GROUP
    records, got, masks, differ = skirts_match(ex, oracle_mod, w, r["nodes"], indexed, 1.0, staged_too=True)
    hanging = np.nonzero(skirt_twin.triangle_masks(records, masks))[0]
    assert (hanging >= TILE * GROUP).any() and (hanging < 2 * TILE).any()        # the device's own records meet the world's conditions
    print("lattice128, %s: %d nodes, %d triangles, %d skirt records, displaced components whose bits differ from the twin's: %d"
          % ("indexed" if indexed else "soup", len(r["nodes"]), T, len(got), differ))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("name", ["lattice64", "parity"])
def test_gpu_crowded_tiles_and_lanes_with_several_faces(device, oracle_mod, name, indexed):
    """Tiles of more than 256 records: the staged emit's chunk loop runs twice, a lane's two records fall into different chunks, later
    chunks have their own shift; lanes with two and three faces advance their slot."""
    w, r, ex = WORLDS[name], reference(oracle_mod, name), device(name)
    ex.set_output_mode(indexed)
    T = extract(ex, w, r["nodes"])
    records, got, masks, differ = skirts_match(ex, oracle_mod, w, r["nodes"], indexed, 1.0, all_faces=True, staged_too=True)
    tmask = skirt_twin.triangle_masks(records, masks)
    assert tile_record_totals(tmask).max() > TILE and (popcount(tmask) >= 2).sum() >= 1000
    print("%s, %s: %d nodes, %d triangles, %d skirt records, displaced components whose bits differ from the twin's: %d"
          % (name, "indexed" if indexed else "soup", len(r["nodes"]), T, len(got), differ))


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast_math", "exact"])
def test_gpu_a_vertex_without_a_normal_in_the_face_stays(device, oracle_mod, exact):
    """The parity world: every central difference is 0, so every normal has l2 = 0 (or is NaN) and no vertex may move.
    check_skirt_properties does not apply: its orientation cap presumes quads with area, and here every quad is its source edge."""
    w, r, ex = WORLDS["parity"], reference(oracle_mod, "parity"), device("parity")
    ex.set_tuning(emit_fast_math=0 if exact else 1)
    T = extract(ex, w, r["nodes"])
    assert T == len(r["soup"]) and T % TILE == 0 and T // TILE > GROUP
    records = device_records(ex, oracle_mod, False)
    with np.errstate(all="ignore"):
        for k in ("n0", "n1", "n2"):                                             # the device's own normals first: l2 not above 0 on every face axis
            n = records[k].astype(f32)
            for axis in range(3):
                u, v = [c for c in range(3) if c != axis]
                assert not (n[:, u] * n[:, u] + n[:, v] * n[:, v] > 0).any(), (k, axis)
    _, got, masks, differ = skirts_match(ex, oracle_mod, w, r["nodes"], False, 1.0, all_faces=True)
    first, second = got[0::2], got[1::2]
    assert len(got) == len(r["skirt"]) and differ == 0
    assert bits(first["p2"]).tobytes() == bits(first["p1"]).tobytes() == bits(second["p1"]).tobytes()      # a' is a, bitwise
    assert bits(second["p2"]).tobytes() == bits(second["p0"]).tobytes()                                  # b' is b
    nan_normals = int(sum(np.isnan(records[k]).any(axis=1).sum() for k in ("n0", "n1", "n2")))
    print("parity, %s: %d nodes, %d triangles, %d skirt records, none moved; corners with a NaN normal: %d" % ("exact" if exact else "fast math", len(r["nodes"]), T, len(got), nan_normals))
    # without ALL_FACES nothing is flagged: every tile leaves at the count kernel's early exit, across two scan groups
    assert ex.lod_skirts(1.0) == 0 and ex.lodskirt_info() == (160, 0, 0)
    none, offsets = ex.lodskirt_read()
    assert len(none) == 0 and len(offsets) == 161 and not offsets.any() and not ex.lodskirt_masks().any()


@pytest.mark.gpu
def test_gpu_selection_off_the_dyadic_world_equals_the_twin(device):
    w, ex = WORLDS["ragged"], device("ragged")
    cases = random_viewers()[:40] + near_tie_viewers()
    want = ragged_selections()[:40] + ragged_selections()[len(random_viewers()):]
    for (viewer, level, split), nodes in zip(cases, want):
        n, T = ex.terrain_extract_lod(viewer, level, split)
        assert n == len(nodes) and np.array_equal(ex.terrain_lod_nodes(), nodes), (viewer, level, split)
    print("ragged: %d viewers, node lists of %d to %d nodes" % (len(cases), min(map(len, want)), max(map(len, want))))


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
def test_gpu_gather_and_skirts_on_a_3_by_2_by_5_root_lattice(device, oracle_mod, indexed):
    w, r, ex = WORLDS["ragged"], reference(oracle_mod, "ragged"), device("ragged")
    assert sorted(set(r["nodes"][:, 3].tolist())) == [0, 1, 2]
    ex.set_output_mode(indexed)
    T = extract(ex, w, r["nodes"])
    assert np.array_equal(bits(lod_tiles(ex, len(r["nodes"]))), bits(r["tiles"]))
    assert T == len(r["soup"]) and np.array_equal(ex.read_cases(), r["cases"])
    worst = assert_tris_match(device_records(ex, oracle_mod, indexed), r["soup"], atol=1e-5)
    _, got, masks, differ = skirts_match(ex, oracle_mod, w, r["nodes"], indexed, 1.0)
    assert np.array_equal(masks, r["masks"]) and len(got) > 0
    _, every, all_masks, _ = skirts_match(ex, oracle_mod, w, r["nodes"], indexed, 1.0, all_faces=True)
    assert np.array_equal(all_masks, interior_masks(w.dims, r["nodes"])) and len(every) > len(got)
    print("ragged, %s: %d nodes, %d triangles, worst deviation from the oracle %g, %d skirt records, displaced components whose bits differ "
          "from the twin's: %d" % ("indexed" if indexed else "soup", len(r["nodes"]), T, worst, len(got), differ))
