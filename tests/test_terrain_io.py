"""Saving a session: the resident terrain as a sparse brick file (vtmc_terrain_save / _load / _write_samples, terrainfile.py).

The CPU half checks the format's numpy mirror on a twin world (terrain_twin.py: oracle.Terrain plus the numpy smooth brush):
RAW bricks survive bit for bit, elided samples come back inside their sign class, and -- the point of the brick rule -- the oracle's
full extraction of the reconstructed grid is the extraction of the original grid, record for record.  The GPU half checks the library
against that mirror (kind tables, files read across, grids as uint32) and the same mesh exactness on the device, byte for byte.

Grids are compared as uint32 (NaN payloads, -0).  Mesh comparisons before / after a save are byte comparisons: the same code extracts
both grids, so nothing but the samples it reads can differ."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib, terrainfile as tf
from surface_twin import DeviceGrid
from terrain_twin import assert_grid, assert_triangles, bits, gpu_mod, twin_update, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INVALID, NO_RESULT = _lib.ERR_INVALID_ARG, _lib.ERR_NO_RESULT
PROTOTYPES = [
    "int32_t vtmc_terrain_save(vtmc_ctx *ctx, const char *path, uint32_t flags, int64_t *bytes_written);",
    "int32_t vtmc_terrain_load(vtmc_ctx *ctx, const char *path, uint32_t flags, int32_t *n_dirty_blocks, int32_t *tri_count);",
    "int32_t vtmc_terrain_write_samples(vtmc_ctx *ctx, const float *src, int64_t stride_x, int64_t stride_y, int64_t stride_z);",
]
NAMES = [re.search(r"(vtmc_\w+)\(", p).group(1) for p in PROTOTYPES]

# The twin world: a plane at a non-integer height through the middle of a 64 x 64 x 48 terrain, so the two brick layers below y = 16
# are FULL and the four above y = 40 VOID (6 of 9 layers elided before the edits), add and erode spheres, a cylinder and a smooth brush
# on the surface, one NaN planted deep in the void and one -0 deep in the solid.
DIMS, SCALE, ORIGIN, SEED = (64, 64, 48), 1.0, (0.0, 0.0, 0.0), 97531
WORLD = [("plane", (30.375, (-1, -1), (70, 70), True)), ("sphere", ((20.5, 31.25, 24.0), 7.5, True)),
         ("sphere", ((44.0, 29.5, 16.0), 6.0, False)), ("cylinder", ((5.0, 33.0, 5.0), (1.0, 0.25, 0.5), 40.0, 3.0, True)),
         ("smooth", ((30.0, 30.0, 24.0), 6.0, 0.75))]
NAN_AT, NEG0_AT = (60, 60, 40), (8, 4, 40)   # [x, y, z]
NAN_BITS, NEG0_BITS = 0x7FC12345, 0x80000000
AFTER = [("sphere", ((36.0, 31.0, 30.0), 5.5, True)), ("sphere", ((12.0, 30.0, 12.0), 4.0, False))]   # an edit after a load
N_BLOCKS = (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
_cache = {}


def plant(grid):
    """The NaN (with a payload) and the -0, as 32-bit words, into a grid indexed [x, y, z]."""
    w = grid.view(np.uint32)
    w[NAN_AT] = NAN_BITS
    w[NEG0_AT] = NEG0_BITS


def twin_world(oracle_mod):
    """The twin world's grid ([x, y, z], read-only) and its event counter; built once."""
    if "world" not in _cache:
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        twin_update(ref, oracle_mod, WORLD)
        plant(ref.grid)
        grid = ref.grid.copy(order="F")   # x fastest
        grid.setflags(write=False)
        _cache["world"] = (grid, ref.events)
    return _cache["world"]


def meta_of(events):
    return {"scale": SCALE, "origin": ORIGIN, "seed": SEED, "events": events}


def twin_file(oracle_mod, tmp_path_factory):
    """The mirror's file of the twin world (default flags) and what the mirror reads back from it; written once."""
    if "file" not in _cache:
        grid, events = twin_world(oracle_mod)
        path = str(tmp_path_factory.mktemp("terrain_io") / "twin.vtmt")
        n = tf.write_terrain(path, grid, meta_of(events))
        _cache["file"] = (path, n) + tf.read_terrain(path)
    return _cache["file"]


def kinds_of_file(path):
    hdr = tf.read_header(path)
    nb = tf.brick_counts(hdr["dims"])
    return hdr, np.fromfile(path, np.uint8, nb[0] * nb[1] * nb[2], offset=64)


def patched(src, dst, offset, data):
    blob = bytearray(open(src, "rb").read())
    blob[offset:offset + len(data)] = data
    open(dst, "wb").write(bytes(blob))
    return str(dst)


def hostile_files(good, tmp_path):
    """(label, path) of every rejection the format lists, made from one good file."""
    blob = open(good, "rb").read()
    hdr, kinds = kinds_of_file(good)
    first_raw, first_elided = int(np.flatnonzero(kinds == 0)[0]), int(np.flatnonzero(kinds != 0)[0])
    p = lambda name: tmp_path / (name + ".vtmt")   # noqa: E731
    out = [
        ("magic", patched(good, p("magic"), 0, b"VTMX")),
        ("version", patched(good, p("version"), 4, struct.pack("<I", 2))),
        ("dims not a multiple of 8", patched(good, p("dims8"), 12, struct.pack("<i", DIMS[0] + 4))),
        ("dims above 1024", patched(good, p("dims1032"), 16, struct.pack("<i", 1032))),
        ("dims negative", patched(good, p("dimsneg"), 20, struct.pack("<i", -8))),
        ("scale nan", patched(good, p("scalenan"), 24, struct.pack("<f", float("nan")))),
        ("scale zero", patched(good, p("scale0"), 24, struct.pack("<f", 0.0))),
        ("scale negative", patched(good, p("scaleneg"), 24, struct.pack("<f", -1.0))),
        ("origin inf", patched(good, p("origin"), 32, struct.pack("<f", float("inf")))),
        ("unknown kind", patched(good, p("kind3"), 64 + first_elided, b"\x03")),
        ("n_raw above the kind-0 count", patched(good, p("count_lo"), 64 + first_raw, b"\x01")),     # same size, one RAW byte fewer
        ("n_raw below the kind-0 count", patched(good, p("count_hi"), 64 + first_elided, b"\x00")),  # same size, one RAW byte more
        ("n_raw larger than the brick count", patched(good, p("nraw"), 52, struct.pack("<I", len(kinds) + 1))),
        ("n_raw huge", patched(good, p("nrawhuge"), 52, struct.pack("<I", 0xFFFFFFFF))),
    ]
    for label, data in (("truncated", blob[:-1]), ("truncated in the kind table", blob[:70]), ("header only", blob[:64]),
                        ("shorter than a header", blob[:40]), ("empty", b""), ("one byte too long", blob + b"\0")):
        path = p(label.replace(" ", "_"))
        path.write_bytes(data)
        out.append((label, str(path)))
    return out


# -- CPU: the interface ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_terrain_io_functions():
    text = " ".join(open(os.path.join(ROOT, "include", "vtmc.h")).read().split())
    for p in PROTOTYPES:
        assert p in text, p
    assert "#define VTMC_TERRAIN_SAVE_EXACT 1u" in text and "#define VTMC_TERRAIN_LOAD_NO_EXTRACT 1u" in text


def test_binding_lists_the_terrain_io_symbols():
    for name in NAMES:
        assert name in _lib.SYMBOLS, name


def test_extractor_has_the_terrain_io_methods():
    for name in ("terrain_save", "terrain_load", "terrain_write_samples"):
        assert callable(getattr(vt.Extractor, name, None)), name
    for name in ("classify_bricks", "write_terrain", "read_terrain"):
        assert callable(getattr(vt, name, None)), name


def test_integration_guide_has_a_dllimport_stub_for_each():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\[DllImport\([^\]]*\)\]\s*public static extern\s+int\s+%s\s*\(" % name, text), name


# -- CPU: the mirror --------------------------------------------------------------------------------------------------------------------
def test_the_twin_world_elides_most_bricks_and_holds_every_kind(oracle_mod):
    """A condition of the tests below, not a measurement: they could not fail on an all-RAW file."""
    grid, _ = twin_world(oracle_mod)
    kinds = tf.classify_bricks(grid)
    assert len(kinds) == 9 * 9 * 7
    n = np.bincount(kinds, minlength=3)
    assert n[tf.RAW] > 0 and n[tf.VOID] > 0 and n[tf.FULL] > 0, n
    assert 2 * (n[tf.VOID] + n[tf.FULL]) >= len(kinds), n
    nb = tf.brick_counts(DIMS)
    brick = lambda at: at[0] // 8 + nb[0] * (at[1] // 8 + nb[1] * (at[2] // 8))   # noqa: E731
    assert kinds[brick(NAN_AT)] == tf.RAW        # a NaN fails both own tests ...
    assert kinds[brick(NAN_AT) - 1] == tf.VOID   # ... and is no `s > 0` for its neighbours
    assert kinds[brick(NEG0_AT)] == tf.RAW and kinds[brick(NEG0_AT) + 1] == tf.RAW   # -0 is not > 0: nothing around it is FULL


def test_classify_bricks_by_the_definition(oracle_mod):
    """classify_bricks against the rule spelled out brick by brick in plain loops."""
    grid, _ = twin_world(oracle_mod)
    nb = tf.brick_counts(DIMS)
    got = tf.classify_bricks(grid).reshape(nb[2], nb[1], nb[0])
    with np.errstate(invalid="ignore"):
        for bz in range(nb[2]):
            for by in range(nb[1]):
                for bx in range(nb[0]):
                    own = grid[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8]
                    hood = grid[max(8 * bx - 8, 0):8 * bx + 16, max(8 * by - 8, 0):8 * by + 16, max(8 * bz - 8, 0):8 * bz + 16]
                    want = 1 if (own <= -1).all() and not (hood > 0).any() else (2 if (own >= 1).all() and (hood > 0).all() else 0)
                    assert got[bz, by, bx] == want, (bx, by, bz)


def test_mirror_round_trip(oracle_mod, tmp_path_factory):
    grid, events = twin_world(oracle_mod)
    path, n_bytes, meta, kinds, back = twin_file(oracle_mod, tmp_path_factory)
    assert np.array_equal(kinds, tf.classify_bricks(grid))
    n_raw = int((kinds == tf.RAW).sum())
    assert n_bytes == os.path.getsize(path) == 64 + tf.pad16(len(kinds)) + 2048 * n_raw == tf.file_size(DIMS, n_raw)
    assert meta["dims"] == DIMS and meta["seed"] == SEED and meta["events"] == events and meta["event"] == events + 1
    assert meta["scale"] == SCALE and meta["origin"] == ORIGIN and meta["n_raw"] == n_raw and meta["flags"] == 0
    nb = tf.brick_counts(DIMS)
    kind_s = np.repeat(np.repeat(np.repeat(kinds.reshape(nb[2], nb[1], nb[0]), 8, 0), 8, 1), 8, 2).transpose(2, 1, 0)[:66, :66, :50]
    raw = kind_s == tf.RAW
    assert np.array_equal(bits(back)[raw], bits(grid)[raw])   # RAW bricks bit for bit ...
    assert bits(back)[NAN_AT] == NAN_BITS and bits(back)[NEG0_AT] == NEG0_BITS   # ... the NaN's payload and the -0 among them
    void, full = back[kind_s == tf.VOID], back[kind_s == tf.FULL]
    assert void.size and (void >= -2).all() and (void < -1).all()   # elided samples: redrawn inside the range of their class ...
    assert full.size and (full >= 1).all() and (full < 2).all()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(back > 0, grid > 0)                   # ... with the inside-flag they had
    assert not np.array_equal(bits(back)[~raw], bits(grid)[~raw])  # redrawn under a new event number, not copied
    idx = np.flatnonzero(kind_s.transpose(2, 1, 0).ravel() == tf.VOID)[:5]
    assert np.array_equal(back.transpose(2, 1, 0).ravel()[idx], tf.terrain_uniform(SEED, events + 1, idx, 0) - f32(2))
    again = tf.read_terrain(path)
    assert np.array_equal(bits(again[2]), bits(back)) and np.array_equal(again[1], kinds)   # reading is deterministic


def test_the_hash_is_the_oracles(oracle_mod):
    """terrain_uniform against the committed oracle: a fresh twin is uniform(seed, 0, index, 0) - 2 at every sample."""
    ref = oracle_mod.Terrain(16, 8, 8, 1.0, ORIGIN, SEED)
    want = tf.terrain_uniform(SEED, 0, np.arange(ref._mem.size), 0) - f32(2)
    assert np.array_equal(bits(ref._mem.ravel()), bits(want))


def test_mirror_exact_save_round_trips_every_bit(oracle_mod, tmp_path):
    grid, events = twin_world(oracle_mod)
    path = str(tmp_path / "exact.vtmt")
    n_bytes = tf.write_terrain(path, grid, meta_of(events), exact=True)
    meta, kinds, back = tf.read_terrain(path)
    assert (kinds == tf.RAW).all() and meta["flags"] == tf.F_EXACT and n_bytes == tf.file_size(DIMS, len(kinds))
    assert np.array_equal(bits(back), bits(grid))


def test_the_rule_is_mesh_exact_on_the_oracle(oracle_mod, tmp_path_factory):
    """The oracle's full extraction of the reconstructed grid is that of the original grid: records as uint32, counts, offsets."""
    grid, _ = twin_world(oracle_mod)
    back = twin_file(oracle_mod, tmp_path_factory)[4]
    want, want_offs, want_cases = oracle_mod.extract_grid(np.ascontiguousarray(grid), threads=8, want_cases=True)
    got, got_offs, got_cases = oracle_mod.extract_grid(np.ascontiguousarray(back), threads=8, want_cases=True)
    assert len(want) > 5000 and len(got) == len(want)
    assert np.array_equal(got_offs, want_offs) and np.array_equal(got_cases, want_cases)
    assert got.tobytes() == want.tobytes()


def test_mirror_rejects_hostile_files(oracle_mod, tmp_path_factory, tmp_path):
    good = twin_file(oracle_mod, tmp_path_factory)[0]
    for label, path in hostile_files(good, tmp_path):
        with pytest.raises(ValueError):
            tf.read_terrain(path)
            pytest.fail("accepted: " + label)


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
def gpu_world(oracle_mod, history=0):
    """The twin world on the device, by the same queue (so the event counters agree), the NaN and the -0 written through
    terrain_write_samples."""
    ex, _ = world(oracle_mod, DIMS, SCALE, ORIGIN, SEED, WORLD)
    g = ex.terrain_read_samples()
    plant(g)
    ex.terrain_write_samples(g)
    assert_grid(ex, twin_world(oracle_mod)[0])
    if history:
        ex.terrain_set_history(history)
    return ex


def full_mesh(ex, indexed):
    """Everything the host can read of the last extract, as bytes."""
    if indexed:
        return tuple(a.tobytes() for a in ex.read_indexed_mesh())
    return tuple(a.tobytes() for a in ex.read_triangles())


def queries(ex):
    """A fixed batch of picks, sphere casts and closest points on the resident terrain, as bytes."""
    xs, zs = np.meshgrid(np.arange(3.0, 62.0, 2.3), np.arange(3.0, 46.0, 2.9))
    o = np.stack([xs.ravel(), np.full(xs.size, 55.0), zs.ravel()], axis=1).astype(f32)
    d = np.tile(f32([0.07, -1.0, 0.04]), (len(o), 1))
    rays = ex.terrain_raycast(o, d)
    assert (rays["triangle"] >= 0).sum() > len(o) // 2
    casts = ex.terrain_spherecast(o, d, 1.5)
    near = ex.terrain_closest_point(o - f32([0.0, 24.0, 0.0]), 4.0)
    assert (near["triangle"] >= 0).any()
    return rays.tobytes(), casts.tobytes(), near.tobytes()


@pytest.mark.gpu
def test_gpu_kinds_and_size_on_the_twin_world(oracle_mod, tmp_path):
    with gpu_world(oracle_mod) as ex:
        for exact in (False, True):
            path = str(tmp_path / ("twin%d.vtmt" % exact))
            n_bytes = ex.terrain_save(path, exact=exact)
            hdr, kinds = kinds_of_file(path)
            want = tf.classify_bricks(ex.terrain_read_samples())
            if exact:
                want[:] = tf.RAW
            assert np.array_equal(kinds, want), np.flatnonzero(kinds != want)[:10]
            n_raw = int((want == tf.RAW).sum())
            assert n_bytes == os.path.getsize(path) == 64 + tf.pad16(len(kinds)) + 2048 * n_raw
            assert hdr["n_raw"] == n_raw and hdr["events"] == len(WORLD) and hdr["seed"] == SEED and hdr["flags"] == int(exact)


@pytest.mark.gpu
def test_gpu_kinds_on_a_noise_world(tmp_path):
    """512 x 256 x 512: 65 x 33 x 65 bricks, rows of 514 samples (4 full 128-sample segments and one of 2), every brick-row shape."""
    dims = (512, 256, 512)
    with vt.Extractor(0) as ex:
        ex.terrain_init(*dims, 1.0, ORIGIN, 11)
        ex.terrain_update([vt.NoiseModifier(5, 5, 4.0 / 512, amplitude=40.0, ramp_scale=1.0, ramp_center=128.0)])
        path = str(tmp_path / "noise.vtmt")
        n_bytes = ex.terrain_save(path)
        assert n_bytes < 512 << 20
        hdr, kinds = kinds_of_file(path)
        want = tf.classify_bricks(ex.terrain_read_samples())
        assert np.array_equal(kinds, want), np.flatnonzero(kinds != want)[:10]
        n = np.bincount(want, minlength=3)
        assert n.min() > 1000, n
        assert n_bytes == os.path.getsize(path) == 64 + tf.pad16(len(kinds)) + 2048 * int(n[tf.RAW])
        assert hdr["dims"] == dims and hdr["events"] == 1


@pytest.mark.gpu
def test_gpu_files_read_across(oracle_mod, tmp_path_factory, tmp_path):
    """A library-saved file read by the mirror is the grid a fresh context holds after loading it, and a mirror-written file loads to
    the bits the mirror reads."""
    grid, events = twin_world(oracle_mod)
    mirror_path, _, _, mirror_kinds, mirror_grid = twin_file(oracle_mod, tmp_path_factory)
    lib_path = str(tmp_path / "lib.vtmt")
    with gpu_world(oracle_mod) as ex:
        ex.terrain_save(lib_path)
    assert open(lib_path, "rb").read() == open(mirror_path, "rb").read()   # the same classification, the same bytes
    meta, kinds, want = tf.read_terrain(lib_path)
    with vt.Extractor(0) as fresh:
        nd, T = fresh.terrain_load(lib_path)
        assert nd == N_BLOCKS and T > 5000
        assert_grid(fresh, want)
    with vt.Extractor(0) as fresh:
        fresh.terrain_load(mirror_path, extract=False)
        assert_grid(fresh, mirror_grid)


@pytest.mark.gpu
@pytest.mark.parametrize("indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("fast_math", [0, 1])
def test_gpu_mesh_is_exact_across_save_and_load(oracle_mod, tmp_path, fast_math, indexed):
    path = str(tmp_path / "w.vtmt")
    with gpu_world(oracle_mod) as ex:
        ex.set_tuning(emit_fast_math=fast_math)
        ex.set_output_mode(indexed)
        dg = DeviceGrid.of_terrain(ex)
        T = ex.extract_volumes_device(dg.ptr, dg.n, dg.strides)
        before, before_queries = full_mesh(ex, indexed), queries(ex)
        ex.terrain_save(path)
    assert (tf.read_header(path)["n_raw"] + 1) * 2 < 9 * 9 * 7   # most of the grid was elided
    with vt.Extractor(0) as fresh:
        fresh.set_tuning(emit_fast_math=fast_math)
        fresh.set_output_mode(indexed)
        nd, T2 = fresh.terrain_load(path)
        assert (nd, T2) == (N_BLOCKS, T) and T > 5000
        assert np.array_equal(fresh.terrain_dirty_blocks(), oracle_mod.all_blocks(*DIMS))
        assert full_mesh(fresh, indexed) == before
        assert queries(fresh) == before_queries


@pytest.mark.gpu
def test_gpu_exact_save_restores_every_bit(oracle_mod, tmp_path):
    grid, _ = twin_world(oracle_mod)
    path = str(tmp_path / "exact.vtmt")
    with gpu_world(oracle_mod) as ex:
        ex.terrain_save(path, exact=True)
    assert np.array_equal(bits(tf.read_terrain(path)[2]), bits(grid))
    with vt.Extractor(0) as fresh:
        fresh.terrain_init(8, 8, 8)   # load replaces an earlier terrain of another size
        fresh.terrain_load(path, extract=False)
        assert_grid(fresh, grid)


@pytest.mark.gpu
def test_gpu_state_after_load(oracle_mod, tmp_path):
    """The event counter runs on from saved + 1, the history is empty with its budget kept, and edits after a load can be undone."""
    grid, events = twin_world(oracle_mod)
    path = str(tmp_path / "w.vtmt")
    with gpu_world(oracle_mod) as ex:
        ex.terrain_save(path)
    meta, _, loaded = tf.read_terrain(path)
    ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
    ref._mem[...] = loaded.transpose(2, 1, 0)
    ref.events = meta["event"]
    assert ref.events == events + 1
    with vt.Extractor(0) as ex:
        ex.terrain_set_history(64 << 20)
        ex.terrain_init(16, 8, 8)
        ex.terrain_update([vt.SphereModifier((8.0, 4.0, 4.0), 3.0, True)])
        assert ex.terrain_history()[:2] == (1, 0)   # a step of the terrain the load replaces
        ex.terrain_load(path)
        assert ex.terrain_history() == (0, 0, 0)
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_undo()
        assert e.value.code == NO_RESULT
        n_dirty, T = ex.terrain_update([gpu_mod(s) for s in AFTER])
        dirty = twin_update(ref, oracle_mod, AFTER)
        assert_grid(ex, ref.grid)   # the clamp draws of the edit hashed events saved + 2, saved + 3
        assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
        nu, nr, used = ex.terrain_history()
        assert (nu, nr) == (1, 0) and used > 0   # the budget was kept: the edit was journaled
        ex.terrain_undo()
        assert_grid(ex, loaded)
        ex.terrain_redo()
        assert_grid(ex, ref.grid)


@pytest.mark.gpu
def test_gpu_load_without_extract_leaves_no_result(oracle_mod, tmp_path_factory):
    path = twin_file(oracle_mod, tmp_path_factory)[0]
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_update([gpu_mod(WORLD[0])])
        assert ex.last_counts()[1] > 0
        assert ex.terrain_load(path, extract=False) == (0, 0)
        with pytest.raises(vt.VtmcError) as e:
            ex.read_triangles()
        assert e.value.code == NO_RESULT
        assert len(ex.terrain_dirty_blocks()) == 0


@pytest.mark.gpu
def test_gpu_save_changes_nothing(oracle_mod, tmp_path):
    with gpu_world(oracle_mod, history=64 << 20) as ex:
        ex.terrain_update([gpu_mod(AFTER[0])])
        grid, mesh, hist, dirty = ex.terrain_read_samples(), full_mesh(ex, False), ex.terrain_history(), ex.terrain_dirty_blocks()
        a, b = str(tmp_path / "a.vtmt"), str(tmp_path / "b.vtmt")
        ex.terrain_save(a)
        ex.terrain_save(b, exact=True)
        assert_grid(ex, grid)
        assert full_mesh(ex, False) == mesh and ex.terrain_history() == hist and np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert tf.read_header(a)["events"] == tf.read_header(b)["events"] == len(WORLD) + 1   # the counter did not move
        ex.terrain_undo()
        assert_grid(ex, twin_world(oracle_mod)[0])


@pytest.mark.gpu
def test_gpu_write_samples_in_every_order(oracle_mod):
    dims = (24, 8, 16)
    dx, dy, dz = (d + 2 for d in dims)
    rng = np.random.default_rng(5)
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    field = (np.sin(x * 0.4) * 2.0 + np.cos(z * 0.3) * 1.5 + 5.0 - y + rng.uniform(-0.2, 0.2, x.shape)).astype(f32)
    clean = field.copy()
    words = field.view(np.uint32)
    words[3, 2, 1], words[dx - 1, dy - 1, dz - 1], words[0, 0, 0] = 0x7FC00BAD, 0x80000000, 0xFF800000   # NaN payload, -0, -inf
    layouts = {"x fastest": np.empty((dz, dy, dx), f32).transpose(2, 1, 0), "z fastest": np.empty((dx, dy, dz), f32),
               "y fastest": np.empty((dx, dz, dy), f32).transpose(0, 2, 1)}
    with vt.Extractor(0) as ex:
        ex.terrain_init(*dims)
        ex.terrain_set_history(1 << 20)
        for name, arr in layouts.items():
            ex.terrain_update([vt.SphereModifier((8.0, 4.0, 8.0), 3.0, True)])
            assert ex.terrain_history()[:2] == (1, 0)
            arr.view(np.uint32)[...] = words
            ex.terrain_write_samples(arr)
            assert ex.terrain_history() == (0, 0, 0), name
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(field)), name
            assert np.array_equal(bits(ex.terrain_read_samples(order="z")), bits(field)), name
        ex.terrain_write_samples(clean)   # the field without the planted specials: its mesh is the oracle's
        dg = DeviceGrid.of_terrain(ex)
        assert dg.n == dims
        T = ex.extract_volumes_device(dg.ptr, dg.n, dg.strides)
        assert T > 500
        assert_triangles(ex, oracle_mod, clean, oracle_mod.all_blocks(*dims), T)
        with pytest.raises(ValueError):
            ex.terrain_write_samples(np.zeros((dx, dy, dz + 8), f32))
        assert ex._L.vtmc_terrain_write_samples(ex._h, None, 1, dx, dx * dy) == INVALID
        assert ex._L.vtmc_terrain_write_samples(ex._h, field.ctypes.data_as(ctypes.c_void_p), 0, dx, dx * dy) == INVALID


@pytest.mark.gpu
def test_gpu_hostile_files_get_a_status_code_and_leave_the_terrain(oracle_mod, tmp_path_factory, tmp_path):
    good = twin_file(oracle_mod, tmp_path_factory)[0]
    with vt.Extractor(0) as ex:
        for fn in (lambda: ex.terrain_save(str(tmp_path / "none.vtmt")), lambda: ex._check(ex._L.vtmc_terrain_write_samples(ex._h, None, 1, 1, 1))):
            with pytest.raises(vt.VtmcError) as e:   # no terrain yet
                fn()
            assert e.value.code == NO_RESULT
    with gpu_world(oracle_mod, history=64 << 20) as ex:
        ex.terrain_update([gpu_mod(AFTER[0])])
        grid, mesh, hist = ex.terrain_read_samples(), full_mesh(ex, False), ex.terrain_history()
        cases = hostile_files(good, tmp_path) + [("missing", str(tmp_path / "no_such_file.vtmt")), ("a directory", str(tmp_path))]
        for label, path in cases:
            with pytest.raises(vt.VtmcError) as e:
                ex.terrain_load(path)
            assert e.value.code == INVALID, label
            assert ex.terrain_history() == hist and full_mesh(ex, False) == mesh, label
        assert_grid(ex, grid)
        L, h = ex._L, ex._h
        assert L.vtmc_terrain_load(h, None, 0, None, None) == INVALID and L.vtmc_terrain_load(h, good.encode(), 2, None, None) == INVALID
        assert L.vtmc_terrain_save(h, None, 0, None) == INVALID and L.vtmc_terrain_save(h, good.encode(), 2, None) == INVALID
        assert L.vtmc_terrain_save(None, good.encode(), 0, None) == INVALID and L.vtmc_terrain_load(None, good.encode(), 0, None, None) == INVALID
        assert L.vtmc_terrain_save(h, str(tmp_path / "no_dir" / "x.vtmt").encode(), 0, None) == INVALID
        assert_grid(ex, grid)
        assert os.path.getsize(good) == tf.file_size(DIMS, tf.read_header(good)["n_raw"])   # the flag error did not touch the file
        ex.terrain_load(good)   # and the context still works
        assert_grid(ex, twin_file(oracle_mod, tmp_path_factory)[4])
