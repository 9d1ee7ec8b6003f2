"""Floating terrain: the fragment query (vtmc_terrain_fragments) and the modifier that removes fragments (VTMC_MOD_DETACH).

The rule (include/vtmc.h, FRAGMENTS) is integers and 32-bit copies, so the device is compared with fragment_twin.py for EQUALITY: records
in order, grids and stamps as uint32.  Fields are placed with terrain_write_samples, so every bit is chosen.

The crafted field (32 x 24 x 32 cells, 34 x 26 x 34 samples, over a solid floor with two holes) holds: a fragment of one sample and one
of two; a one-sample-thick serpentine whose seed is the far end of the path; a U whose arms meet only in a far tile; a hollow shell with
a ball in it; a piece that touches the floor only across an edge and one only across a corner; a piece that reaches the interior box's
face with one corner sample; a row split by a NaN with a +0.0f and a -0.0f beside it; slabs of MAX_SAMPLES and MAX_SAMPLES + 1 samples.

The labelling kernel's tiles are 64 x 8 x 8 samples.  The serpentine of the crafted field crosses the tile borders along y six times and
along z nine times; a 34-sample axis has no border of a 64-sample tile, so the crossings along x (and a seed in the last tile along x)
are what test_gpu_wide_terrain_crosses_the_tile_borders_along_x is for, on a terrain of 194 samples along x."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
from volumetricterrain_amd.terrainfile import terrain_uniform
import fragment_twin as twin
from host_check import run_host_check
from extract_checks import assert_tris_match
from terrain_twin import bits, block_list, dirty_ids, image_bytes, invalid, no_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (32, 24, 32), 0.5, (-3.0, 1.0, 2.0), 4242
MAX_SAMPLES = 250
AIR, SOLID = f32(-0.75), f32(0.5)
HISTORY = 64 << 20


def world_of(sample, origin=ORIGIN, scale=SCALE):
    """The world position of a sample index triple: exact for these dyadic values, also as float32."""
    w = tuple(origin[k] + sample[k] * scale for k in range(3))
    assert all(float(f32(v)) == v for v in w)
    return w


# name -> (lower, upper) in world space
BOXES = {"far": ((-1e6,) * 3, (1e6,) * 3),                                  # clamps to the whole grid, the two extra sample planes included
         "interior": (world_of((4, 3, 7)), world_of((24, 15, 25))),          # 21 x 13 x 19 samples, origin no multiple of 8: cuts pieces
         "outside": ((1000.0,) * 3, (1010.0,) * 3)}                          # wholly outside the grid
CASES = [("far", 0), ("far", MAX_SAMPLES), ("interior", 0), ("outside", 0)]
CASE_IDS = ["%s-max%d" % c for c in CASES]


def fill(g, xs, ys, zs, value=SOLID):
    """Inclusive index ranges (a number or a (first, last) pair, either way round)."""
    sl = []
    for r in (xs, ys, zs):
        a, b = (r, r) if np.isscalar(r) else (min(r), max(r))
        sl.append(slice(a, b + 1))
    g[tuple(sl)] = value


@functools.lru_cache(maxsize=None)
def crafted_field():
    g = np.full(tuple(d + 2 for d in DIMS), AIR, f32)
    fill(g, (0, 33), (0, 1), (0, 33), f32(1.25))                     # the floor: two planes, anchored by every face it lies on
    fill(g, (12, 16), (0, 1), (3, 7), f32(-1.5))                     # hole 1
    fill(g, (12, 18), (0, 1), (12, 18), f32(-1.5))                   # hole 2, with a pillar in it that stands on the grid's face
    fill(g, 16, (0, 1), 16, f32(1.0))
    # 1. one sample, and two
    fill(g, 3, 4, 3)
    fill(g, (6, 7), 4, 3, f32(0.25))
    # 2. the serpentine: a simple path; its smallest grid index, (20, 4, 2), is one end of it
    fill(g, 20, 4, (2, 30))
    fill(g, 20, (4, 22), 30)
    fill(g, 20, 22, (4, 30))
    fill(g, (20, 22), 22, 4)
    fill(g, 22, (5, 22), 4)
    fill(g, 22, 5, (4, 28))
    fill(g, (22, 24), 5, 28)
    fill(g, 24, (5, 23), 28, f32(1.75))
    # 3. a U: two arms along z that meet only at z = 29
    fill(g, 28, 10, (3, 29))
    fill(g, 28, 12, (3, 29))
    fill(g, 28, 11, 29)
    # 4. a hollow shell and a ball in it: nested bounds
    fill(g, (3, 9), (8, 14), (10, 16), f32(0.75))
    fill(g, (4, 8), (9, 13), (11, 15), AIR)
    fill(g, (5, 7), 11, 13, f32(0.125))
    fill(g, 6, (10, 12), 13, f32(0.125))
    fill(g, 6, 11, (12, 14), f32(0.125))
    # 5. contact with anchored samples across an edge only (the floor beside hole 1) and across a corner only (the pillar in hole 2)
    fill(g, 12, 2, 5)
    fill(g, 15, 2, 15)
    # 6. three samples, the last on the interior box's face x = 24
    fill(g, (22, 24), 13, 20)
    # a small piece well inside the interior box
    fill(g, 15, (10, 11), 15)
    # 7. a row split by a NaN; a +0 and a -0 beside it: none of the three is solid
    fill(g, (3, 7), 18, 22, f32(0.5))
    g[5, 18, 22] = f32(np.nan)
    g[4, 19, 22] = f32(0.0)
    g[6, 19, 22] = f32(-0.0)
    # 8. slabs of exactly MAX_SAMPLES samples and of one more
    fill(g, (10, 19), 20, (3, 27), f32(1.5))
    fill(g, (10, 19), 24, (3, 27), f32(1.5))
    fill(g, 10, 24, 28, f32(1.5))
    g.setflags(write=False)
    return g


def sample_box(name, dims=DIMS, origin=ORIGIN, scale=SCALE, boxes=None):
    lower, upper = (boxes or BOXES)[name]
    return twin.sample_box(lower, upper, dims, scale, origin)


@functools.lru_cache(maxsize=None)
def crafted_case(name, most):
    """What the twin says about one case of the crafted field, computed once: the box, the records, the labels, and the grid after a
    detach under event number 1."""
    first, ext, low, up = sample_box(name)
    recs, lab = twin.fragments(crafted_field(), first, ext, most)
    gone, recs2 = twin.detach(crafted_field(), first, ext, most, SEED, 1)
    assert recs2.tobytes() == recs.tobytes()
    gone.setflags(write=False)
    return dict(first=first, ext=ext, low=low, up=up, recs=recs, lab=lab, detached=gone)


def new_world(field, dims=DIMS, origin=ORIGIN, scale=SCALE, history=0):
    ex = vt.Extractor(0)
    ex.terrain_init(*dims, scale, origin, SEED)
    ex.terrain_write_samples(np.array(field))
    if history:
        ex.terrain_set_history(history)
    return ex


def same_records(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def raw_query(ex, lower, upper, most, least, dst, capacity):
    """vtmc_terrain_fragments as it is: (status, *n_fragments)."""
    lo, up, n = (ctypes.c_float * 3)(*lower), (ctypes.c_float * 3)(*upper), ctypes.c_int32(-7)
    rc = ex._L.vtmc_terrain_fragments(ex._h, ctypes.byref(lo), ctypes.byref(up), most, least, None if dst is None else dst.ctypes.data, capacity,
                                      ctypes.byref(n))
    return rc, n.value


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_kind_and_the_struct():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vtmc.h")).read(), flags=re.S)
    m = re.search(r"#define\s+VTMC_MOD_DETACH\s+(\d+)", text)
    assert m and int(m.group(1)) == 11 == _lib.MOD_DETACH == vt.DetachModifier.kind
    body = re.search(r"typedef struct vtmc_fragment \{(.*?)\} vtmc_fragment;", text, re.S)
    assert body
    assert [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()] == [
        "int32_t seed[3]", "int32_t lo[3]", "int32_t hi[3]", "int32_t n_samples", "int32_t stamp_id", "int32_t reserved"]
    assert "vtmc_terrain_fragments" in _lib.SYMBOLS and re.search(r"int32_t vtmc_terrain_fragments\(", text)


def test_mirror_struct_layout():
    F = _lib.Fragment
    assert ctypes.sizeof(F) == 48 == _lib.FRAGMENT_DTYPE.itemsize == vt.FRAGMENT_DTYPE.itemsize
    want = [("seed", 0), ("lo", 12), ("hi", 24), ("n_samples", 36), ("stamp_id", 40), ("reserved", 44)]
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == want
    assert [(n, _lib.FRAGMENT_DTYPE.fields[n][1]) for n in _lib.FRAGMENT_DTYPE.names] == want


def test_the_documents_state_the_rule_and_the_flow():
    for doc in ("include/vtmc.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "vtmc_terrain_fragments" in text and "VTMC_MOD_DETACH" in text, doc
    header = " ".join(open(os.path.join(ROOT, "include", "vtmc.h")).read().split())
    assert "6-connectivity" in header and "LIBRARY'S OWN" in header and "ONE undo step" in header and "NaN is not solid" in header
    assert re.search(r"DllImport[^;]*vtmc_terrain_fragments", open(os.path.join(ROOT, "INTEGRATION.md")).read(), re.S)


def test_detach_modifier_to_struct():
    m = vt.DetachModifier((1.5, -2.0, 3.25), (4.0, 5.5, 6.0), 77).to_struct()
    assert (m.kind, m.add_or_erode, m.data, tuple(m.data_dims)) == (11, 0, None, (77, 0))
    assert tuple(m.lower) == (1.5, -2.0, 3.25) and tuple(m.upper) == (4.0, 5.5, 6.0) and tuple(m.p) == (0.0,) * 8
    m = vt.DetachModifier().to_struct()                                  # the whole terrain, no limit
    assert tuple(m.lower) == (-np.inf,) * 3 and tuple(m.upper) == (np.inf,) * 3 and tuple(m.data_dims) == (0, 0) and m.add_or_erode == 0
    assert tuple(vt.DetachModifier(max_samples=2 ** 31 - 1).to_struct().data_dims) == (2 ** 31 - 1, 0)


@pytest.mark.parametrize("args", [((np.nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, np.nan, 1)), ((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1, 1)),
                                  ((0, 0, 0), (1, 1, 1), -1), ((0, 0, 0), (1, 1, 1), 1.5), ((0, 0, 0), (1, 1, 1), 2 ** 31),
                                  ((0, 0, 0), (1, 1, 1), True)])
def test_mirror_rejects_what_the_library_rejects_by_value(args):
    with pytest.raises(ValueError):
        vt.DetachModifier(*args)


def test_null_pointers_are_errors_not_crashes():
    L = vt.load()
    n = ctypes.c_int32()
    lo, up = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    buf = np.zeros(4, _lib.FRAGMENT_DTYPE)
    assert L.vtmc_terrain_fragments(None, ctypes.byref(lo), ctypes.byref(up), 0, 0, buf.ctypes.data, 4, ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert L.vtmc_terrain_fragments(None, None, None, 0, 0, None, 0, None) == _lib.ERR_INVALID_ARG


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/fragments_host_check.cpp: the host half (csrc/terrain_fragments.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("fragments_host_check", tmp_path)


# -- CPU: the twin ----------------------------------------------------------------------------------------------------------------------
def test_twin_on_a_hand_written_case():
    """A 6 x 6 x 6 grid, the box all of it; the records below are typed in, not computed."""
    g = np.full((6, 6, 6), f32(-1.0), f32)
    g[1, 1, 1] = 0.5                                   # one sample
    g[3, 1, 1] = g[4, 1, 1] = 0.25                     # two
    g[1, 3, 3] = g[2, 4, 3] = 1.0                      # touch across an edge only: two fragments
    g[4, 2, 3] = g[4, 2, 4] = g[4, 3, 4] = 0.75        # an L of three
    g[2, 2, 0] = g[2, 2, 1] = 1.5                      # on the face z = 0: anchored
    g[3, 3, 3] = np.nan                                # not solid
    g[2, 3, 3] = 0.0                                   # not solid
    first, ext = (0, 0, 0), (6, 6, 6)
    recs, lab = twin.fragments(g, first, ext)
    want = [((1, 1, 1), (1, 1, 1), (1, 1, 1), 1), ((3, 1, 1), (3, 1, 1), (4, 1, 1), 2), ((4, 2, 3), (4, 2, 3), (4, 3, 4), 3),
            ((1, 3, 3), (1, 3, 3), (1, 3, 3), 1), ((2, 4, 3), (2, 4, 3), (2, 4, 3), 1)]
    assert [(tuple(r["seed"]), tuple(r["lo"]), tuple(r["hi"]), int(r["n_samples"])) for r in recs] == want
    assert (recs["stamp_id"] == 0).all() and (recs["reserved"] == 0).all()
    assert lab[2, 2, 1] == lab[2, 2, 0] == 2 + 6 * 2 and lab[3, 3, 3] == -1 and lab[2, 3, 3] == -1 and lab[4, 3, 4] == 4 + 6 * (2 + 6 * 3)
    small, _ = twin.fragments(g, first, ext, 2)        # the size limit leaves the L alone
    assert [tuple(r["seed"]) for r in small] == [(1, 1, 1), (3, 1, 1), (1, 3, 3), (2, 4, 3)]
    # a box that cuts the pair: its sample at x = 3 lies on the face x = 3 of the box [0, 3]^3 -- anchored, and no longer listed
    cut, _ = twin.fragments(g, first, (4, 4, 4))
    assert [tuple(r["seed"]) for r in cut] == [(1, 1, 1)]
    # the detach write: the void draw of the event at the sample's grid index, every other sample its bits
    out, _ = twin.detach(g, first, ext, 2, seed=9, event=5)
    for x, y, z in [(1, 1, 1), (3, 1, 1), (4, 1, 1), (1, 3, 3), (2, 4, 3)]:
        v = terrain_uniform(9, 5, np.array([x + 6 * (y + 6 * z)], np.uint64), 2)[0] - f32(2)
        assert out[x, y, z] == v and -2 <= v < -1
        out[x, y, z] = g[x, y, z]
    assert same_bits(out, g)
    # the stamp of the single sample: [0, 3]^3; the pair's first sample and the anchored piece in it become equally deep air
    a, n, s = twin.stamp(g, lab, recs[0], first, ext)
    assert a == (0, 0, 0) and n == (4, 4, 4) and s[1, 1, 1] == f32(0.5) and s[3, 1, 1] == f32(-0.25) and s[2, 2, 0] == f32(-1.5) and s[2, 2, 1] == f32(-1.5)
    assert s[1, 3, 3] == f32(-1.0)
    s[3, 1, 1], s[2, 2, 0], s[2, 2, 1], s[1, 3, 3] = 0.25, 1.5, 1.5, 1.0
    assert same_bits(s, g[:4, :4, :4])
    assert twin.stamp_box(recs[2], first, ext) == ((2, 0, 1), (4, 6, 5))


def test_the_crafted_field_holds_what_it_claims():
    g = crafted_field()
    far, far_small, inner, outside = (crafted_case(*c) for c in CASES)
    assert far["first"] == (0, 0, 0) and far["ext"] == (34, 26, 34)
    assert inner["first"] == (4, 3, 7) and inner["ext"] == (21, 13, 19)
    assert min(outside["ext"]) == 0 and len(outside["recs"]) == 0 and same_bits(outside["detached"], g)
    by_seed = {tuple(r["seed"]): r for r in far["recs"]}
    n_of = lambda seed: int(by_seed[seed]["n_samples"])   # noqa: E731
    assert n_of((3, 4, 3)) == 1 and n_of((6, 4, 3)) == 2
    assert n_of((20, 4, 2)) == 29 + 18 + 26 + 2 + 17 + 24 + 2 + 18                       # the serpentine, one piece
    assert tuple(by_seed[(20, 4, 2)]["hi"]) == (24, 23, 30)
    assert n_of((28, 10, 3)) == 27 + 27 + 1                                            # the U, one piece
    shell, ball = by_seed[(3, 8, 10)], by_seed[(6, 11, 12)]
    assert int(shell["n_samples"]) == 343 - 125 and int(ball["n_samples"]) == 7
    assert (shell["lo"] < ball["lo"]).all() and (ball["hi"] < shell["hi"]).all()        # nested bounds
    assert n_of((12, 2, 5)) == 1 and n_of((15, 2, 15)) == 1                            # edge and corner contact: still fragments
    assert n_of((22, 13, 20)) == 3 and (22, 13, 20) not in {tuple(r["seed"]) for r in inner["recs"]}   # anchored by the interior box's face
    assert n_of((3, 18, 22)) == 2 and n_of((6, 18, 22)) == 2                           # split by the NaN
    assert n_of((10, 20, 3)) == MAX_SAMPLES and n_of((10, 24, 3)) == MAX_SAMPLES + 1
    small = {tuple(r["seed"]) for r in far_small["recs"]}
    assert (10, 20, 3) in small and (10, 24, 3) not in small and len(far_small["recs"]) == len(far["recs"]) - 1
    inner_seeds = {tuple(r["seed"]) for r in inner["recs"]}
    assert (6, 11, 12) in inner_seeds and (15, 10, 15) in inner_seeds and (3, 8, 10) not in inner_seeds   # the ball stays loose, the cut shell hangs on the face
    assert len(far["recs"]) == 14 and same_bits(g[0], far["detached"][0])


# -- GPU --------------------------------------------------------------------------------------------------------------------------------
def state_of(ex):
    T = ex.last_counts()[1]
    tris = ex.read_triangles()[0].tobytes() if T else b""
    return bits(ex.terrain_read_samples()).tobytes(), ex.terrain_history(), ex.terrain_dirty_blocks().tobytes(), ex.last_counts(), tris


@pytest.mark.gpu
@pytest.mark.parametrize("name,most", CASES, ids=CASE_IDS)
def test_gpu_query_lists_the_twins_records_and_changes_nothing(name, most):
    want = crafted_case(name, most)["recs"]
    lower, upper = BOXES[name]
    with new_world(crafted_field(), history=HISTORY) as ex:
        # a session with something in every state the query must leave alone: a dig, taken back (the grid is the crafted field again)
        ex.terrain_update([vt.SphereModifier(world_of((20, 8, 16)), 2.0, False)])
        ex.terrain_undo()
        assert same_bits(ex.terrain_read_samples(), crafted_field())
        before = state_of(ex)
        assert before[1][:2] == (0, 1) and before[3][1] > 0
        got = ex.terrain_fragments(lower, upper, most)
        assert same_records(got, want), (got, want)
        # count only; too little room
        assert raw_query(ex, lower, upper, most, 1, None, 1000) == (_lib.OK, len(want))
        if len(want):
            buf = np.zeros(len(want), _lib.FRAGMENT_DTYPE)
            assert raw_query(ex, lower, upper, most, 1, buf, len(want) - 1) == (_lib.ERR_CAPACITY, len(want))
            assert not buf.tobytes().strip(b"\0")
        assert state_of(ex) == before
        assert ex.stamp_capture((0, 0, 0), (2, 2, 2)) == 1                 # neither call above captured anything: no stamp id was taken


@pytest.mark.gpu
@pytest.mark.parametrize("name,most", CASES, ids=CASE_IDS)
def test_gpu_detach_writes_the_twins_grid(name, most, oracle_mod):
    case = crafted_case(name, most)
    lower, upper = BOXES[name]
    nb = tuple(d // 8 for d in DIMS)
    dirty = block_list(dirty_ids(case["low"], case["up"], nb), nb)
    with new_world(crafted_field()) as ex:
        n_dirty, T = ex.terrain_update([vt.DetachModifier(lower, upper, most)])
        assert same_bits(ex.terrain_read_samples(), case["detached"])
        assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)      # those of any modifier with that box
        if len(dirty) == 0:
            assert T == 0
        else:
            tris, offs, _ = oracle_mod.extract_grid(np.ascontiguousarray(case["detached"]), dirty, threads=8)
            assert T == len(tris) and T > 0
            got, got_offs = ex.read_triangles()
            assert np.array_equal(got_offs, offs)
            assert_tris_match(got, tris)
        assert len(ex.terrain_fragments(lower, upper, most)) == 0
        left = ex.terrain_fragments(lower, upper, 0)                                           # what the size limit protected
        assert [int(n) for n in left["n_samples"]] == ([MAX_SAMPLES + 1] if most else [])


def pillar_field():
    """A floor, a 3 x 3 pillar on it and a block on top of the pillar: the dig at the pillar's neck leaves the block in the air."""
    g = np.full(tuple(d + 2 for d in DIMS), f32(-1.0), f32)
    fill(g, (0, 33), (0, 1), (0, 33), f32(1.0))
    fill(g, (15, 17), (2, 13), (15, 17), f32(1.0))
    fill(g, (12, 20), (14, 17), (12, 20), f32(1.0))
    return g


@pytest.mark.gpu
def test_gpu_a_dig_and_what_falls_off_are_one_undo_step(oracle_mod):
    field = pillar_field()
    centre, radius = world_of((16, 8, 16)), 2.0                                   # 4 samples: through the whole neck
    lower, upper = world_of((8, 0, 8)), world_of((24, 22, 24))
    ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
    ref.grid[...] = field
    sphere = oracle_mod.sphere_modifier(centre, radius, False)
    ref.update([sphere])
    first, ext, _, _ = twin.sample_box(lower, upper, DIMS, SCALE, ORIGIN)
    assert first == (8, 0, 8) and ext == (17, 23, 17)
    want, recs = twin.detach(ref.grid, first, ext, 0, SEED, 2)
    assert len(recs) == 1 and int(recs[0]["n_samples"]) == 9 * 9 * 4 + 9 + 8                # the block and the stub of the pillar under it: the plane y = 12 keeps all but its middle
    sphere_ext = twin.sample_box(sphere.lower, sphere.upper, DIMS, SCALE, ORIGIN)[1]
    step = image_bytes(sphere_ext) + image_bytes(ext)
    with new_world(field, history=HISTORY) as ex:
        ex.terrain_update([vt.SphereModifier(centre, radius, False), vt.DetachModifier(lower, upper)])
        assert same_bits(ex.terrain_read_samples(), want)
        assert ex.terrain_history() == (1, 0, step)
        ex.terrain_undo()
        assert same_bits(ex.terrain_read_samples(), field) and ex.terrain_history() == (0, 1, step)
        ex.terrain_redo()
        assert same_bits(ex.terrain_read_samples(), want) and ex.terrain_history() == (1, 0, step)
        assert len(ex.terrain_fragments()) == 0


@pytest.mark.gpu
def test_gpu_capture_makes_the_twins_stamps_and_a_paste_puts_a_fragment_back():
    case = crafted_case("far", 0)
    g, first, ext, lab = crafted_field(), case["first"], case["ext"], case["lab"]
    least = 3
    with new_world(g) as ex:
        got = ex.terrain_fragments(*BOXES["far"], 0, least)
        ids = got["stamp_id"].copy()
        got["stamp_id"] = 0
        assert same_records(got, case["recs"])
        assert ((ids > 0) == (got["n_samples"] >= least)).all() and (ids == 0).any()
        assert sorted(ids[ids > 0]) == list(range(1, int((ids > 0).sum()) + 1))
        for rec, sid in zip(got, ids):
            if sid:
                a, n, s = twin.stamp(g, lab, rec, first, ext)
                assert ex.fragment_stamp_box(rec) == (a, n) == twin.stamp_box(rec, first, ext)
                assert ex.stamp_dims(int(sid)) == n and min(n) >= 3
                assert same_bits(ex.stamp_read(int(sid)), s)
        ex.terrain_update([vt.DetachModifier()])
        assert same_bits(ex.terrain_read_samples(), case["detached"])
        # the U back where it was: unturned, in replace mode, at its own box
        k = [tuple(r["seed"]) for r in got].index((28, 10, 3))
        a, n = twin.stamp_box(got[k], first, ext)
        centre = world_of(tuple(a[i] + (n[i] - 1) / 2 for i in range(3)))
        ex.terrain_update([vt.StampModifier(int(ids[k]), n, centre, pitch=SCALE, mode="replace")])
        now = ex.terrain_read_samples()
        mine = lab == lab[28, 10, 3]
        assert mine.sum() == 55 and same_bits(now[mine], g[mine])
        back = ex.terrain_fragments()
        assert len(back) == 1 and same_records(back[:1], case["recs"][k:k + 1])
        ex.stamp_destroy(int(ids[k]))


NOISE_DIMS, NOISE_SEED = (64, 32, 64), 20


@functools.lru_cache(maxsize=None)
def noise_field():
    """Thresholded blocky noise over a floor: cubes of 4 samples, one coarse cell in six solid, and a sprinkle of single samples.  The seed
    was chosen on the CPU (the asserts of the test below)."""
    rng = np.random.default_rng(NOISE_SEED)
    shape = tuple(d + 2 for d in NOISE_DIMS)
    coarse = rng.random((17, 9, 17)) < 0.16
    solid = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]]
    solid |= rng.random(shape) < 0.002
    solid[:, :2, :] = True
    g = np.where(solid, rng.uniform(0.05, 1.9, shape), -rng.uniform(0.05, 1.9, shape)).astype(f32)
    g.setflags(write=False)
    return g


@pytest.mark.gpu
def test_gpu_many_components_on_the_whole_grid():
    g = noise_field()
    first, ext, _, _ = twin.sample_box(*BOXES["far"], NOISE_DIMS, SCALE, ORIGIN)
    assert ext == g.shape
    want, recs = twin.detach(g, first, ext, 0, SEED, 1)
    _, lab = twin.fragments(g, first, ext)
    assert len(recs) >= 100
    assert lab[0, 0, 0] in twin.anchored_roots(lab)
    x, y, z = np.nonzero(lab == lab[0, 0, 0])
    assert len(set(zip(x // 64, y // 8, z // 8))) > 4                                # the floor's component spans every tile of its layer
    with new_world(g, dims=NOISE_DIMS) as ex:
        assert same_records(ex.terrain_fragments(), recs)
        ex.terrain_update([vt.DetachModifier()])
        assert same_bits(ex.terrain_read_samples(), want)


WIDE_DIMS = (192, 8, 8)
WIDE_BOXES = {"far": BOXES["far"], "interior": (world_of((3, 1, 1)), world_of((193, 8, 8)))}


@functools.lru_cache(maxsize=None)
def wide_field():
    """194 x 10 x 10 samples: a serpentine that runs the length of x three times (tile borders at x = 64, 128, 192) and ends in a tail
    whose last sample, (192, 7, 2), is the smallest grid index of the piece: the seed lies in the last tile along x, at the far end of
    the path.  Beside it a fragment inside one tile, one astride a border, and a bar that reaches the grid's face."""
    g = np.full(tuple(d + 2 for d in WIDE_DIMS), AIR, f32)
    fill(g, (2, 192), 3, 3)
    fill(g, 192, (3, 5), 3)
    fill(g, (2, 192), 5, 3)
    fill(g, 2, (5, 7), 3)
    fill(g, (2, 192), 7, 3)
    fill(g, 192, 7, (2, 3))
    fill(g, (10, 12), 3, 6, f32(0.25))
    fill(g, (62, 66), 5, 6, f32(0.25))
    fill(g, (120, 193), 7, 7, f32(1.0))
    g.setflags(write=False)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["far", "interior"])
def test_gpu_wide_terrain_crosses_the_tile_borders_along_x(name):
    g = wide_field()
    lower, upper = WIDE_BOXES[name]
    first, ext, _, _ = twin.sample_box(lower, upper, WIDE_DIMS, SCALE, ORIGIN)
    assert ext == ((194, 10, 10) if name == "far" else (191, 8, 8))
    want, recs = twin.detach(g, first, ext, 0, SEED, 1)
    if name == "far":
        assert [tuple(r["seed"]) for r in recs] == [(192, 7, 2), (10, 3, 6), (62, 5, 6)] and int(recs[0]["n_samples"]) == 3 * 191 + 1 + 1 + 1
    else:
        assert [tuple(r["seed"]) for r in recs] == [(10, 3, 6), (62, 5, 6)]           # the box's face x = 3 cuts the rows: anchored
    with new_world(g, dims=WIDE_DIMS) as ex:
        assert same_records(ex.terrain_fragments(lower, upper), recs)
        ex.terrain_update([vt.DetachModifier(lower, upper)])
        assert same_bits(ex.terrain_read_samples(), want)


@pytest.mark.gpu
def test_gpu_rejections_leave_the_grid_and_the_history_untouched():
    g = crafted_field()
    with new_world(g, history=HISTORY) as ex:
        ex.terrain_update([vt.SphereModifier(world_of((20, 8, 16)), 2.0, False)])
        ex.terrain_undo()
        before = state_of(ex)
        dig = vt.SphereModifier(world_of((8, 8, 8)), 3.0, False).to_struct()
        keep = np.zeros(4, f32)

        def bad(**fields):
            m = vt.DetachModifier(*BOXES["interior"], 5).to_struct()
            for k, v in fields.items():
                if k == "dims":
                    m.data_dims[:] = v
                else:
                    setattr(m, k, v)
            return m

        for m in (bad(add_or_erode=1), bad(data=keep.ctypes.data), bad(dims=(5, 1)), bad(dims=(-1, 0))):
            assert "modifier 0" in invalid(ex, [m])
            assert "modifier 1" in invalid(ex, [dig, m])                        # history on: the queue is checked before its first write
            assert state_of(ex) == before
        nan = float("nan")
        for lower, upper in (((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, nan))):
            assert raw_query(ex, lower, upper, 0, 0, None, 0)[0] == _lib.ERR_INVALID_ARG
        assert raw_query(ex, (0, 0, 0), (1, 1, 1), -1, 0, None, 0)[0] == _lib.ERR_INVALID_ARG
        assert raw_query(ex, (0, 0, 0), (1, 1, 1), 0, -1, None, 0)[0] == _lib.ERR_INVALID_ARG
        assert ex._L.vtmc_terrain_fragments(ex._h, None, None, 0, 0, None, 0, None) == _lib.ERR_INVALID_ARG
        assert state_of(ex) == before
    with vt.Extractor(0) as ex:
        no_result(lambda: ex._check(raw_query(ex, (0, 0, 0), (1, 1, 1), 0, 0, None, 0)[0]))
