"""The path modifier of the device-resident terrain (VTMC_MOD_PATH: the union of tapered capsules over a segment soup): every write bit for
bit against the twin of path_twin.py, a numpy FP32 restatement of include/vtmc.h's rule that evaluates every segment on every sample of
the box.  The kernel prunes segments per tile; the header promises that the result never depends on it, so agreement with the un-pruned
twin on boxes of several tiles is the check.

That yardstick is itself checked here on the CPU without the code under test, against a scalar loop of the header's steps.

Grids are compared as uint32, every sample; triangles as in test_terrain.py: offsets and `block` exact, floats within 1e-5."""
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import terrain_twin
from terrain_twin import assert_grid, assert_triangles, bits, box_of, image_bytes, invalid
import path_twin
from path_twin import assert_update, path_density, path_host, step_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (64, 32, 64), 0.5, (-3.3, 1.7, 2.9), 97531   # 66 x 34 x 66 samples: 2 x 3 x 17 tiles of 64 x 16 x 4
PLANE = [("plane", (9.6, (-10, -10), (40, 40), True))]
C = _lib.PATH_CHUNK


def world(oracle_mod, specs=(), history=0, origin=ORIGIN):
    return terrain_twin.world(oracle_mod, DIMS, SCALE, origin, SEED, list(specs), history)


def path(segments, add=False, box=None):
    spec = ("path", dict(segments=np.asarray(segments, np.float64), addOrErode=add))
    return spec + (box,) if box else spec


def pos(i, k, origin=ORIGIN):
    """World coordinate of sample i on axis k, as the kernel computes it."""
    return float(f32(i) * f32(SCALE) + f32(origin[k]))


def winding(n=40, origin=ORIGIN):
    """A polyline of n segments across the whole grid along x, winding in y and z, its radius tapering from 3.0 to 0.6."""
    s = np.linspace(0.0, 1.0, n + 1)
    pts = np.stack([origin[0] + 33.0 * s, origin[1] + 8.5 + 4.5 * np.sin(7.0 * s), origin[2] + 16.0 + 11.0 * np.sin(11.0 * s + 0.4)], axis=1)
    return pts, 3.0 - 2.4 * s


def spans_tiles(ref, spec):
    first, ext, _ = box_of(ref, path_twin.gpu_struct(spec))
    return ext[0] > 64 and ext[1] > 16 and ext[2] > 4


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_path_kind():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    m = re.search(r"#define\s+VTMC_MOD_PATH\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.MOD_PATH == 10
    assert "bit for bit" in text[m.end():m.end() + 5000] and "never depends on how the kernel prunes" in text
    src = open(os.path.join(ROOT, "volumetricterrain_amd", "csrc", "terrain_path.h")).read()
    assert int(re.search(r"kPathChunk\s*=\s*(\d+)", src).group(1)) == C
    assert int(re.search(r"kPathMaxSegments\s*=\s*(\d+)", src).group(1)) == _lib.PATH_MAX_SEGMENTS == 65536


def test_path_mirror_bounds_and_struct():
    seg = np.array([[1.0, 2.0, 3.0, 0.5, 4.0, -1.0, 3.5, 2.0], [0.1, 7.3, -2.0, 1.25, 0.2, 7.0, 9.0, 0.0]], np.float64)
    p = vt.PathModifier(seg)
    s32 = seg.astype(f32)
    assert p.segments.dtype == f32 and np.array_equal(p.segments, s32)
    ends = np.concatenate([s32[:, 0:4], s32[:, 4:8]])
    assert np.array_equal(p.LowerBound, (ends[:, :3] - ends[:, 3:]).min(axis=0)) and p.LowerBound.dtype == f32
    assert np.array_equal(p.UpperBound, (ends[:, :3] + ends[:, 3:]).max(axis=0)) and p.UpperBound.dtype == f32
    assert np.array_equal(p.LowerBound, f32([-1.15, -3.0, -3.25])) and np.array_equal(p.UpperBound, f32([6.0, 8.55, 9.0]))
    m = p.to_struct()
    assert (m.kind, m.add_or_erode, tuple(m.data_dims)) == (_lib.MOD_PATH, 0, (2, 8)) and m.data == p.segments.ctypes.data
    assert all(v == 0.0 for v in m.p)
    assert np.array_equal(np.array(m.lower, f32), p.LowerBound) and np.array_equal(np.array(m.upper, f32), p.UpperBound)
    assert np.array_equal(path_twin.struct_segments(m), s32)
    assert vt.PathModifier(seg, addOrErode=True).to_struct().add_or_erode == 1
    # the struct keeps the array alive on its own
    m2 = vt.PathModifier(seg + 1.0).to_struct()
    assert np.array_equal(path_twin.struct_segments(m2), (seg + 1.0).astype(f32))


def test_path_mirror_polyline_and_tree_layout():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [4.0, 4.0, 4.0], [5.0, 3.0, 1.0]])
    r = np.array([1.0, 2.0, 0.5, 0.25])
    p = vt.PathModifier.from_polyline(pts, r)
    want = np.array([[*pts[i], r[i], *pts[i + 1], r[i + 1]] for i in range(3)], f32)
    assert np.array_equal(p.segments, want) and not p.AddOrErode
    assert np.array_equal(vt.PathModifier.from_polyline(pts, 0.75, addOrErode=True).segments[:, [3, 7]], np.full((3, 2), 0.75, f32))
    # RiverNode's shape: node 0 is the root; 1 and 2 hang off it, 3 off 1, 4 off 3; node 5 is a second root with child 6
    pos_ = np.arange(21, dtype=np.float64).reshape(7, 3)
    rad = np.array([3.0, 2.5, 2.0, 1.5, 1.0, 0.7, 0.4])
    parent = [-1, 0, 0, 1, 3, -1, 5]
    t = vt.PathModifier.from_tree(pos_, rad, parent)
    kids = [1, 2, 3, 4, 6]
    want = np.array([[*pos_[parent[k]], rad[parent[k]], *pos_[k], rad[k]] for k in kids], f32)
    assert np.array_equal(t.segments, want)


@pytest.mark.parametrize("bad", [np.zeros((0, 8)), np.zeros((3, 7)), np.zeros(8), np.zeros((65537, 8)),
                                 [[0, 0, 0, 1, 1, 1, 1, np.nan]], [[np.inf, 0, 0, 1, 1, 1, 1, 1]], [[0, 0, 0, -0.5, 1, 1, 1, 1]],
                                 [[0, 0, 0, 1, 1, 1, 1, -1e-3]], [[0, 0, 2.0 ** 20 + 1, 1, 1, 1, 1, 1]], [[0, 0, 0, 1, -1.1e6, 1, 1, 1]],
                                 [[0, 0, 0, 1, 1, 1, 1, 1e300]]])
def test_path_mirror_rejects_what_the_library_rejects(bad):
    with pytest.raises(ValueError):
        vt.PathModifier(bad)


def test_path_mirror_rejects_bad_curves():
    with pytest.raises(ValueError):
        vt.PathModifier.from_polyline([[0, 0, 0]], 1.0)
    with pytest.raises(ValueError):
        vt.PathModifier.from_tree([[0, 0, 0], [1, 1, 1]], 1.0, [-1, -1])
    with pytest.raises(ValueError):
        vt.PathModifier.from_tree([[0, 0, 0], [1, 1, 1]], 1.0, [-1, 2])


# -- CPU: the yardstick, without the code under test ----------------------------------------------------------------------------------------
def scalar_density(seg, p):
    """include/vtmc.h's steps, one float32 operation at a time, for one sample position."""
    q = f32(-np.inf)
    for s in np.asarray(seg, f32):
        ax, ay, az, ra, bx, by, bz, rb = s
        ex, ey, ez = f32(bx - ax), f32(by - ay), f32(bz - az)
        ll = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(ez * ez))
        il = f32(f32(1) / ll) if ll >= f32(1e-30) else f32(0)
        dr = f32(rb - ra)
        dx, dy, dz = f32(p[0] - ax), f32(p[1] - ay), f32(p[2] - az)
        t = f32(f32(f32(f32(dx * ex) + f32(dy * ey)) + f32(dz * ez)) * il)
        t = f32(0) if t < 0 else (f32(1) if t > 1 else t)
        cx, cy, cz = f32(dx - f32(ex * t)), f32(dy - f32(ey * t)), f32(dz - f32(ez * t))
        d = f32(np.sqrt(f32(f32(f32(cx * cx) + f32(cy * cy)) + f32(cz * cz))))
        r = f32(ra + f32(dr * t))
        f = f32(r - d)
        if f > q:
            q = f
    return q


def test_twin_density_is_the_scalar_loop():
    rng = np.random.default_rng(5)
    pts, rad = winding(12)
    seg = vt.PathModifier.from_polyline(pts, rad).segments
    seg = np.concatenate([seg, [[4.0, 9.0, 12.0, 1.5, 4.0, 9.0, 12.0, 1.5], [8.0, 6.0, 20.0, 0.0, 9.0, 8.0, 21.0, 1.0]]]).astype(f32)   # a zero-length one, a cone
    px = (rng.integers(0, 66, 7).astype(f32) * f32(SCALE) + f32(ORIGIN[0]))
    py = (rng.integers(0, 34, 6).astype(f32) * f32(SCALE) + f32(ORIGIN[1]))
    pz = (rng.integers(0, 66, 8).astype(f32) * f32(SCALE) + f32(ORIGIN[2]))
    got = path_density(seg, px[None, None, :], py[None, :, None], pz[:, None, None])
    assert got.shape == (8, 6, 7) and got.dtype == f32
    want = np.array([[[scalar_density(seg, (x, y, z)) for x in px] for y in py] for z in pz], f32)
    assert np.array_equal(bits(got), bits(want))
    assert (got > 0).any() and (got < -2).any()
    # the zero-length segment alone is SphereModifier's density, with t = +-0
    e, il, dr = path_host(seg[-2:-1])
    assert not e.any() and il[0] == 0 and dr[0] == 0
    d = np.sqrt(((px - f32(4))[None, None, :] ** 2 + (py - f32(9))[None, :, None] ** 2) + (pz - f32(12))[:, None, None] ** 2)
    assert np.array_equal(bits(path_density(seg[-2:-1], px[None, None, :], py[None, :, None], pz[:, None, None])), bits(f32(1.5) - d))


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("add", [True, False], ids=["add_on_fresh", "erode_on_plane"])
def test_gpu_winding_polyline_bitwise(oracle_mod, add):
    ex, ref = world(oracle_mod, () if add else PLANE)
    with ex:
        pts, rad = winding(40)
        spec = path(vt.PathModifier.from_polyline(pts, rad).segments, add)
        assert spans_tiles(ref, spec)
        taken = {"low": 0, "high": 0}
        n_dirty, T = assert_update(ex, ref, oracle_mod, [spec], taken)
        assert n_dirty > 0 and T > 0
        assert taken["low"] > 0 and taken["high"] > 0   # both clamp branches in the one call


def cluster(n, seed):
    """n short segments around one point of the box's first tile: every one reaches that tile."""
    rng = np.random.default_rng(seed)
    a = np.array([pos(20, 0), pos(8, 1), pos(2, 2)]) + rng.uniform(-2.0, 2.0, (n, 3))
    b = a + rng.uniform(-1.5, 1.5, (n, 3))
    return np.column_stack([a, rng.uniform(0.2, 1.2, n), b, rng.uniform(0.2, 1.2, n)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, C - 1, C, C + 1, 3 * C + 7])
def test_gpu_chunk_edges(oracle_mod, n):
    ex, ref = world(oracle_mod, PLANE)
    with ex:
        seg = cluster(n, n)
        box = ((pos(0, 0) - 1.0, pos(0, 1) - 1.0, pos(0, 2) - 1.0), (pos(65, 0) + 1.0, pos(17, 1) - 0.1, pos(5, 2) - 0.1))   # 66 x 18 x 6 samples: 2 x 2 x 2 tiles
        spec = path(seg, n % 2 == 0, box)
        first, ext, _ = box_of(ref, path_twin.gpu_struct(spec))
        assert (tuple(first), tuple(ext)) == ((0, 0, 0), (66, 18, 6))
        assert_update(ex, ref, oracle_mod, [spec])


SWEEP = (-0.2, -0.1, -0.02, 0.0, 0.02, 0.1, 0.2)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["origin", "origin_plus_1000"])
def test_gpu_pruning_boundary(oracle_mod, shift):
    """Segments parallel to a tile face, at max(ra, rb) + 2 + delta from it: delta runs over both sides of the kernel's pruning reach
    (its slack is 0.01 in the first world and about 0.1 in the shifted one), so the tile beyond the face takes the segment in some
    updates and skips it in others.  Each update also carries segments wholly outside the grid."""
    origin = tuple(o + shift for o in ORIGIN)
    ex, ref = world(oracle_mod, PLANE, origin=origin)
    with ex:
        mid = [pos(33, k, origin) for k in range(3)]
        whole = (tuple(o - 1.0 for o in origin), tuple(o + 40.0 for o in origin))   # every sample of the grid: the tiles start at sample 0
        far = [[origin[0] - 60.0, mid[1], mid[2], 1.0, origin[0] - 50.0, mid[1] + 3.0, mid[2], 2.0],
               [mid[0], origin[1] + 70.0, mid[2], 0.5, mid[0] + 5.0, origin[1] + 75.0, mid[2] + 5.0, 0.5]]
        ra, rb = 0.7, 1.1
        n = 0
        # (axis, the last sample of a tile on it): the face between that tile and the next
        for axis, last in ((0, 63), (1, 15), (2, 31)):
            u, v = [k for k in range(3) if k != axis]
            for side in (-1, 1):   # the segment lies before the face (the tile behind it may skip it) or behind it
                face = pos(last + 1, axis, origin) if side < 0 else pos(last, axis, origin)
                for delta in SWEEP:
                    a, b = [0.0] * 3, [0.0] * 3
                    a[axis] = b[axis] = face + side * (max(ra, rb) + 2.0 + delta)
                    a[u], b[u] = mid[u] - 4.0, mid[u] + 4.0
                    a[v], b[v] = mid[v] - 2.0, mid[v] + 3.0
                    spec = path([[*a, ra, *b, rb]] + far, n % 2 == 0, whole)
                    ex.terrain_update([path_twin.gpu_struct(spec)])
                    path_twin.twin_update(ref, oracle_mod, [spec])
                    assert np.array_equal(bits(ex.terrain_read_samples()), bits(ref.grid)), (axis, side, delta)
                    n += 1
        assert n == 42
        before = ref.grid.copy()
        assert_update(ex, ref, oracle_mod, [path(far, False, whole)])   # every tile skips every segment and still writes: md is the void draw
        assert not np.array_equal(bits(ref.grid), bits(before))


@pytest.mark.gpu
@pytest.mark.parametrize("add", [True, False], ids=["add", "erode"])
def test_gpu_single_point_segment_is_the_sphere(oracle_mod, add):
    c, r = (13.1, 10.3, 19.6), 16.6   # the box is the whole grid
    ex, ref = world(oracle_mod, PLANE)
    ex2, ref2 = world(oracle_mod, PLANE)
    with ex, ex2:
        sphere = ("sphere", (c, r, add))
        spec = path([[*c, r, *c, r]], add)
        ms, mp = terrain_twin.gpu_struct(sphere), path_twin.gpu_struct(spec)
        assert tuple(ms.lower) == tuple(mp.lower) and tuple(ms.upper) == tuple(mp.upper)   # SphereModifier's box
        assert spans_tiles(ref, spec)
        assert_update(ex, ref, oracle_mod, [spec])
        terrain_twin.assert_update(ex2, ref2, oracle_mod, [sphere])
        assert np.array_equal(bits(ref.grid), bits(ref2.grid))   # the twins agree: the path rule reduces to the oracle's sphere
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(ex2.terrain_read_samples()))


@pytest.mark.gpu
def test_gpu_degenerate_segments(oracle_mod):
    ex, ref = world(oracle_mod, PLANE)
    with ex:
        pts, rad = winding(9)
        seg = list(vt.PathModifier.from_polyline(pts, rad).segments.astype(np.float64))
        seg.insert(4, [5.0, 10.0, 12.0, 1.8, 5.0, 10.0, 12.0, 0.6])     # zero length, the radii differ: the first one counts
        seg.insert(2, [2.0, 8.0, 25.0, 0.0, 9.0, 11.0, 30.0, 2.2])      # ra = 0: a cone
        seg.append([20.0, 12.0, 9.0, 2.5, 24.0, 7.0, 6.0, 0.0])         # rb = 0
        seg.append([15.0, 9.0, 30.0, 0.0, 15.0, 9.0, 30.0, 0.0])        # a point of radius 0
        seg.append([0.0, 9.0, 9.0, 1.0, 1e-20, 9.0, 9.0, 1.0])          # ll = 1e-40 is below 1e-30: il = 0
        for add in (False, True):
            spec = path(seg, add)
            assert spans_tiles(ref, spec)
            assert_update(ex, ref, oracle_mod, [spec])


@pytest.mark.gpu
def test_gpu_two_paths_in_one_queue(oracle_mod):
    ex, ref = world(oracle_mod)
    with ex:
        pts, rad = winding(24)
        river = vt.PathModifier.from_polyline(pts, rad).segments
        road = vt.PathModifier.from_polyline([[0.0, 12.0, 30.0], [10.0, 9.0, 22.0], [22.0, 8.0, 24.0], [28.0, 11.0, 8.0]], [1.4, 2.6, 1.0, 1.9]).segments
        queue = [PLANE[0], path(river, False), ("sphere", ((14.0, 9.0, 18.0), 3.1, True)), path(road, True)]
        events = ref.events
        n_dirty, T = assert_update(ex, ref, oracle_mod, queue)
        assert ref.events == events + 4 and n_dirty > 0 and T > 0   # one event number per modifier
        # the same four as four updates: the event numbers, and so every draw, are the same
        ex2, ref2 = world(oracle_mod)
        with ex2:
            for spec in queue:
                ex2.terrain_update([path_twin.gpu_struct(spec)])
            assert_grid(ex2, ref.grid)
        # swapped data would show: the second path alone differs from the first
        assert not np.array_equal(river[:4], road[:4]) and len(river) != len(road)


@pytest.mark.gpu
def test_gpu_history_one_step_one_box(oracle_mod):
    ex, ref = world(oracle_mod, PLANE, history=32 << 20)
    with ex:
        pts, rad = winding(40)
        spec = path(vt.PathModifier.from_polyline(pts, rad).segments, False)
        before = ref.grid.copy()
        n_dirty, T = assert_update(ex, ref, oracle_mod, [spec])
        dirty = ex.terrain_dirty_blocks().copy()
        after = ref.grid.copy()
        first, ext, _ = box_of(ref, path_twin.gpu_struct(spec))
        assert ex.terrain_history() == (1, 0, image_bytes(ext)) and image_bytes(ext) == step_bytes(ref, [spec])   # one step, one box, no halo
        nd, T_undone = ex.terrain_undo()
        assert nd == n_dirty
        assert_grid(ex, before)
        assert np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert_triangles(ex, oracle_mod, before, dirty, T_undone)
        assert ex.terrain_history() == (0, 1, image_bytes(ext))
        assert ex.terrain_redo() == (n_dirty, T)
        assert_grid(ex, after)
        assert np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert_triangles(ex, oracle_mod, after, dirty, T)
        assert ex.terrain_history() == (1, 0, image_bytes(ext))


def raw_path(seg, n=None, width=8, null=False, add=0):
    """A vtmc_modifier the mirror would refuse to build."""
    seg = np.ascontiguousarray(seg, f32)
    m = _lib.Modifier(_lib.MOD_PATH, add)
    m.lower[:], m.upper[:] = (2.0, 5.0, 7.0), (12.0, 14.0, 20.0)
    m.data = None if null else seg.ctypes.data
    m.data_dims[:] = (len(seg) if n is None else n, width)
    m._keep = seg
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("history", [0, 32 << 20], ids=["history_off", "history_on"])
def test_gpu_rejections_name_the_modifier_and_write_nothing(oracle_mod, history):
    ex, ref = world(oracle_mod, PLANE, history)
    with ex:
        ok = np.array([[4.0, 9.0, 10.0, 1.5, 9.0, 10.0, 15.0, 0.8], [9.0, 10.0, 15.0, 0.8, 10.0, 8.0, 18.0, 1.1]], f32)

        def with_value(row, col, v):
            s = ok.copy()
            s[row, col] = v
            return s
        bad = [(raw_path(ok, null=True), "null"), (raw_path(ok, n=0), "segment count"), (raw_path(ok, n=-3), "segment count"),
               (raw_path(ok, n=65537), "segment count"), (raw_path(ok, width=7), "8 floats"), (raw_path(ok, width=9), "8 floats")]
        bad += [(raw_path(with_value(k % 2, k, v)), "not finite") for k in range(8) for v in (np.nan, np.inf, -np.inf)]
        bad += [(raw_path(with_value(1, 3, -0.25)), "radius"), (raw_path(with_value(0, 7, -1e-6)), "radius")]
        bad += [(raw_path(with_value(k % 2, k, v)), "2^20") for k in range(8) for v in (2.0 ** 20 + 1.0, -3e7) if not (k in (3, 7) and v < 0)]
        first = [] if not history else [vt.SphereModifier((9.0, 8.0, 14.0), 2.0, True)]   # history on: the whole queue is checked first
        for m, word in bad:
            msg = invalid(ex, first + [m])
            assert "modifier %d" % len(first) in msg and word in msg, msg
            assert_grid(ex, ref.grid)
            assert ex.terrain_history() == (0, 0, 0)
        ex.terrain_update([raw_path(ok)])                              # the well-formed one is accepted,
        ex.terrain_update([raw_path(with_value(0, 0, 2.0 ** 20))])     # and 2^20 itself is inside the limit
