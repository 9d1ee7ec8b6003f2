"""Stamps (vtmc_stamp_*) and the stamp modifier (VTMC_MOD_STAMP): every paste bit for bit against the twin of stamp_twin.py, a numpy
FP32 restatement of include/vtmc.h's rule on the memory of the terrain twin.

That yardstick is itself checked here on the CPU without the code under test: its interpolation against scipy.ndimage.map_coordinates,
its coordinates against the same map in float64, and the exact-copy property on a random grid.

Grids are compared as uint32, every sample; triangles as in test_terrain.py: offsets and `block` exact, floats within 1e-5."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
from volumetricterrain_amd.terrainfile import terrain_uniform
import terrain_twin
from terrain_twin import assert_grid, assert_triangles, bits, box_of, invalid, no_result
import stamp_twin
from stamp_twin import apply_stamp, assert_update, footprint, stamp_coords, stamp_map, stamp_values, step_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (48, 24, 40), 0.5, (-3.0, 1.5, 2.5), 2468
WORLD = [("plane", (7.3, (-10, -10), (40, 40), True)), ("sphere", ((6.0, 8.0, 12.0), 3.2, True)), ("sphere", ((14.0, 7.0, 10.0), 2.6, False)),
         ("noise", dict(seed=5, octaves=3, frequency=0.35, amplitude=0.8, ramp_scale=0.4, ramp_center=7.0, lower=(-5.0, 0.0, 0.0), upper=(30.0, 20.0, 30.0)))]
SKEW = (0.3, -0.5, 0.2, 0.79)   # about a skew axis, not normalised
MODES = ("add", "erode", "replace")


def world(oracle_mod, history=0):
    return terrain_twin.world(oracle_mod, DIMS, SCALE, ORIGIN, SEED, WORLD, history)


def smooth_field(dims, seed=3, amplitude=1.5):
    """A smooth random field in [-amplitude, amplitude], indexed [x, y, z]: a few random plane waves."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims), indexing="ij")
    f = np.zeros(dims)
    for _ in range(6):
        k = rng.uniform(-0.6, 0.6, 3)
        f += rng.uniform(0.5, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
    return (f * (amplitude / np.abs(f).max())).astype(f32)


def stamp(stamp_id, dims, position, rotation=(0.0, 0.0, 0.0, 1.0), pitch=SCALE, mode="add"):
    return ("stamp", dict(stamp_id=stamp_id, dims=tuple(dims), position=position, rotation=rotation, pitch=pitch, mode=mode))


def raw_stamp(stamp_id, p=(5.0, 8.0, 10.0, 0.0, 0.0, 0.0, 1.0, 0.5), mode=0, lower=(2.0, 5.0, 7.0), upper=(8.0, 11.0, 13.0), add=1):
    """A vtmc_modifier the mirror would refuse to build, or one with a box of the test's own."""
    m = _lib.Modifier(_lib.MOD_STAMP, add)
    m.p[0:8] = tuple(float(v) for v in p)
    m.lower[:], m.upper[:] = lower, upper
    m.data_dims[:] = (stamp_id, mode)
    return m


def sample_pos(i, k):
    """World coordinate of sample i on axis k."""
    return float(f32(i) * f32(SCALE) + f32(ORIGIN[k]))


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_stamp_kind():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    m = re.search(r"#define\s+VTMC_MOD_STAMP\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.MOD_STAMP == 9
    assert not re.search(r"#define\s+VTMC_MOD_\w+\s+[67]\b", text)   # 6 and 7 stay unknown kinds
    for name in ("vtmc_stamp_create", "vtmc_stamp_capture", "vtmc_stamp_info", "vtmc_stamp_read", "vtmc_stamp_destroy"):
        assert name in text and name in _lib.SYMBOLS


def test_stamp_mirror_fills_the_struct():
    m = vt.StampModifier(7, (20, 12, 16), (1.5, -2.25, 3.0), SKEW, 0.37, "erode").to_struct()
    assert (m.kind, m.add_or_erode, tuple(m.data_dims)) == (_lib.MOD_STAMP, 0, (7, 0)) and not m.data
    assert np.array_equal(np.array(m.p, f32), f32([1.5, -2.25, 3.0, *SKEW, 0.37]))
    assert tuple(vt.StampModifier(7, (20, 12, 16), (0, 0, 0), mode="replace").to_struct().data_dims) == (7, 1)
    assert vt.StampModifier(7, (20, 12, 16), (0, 0, 0)).to_struct().add_or_erode == 1
    # identity: t -/+ h (n - 1) / 2, exactly
    t, h, n = np.array([1.5, -2.25, 3.0]), float(f32(0.37)), np.array([20, 12, 16])
    b = vt.StampModifier(7, n, t, pitch=0.37)
    assert np.array_equal(b.LowerBound, (t - h * (n - 1) / 2).astype(f32)) and np.array_equal(b.UpperBound, (t + h * (n - 1) / 2).astype(f32))
    s = b.to_struct()
    assert np.array_equal(np.array(s.lower, f32), b.LowerBound) and np.array_equal(np.array(s.upper, f32), b.UpperBound)
    # a quarter turn about z: the x and y extents swap
    r = np.sqrt(0.5)
    q = vt.StampModifier(7, n, t, (0.0, 0.0, r, r), 0.37)
    ext = (h * (n - 1) / 2)[[1, 0, 2]]
    assert np.array_equal(q.LowerBound, (t - ext).astype(f32)) and np.array_equal(q.UpperBound, (t + ext).astype(f32))
    # the box of a skew turn contains every corner of the stamp box
    k = vt.StampModifier(7, n, t, SKEW, 0.37)
    R = vt.modifiers.stamp_rotation(SKEW)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15)
    for c in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).reshape(3, -1).T:
        corner = t + R @ (c * h * (n - 1) / 2)
        assert (corner >= k.LowerBound - 1e-6).all() and (corner <= k.UpperBound + 1e-6).all()


@pytest.mark.parametrize("kw", [dict(position=(np.nan, 0, 0)), dict(position=(0, np.inf, 0)), dict(rotation=(0, 0, 0, 0)), dict(rotation=(0, np.nan, 0, 1)),
                                dict(rotation=(np.inf, 0, 0, 1)), dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=np.nan), dict(pitch=np.inf), dict(pitch=1e300),
                                dict(mode="paste"), dict(mode=1), dict(stamp_id=0), dict(stamp_id=-3), dict(stamp_id=1.5), dict(dims=(1, 8, 8)),
                                dict(dims=(8, 1027, 8)), dict(dims=(1026, 1026, 1026)), dict(dims=(8, 8))])
def test_stamp_mirror_rejects_what_the_library_rejects(kw):
    args = dict(stamp_id=1, dims=(8, 8, 8), position=(0.0, 0.0, 0.0))
    args.update(kw)
    with pytest.raises(ValueError):
        vt.StampModifier(**args)


# -- CPU: the yardstick, without the code under test ----------------------------------------------------------------------------------------
TWIN_CASES = [((0.0, 0.0, 0.0, 1.0), 0.5), (SKEW, 0.37), ((0.9, 0.1, -0.4, -0.2), 1.3), ((0.0, 0.0, 2.0, 2.0), 0.25)]


def twin_case(rotation, pitch, dims=(20, 12, 16)):
    t = (4.25, 8.5, 11.75)
    p = [*t, *rotation, pitch]
    px, py, pz = (np.arange(-6, 60).astype(f32) * f32(0.5) + f32(o) for o in ORIGIN)
    return p, dims, (px, py, pz), stamp_coords(px, py, pz, p, dims)


@pytest.mark.parametrize("rotation, pitch", TWIN_CASES)
def test_twin_interpolation_is_scipys(rotation, pitch):
    from scipy.ndimage import map_coordinates
    p, dims, _, (u, v, w) = twin_case(rotation, pitch)
    s = smooth_field(dims, amplitude=2.0)
    inside = footprint(u, v, w, dims)
    assert inside.sum() > 300
    got = stamp_values(s, u[inside], v[inside], w[inside])
    want = map_coordinates(s.astype(np.float64), np.stack([u[inside], v[inside], w[inside]]).astype(np.float64), order=1, mode="nearest")
    err = np.abs(got - want).max()
    print("max |twin - scipy| = %.3g over %d samples" % (err, inside.sum()))
    assert err <= 1e-5


@pytest.mark.parametrize("rotation, pitch", TWIN_CASES)
def test_twin_coordinates_are_the_float64_map(rotation, pitch):
    p, dims, (px, py, pz), got = twin_case(rotation, pitch)
    q = np.array(rotation, f32).astype(np.float64)
    x, y, z, w = q / np.sqrt((q * q).sum())
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    h = float(f32(pitch))
    d = np.stack(np.broadcast_arrays((px.astype(np.float64) - p[0])[None, None, :], (py.astype(np.float64) - p[1])[None, :, None],
                                     (pz.astype(np.float64) - p[2])[:, None, None]))
    want = np.einsum("ji,jzyx->izyx", R, d) / h + (np.array(dims, np.float64)[:, None, None, None] - 1) / 2
    tol = 16 * 2.0 ** -24 * (max(np.abs(a).max() for a in (px, py, pz)) / h + max(dims))
    err = max(np.abs(got[k] - want[k]).max() for k in range(3))
    print("max |twin - float64| = %.3g, bound %.3g" % (err, tol))
    assert err <= tol


def test_twin_identity_paste_is_an_exact_copy(oracle_mod):
    ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
    rng = np.random.default_rng(11)
    ref._mem[...] = rng.uniform(-2.0, 2.0, ref._mem.shape).astype(f32)
    first, n, shift = (3, 2, 5), (21, 14, 18), (12, 7, 9)
    src = ref.grid[tuple(slice(a, a + b) for a, b in zip(first, n))].copy()
    centre = tuple(sample_pos(first[k] + shift[k] + (n[k] - 1) / 2, k) for k in range(3))
    before = ref.grid.copy()
    _, n_in = apply_stamp(ref, vt.StampModifier(1, n, centre, pitch=SCALE, mode="replace").to_struct(), src)
    assert n_in == n[0] * n[1] * n[2]
    dst = tuple(slice(a + c, a + c + b) for a, b, c in zip(first, n, shift))
    assert np.array_equal(bits(ref.grid[dst]), bits(src))
    before[dst] = src
    assert np.array_equal(bits(ref.grid), bits(before))   # and nothing else changed


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("history", [0, 32 << 20], ids=["history_off", "history_on"])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_paste_bitwise(oracle_mod, mode, history):
    ex, ref = world(oracle_mod, history)
    with ex:
        s = smooth_field((20, 12, 16))
        sid = ex.stamp_create(s)
        assert ex.stamp_dims(sid) == (20, 12, 16) and np.array_equal(bits(ex.stamp_read(sid)), bits(s))
        spec = stamp(sid, s.shape, (-1.5, 8.0, 21.5), SKEW, 0.37, mode)
        first, ext, _ = box_of(ref, stamp_twin.gpu_mod(spec).to_struct())
        # cut by the grid's x = 0 and z = top faces; no extent a multiple of the launch shape's 64 x 16 x 4 (the exact move and the 1024^3
        # paste walk more than one run along y)
        assert first[0] == 0 and first[2] + ext[2] == DIMS[2] + 2 and ext[0] % 64 and ext[1] % 16 and ext[2] % 4, (first, ext)
        counts = []
        n_dirty, T = assert_update(ex, ref, oracle_mod, [spec], {sid: s}, counts)
        assert n_dirty > 0 and T > 0 and 0 < counts[0] < ext[0] * ext[1] * ext[2]   # some samples of the box inside the footprint, some not
        assert ex.terrain_history() == ((1, 0, step_bytes(ref, [spec])) if history else (0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(7, 5, 9), (6, 8, 4), (7, 6, 5)], ids=["odd", "even", "mixed"])
def test_gpu_footprint_edges(oracle_mod, n):
    """Identity, pitch = the voxel scale, the centre on a sample for an odd n and between two for an even n: u runs over 0 .. n - 1
    exactly.  The samples at u = 0 and u = n - 1 are written (the last one takes the clamped upper neighbour with weight 0); their
    neighbours outside the footprint, which the enlarged box hands to the kernel, keep their bits."""
    ex, ref = world(oracle_mod)
    with ex:
        first = (11, 6, 17)
        centre = tuple(sample_pos(first[k] + (n[k] - 1) / 2, k) for k in range(3))
        dst = tuple(slice(a, a + b) for a, b in zip(first, n))
        for seed, (lower, upper) in enumerate([(None, None), ([c - 6.0 for c in centre], [c + 6.0 for c in centre])]):
            s = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(f32)
            sid = ex.stamp_create(s)
            before = ex.terrain_read_samples().copy()
            mod = vt.StampModifier(sid, n, centre, pitch=SCALE, mode="replace").to_struct()
            if lower:
                mod.lower[:], mod.upper[:] = lower, upper
            box_first, ext, _ = box_of(ref, mod)
            if not lower:
                assert (tuple(box_first), tuple(ext)) == (first, n)   # the mirror's bounds are exactly the footprint
            else:
                assert all(box_first[k] < first[k] and box_first[k] + ext[k] > first[k] + n[k] for k in range(3))
            ex.terrain_update([mod])
            _, n_in = apply_stamp(ref, mod, s)
            assert n_in == n[0] * n[1] * n[2]
            got = ex.terrain_read_samples()
            assert np.array_equal(bits(got), bits(ref.grid))
            assert np.array_equal(bits(got[dst]), bits(s))
            before[dst] = s
            assert np.array_equal(bits(got), bits(before))


def tile_blocks(first, n):
    """The blocks whose 10^3 tile (samples 8b .. 8b + 9 per axis) lies inside the box [first, first + n)."""
    r = [[b for b in range(DIMS[k] // 8) if 8 * b >= first[k] and 8 * b + 9 <= first[k] + n[k] - 1] for k in range(3)]
    return [(bx, by, bz) for bz in r[2] for by in r[1] for bx in r[0]]


@pytest.mark.gpu
def test_gpu_exact_move(oracle_mod):
    ex, ref = world(oracle_mod)
    with ex, vt.Extractor(0) as ex2:
        ex.set_tuning(emit_fast_math=0)
        ex2.set_tuning(emit_fast_math=0)
        first, n, shift = (4, 4, 4), (26, 18, 26), (16, 0, 8)
        events = ref.events
        before = ex.terrain_read_samples().copy()
        sid = ex.stamp_capture(first, n)
        src = before[tuple(slice(a, a + b) for a, b in zip(first, n))]
        assert ex.stamp_dims(sid) == n and np.array_equal(bits(ex.stamp_read(sid)), bits(src))
        assert ((src > 0).any() and (src < 0).any())   # the box holds surface
        assert_grid(ex, before)                        # a capture changes nothing
        centre = tuple(sample_pos(first[k] + shift[k] + (n[k] - 1) / 2, k) for k in range(3))
        spec = stamp(sid, n, centre, mode="replace")
        n_dirty, T = assert_update(ex, ref, oracle_mod, [spec], {sid: src})
        assert ref.events == events + 1                # the capture took no event number
        after = ex.terrain_read_samples()
        dst_first = tuple(a + c for a, c in zip(first, shift))
        assert np.array_equal(bits(after[tuple(slice(a, a + b) for a, b in zip(dst_first, n))]), bits(src))
        # every block whose tile lies inside the pasted box meshes as the block 2, 0, 1 blocks back did in the source
        blocks = tile_blocks(dst_first, n)
        assert len(blocks) == 4
        tris, offs = ex.read_triangles()
        dirty = [tuple(b) for b in ex.terrain_dirty_blocks()]
        src_blocks = np.array([(bx - 2, by, bz - 1) for bx, by, bz in blocks], np.int32)
        T2 = ex2.extract_grid(before, src_blocks)
        want, want_offs = ex2.read_triangles()
        assert T2 > 0
        for i, b in enumerate(blocks):
            k = dirty.index(b)
            got_b, want_b = tris[offs[k]:offs[k + 1]], want[want_offs[i]:want_offs[i + 1]]
            assert len(got_b) == len(want_b)
            for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
                assert np.array_equal(bits(got_b[f]), bits(want_b[f])), (b, f)
        # a paste that overlaps its own source: the stamp is a copy, the twin agrees
        near = tuple(sample_pos(first[k] + (4, 0, 2)[k] + (n[k] - 1) / 2, k) for k in range(3))
        assert_update(ex, ref, oracle_mod, [stamp(sid, n, near, mode="replace")], {sid: src})


@pytest.mark.gpu
def test_gpu_queue_and_history(oracle_mod):
    ex, ref = world(oracle_mod, history=64 << 20)
    with ex:
        s = smooth_field((20, 12, 16), seed=8)
        sid = ex.stamp_create(s)
        stamps = {sid: s}
        queue = [("sphere", ((9.0, 8.0, 14.0), 2.5, True)), stamp(sid, s.shape, (8.0, 8.5, 13.0), SKEW, 0.37, "add"), ("smooth", ((9.0, 8.0, 13.0), 3.0, 0.8)),
                 stamp(sid, s.shape, (11.0, 7.5, 12.0), (0.1, 0.7, -0.2, 0.6), 0.3, "erode"),
                 ("noise", dict(seed=9, octaves=2, frequency=0.4, amplitude=0.7, lower=(4.0, 4.0, 8.0), upper=(14.0, 12.0, 18.0), add_or_erode=False))]
        only = [stamp(sid, s.shape, (15.0, 8.0, 9.0), (0.0, 0.38, 0.0, 0.92), 0.45, "replace")]
        snaps, results, events = [ref.grid.copy()], [], ref.events
        for specs in (queue, only):
            results.append(assert_update(ex, ref, oracle_mod, specs, stamps) + (ex.terrain_dirty_blocks(),))
            snaps.append(ref.grid.copy())
        assert ref.events == events + len(queue) + 1   # one event number per modifier, the stamps included
        want_bytes = step_bytes(ref, queue) + step_bytes(ref, only)
        assert ex.terrain_history() == (2, 0, want_bytes)
        for k in (1, 0):
            n_dirty, T = ex.terrain_undo()
            assert_grid(ex, snaps[k])
            assert n_dirty == results[k][0] and np.array_equal(ex.terrain_dirty_blocks(), results[k][2])
            assert_triangles(ex, oracle_mod, snaps[k], results[k][2], T)
        ex.stamp_destroy(sid)   # redo puts the journal's values back: the stamp is not read again
        for k in (0, 1):
            assert ex.terrain_redo() == results[k][:2]
            assert_grid(ex, snaps[k + 1])
        assert ex.terrain_history() == (2, 0, want_bytes)
        ex.terrain_undo()
        assert_grid(ex, snaps[1])


@pytest.mark.gpu
@pytest.mark.parametrize("history", [0, 32 << 20], ids=["history_off", "history_on"])
def test_gpu_rejections_name_the_modifier_and_write_nothing(oracle_mod, history):
    ex, ref = world(oracle_mod, history)
    with ex:
        sid, gone = ex.stamp_create(smooth_field((8, 6, 5))), ex.stamp_create(smooth_field((4, 4, 4)))
        ex.stamp_destroy(gone)
        ok = (5.0, 8.0, 10.0, 0.0, 0.0, 0.0, 1.0, 0.5)
        bad = [(raw_stamp(sid, ok[:k] + (v,) + ok[k + 1:]), "p[%d]" % k) for k in range(8) for v in (np.nan, np.inf)]
        bad += [(raw_stamp(sid, ok[:3] + (0.0, 0.0, 0.0, 0.0, 0.5)), "quaternion"), (raw_stamp(sid, ok[:7] + (0.0,)), "pitch"),
                (raw_stamp(sid, ok[:7] + (-0.5,)), "pitch"), (raw_stamp(sid + 100), "stamp id"), (raw_stamp(0), "stamp id"), (raw_stamp(gone), "stamp id"),
                (raw_stamp(sid, mode=2), "mode"), (raw_stamp(sid, mode=-1), "mode")]
        first = [] if not history else [vt.SphereModifier((9.0, 8.0, 14.0), 2.0, True)]   # history on: the whole queue is checked first
        for m, word in bad:
            msg = invalid(ex, first + [m])
            assert "modifier %d" % len(first) in msg and word in msg, msg
            assert_grid(ex, ref.grid)
            assert ex.terrain_history() == (0, 0, 0)
        for kind in (6, 7):
            m = raw_stamp(sid)
            m.kind = kind
            assert "unknown kind" in invalid(ex, [m])
        ex.terrain_update([raw_stamp(sid)])   # the well-formed one is accepted


def stamp_call_invalid(fn):
    with pytest.raises(vt.VtmcError) as e:
        fn()
    assert e.value.code == _lib.ERR_INVALID_ARG
    return str(e.value)


@pytest.mark.gpu
def test_gpu_stamp_calls_reject_bad_arguments():
    with vt.Extractor(0) as ex:
        no_result(lambda: ex.stamp_capture((0, 0, 0), (4, 4, 4)))   # before any terrain
        s = smooth_field((6, 5, 4))
        for at in ((0, 0, 0), (5, 4, 3), (2, 3, 1)):
            for v in (np.nan, np.inf, -np.inf):
                t = s.copy()
                t[at] = v
                assert "not finite" in stamp_call_invalid(lambda: ex.stamp_create(t))
        few, sid = np.zeros(64, f32), ctypes.c_int32()   # the dims are refused before a sample is read
        for nx, ny, nz in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1027, 4, 4), (4, 4, 1027), (1026, 1026, 1026), (512, 512, 513), (0, 4, 4), (-4, 4, 4)):
            stamp_call_invalid(lambda: ex._check(ex._L.vtmc_stamp_create(ex._h, few.ctypes.data, nx, ny, nz, 1, nx, nx * ny, ctypes.byref(sid))))
        for strides in ((0, 4, 16), (1, -4, 16), (1, 4, 0)):
            stamp_call_invalid(lambda: ex._check(ex._L.vtmc_stamp_create(ex._h, few.ctypes.data, 4, 4, 4, *strides, ctypes.byref(sid))))
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        before = ex.terrain_read_samples().copy()
        for first, n in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (51, 4, 4)), ((47, 0, 0), (4, 4, 4)), ((0, 23, 0), (4, 4, 4)), ((0, 0, 40), (4, 4, 4)),
                         ((0, 0, 0), (1, 4, 4)), ((0, 0, 0), (4, 4, 1027))):
            stamp_call_invalid(lambda: ex.stamp_capture(first, n))
        whole = ex.stamp_capture((0, 0, 0), tuple(d + 2 for d in DIMS))   # the whole grid is inside
        assert np.array_equal(bits(ex.stamp_read(whole)), bits(before))
        for bad_id in (0, -1, whole + 1):
            stamp_call_invalid(lambda: ex.stamp_dims(bad_id))
            stamp_call_invalid(lambda: ex.stamp_read(bad_id))
            stamp_call_invalid(lambda: ex.stamp_destroy(bad_id))
        ex.stamp_destroy(whole)
        stamp_call_invalid(lambda: ex.stamp_destroy(whole))
        assert ex.stamp_create(s) == whole + 1   # a refused call takes no id
        t = np.asfortranarray(s)[:, ::2, :]   # strides that are not the packed ones
        sid = ex.stamp_create(t)
        assert ex.stamp_dims(sid) == t.shape and np.array_equal(bits(ex.stamp_read(sid)), bits(t))
        assert_grid(ex, before)
        assert ex.terrain_history() == (0, 0, 0)


class _BoxAt:
    """A box of a grid standing in for the whole [z, y, x] memory: indexed with grid slices inside the box only."""

    def __init__(self, box, first):
        self.box, self.first = box, first   # box [z, y, x]; first (x, y, z)

    def _local(self, key):
        off = self.first[::-1]
        return tuple(slice(s.start - o, s.stop - o) for s, o in zip(key, off))

    def __getitem__(self, key):
        return self.box[self._local(key)]

    def __setitem__(self, key, value):
        self.box[self._local(key)] = value


@pytest.mark.gpu
def test_gpu_paste_into_a_1024_cube_terrain():
    """A turned CSG add near the far corner of a 1026^3-sample grid (4.3 GB: the box's byte offsets straddle 2^32; 64-bit sample indices in the
    kernel and in the clamp draws' hash), read back through a captured stamp and compared with the twin rule on that box alone: its samples before the paste are
    terrain_init's, uniform(seed, 0, index, 0) - 2."""
    W, seed = 1024, 17
    s = smooth_field((24, 16, 20), seed=4, amplitude=1.9)
    mod = vt.StampModifier(1, s.shape, (1015.0, 1012.0, 1018.0), SKEW, 0.9, "add").to_struct()

    class Twin:
        dims, scale, origin = (W, W, W), 1.0, np.zeros(3, f32)

    twin = Twin()
    twin.seed, twin.events = seed, 0
    first, ext, _ = box_of(twin, mod)
    assert first[0] + ext[0] == first[2] + ext[2] == W + 2 and min(ext) > 16   # cut by the far x and z faces; two runs along y
    x, y, z = (np.arange(first[k], first[k] + ext[k], dtype=np.uint64) for k in range(3))
    index = x[None, None, :] + np.uint64(W + 2) * (y[None, :, None] + np.uint64(W + 2) * z[:, None, None])
    assert 4 * int(index.min()) < 2 ** 32 < 4 * int(index.max())   # the box's byte offsets straddle 32 bits
    twin._mem = _BoxAt((terrain_uniform(seed, 0, index, 0) - f32(2)).astype(f32), first)
    _, n_in = apply_stamp(twin, mod, s)
    assert n_in > 1000
    with vt.Extractor(0) as ex:
        ex.terrain_init(W, W, W, 1.0, (0.0, 0.0, 0.0), seed)
        assert ex.stamp_create(s) == 1
        n_dirty, T = ex.terrain_update([mod])
        assert n_dirty > 0 and T > 0
        got = ex.stamp_read(ex.stamp_capture(first, ext))
    assert np.array_equal(bits(got.transpose(2, 1, 0)), bits(twin._mem.box))


@pytest.mark.gpu
def test_gpu_stamp_lifetime(tmp_path):
    ex = vt.Extractor(0)
    s = smooth_field((9, 7, 5))
    a = ex.stamp_create(s)
    ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
    ex.terrain_update([terrain_twin.gpu_mod(m) for m in WORLD])
    b = ex.stamp_capture((3, 3, 3), (10, 12, 14))
    kept = ex.stamp_read(b)
    assert (a, b) == (1, 2)
    path = str(tmp_path / "t.vtmt")
    ex.terrain_save(path)
    ex.terrain_init(32, 16, 24, 1.0, (0.0, 0.0, 0.0), 3)   # another terrain: the stamps stay
    assert np.array_equal(bits(ex.stamp_read(a)), bits(s)) and np.array_equal(bits(ex.stamp_read(b)), bits(kept))
    ex.terrain_load(path)
    assert ex.stamp_dims(a) == s.shape and np.array_equal(bits(ex.stamp_read(b)), bits(kept))
    n_dirty, T = ex.terrain_update([vt.StampModifier(b, (10, 12, 14), (8.0, 8.0, 12.0), mode="replace", pitch=SCALE)])   # and still paste
    assert n_dirty > 0
    ex.stamp_destroy(a)
    assert ex.stamp_create(s) == 3 and ex.stamp_capture((0, 0, 0), (2, 2, 2)) == 4   # ids are not reused
    with pytest.raises(vt.VtmcError):
        ex.stamp_read(a)
    ex.close()   # with three live stamps
    with vt.Extractor(0) as ex2:   # a new context counts from 1 again and knows none of them
        with pytest.raises(vt.VtmcError):
            ex2.stamp_dims(b)
        assert ex2.stamp_create(s) == 1
