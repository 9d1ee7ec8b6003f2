"""The noise modifier of the device-resident terrain (VTMC_MOD_NOISE: fBm, billow, ridged multifractal): every write bit for bit against
the twin of terrain_twin.py, whose noise_density is a numpy FP32 restatement of include/vtmc.h's rule and whose csg_write restates the
clamp draws (terrain_uniform / clamp_drawn).

That yardstick is itself checked here on the CPU against the committed oracle, not against the code under test: the twin's fBm equals
oracle/density_ref.c bit for bit, its permutation equals the oracle's, and its clamp draws and add / erode rule reproduce an oracle.Terrain
update.  Queues that mix kinds run the reference kinds on oracle.Terrain and brushes and noise on its memory, one event number each.

Grids are compared as uint32, every sample; triangles as in test_terrain.py: offsets and `block` exact, floats within 1e-5."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import terrain_twin
from terrain_twin import (assert_grid, assert_triangles, assert_update, bits, csg_write, gpu_mod, invalid, noise_density, oracle_mod_of,
                          permutation, positions, sample_range, step_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SEED = (64, 24, 48), 4321
WORLD = [("plane", (9.375, (-1, -1), (70, 70), True)), ("sphere", ((20.5, 10.25, 30.0), 7.5, True)),
         ("sphere", ((44.0, 9.5, 16.0), 6.0, False)), ("cylinder", ((5.0, 12.0, 5.0), (1.0, 0.25, 0.5), 50.0, 3.0, True))]
PLACES = [(1.0, (0.0, 0.0, 0.0)), (0.5, (-3.25, 1.5, 2.125))]   # (voxel scale, terrain origin)
BASES = ("fbm", "billow", "ridged")


def world(oracle_mod, place=PLACES[0], history=0):
    return terrain_twin.world(oracle_mod, DIMS, *place, SEED, WORLD, history)


def noise(basis="fbm", add=True, lower=None, upper=None, **kw):
    spec = dict(seed=77, octaves=4, frequency=0.11, basis=basis, add_or_erode=add, lower=lower, upper=upper)
    spec.update(kw)
    return ("noise", spec)


def raw_noise(p=(0.1, 2.0, 0.5, 1.0, 0.0, 0.0, 0.0, 1.0), seed=5, octaves=4, basis=0, lower=(10.0, 4.0, 10.0), upper=(30.0, 16.0, 30.0), kind=None):
    """A vtmc_modifier the mirror would refuse to build."""
    m = _lib.Modifier(_lib.MOD_NOISE if kind is None else kind, 1)
    m.p[0:8] = tuple(float(v) for v in p)
    m.lower[:], m.upper[:] = lower, upper
    m.data_dims[:] = (seed, octaves | (basis << 8))
    return m


# -- CPU: the interface -----------------------------------------------------------------------------------------------------------------
def test_header_defines_the_noise_kind():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    m = re.search(r"#define\s+VTMC_MOD_NOISE\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.MOD_NOISE == 8
    assert not re.search(r"#define\s+VTMC_MOD_\w+\s+[67]\b", text)   # 6 and 7 stay unknown kinds
    assert "LibNoise" in text   # the header says whose noise this is


def test_noise_mirror_fills_the_struct():
    b = vt.NoiseModifier(-12345, 6, 0.02, lacunarity=2.1, gain=0.45, basis="ridged", amplitude=1.5, bias=-0.25, ramp_scale=0.01,
                         ramp_center=12.0, ridge_offset=0.9, lower=(1.0, 2.0, 3.0), upper=(40.5, 20.0, 30.25), add_or_erode=False)
    m = b.to_struct()
    assert (m.kind, m.add_or_erode) == (_lib.MOD_NOISE, 0)
    assert np.array_equal(np.array(m.lower, f32), f32([1.0, 2.0, 3.0])) and np.array_equal(np.array(m.upper, f32), f32([40.5, 20.0, 30.25]))
    assert np.array_equal(np.array(m.p, f32), f32([0.02, 2.1, 0.45, 1.5, -0.25, 0.01, 12.0, 0.9]))
    assert tuple(m.data_dims) == (-12345, 6 | (2 << 8)) and not m.data
    d = vt.NoiseModifier(7, 3, 0.5).to_struct()   # defaults: fBm, lacunarity 2, gain .5, amplitude 1, the reference class's bounds
    assert np.array_equal(np.array(d.p, f32), f32([0.5, 2.0, 0.5, 1.0, 0.0, 0.0, 0.0, 1.0]))
    assert tuple(d.lower) == (0.0, 0.0, 0.0) and tuple(d.upper) == (1000.0, 1000.0, 1000.0)
    assert (d.kind, d.add_or_erode, tuple(d.data_dims)) == (8, 1, (7, 3))
    assert vt.NoiseModifier(2 ** 32 - 1, 1, 1.0, basis="billow").to_struct().data_dims[:] == [-1, 1 | (1 << 8)]   # the C# int _seed


@pytest.mark.parametrize("kw", [dict(octaves=0), dict(octaves=17), dict(octaves=2.5), dict(basis="simplex"), dict(basis=2), dict(frequency=np.nan),
                                dict(frequency=np.inf), dict(lacunarity=-np.inf), dict(gain=np.nan), dict(amplitude=np.inf), dict(bias=np.nan),
                                dict(ramp_scale=np.inf), dict(ramp_center=np.nan), dict(ridge_offset=np.inf), dict(frequency=1e300)])
def test_noise_mirror_rejects_what_the_library_rejects(kw):
    args = dict(seed=1, octaves=4, frequency=0.1)
    args.update(kw)
    with pytest.raises(ValueError):
        vt.NoiseModifier(**args)


# -- CPU: the yardstick against the committed oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1337, 2 ** 32 - 1, 0xDEADBEEF12345])
def test_twin_permutation_is_the_oracles(oracle_mod, seed):
    assert np.array_equal(permutation(seed), oracle_mod.permutation(seed).astype(np.int64))
    assert sorted(permutation(seed)) == list(range(256))


@pytest.mark.parametrize("prm, org", [
    ((1337, 0.0625, 8, 2.0, 0.5, 0.03125, 12.0), (0, 0, 0)),
    ((99, 0.113, 5, 2.17, 0.47, 0.0, 0.0), (-37, -5, -1000)),
    ((4242424242, 0.731, 1, 2.0, 0.5, -0.02, -3.5), (-9, 40, -3)),
    ((7, 0.25, 8, 2.0, 0.6, 0.011, 7.25), (-20, -13, -17)),        # lattice points: exact zeros and their signs
])
def test_twin_fbm_is_the_oracles_density_bit_for_bit(oracle_mod, prm, org):
    dx, dy, dz = 40, 26, 34
    seed, f, octaves, L, g, rs, rc = prm
    want = np.empty((dz, dy, dx), f32)
    p = oracle_mod.DensityParams(seed, f, octaves, L, g, rs, rc)
    oracle_mod.lib().vto_density_fill(ctypes.byref(p), org[0], org[1], org[2], dx, dy, dz, 1, dx, dx * dy, want.ctypes.data_as(ctypes.c_void_p))
    # positions as the terrain forms them at scale 1: (float)index * 1 + origin, exact for integers
    px, py, pz = (np.arange(n).astype(f32) * f32(1) + f32(o) for n, o in zip((dx, dy, dz), org))
    got = noise_density(permutation(seed), px[None, None, :], py[None, :, None], pz[:, None, None], octaves, 0, f, L, g, 1.0, 0.0, rs, rc)
    assert np.array_equal(bits(got), bits(want))


def test_twin_clamp_draws_reproduce_an_oracle_terrain_update(oracle_mod):
    """A plane and an eroding sphere through the twin's clamp draws and add / erode rule, against oracle/terrain_ref.c."""
    dims, scale, origin, seed = (32, 24, 40), 0.75, (-2.5, 1.25, 3.0), 991
    ref, twin = oracle_mod.Terrain(*dims, scale, origin, seed), oracle_mod.Terrain(*dims, scale, origin, seed)
    dims_s = tuple(d + 2 for d in dims)
    taken = np.zeros(2, np.int64)
    for spec in (("plane", (9.375, (-5, -5), (60, 60), True)), ("sphere", ((10.0, 8.0, 16.0), 6.5, False)), ("sphere", ((14.0, 9.0, 20.0), 4.0, True))):
        om = oracle_mod_of(oracle_mod, spec)
        ref.update([om])
        _, _, first, ext = sample_range(om, dims_s, scale, origin)
        px, py, pz = positions(twin, first, ext)
        if spec[0] == "plane":
            q = np.broadcast_to(f32(om.p[0]) - py[None, :, None], (ext[2], ext[1], ext[0]))
        else:
            ddx, ddy, ddz = px - f32(om.p[0]), py - f32(om.p[1]), pz - f32(om.p[2])
            q = f32(om.p[3]) - np.sqrt(((ddx * ddx)[None, None, :] + (ddy * ddy)[None, :, None]) + (ddz * ddz)[:, None, None])
        taken += csg_write(twin, first, ext, q, bool(om.add_or_erode))
        assert np.array_equal(bits(twin._mem), bits(ref._mem)), spec
    assert twin.events == ref.events == 3 and taken[0] > 0 and taken[1] > 0


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
def boxes(place):
    """World AABBs of one place: interior, clipped by the grid, one sample thick (on a sample plane of y), and wholly outside."""
    scale, origin = place
    w = lambda i, k: float(f32(i) * f32(scale) + f32(origin[k]))   # noqa: E731  world coordinate of sample i on axis k
    return [((w(9.5, 0), w(5.25, 1), w(11.5, 2)), (w(41.25, 0), w(19.5, 1), w(37.0, 2))),
            ((w(-20, 0), w(-20, 1), w(30.5, 2)), (w(33.5, 0), w(12.5, 1), w(300, 2))),
            ((w(3.5, 0), w(11, 1), w(4.5, 2)), (w(60.5, 0), w(11, 1), w(44.5, 2))),
            ((w(-40, 0), w(2, 1), w(2, 2)), (w(-3, 0), w(20, 1), w(40, 2)))]


@pytest.mark.gpu
@pytest.mark.parametrize("place", PLACES, ids=["unit", "scaled"])
@pytest.mark.parametrize("add", [True, False], ids=["add", "erode"])
@pytest.mark.parametrize("basis", BASES)
def test_gpu_noise_bitwise(oracle_mod, basis, add, place):
    ex, ref = world(oracle_mod, place)
    with ex:
        taken = {"low": 0, "high": 0}
        inner, clipped, thin, outside = boxes(place)
        f = 0.09 / place[0]
        # amplitude 3 (and a bias that centres the billow / ridged sums): both clamp branches are taken
        common = dict(frequency=f, amplitude=3.0, bias={"fbm": 0.0, "billow": 1.5, "ridged": -3.0}[basis], ridge_offset=0.95)
        n_dirty, T = assert_update(ex, ref, oracle_mod, [noise(basis, add, *inner, octaves=5, **common)], taken)
        assert n_dirty > 0 and T > 0
        assert taken["low"] > 0 and taken["high"] > 0, taken
        n_dirty, _ = assert_update(ex, ref, oracle_mod, [noise(basis, add, *clipped, octaves=3, seed=-5, lacunarity=2.3, gain=0.6, ramp_scale=0.2 / place[0],
                                                               ramp_center=clipped[1][1] - 3 * place[0], **common)])
        assert n_dirty > 0
        n_dirty, _ = assert_update(ex, ref, oracle_mod, [noise(basis, add, *thin, octaves=16, lacunarity=1.5, gain=0.7, **common)])
        assert n_dirty > 0
        before = ref.grid.copy()
        assert assert_update(ex, ref, oracle_mod, [noise(basis, add, *outside, **common)]) == (0, 0)
        assert_grid(ex, before)
        assert len(ex.terrain_dirty_blocks()) == 0


MIXED = [("sphere", ((28.0, 11.0, 22.0), 6.0, True)), noise("ridged", False, (15.0, 3.0, 10.0), (45.0, 15.0, 36.0), frequency=0.13, bias=-0.9, octaves=3),
         ("smooth", ((30.0, 11.0, 23.0), 7.0, 0.8)), ("cylinder", ((18.0, 10.0, 15.0), (1.0, 0.1, 0.6), 25.0, 2.5, False)),
         noise("billow", True, (0.0, 0.0, 0.0), (30.0, 9.0, 30.0), frequency=0.2, amplitude=0.8, ramp_scale=0.3, ramp_center=6.0, seed=3),
         ("flatten", ((27.0, 10.0, 21.0), (0.2, 1.0, 0.1), 8.0, 0.9)), ("plane", (3.5, (40, 30), (70, 70), True)),
         noise("fbm", False, (36.0, 6.0, 20.0), (50.0, 14.0, 40.0), frequency=0.3, amplitude=2.5, octaves=2), ("sphere", ((31.0, 9.0, 24.0), 4.0, False))]


@pytest.mark.gpu
def test_gpu_mixed_queue_takes_one_event_per_modifier(oracle_mod):
    ex, ref = world(oracle_mod)
    hm = np.random.default_rng(2).uniform(2.0, 14.0, (9, 7)).astype(f32)
    with ex:
        events = ref.events
        assert_update(ex, ref, oracle_mod, MIXED)
        assert ref.events == events + len(MIXED)
        # the clamp draws of what follows hash the event numbers the noise modifiers took
        assert_update(ex, ref, oracle_mod, [("island", (hm, 50.0, 40.0, 14.0, True)), noise("ridged", True, frequency=0.07, bias=-1.2, ramp_scale=0.1, ramp_center=8.0),
                                            ("sphere", ((20.0, 10.0, 30.0), 5.0, False))])
        assert ref.events == events + len(MIXED) + 3


@pytest.mark.gpu
def test_gpu_world_build_is_the_density_field(oracle_mod):
    """A fresh terrain and one whole-grid fBm-8 + ramp add at scale 1 / origin 0: every sample whose density lies in [-1, 1] holds
    vto_density_fill's value; above 1 it holds a full value in [1, 2); below -1 it stays a void value, the larger of the one it had and
    the modifier's clamped one (S = max(S, md), md = max(q, its void draw)) -- which of the two, the twin checks bit for bit."""
    dims = (64, 40, 48)
    Dx, Dy, Dz = (d + 2 for d in dims)
    prm = dict(seed=1337, octaves=8, frequency=4.0 / 64, ramp_scale=2.0 / 24, ramp_center=20.0)
    want = np.empty((Dz, Dy, Dx), f32)
    p = oracle_mod.DensityParams(prm["seed"], prm["frequency"], 8, 2.0, 0.5, prm["ramp_scale"], prm["ramp_center"])
    oracle_mod.lib().vto_density_fill(ctypes.byref(p), 0, 0, 0, Dx, Dy, Dz, 1, Dx, Dx * Dy, want.ctypes.data_as(ctypes.c_void_p))
    with vt.Extractor(0) as ex:
        ex.terrain_init(*dims, 1.0, (0.0, 0.0, 0.0), 11)
        ref = oracle_mod.Terrain(*dims, 1.0, (0.0, 0.0, 0.0), 11)
        void = ref._mem.copy()
        n_dirty, T = assert_update(ex, ref, oracle_mod, [noise(lower=(-1.0, -1.0, -1.0), upper=(100.0, 100.0, 100.0), **prm)])
        assert n_dirty == 8 * 5 * 6 and T > 0
        got = ex.terrain_read_samples().transpose(2, 1, 0)
    mid, high, low = (want >= -1) & (want <= 1), want > 1, want < -1
    assert mid.sum() > 1000 and high.sum() > 1000 and low.sum() > 1000
    assert np.array_equal(bits(got[mid]), bits(want[mid]))
    assert ((got[high] >= 1) & (got[high] < 2)).all()
    assert ((got[low] >= void[low]) & (got[low] < -1)).all() and (got[low] == void[low]).any()


HISTORY_STEPS = [
    [noise("fbm", True, (10.0, 4.0, 10.0), (40.0, 18.0, 40.0), amplitude=2.0)],
    [noise("ridged", False, (5.0, 2.0, 5.0), (60.0, 16.0, 44.0), frequency=0.12, bias=-0.8), ("sphere", ((30.0, 10.0, 20.0), 5.0, True))],
    [noise("billow", True, (-10.0, -10.0, -10.0), (100.0, 100.0, 100.0), frequency=0.05, ramp_scale=0.2, ramp_center=9.0)],   # the whole grid
    [("smooth", ((30.0, 10.5, 20.0), 6.0, 1.0)), noise("fbm", False, (20.0, 8.0, 10.0), (44.0, 14.0, 30.0), frequency=0.2, octaves=2)],
]


@pytest.mark.gpu
def test_gpu_history_restores_noise_bitwise(oracle_mod):
    ex, ref = world(oracle_mod, history=64 << 20)
    with ex:
        snaps, results, want_bytes = [ref.grid.copy()], [], 0
        for specs in HISTORY_STEPS:
            results.append(assert_update(ex, ref, oracle_mod, specs) + (ex.terrain_dirty_blocks(),))
            snaps.append(ref.grid.copy())
            want_bytes += step_bytes(ref, specs)
        n = len(HISTORY_STEPS)
        assert ex.terrain_history() == (n, 0, want_bytes)   # the boxes' image sizes
        for k in reversed(range(n)):
            n_dirty, T = ex.terrain_undo()
            assert_grid(ex, snaps[k])
            assert n_dirty == results[k][0] and np.array_equal(ex.terrain_dirty_blocks(), results[k][2])
            assert_triangles(ex, oracle_mod, snaps[k], results[k][2], T)
        for k in range(n):
            n_dirty, T = ex.terrain_redo()
            assert_grid(ex, snaps[k + 1])
            assert (n_dirty, T) == results[k][:2]
        assert ex.terrain_history() == (n, 0, want_bytes)
        # a noise edit after two undos drops the redo stack
        ex.terrain_undo()
        ex.terrain_undo()
        assert ex.terrain_history()[:2] == (n - 2, 2)
        ref._mem[...] = snaps[n - 2].transpose(2, 1, 0)   # rewound two steps; the event counter is not
        edit = [noise("ridged", False, (12.0, 5.0, 12.0), (30.0, 15.0, 30.0), frequency=0.15, bias=-0.7, seed=9)]
        assert_update(ex, ref, oracle_mod, edit)
        assert ex.terrain_history() == (n - 1, 0, want_bytes - sum(step_bytes(ref, s) for s in HISTORY_STEPS[n - 2:]) + step_bytes(ref, edit))
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_redo()
        assert e.value.code == _lib.ERR_NO_RESULT
        ex.terrain_undo()
        assert_grid(ex, snaps[n - 2])


@pytest.mark.gpu
def test_gpu_picking_hits_the_carved_surface():
    """Rays after a ridged erode: byte for byte the pick on a fresh extract of the read-back grid, and not what they hit before."""
    import torch
    xs, zs = np.meshgrid(np.arange(6.0, 58.0, 0.8), np.arange(6.0, 42.0, 0.8))
    origins = np.stack([xs.ravel(), np.full(xs.size, 40.0), zs.ravel()], 1).astype(f32)
    directions = np.tile(f32([0.05, -1.0, 0.02]), (len(origins), 1))
    with vt.Extractor(0) as ex, vt.Extractor(0) as ex2:
        ex.terrain_init(*DIMS, 1.0, (0.0, 0.0, 0.0), SEED)
        ex.terrain_update([gpu_mod(s) for s in WORLD])
        before = ex.terrain_raycast(origins, directions)
        ex.terrain_update([vt.NoiseModifier(21, 4, 0.08, basis="ridged", bias=-0.85, lower=(2.0, 2.0, 2.0), upper=(62.0, 22.0, 46.0), add_or_erode=False)])
        after = ex.terrain_raycast(origins, directions)
        assert (after["triangle"] >= 0).sum() > 100
        assert ((after["distance"] > before["distance"]) & (before["triangle"] >= 0)).sum() > 50   # carved: the surface moved away
        mem = np.ascontiguousarray(ex.terrain_read_samples().transpose(2, 1, 0))
        d_g, d_o, d_d = torch.from_numpy(mem).cuda(), torch.from_numpy(origins).cuda(), torch.from_numpy(directions).cuda()
        d_h = torch.zeros(len(origins) * vt.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        Dx, Dy = DIMS[0] + 2, DIMS[1] + 2
        ex2.raycast_device(d_g.data_ptr(), DIMS, (1, Dx, Dx * Dy), (0.0, 0.0, 0.0), 1.0, d_o.data_ptr(), d_d.data_ptr(), len(origins), d_h.data_ptr())
        fresh = ex2.copy_to_host(d_h.data_ptr(), d_h.numel()).view(vt.RAY_HIT_DTYPE)
        assert fresh.tobytes() == after.tobytes()


REJECTED = [(raw_noise(p=(np.nan, 2, .5, 1, 0, 0, 0, 1)), "p[0]"), (raw_noise(p=(.1, np.inf, .5, 1, 0, 0, 0, 1)), "p[1]"),
            (raw_noise(p=(.1, 2, -np.inf, 1, 0, 0, 0, 1)), "p[2]"), (raw_noise(p=(.1, 2, .5, np.nan, 0, 0, 0, 1)), "p[3]"),
            (raw_noise(p=(.1, 2, .5, 1, np.inf, 0, 0, 1)), "p[4]"), (raw_noise(p=(.1, 2, .5, 1, 0, np.nan, 0, 1)), "p[5]"),
            (raw_noise(p=(.1, 2, .5, 1, 0, 0, np.inf, 1)), "p[6]"), (raw_noise(p=(.1, 2, .5, 1, 0, 0, 0, np.nan)), "p[7]"),
            (raw_noise(octaves=0), "octaves"), (raw_noise(octaves=17), "octaves"), (raw_noise(basis=3), "basis"), (raw_noise(basis=-1), "basis"),
            # lattice reach: 30 * 1e6 > 2^24;  30 * 0.1 * 64^5 > 2^24;  a negative frequency and lacunarity count by magnitude
            (raw_noise(p=(1e6, 2, .5, 1, 0, 0, 0, 1)), "lattice"), (raw_noise(p=(.1, 64, .5, 1, 0, 0, 0, 1), octaves=6), "lattice"),
            (raw_noise(p=(-1e6, 2, .5, 1, 0, 0, 0, 1)), "lattice"), (raw_noise(p=(.1, -64, .5, 1, 0, 0, 0, 1), octaves=6), "lattice"),
            (raw_noise(p=(1e30, 1e30, .5, 1, 0, 0, 0, 1), octaves=16), "lattice")]


@pytest.mark.gpu
@pytest.mark.parametrize("history", [0, 64 << 20], ids=["history_off", "history_on"])
def test_gpu_rejections_name_the_modifier_and_write_nothing(oracle_mod, history):
    ex, ref = world(oracle_mod, history=history)
    with ex:
        first = [] if not history else [vt.SphereModifier((30.0, 10.0, 20.0), 4.0, True)]   # history on: the whole queue is checked first
        for bad, word in REJECTED:
            msg = invalid(ex, first + [bad])
            assert "modifier %d" % len(first) in msg and word in msg, msg
            assert_grid(ex, ref.grid)
            assert ex.terrain_history() == (0, 0, 0)
        for kind in (6, 7):
            assert "unknown kind" in invalid(ex, [raw_noise(kind=kind)])
        # the limits themselves are accepted: 16 octaves, a reach just below 2^24 (35 * 14 * 2^15 = 1.61e7), a box outside the grid with any frequency
        ex.terrain_update([raw_noise(p=(14.0, 2, .5, 1, 0, 0, 0, 1), octaves=16, upper=(30.0, 16.0, 35.0)), raw_noise(p=(1e30, 2, .5, 1, 0, 0, 0, 1), lower=(-50.0, 0.0, 0.0), upper=(-20.0, 5.0, 5.0))])


@pytest.mark.gpu
def test_gpu_ridged_erode_a_1024_cube_terrain():
    """A ridged erode whose box covers a 1026^3-sample grid (4.3 GB: 64-bit sample indices in the kernel and in the hash), checked sample
    for sample on six full z-slabs, the first and the last among them."""
    W = 1024

    class Twin:   # what csg_write needs of oracle.Terrain, over one z-slab
        dims, scale, origin, seed = (W, W, W), 1.0, np.zeros(3, f32), 17

    with vt.Extractor(0) as ex:
        ex.terrain_init(W, W, W, 1.0, (0.0, 0.0, 0.0), 17)
        ex.terrain_update([vt.PlaneModifier(500.5, (-1, -1), (W + 2, W + 2), True), vt.SphereModifier((300.0, 500.0, 700.0), 40.0, True)])
        before = ex.terrain_read_samples().transpose(2, 1, 0)     # [z, y, x], x fastest
        carve = vt.NoiseModifier(123, 6, 1.0 / 96, gain=0.35, basis="ridged", amplitude=1.5, bias=-2.2, ramp_scale=0.001, ramp_center=400.0,
                                 lower=(-10.0, -10.0, -10.0), upper=(2000.0, 2000.0, 2000.0), add_or_erode=False)
        m = carve.to_struct()
        n_dirty, T = ex.terrain_update([carve])
        assert n_dirty == (W // 8) ** 3 and T > 0
        after = ex.terrain_read_samples().transpose(2, 1, 0)
    perm = permutation(123)
    p = np.arange(W + 2).astype(f32)
    for z in (0, 1, 333, 512, W, W + 1):
        twin = Twin()
        twin.events = 2
        twin._mem = _SlabAt(before[z:z + 1].copy(), z)
        q = noise_density(perm, p[None, None, :], p[None, :, None], p[z:z + 1, None, None], 6, 2, *m.p[0:8])
        csg_write(twin, (0, 0, z), (W + 2, W + 2, 1), q, False)
        assert np.array_equal(bits(after[z:z + 1]), bits(twin._mem.slab)), z


class _SlabAt:
    """One z-slab of a grid standing in for the whole [z, y, x] memory: indexed with the slab's own z only."""

    def __init__(self, slab, z):
        self.slab, self.z = slab, z

    def _local(self, key):
        assert key[0] == slice(self.z, self.z + 1)
        return (slice(0, 1),) + tuple(key[1:])

    def __getitem__(self, key):
        return self.slab[self._local(key)]

    def __setitem__(self, key, value):
        self.slab[self._local(key)] = value


@pytest.mark.gpu
def test_gpu_the_same_queue_twice_gives_the_same_bits():
    grids = []
    for _ in range(2):
        with vt.Extractor(0) as ex:
            ex.terrain_init(*DIMS, 0.5, (-3.25, 1.5, 2.125), SEED)
            ex.terrain_update([gpu_mod(s) for s in WORLD])
            T = ex.terrain_update([gpu_mod(s) for s in MIXED])[1]
            tris, offs = ex.read_triangles()
            grids.append((bits(ex.terrain_read_samples()).copy(), T, tris.tobytes(), offs.tobytes()))
    assert np.array_equal(grids[0][0], grids[1][0]) and grids[0][1:] == grids[1][1:]
