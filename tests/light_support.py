"""What the lighting tests share (test_terrain_light.py): the crafted field, its boxes and its cases, the twin's results on them, computed
once, and the helpers that compare a device result with the twin.  No tests here.  Positions, bounds and the device context come from
water_support.py, whose dyadic world (scale 0.5, origin (-3, 1, 2)) this one shares.

The terrain is 72 x 24 x 24 cells = 74 x 26 x 26 samples: two tiles of 64 along x, the second ragged, and four along y and z.  Rock
everywhere under a sky from plane 22 up, and in the rock:
  the corridor   y 4, z 6, x 2..12, continued by a NaN, a +0 and a -0 sample (x 13..15): open oddities.
  the tunnel     one sample wide, 262 hops from (20, 6, 9) to (70, 10, 17): five runs along x that cross the x tile face, joined at their
                 ends by hops in z, and once by a climb from plane 6 to plane 10 (the y tile face); the last hop in z crosses the z tile face.
  the pit        a shaft x 30..33, z 2..5 from plane 12 up to the sky, with a room x 34..44 on planes 12..14 under a roof of rock.
  the cave       x 50..55, y 14..17, z 2..5, sealed."""
import ctypes
import functools

import numpy as np

import light_twin as twin
import water_support as ws

f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (72, 24, 24), ws.SCALE, ws.ORIGIN, 43
SHAPE = tuple(d + 2 for d in DIMS)
ROCK, AIR = f32(0.5), f32(-0.75)
TUNNEL = [(20, 6, 9), (70, 6, 9), (70, 6, 11), (20, 6, 11), (20, 6, 13), (20, 10, 13), (70, 10, 13), (70, 10, 15), (20, 10, 15), (20, 10, 17), (70, 10, 17)]
TUNNEL_HOPS = sum(sum(abs(a[k] - b[k]) for k in range(3)) for a, b in zip(TUNNEL, TUNNEL[1:]))


@functools.lru_cache(maxsize=None)
def crafted_field():
    g = np.full(SHAPE, ROCK, f32)

    def fill(x, y, z, value=AIR):
        span = [slice(a[0], a[1] + 1) if isinstance(a, tuple) else slice(a, a + 1) for a in (x, y, z)]
        g[span[0], span[1], span[2]] = value

    fill((0, 73), (22, 25), (0, 25))       # sky
    fill((2, 12), 4, 6)                    # corridor
    g[13, 4, 6], g[14, 4, 6], g[15, 4, 6] = f32(np.nan), f32(0.0), f32(-0.0)   # open oddities
    for a, b in zip(TUNNEL, TUNNEL[1:]):   # tunnel: axis-parallel pieces
        fill(*[(min(a[k], b[k]), max(a[k], b[k])) for k in range(3)])
    fill((30, 33), (12, 21), (2, 5))       # shaft
    fill((34, 44), (12, 14), (2, 5))       # room under the overhang
    fill((50, 55), (14, 17), (2, 5))       # sealed cave
    g.setflags(write=False)
    return g


def world_of(sample):
    return ws.world_of(sample)


def source(sample, level, off=(0.0, 0.0, 0.0)):
    """A torch on a sample, `off` world units away from it (less than a quarter: the sample stays the nearest)."""
    w = world_of(sample)
    return (w[0] + off[0], w[1] + off[1], w[2] + off[2], level)


# name -> (first sample, samples per axis): the whole grid; an interior box with an odd low corner whose faces lie on no tile boundary of
# the grid; a box one sample thick, the plane of the tunnel's first two runs
BOXES = {"whole": ((0, 0, 0), SHAPE), "interior": ((3, 1, 5), (67, 9, 13)), "thin": ((0, 6, 0), (74, 1, 26))}
# name -> (sky_level, sky_falloff, torch_falloff, sources)
CASES = {
    "corridor": (0, 1, 3, [source((3, 4, 6), 10)]),
    "tunnel": (0, 1, 1, [source(TUNNEL[0], 255)]),
    "tunnel dies": (0, 1, 255, [source(TUNNEL[0], 255)]),
    "sky": (255, 16, 16, []),
    "sources": (200, 7, 5, [source((40, 4, 20), 250),                      # in rock: dark
                            (500.0, 6.0, 10.0, 99),                        # outside every box
                            source((3, 4, 6), 10, (0.1, -0.1, 0.2)), source((3, 4, 6), 90), source((3, 4, 6), 40, (-0.2, 0.0, 0.0)),   # three on one sample
                            source((31, 13, 3), 120), source((52, 15, 3), 60, (0.0, 0.2, 0.0)), source((45, 6, 11), 255)]),   # the pit, the cave, the tunnel
    "oddities": (0, 1, 2, [source((12, 4, 6), 20)]),
    "sky level 0": (0, 16, 4, [source((31, 13, 3), 100)]),
}


def bounds_of(box):
    return ws.bounds_of(BOXES[box] if isinstance(box, str) else box, ws.WORLD, DIMS)


@functools.lru_cache(maxsize=None)
def twin_of(case, box):
    sky, sky_falloff, torch_falloff, rows = CASES[case]
    return twin.light(crafted_field(), *BOXES[box], SCALE, ORIGIN, sky, sky_falloff, torch_falloff, twin.sources_of(rows))


def params_of(case):
    import volumetricterrain_amd as vt
    return vt.LightParams(*CASES[case][:3])


def random_case(seed):
    """A random field on DIMS, open with probability 0.45 -- above the cubic lattice's site-percolation threshold, so light finds long ways
    round --, 16 sources at random positions, in rock or not, a random sky level and random falloffs."""
    rng = np.random.default_rng(seed)
    g = np.where(rng.random(SHAPE) < 0.45, AIR, ROCK).astype(f32)
    lo, hi = np.asarray(world_of((-1, -1, -1))), np.asarray(world_of(SHAPE))
    rows = [tuple(rng.uniform(lo, hi)) + (int(rng.integers(1, 256)),) for _ in range(16)]
    return g, (int(rng.integers(1, 256)), int(rng.integers(1, 40)), int(rng.integers(1, 40))), twin.sources_of(rows)


# -- the device ------------------------------------------------------------------------------------------------------------------------------
def terrain(grid=None, indexed=False):
    import volumetricterrain_amd as vt
    ex = vt.Extractor(0)
    ex.set_output_mode(indexed)
    ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
    if grid is not None:
        ex.terrain_write_samples(grid)
    return ex


def device_volume(ex):
    """The volume as it lies behind vtmc_light_device_results, indexed [x, y, z]."""
    import volumetricterrain_amd as vt
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    p, d = ex.device_light()
    out = np.zeros(d[::-1], vt.LIGHT_SAMPLE_DTYPE)
    assert p and hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
    return out.transpose(2, 1, 0)


def raw(volume):
    return np.ascontiguousarray(volume).tobytes()


def same_result(ex, want, lit):
    """Everything a light call leaves, through the host readers, against the twin: EQUAL, the volume as raw bytes; and the round count
    within the rule's bound."""
    import volumetricterrain_amd as vt
    lo, d, n_sky, n_torch, rounds = ex.light_info()
    assert (lo, d, n_sky, n_torch) == (want.first if min(want.ext) else lo, want.ext, want.n_sky, want.n_torch)
    assert 0 <= rounds <= vt._lib.LIGHT_MAX_ROUNDS and (rounds >= 1 or min(want.ext) == 0)
    assert lit.dtype == np.uint8 and np.array_equal(lit, want.source_lit)
    volume = ex.light_read()
    assert volume.shape == want.ext and volume.dtype == vt.LIGHT_SAMPLE_DTYPE and raw(volume) == raw(want.volume)
    return rounds
