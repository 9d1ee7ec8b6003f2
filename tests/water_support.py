"""What the water tests share (test_terrain_water.py): the crafted field, its boxes and source sets, and the twin's results on them,
computed once.  No tests here.

The terrain is 136 x 24 x 40 cells = 138 x 26 x 42 samples, scale 0.5, origin (-3, 1, 2): three tiles of 64 along x, the last ragged.  The
height of plane j is h(j) = 1 + 0.5 j exactly.  Rock everywhere under a sky from plane 18 up; two basins A and B with a notch in the sill
between them (planes 14..17), a tunnel from A to a chamber, a sealed pocket, a channel that leaves B's floor sideways, dives to plane 3 and
runs to x = 134, one sample that touches A's corner diagonally, and NaN, +0 and -0 under A's floor."""
import functools

import numpy as np

import water_twin as twin

f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (136, 24, 40), 0.5, (-3.0, 1.0, 2.0), 41
ROCK, AIR = f32(0.5), f32(-0.75)


@functools.lru_cache(maxsize=None)
def crafted_field():
    g = np.full(tuple(d + 2 for d in DIMS), ROCK, f32)

    def fill(x, y, z, value=AIR):
        span = [slice(a[0], a[1] + 1) if isinstance(a, tuple) else slice(a, a + 1) for a in (x, y, z)]
        g[span[0], span[1], span[2]] = value

    fill((0, 137), (18, 25), (0, 41))      # sky
    fill((4, 40), (8, 17), (4, 20))        # basin A
    fill((50, 130), (10, 17), (4, 20))     # basin B
    fill((41, 49), (14, 17), (10, 12))     # notch in the sill
    fill(20, 9, (21, 36))                  # tunnel
    fill((14, 26), (8, 12), (30, 36))      # chamber
    fill((60, 64), (3, 6), (30, 34))       # sealed pocket
    fill(126, 11, (21, 38))                # channel, part 1
    fill((66, 126), 11, 38)                # channel, part 2
    fill(66, (3, 11), 38)                  # channel, part 3
    fill((66, 134), 3, 38)                 # channel, part 4
    fill(3, 7, 3)                          # corner contact
    g[10, 7, 10], g[11, 7, 10], g[12, 7, 10] = f32(np.nan), f32(0.0), f32(-0.0)   # open oddities
    g.setflags(write=False)
    return g


def h(j):
    return 1.0 + 0.5 * j


def world_of(sample):
    w = tuple(ORIGIN[k] + sample[k] * SCALE for k in range(3))
    assert all(float(f32(v)) == v for v in w)
    return w


def source(sample, level):
    return world_of(sample) + (level,)


# name -> (first sample, samples per axis); the world bounds of a box are those of its first and last sample
BOXES = {"whole": ((0, 0, 0), (138, 26, 42)), "interior": ((30, 2, 2), (80, 20, 30))}
CASES = {
    "separate": [source((20, 9, 10), h(12)), source((60, 11, 10), h(13)), source((62, 4, 32), h(5)), source((70, 2, 10), h(20)),
                 source((20, 16, 10), h(12)), source((66, 3, 38), h(13))],
    "spill": [source((20, 9, 10), h(12)), source((60, 11, 10), h(15.5)), source((62, 4, 32), h(5))],
    "sky": [source((0, 25, 0), h(25))],
}


def bounds_of(box):
    first, ext = BOXES[box]
    return world_of(first), world_of(tuple(first[k] + ext[k] - 1 for k in range(3)))


@functools.lru_cache(maxsize=None)
def twin_of(case, box):
    return twin.flood(crafted_field(), *BOXES[box], SCALE, ORIGIN, twin.sources_of(CASES[case]))


def same_result(ex, want, source_body, n_bodies):
    """Everything a flood leaves, through the host readers, against the twin: EQUAL, records and volumes as raw bytes."""
    lo, d, vd, n, wet = ex.water_info()
    assert (lo, d, vd, n, wet) == (want.first if min(want.ext) else lo, want.ext, want.vd, len(want.bodies), want.wet)
    assert n_bodies == n and source_body.dtype == np.int32 and np.array_equal(source_body, want.source_body)
    assert ex.water_bodies().tobytes() == want.bodies.tobytes()
    water, body = ex.water_read()
    assert water.shape == body.shape == want.vd and water.dtype == f32 and body.dtype == np.int32
    assert np.array_equal(body, want.body)
    assert np.ascontiguousarray(water).tobytes() == np.ascontiguousarray(want.water).tobytes()
