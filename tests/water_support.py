"""What the water tests share (test_terrain_water.py, test_terrain_water_edges.py): the crafted field, its boxes and source sets in two
worlds, the twin's results on them, computed once, and the helpers that place sources, bounds and levels by the rule's own FP32 formulas.
No tests here.

The terrain is 136 x 24 x 40 cells = 138 x 26 x 42 samples: three tiles of 64 along x, the last ragged.  Rock everywhere under a sky from
plane 18 up; two basins A and B with a notch in the sill between them (planes 14..17), a tunnel from A to a chamber, a sealed pocket, a
channel that leaves B's floor sideways, dives to plane 3 and runs to x = 134, one sample that touches A's corner diagonally, and NaN, +0 and
-0 under A's floor.  The field is indices only; a WORLD (scale, origin) places it.
  WORLD     scale 0.5, origin (-3, 1, 2): dyadic.  The height of plane j is h(j) = 1 + 0.5 j exactly and no FP32 step of the rule rounds, so a
            kernel that fuses, reassociates or multiplies by 1 / scale gives the rule's bits all the same.
  WORLD_B   scale 0.3, origin (-3.1, 1.7, 2.3), session_twin's world "b": every step rounds.  Its levels, its half-way sources and its probes
            are chosen here so that each of those wrong variants changes the result (test_terrain_water_edges.py proves it on the twin)."""
import ctypes
import functools

import numpy as np

import fragment_twin
import water_twin as twin

f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (136, 24, 40), 0.5, (-3.0, 1.0, 2.0), 41
WORLD, WORLD_B = (SCALE, ORIGIN), (0.3, (-3.1, 1.7, 2.3))
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


# -- a world: positions, heights and bounds by the rule's formulas, in float32 ---------------------------------------------------------------
def position(j, k, world=WORLD):
    """The world coordinate of sample index j along axis k, the terrain's own position formula: f32(f32(j) * f32(scale)) + f32(origin_k)."""
    scale, origin = world
    return float(f32(f32(f32(j) * f32(scale)) + f32(origin[k])))


def world_of(sample, world=WORLD):
    w = tuple(position(sample[k], k, world) for k in range(3))
    if world == WORLD:
        assert w == tuple(ORIGIN[k] + sample[k] * SCALE for k in range(3))      # exactly representable: nothing rounded
    return w


def source(sample, level, world=WORLD):
    return world_of(sample, world) + (level,)


def height(j, world):
    """The rule's height of plane j."""
    return float(twin.plane_height(j, world[0], world[1][1]))


def below(v):
    return float(np.nextafter(f32(v), f32(-np.inf)))


# name -> (first sample, samples per axis); the world bounds of a box are those of its first and last sample
BOXES = {"whole": ((0, 0, 0), (138, 26, 42)), "interior": ((30, 2, 2), (80, 20, 30))}
CASES = {
    "separate": [source((20, 9, 10), h(12)), source((60, 11, 10), h(13)), source((62, 4, 32), h(5)), source((70, 2, 10), h(20)),
                 source((20, 16, 10), h(12)), source((66, 3, 38), h(13))],
    "spill": [source((20, 9, 10), h(12)), source((60, 11, 10), h(15.5)), source((62, 4, 32), h(5))],
    "sky": [source((0, 25, 0), h(25))],
}


def bounds_of(box, world=WORLD, dims=DIMS):
    """World bounds that clamp to the box (a name of BOXES or (first sample, samples per axis)): the positions of its first and last sample.
    Off the dyadic world the library's (bound - origin) / scale may land a hair outside the index it came from, where floor / ceil would add
    a sample: such a bound moves inward, one float32 at a time, until the box is the one asked for (fragment_twin.sample_box is the judge)."""
    first, ext = BOXES[box] if isinstance(box, str) else box
    last = tuple(first[k] + ext[k] - 1 for k in range(3))
    lower, upper = [f32(v) for v in world_of(first, world)], [f32(v) for v in world_of(last, world)]
    for k in range(3):
        for _ in range(8):
            got_first, got_ext = fragment_twin.sample_box(lower, upper, dims, *world)[:2]
            if got_first[k] < first[k]:
                lower[k] = np.nextafter(lower[k], f32(np.inf))
            elif got_first[k] + got_ext[k] - 1 > last[k]:
                upper[k] = np.nextafter(upper[k], f32(-np.inf))
    assert fragment_twin.sample_box(lower, upper, dims, *world)[:2] == (tuple(first), tuple(ext))
    return tuple(float(v) for v in lower), tuple(float(v) for v in upper)


# -- the rule's neighbours: what a kernel computes that fuses, or multiplies by 1 / scale ----------------------------------------------------
def fused_height(j, scale, origin_y):
    """The plane height as ONE operation (a fused multiply-add): the float64 product and sum are exact for these operands up to one rounding
    far below float32's, and that is rounded once."""
    y = (np.asarray(j).astype(f32).astype(np.float64) * np.float64(f32(scale)) + np.float64(f32(origin_y))).astype(f32)
    return y if np.ndim(j) else f32(y)


def reciprocal_depth(level, height_, scale):
    """clamped_depth with t * (1 / scale) in place of t / scale."""
    with np.errstate(all="ignore"):
        t = (np.asarray(level, f32) - np.asarray(height_, f32)).astype(f32)
        t = (t * f32(f32(1) / f32(scale))).astype(f32)
    return np.clip(t, f32(-1), f32(1)).astype(f32)


def reciprocal_nearest(p, origin, scale):
    """nearest with (p - origin) * (1 / scale) in place of (p - origin) / scale."""
    with np.errstate(all="ignore"):
        g = f32(f32(p) - f32(origin))
        g = f32(g * f32(f32(1) / f32(scale)))
        g = np.floor(f32(g + f32(0.5)))
    return None if np.isnan(g) else int(min(max(float(g), -2.0 ** 31), 2.0 ** 31 - 1))


def level_over(plane, world, rng):
    """A level strictly between the heights of `plane` and the next one at which t / scale and t * (1 / scale) differ on `plane` itself,
    where t lies in (0, 1) and nothing clamps: a seeded search, about every third draw qualifies."""
    scale = world[0]
    lo, hi = height(plane, world), height(plane + 1, world)
    for _ in range(1000):
        level = f32(rng.uniform(lo, hi))
        if lo < level < hi and twin.bits(twin.clamped_depth(level, f32(lo), scale)) != twin.bits(reciprocal_depth(level, f32(lo), scale)):
            assert 0 < twin.clamped_depth(level, f32(lo), scale) < 1
            return float(level)
    raise AssertionError("no level over plane %d tells the division from the reciprocal" % plane)


def halfway(j, k, world):
    """The three float32 positions around the point half-way between samples j and j + 1 of axis k: origin + (j + 0.5) * scale in float32,
    and its neighbour on either side."""
    scale, origin = world
    mid = f32(f32(f32(f32(j) + f32(0.5)) * f32(scale)) + f32(origin[k]))
    return [float(np.nextafter(mid, f32(-np.inf))), float(mid), float(np.nextafter(mid, f32(np.inf)))]


def halfway_flips(k, n, world):
    """The j of -1..n-1 along axis k at which the reciprocal form of the nearest-sample rule picks the other sample for one of halfway()'s
    positions, and the rule itself puts the first of them on j and the last on j + 1."""
    scale, origin = world
    out = []
    for j in range(-1, n):
        rule = [twin.nearest(p, origin[k], scale) for p in halfway(j, k, world)]
        if rule != [reciprocal_nearest(p, origin[k], scale) for p in halfway(j, k, world)] and (rule[0], rule[2]) == (j, j + 1):
            out.append(j)
    return out


def halfway_sites(wet, solid, world, per_flip, rng):
    """Triples of positions on the shore of a flood (wet, solid: bool arrays over the box, which starts at sample 0): for every axis k and every
    j of halfway_flips, up to per_flip places where sample j is wet and j + 1 is rock or outside the box, or the other way round -- never an
    open dry sample, which a source would flood --, as (k, j, [three positions])."""
    wet_p, ground_p = np.pad(wet, 1, constant_values=False), np.pad(solid & ~wet, 1, constant_values=True)   # index + 1; outside the box is dry ground
    inner = (slice(1, -1),) * 2
    out = []
    for k in range(3):
        u, v = [a for a in range(3) if a != k]
        for j in halfway_flips(k, wet.shape[k], world):
            w0, w1 = np.take(wet_p, j + 1, axis=k)[inner], np.take(wet_p, j + 2, axis=k)[inner]
            g0, g1 = np.take(ground_p, j + 1, axis=k)[inner], np.take(ground_p, j + 2, axis=k)[inner]
            places = np.argwhere((w0 & g1) | (w1 & g0))
            for place in places[np.sort(rng.choice(len(places), min(per_flip, len(places)), replace=False))]:
                rows = []
                for p in halfway(j, k, world):
                    c = [0.0, 0.0, 0.0]
                    c[k], c[u], c[v] = p, position(int(place[0]), u, world), position(int(place[1]), v, world)
                    rows.append(tuple(c))
                out.append((k, j, rows))
    return out


# -- the crafted field in WORLD_B ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def levels_b():
    """The eight levels of the crafted field in WORLD_B, by the part they play.  A fused plane height differs from the rule's on planes 10, 14,
    15, 19 and 20: two levels are such a height exactly (the wet samples of that plane hold 0 by the rule and something else fused), two are
    the float32 just below one, and four lie between planes where the division and the reciprocal part."""
    rng = np.random.default_rng(2610)
    W = WORLD_B
    return {"A": height(10, W), "B": level_over(13, W, rng), "pocket": level_over(4, W, rng), "rock": below(height(20, W)),
            "A under the spill": below(height(14, W)), "B spilling": height(15, W), "pocket 2": level_over(5, W, rng), "sky": level_over(25, W, rng)}


@functools.lru_cache(maxsize=None)
def cases_b():
    """The source sets of CASES in WORLD_B -- two basins, the spill through the notch, the sealed pocket, the channel, one dry source in rock,
    one above its level, the sky -- and "shore": the sky's source and, at its level, sources half-way between a wet sample and dry ground
    where the reciprocal form of the nearest-sample rule picks the other one."""
    L, W = levels_b(), WORLD_B
    cases = {
        "separate": [source((20, 9, 10), L["A"], W), source((60, 11, 10), L["B"], W), source((62, 4, 32), L["pocket"], W), source((70, 2, 10), L["rock"], W),
                     source((20, 16, 10), L["A"], W), source((66, 3, 38), L["B"], W)],
        "spill": [source((20, 9, 10), L["A under the spill"], W), source((60, 11, 10), L["B spilling"], W), source((62, 4, 32), L["pocket 2"], W)],
        "sky": [source((0, 25, 0), L["sky"], W)],
    }
    cases["shore"] = cases["sky"] + [p + (L["sky"],) for _, _, rows in shore_sites() for p in rows]
    return cases


@functools.lru_cache(maxsize=None)
def shore_sites():
    sky = twin.flood(crafted_field(), *BOXES["whole"], *WORLD_B, twin.sources_of([source((0, 25, 0), levels_b()["sky"], WORLD_B)]))
    dx, dy, dz = sky.ext
    return halfway_sites(sky.body[:dx, :dy, :dz] >= 0, crafted_field() > 0, WORLD_B, 6, np.random.default_rng(2611))


@functools.lru_cache(maxsize=None)
def twin_of(case, box, world=WORLD):
    return twin.flood(crafted_field(), *BOXES[box], *world, twin.sources_of((CASES if world == WORLD else cases_b())[case]))


def figures(r):
    """A result as a row of the pinned tables: (source_body, [(level, n_samples, n_surface, lo, hi, flags, n_sources)], wet, volume_counts)."""
    bodies = [(float(b["level"]), int(b["n_samples"]), int(b["n_surface"]), tuple(b["lo"].tolist()), tuple(b["hi"].tolist()), int(b["flags"]), int(b["n_sources"]))
              for b in r.bodies]
    return r.source_body.tolist(), bodies, r.wet, twin.volume_counts(r)


def random_field(rng, dims):
    """A random field on `dims` cells, open with probability 0.33 -- just above the cubic lattice's site-percolation threshold, so components
    are long and cross many tiles."""
    return np.where(rng.random(tuple(d + 2 for d in dims)) < 0.33, f32(-0.5), f32(0.5)).astype(f32)


# -- the device ------------------------------------------------------------------------------------------------------------------------------
def terrain(grid=None, dims=DIMS, world=WORLD):
    import volumetricterrain_amd as vt
    ex = vt.Extractor(0)
    ex.terrain_init(*dims, world[0], world[1], SEED)
    if grid is not None:
        ex.terrain_write_samples(grid)
    return ex


def device_volumes(ex):
    """The two volumes as they lie behind vtmc_water_device_results, indexed [x, y, z]."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    w, b, vd = ex.device_water()
    water, body = np.empty(vd[::-1], f32), np.empty(vd[::-1], np.int32)
    assert w and b and hip.hipMemcpy(water.ctypes.data, w, water.nbytes, 2) == 0 and hip.hipMemcpy(body.ctypes.data, b, body.nbytes, 2) == 0
    return water.transpose(2, 1, 0), body.transpose(2, 1, 0)


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
