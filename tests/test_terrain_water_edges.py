"""The flood (include/vtmc_water.h, csrc/terrain_water.hip) off its dyadic world and at its numbering limits.  test_terrain_water.py floods at
scale 0.5 with origin (-3, 1, 2), where no FP32 step of the rule WATER rounds: a kernel that fused the plane height, multiplied by 1 / scale
or reassociated would give the rule's bits there all the same.  Here:
  A   the crafted field at scale 0.3 with origin (-3.1, 1.7, 2.3) (water_support.WORLD_B), at levels on, just below and between plane heights,
      with sources and probes half-way between samples, and the water's extraction;
  B   on the CPU, the proof that A's inputs tell the rule from those neighbours: three mutants of the twin each change its result on them,
      and change nothing in the dyadic world -- which is the gap this file closes;
  C   water_number_kernel at its size: 4096 distinct roots in one level, a second level numbered from base 2048, duplicates spread over the
      1024-lane stride on 8 levels;
  D   a level under the box's bottom plane: no labelling, and a source may still join;
  E   boxes one sample thick, 63..66 samples long, and the volume dim's step from 10 to 18.
Every GPU comparison is for EQUALITY with the twin (water_support.same_result); only the extraction goes through extract_checks."""
import contextlib
import functools

import numpy as np
import pytest

from volumetricterrain_amd import _lib
import water_support as ws
import water_twin as twin

f32 = np.float32
W = ws.WORLD_B
FUSED_DIFFERS = (10, 14, 15, 19, 20)          # the planes of 0..25 on which a fused height is not the rule's, in WORLD_B

# case, box -> (source_body, [(level, n_samples, n_surface, lo, hi, at a face, n_sources)], wet, (near, refused, values > 0, wet values == 0)); "shore" apart
TABLE_B = {
    ("separate", "whole"): ([1, 0, 2, -1, -1, 0], [(5.8376054763793945, 5662, 1377, (50, 3, 4), (134, 13, 38), 0, 2), (4.699999809265137, 2172, 720, (4, 7, 4), (40, 10, 36), 0, 1),
                                                   (3.15761661529541, 50, 25, (60, 3, 30), (64, 4, 34), 0, 1)], 7884, (7618, 1, 12102, 720)),
    ("separate", "interior"): ([-1, 0, -1, -1, -1, -1], [(5.8376054763793945, 4080, 1020, (50, 10, 4), (109, 13, 20), 1, 1)], 4080, (2874, 0, 5795, 0)),
    ("spill", "whole"): ([0, 0, 1], [(6.199999809265137, 13969, 2033, (4, 3, 4), (134, 15, 38), 0, 2), (3.271470546722412, 75, 25, (60, 3, 30), (64, 5, 34), 0, 1)], 14044,
                         (8776, 1, 18064, 2033)),
    ("spill", "interior"): ([-1, 0, -1], [(6.199999809265137, 7670, 1234, (30, 8, 4), (109, 15, 20), 1, 1)], 7670, (4022, 0, 8848, 1234)),
    ("sky", "whole"): ([0], [(9.341023445129395, 64403, 0, (0, 3, 0), (137, 25, 41), 1, 1)], 64403, (10336, 1, 74738, 0)),
    ("sky", "interior"): ([-1], [], 0, (0, 0, 0, 0)),
}
# "shore", per box: (wet sources, the bodies, wet, the volume's counts); which of its 91 sources are wet, test_the_shore_of_world_b says
SHORE = {"whole": (37, [(9.341023445129395, 64403, 0, (0, 3, 0), (137, 25, 41), 1, 37)], 64403, (10336, 1, 74738, 0)),
         "interior": (2, [(9.341023445129395, 19738, 0, (30, 8, 2), (109, 21, 31), 1, 2)], 19738, (3954, 0, 23692, 0))}


def flood_b(case, box, world=W, cases=None):
    """The twin's flood of a row, computed afresh: what a mutant of the twin changes."""
    return twin.flood(ws.crafted_field(), *ws.BOXES[box], *world, twin.sources_of((cases or ws.cases_b())[case]))


def volume_bytes_differ(a, b):
    return np.ascontiguousarray(a.water).view(np.uint32) != np.ascontiguousarray(b.water).view(np.uint32)


# -- A on the CPU: the inputs, and the twin's figures on them ---------------------------------------------------------------------------------
def test_the_levels_of_world_b():
    """Eight levels: two are a plane height on which a fused height differs, two the float32 just below one, four between planes where on the
    highest plane under them -- wet, unclamped -- t / scale and t * (1 / scale) part."""
    L, s, oy = ws.levels_b(), W[0], W[1][1]
    assert len({twin.bits(v) for v in L.values()}) == 8
    assert [j for j in range(26) if twin.bits(ws.fused_height(j, s, oy)) != twin.bits(twin.plane_height(j, s, oy))] == list(FUSED_DIFFERS)
    heights = [ws.height(j, W) for j in range(27)]
    assert L["A"] == heights[10] and L["B spilling"] == heights[15]
    assert L["A under the spill"] == ws.below(heights[14]) and L["rock"] == ws.below(heights[20])
    assert [twin.plane_of(L[k], s, oy, 26) for k in ("A", "B spilling", "A under the spill", "rock")] == [10, 15, 13, 19]
    parted = 0
    for name, plane in (("B", 13), ("pocket", 4), ("pocket 2", 5), ("sky", 25)):
        assert heights[plane] < L[name] < heights[plane + 1] and twin.plane_of(L[name], s, oy, 26) == plane
        t, r = twin.clamped_depth(L[name], f32(heights[plane]), s), ws.reciprocal_depth(L[name], f32(heights[plane]), s)
        parted += bool(0 < t < 1 and twin.bits(t) != twin.bits(r))
    assert parted >= 4
    assert set(np.asarray(sum(ws.cases_b().values(), []), f32)[:, 3].tolist()) == {float(f32(v)) for v in L.values()}      # every one is used


def test_the_shore_of_world_b():
    """At least 48 sources half-way between a wet sample and dry ground, on each axis, at j where the reciprocal form picks the other sample."""
    sites = ws.shore_sites()
    assert len(sites) >= 20 and 3 * len(sites) + 1 == len(ws.cases_b()["shore"]) >= 49 and {k for k, _, _ in sites} == {0, 1, 2}
    r = ws.twin_of("shore", "whole", W)
    for i, (k, j, rows) in enumerate(sites):
        rule = [twin.nearest(p[k], W[1][k], W[0]) for p in rows]
        assert (rule[0], rule[2]) == (j, j + 1) and rule != [ws.reciprocal_nearest(p[k], W[1][k], W[0]) for p in rows]
        got = r.source_body[1 + 3 * i:4 + 3 * i].tolist()
        assert sorted((got[0], got[2])) == [-1, 0], (k, j, got)       # wet on one side, dry on the other
    assert len(r.bodies) == 1 and r.wet == ws.twin_of("sky", "whole", W).wet      # the shore's sources flood nothing of their own


@pytest.mark.parametrize("case,box", [(c, b) for c in ("separate", "spill", "sky", "shore") for b in ("whole", "interior")])
def test_twin_reproduces_the_table_of_world_b(case, box):
    r = ws.twin_of(case, box, W)
    if case == "shore":
        source_body, bodies, wet, counts = ws.figures(r)
        assert (sum(v >= 0 for v in source_body), bodies, wet, counts) == SHORE[box]
    else:
        assert ws.figures(r) == TABLE_B[(case, box)]
    assert r.vd == tuple(twin.volume_dim(d) for d in ws.BOXES[box][1]) and r.water.shape == r.body.shape == r.vd


@functools.lru_cache(maxsize=None)
def probes_b():
    """4096 random positions, a quarter of them where the basins are, and the shore's half-way positions; with the twin's answer on the
    "shore" flood of the whole terrain."""
    rng = np.random.default_rng(2612)
    p = rng.uniform(ws.world_of((-2, -2, -2), W), ws.world_of((140, 28, 44), W), (4096, 3)).astype(f32)
    p[:1024] = rng.uniform(ws.world_of((2, 6, 2), W), ws.world_of((132, 19, 22), W), (1024, 3)).astype(f32)
    p = np.concatenate([p, np.asarray([q for _, _, rows in ws.shore_sites() for q in rows], f32)])
    p.setflags(write=False)
    return p, twin.probe(ws.twin_of("shore", "whole", W), p, *W)


def test_the_probes_of_world_b():
    p, (body, depth) = probes_b()
    assert (body >= 0).sum() >= 300 and (body < 0).sum() >= 300
    sides = body[4096:].reshape(-1, 3)
    assert ((sides[:, 0] >= 0) != (sides[:, 2] >= 0)).sum() >= 20
    assert (depth[body >= 0] == f32(ws.levels_b()["sky"]) - p[body >= 0, 1]).all() and (depth[body < 0] == 0).all()


# -- B: three mutants of the twin -------------------------------------------------------------------------------------------------------------
_rule_height = twin.plane_height


def plane_of_by_the_rule(level, scale, origin_y, dim_y):
    """twin.plane_of on the rule's height: the level -> plane search is the host's; the fused mutant is the volume kernel's height alone."""
    under = np.nonzero(_rule_height(np.arange(dim_y), scale, origin_y) <= f32(level))[0]
    return int(under.max()) if len(under) else -1


MUTANTS = {
    "fused height": dict(plane_height=ws.fused_height, plane_of=plane_of_by_the_rule),
    "reciprocal depth": dict(clamped_depth=ws.reciprocal_depth),
    "reciprocal nearest": dict(nearest=ws.reciprocal_nearest),
}


@contextlib.contextmanager
def mutant(name):
    """The twin with one function of the rule swapped for its neighbour."""
    kept = {n: getattr(twin, n) for n in MUTANTS[name]}
    try:
        for n, f in MUTANTS[name].items():
            setattr(twin, n, f)
        yield
    finally:
        for n, f in kept.items():
            setattr(twin, n, f)


def test_a_fused_height_shows_in_world_b():
    changed, zeros_rule, zeros_fused = 0, 0, 0
    for case, box in (("separate", "whole"), ("spill", "whole"), ("spill", "interior")):
        rule = ws.twin_of(case, box, W)
        with mutant("fused height"):
            fused = flood_b(case, box)
        assert np.array_equal(fused.body, rule.body) and fused.bodies.tobytes() == rule.bodies.tobytes()       # the flood itself is integers
        changed += int(volume_bytes_differ(rule, fused).sum())
        zeros_rule, zeros_fused = zeros_rule + twin.volume_counts(rule)[3], zeros_fused + twin.volume_counts(fused)[3]
    assert changed >= 1000 and zeros_rule >= 1000 and zeros_fused != zeros_rule, (changed, zeros_rule, zeros_fused)


def test_a_reciprocal_depth_shows_in_world_b():
    """... on wet samples of at least four levels."""
    levels = set()
    for case, box in (("separate", "whole"), ("spill", "whole"), ("sky", "whole")):
        rule = ws.twin_of(case, box, W)
        with mutant("reciprocal depth"):
            other = flood_b(case, box)
        where = volume_bytes_differ(rule, other) & (rule.body >= 0)
        levels |= {twin.bits(v) for v in rule.bodies["level"][rule.body[where]]}
    assert len(levels) >= 4, levels


def test_a_reciprocal_nearest_shows_in_world_b():
    rule = ws.twin_of("shore", "whole", W)
    p, (body, _) = probes_b()
    with mutant("reciprocal nearest"):
        other = flood_b("shore", "whole")
        other_body, _ = twin.probe(rule, p, *W)
    assert (other.source_body != rule.source_body).sum() >= 16 and (other_body != body).sum() >= 16
    assert (other_body[:4096] == body[:4096]).all()      # random positions do not show it: only the half-way ones do


def test_the_dyadic_world_rounds_nothing():
    """Function by function: at scale 0.5 with origin (-3, 1, 2) each neighbour of the rule computes the rule's bits."""
    s, o = ws.WORLD
    planes = np.arange(26)
    heights = twin.plane_height(planes, s, o[1])
    assert ws.fused_height(planes, s, o[1]).tobytes() == heights.tobytes()
    for level in sorted({row[3] for rows in ws.CASES.values() for row in rows} | {ws.h(j) + d for j in range(26) for d in (0.125, 0.375)}):
        assert ws.reciprocal_depth(f32(level), heights, s).tobytes() == twin.clamped_depth(f32(level), heights, s).tobytes()
    rng = np.random.default_rng(2613)
    for k, n in enumerate(ws.BOXES["whole"][1]):
        assert ws.halfway_flips(k, n, ws.WORLD) == [] and len(ws.halfway_flips(k, n, W)) >= 2
        for p in rng.uniform(ws.position(-2, k), ws.position(n + 2, k), 1024).astype(f32):
            assert ws.reciprocal_nearest(p, o[k], s) == twin.nearest(p, o[k], s)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_no_mutant_shows_in_the_dyadic_world(name):
    """The gap, stated as a test: there the mutants flood and probe as the rule does, so no test in that world can tell them from it."""
    for case, box in (("separate", "whole"), ("spill", "interior"), ("sky", "whole")):
        rule = ws.twin_of(case, box)
        with mutant(name):
            other = flood_b(case, box, ws.WORLD, ws.CASES)
        assert ws.figures(other) == ws.figures(rule) and np.array_equal(other.body, rule.body) and not volume_bytes_differ(rule, other).any()
    s, o = ws.WORLD
    p = np.asarray([q for k, n in enumerate(ws.BOXES["whole"][1]) for j in range(0, n, 3) for q in
                    [tuple(v if a == k else ws.position(9 + a, a) for a in range(3)) for v in ws.halfway(j, k, ws.WORLD)]], f32)
    rule = ws.twin_of("spill", "interior")
    want = twin.probe(rule, p, s, o)
    with mutant(name):
        got = twin.probe(rule, p, s, o)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


# -- A on the GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted_b():
    with ws.terrain(ws.crafted_field(), world=W) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("case,box", [(c, b) for c in ("separate", "spill", "sky", "shore") for b in ("whole", "interior")])
def test_gpu_flood_in_world_b_equals_the_twin(crafted_b, case, box):
    ex, want = crafted_b, ws.twin_of(case, box, W)
    ws.same_result(ex, want, *ex.terrain_flood(twin.sources_of(ws.cases_b()[case]), *ws.bounds_of(box, W)))
    water, body = ws.device_volumes(ex)
    assert np.array_equal(body, want.body) and np.ascontiguousarray(water).tobytes() == np.ascontiguousarray(want.water).tobytes()


@pytest.mark.gpu
def test_gpu_probe_in_world_b_equals_the_twin(crafted_b):
    ex = crafted_b
    ex.terrain_flood(twin.sources_of(ws.cases_b()["shore"]), *ws.bounds_of("whole", W))
    p, (want_body, want_depth) = probes_b()
    for n in (1, 255, 256, 257, len(p)):
        body, depth = ex.water_probe(p[:n])
        assert np.array_equal(body, want_body[:n]) and depth.tobytes() == want_depth[:n].tobytes(), n
    body, depth = ex.water_probe(p[4096:])                  # the half-way positions alone, in the first lanes
    assert np.array_equal(body, want_body[4096:]) and depth.tobytes() == want_depth[4096:].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("box", ["whole", "interior"])
def test_gpu_extraction_in_world_b(crafted_b, box):
    """water_extract of the device's volume against the CPU oracle's extract of the twin's volume."""
    import oracle
    from extract_checks import assert_tris_match
    ex, want = crafted_b, ws.twin_of("spill", box, W)
    ws.same_result(ex, want, *ex.terrain_flood(twin.sources_of(ws.cases_b()["spill"]), *ws.bounds_of(box, W)))
    T = ex.water_extract()
    got, offs = ex.read_triangles()
    want_tris, want_offs, _ = oracle.extract_grid(want.water, threads=4)
    assert T == len(want_tris) > 1000 and np.array_equal(offs, want_offs)
    assert_tris_match(got, want_tris)


# -- C: the numbering kernel at its size ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pocket_field():
    """Rock with 68 x 8 x 20 = 10 880 single-sample pockets, none touching another; and their samples in ascending grid index."""
    g = np.full(tuple(d + 2 for d in ws.DIMS), ws.ROCK, f32)
    g[1:136:2, 2:17:2, 1:40:2] = ws.AIR
    x, y, z = np.nonzero(~(g > 0))
    order = np.argsort(grid_index(np.stack([x, y, z], axis=1)))
    g.setflags(write=False)
    return g, np.stack([x, y, z], axis=1)[order]


def grid_index(samples):
    dx, dy, _ = ws.BOXES["whole"][1]
    return samples[:, 0] + dx * (samples[:, 1] + dy * samples[:, 2].astype(np.int64))


def rows_on(samples, levels, rng):
    """Sources a little off their samples (under a third of a sample's width)."""
    p = np.asarray([ws.world_of(tuple(int(v) for v in s), W) for s in samples]) + rng.uniform(-0.09, 0.09, (len(samples), 3))
    return twin.sources_of(np.concatenate([p, np.asarray(levels, np.float64).reshape(-1, 1)], axis=1))


HIGH = ws.height(17, W) + 0.1                 # over every pocket
C3_LEVELS = [HIGH] + [ws.height(j, W) + 0.1 for j in (15, 13, 11, 9, 7, 5, 3)]


@functools.lru_cache(maxsize=None)
def numbering_case(name):
    """(sources, the samples they stand on or None, the twin's flood) of C1, C2 and C3."""
    g, pockets = pocket_field()
    rng = np.random.default_rng([2620, ("C1", "C2", "C3").index(name)])
    if name == "C1":                            # 4096 distinct pockets, shuffled, one level
        on = pockets[rng.permutation(len(pockets))[:4096]]
        src = rows_on(on, [HIGH] * 4096, rng)
    elif name == "C2":                          # two levels of 2048 distinct pockets each, under both, interleaved at random
        on = pockets[rng.permutation(len(pockets))[:4096]]
        src = rows_on(on, np.where(rng.permutation(4096) < 2048, HIGH, ws.below(HIGH)), rng)
    else:                                       # 8 levels, about 1500 pockets with repeats, a few of them often; rock, outside, above the level
        some = pockets[rng.permutation(len(pockets))[:1500]]
        weight = np.where(np.arange(1500) < 16, 12.0, 1.0)
        on = some[rng.choice(1500, 4096, p=weight / weight.sum())].copy()
        levels = rng.choice(C3_LEVELS, 4096, p=[0.58] + [0.06] * 7)
        kind = rng.random(4096)
        on[kind < 0.01, 0] += 1                 # the rock next to the pocket
        on[(kind >= 0.01) & (kind < 0.02), 0] -= 200   # outside the box
        src = rows_on(on, levels, rng)
    return src, on, twin.flood(g, *ws.BOXES["whole"], *W, src)


def test_numbering_c1_on_the_twin():
    src, on, r = numbering_case("C1")
    assert len(r.bodies) == 4096 == _lib.WATER_MAX_SOURCES and len(np.unique(grid_index(on))) == 4096
    assert np.array_equal(grid_index(r.bodies["seed"]), np.sort(grid_index(on)))           # body k's seed is the k-th smallest grid index
    assert (r.bodies["n_samples"] == 1).all() and (r.bodies["n_sources"] == 1).all() and (r.bodies["flags"] == 0).all() and (r.bodies["n_surface"] == 0).all()
    assert np.array_equal(np.sort(r.source_body), np.arange(4096)) and np.array_equal(grid_index(r.bodies["seed"][r.source_body]), grid_index(on))
    assert (r.source_body[:-1] > r.source_body[1:]).sum() > 1000                           # in a shuffled order


def test_numbering_c2_on_the_twin():
    src, on, r = numbering_case("C2")
    first = src["level"] == f32(HIGH)
    assert len(r.bodies) == 4096 and first.sum() == 2048 and len({twin.bits(v) for v in src["level"]}) == 2
    assert (r.bodies["level"][:2048] == f32(HIGH)).all() and (r.bodies["level"][2048:] == f32(ws.below(HIGH))).all()
    for part, sel in ((r.bodies[:2048], first), (r.bodies[2048:], ~first)):
        assert np.array_equal(grid_index(part["seed"]), np.sort(grid_index(on[sel])))      # each level by seed; the second numbered from 2048
    assert r.source_body[first].max() == 2047 and r.source_body[~first].min() == 2048 and np.array_equal(np.sort(r.source_body), np.arange(4096))


def test_numbering_c3_on_the_twin():
    src, on, r = numbering_case("C3")
    per_level = [int((r.bodies["level"] == f32(v)).sum()) for v in C3_LEVELS]
    assert len({twin.bits(v) for v in src["level"]}) == 8 and max(per_level) > 1024 and sum(v > 0 for v in per_level) >= 4, per_level
    assert (r.bodies["n_sources"] > 1).sum() >= 500 and r.bodies["n_sources"].max() >= 8 and (r.source_body < 0).sum() >= 100
    assert r.bodies["n_sources"].sum() == (r.source_body >= 0).sum() and (r.bodies["n_samples"] == 1).all()
    wet_rows = r.source_body >= 0
    joined = wet_rows & (src["level"] < r.bodies["level"][np.maximum(r.source_body, 0)])
    assert joined.sum() >= 100                                                             # a duplicate at a lower level joins
    g = pocket_field()[0]
    inside = (on[:, 0] >= 0)
    in_rock = inside & (g[np.maximum(on[:, 0], 0), on[:, 1], on[:, 2]] > 0)
    over = inside & ~in_rock & ~wet_rows
    assert (~inside).sum() >= 20 and in_rock.sum() >= 20 and over.sum() >= 50 and not wet_rows[~inside | in_rock].any()


@pytest.fixture(scope="module")
def pocket_ex():
    with ws.terrain(pocket_field()[0], world=W) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_gpu_numbering_equals_the_twin(pocket_ex, name):
    src, _, want = numbering_case(name)
    source_body, n = pocket_ex.terrain_flood(src, *ws.bounds_of("whole", W))
    assert n == len(want.bodies) and (name == "C3" or n == 4096)
    ws.same_result(pocket_ex, want, source_body, n)


# -- D: a level under the box ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def under_the_box():
    """The crafted field has no open sample on plane 2, the bottom plane of the box "interior": the pocket's floor is plane 3.  So ONE sample is
    dug here in a copy, (62, 2, 31) under the pocket's floor.  A source in the pocket at the pocket's level wets it.  The low level lies
    between planes 1 and 2: under the box.  Its sources: one on the dug sample, which joins; one on an open, dry sample of basin A."""
    g = ws.crafted_field().copy()
    assert (g[30:110, 2, 2:32] > 0).all()
    g[62, 2, 31] = ws.AIR
    low = ws.height(1, W) + 0.1
    assert ws.height(1, W) < low < ws.height(2, W) and twin.plane_of(low, W[0], W[1][1], 26) - ws.BOXES["interior"][0][1] == -1
    sources = [ws.source((62, 4, 31), ws.levels_b()["pocket"], W), ws.source((62, 2, 31), low, W), ws.source((35, 9, 10), low, W)]
    flood = lambda rows: twin.flood(g, *ws.BOXES["interior"], *W, twin.sources_of(rows))
    return g, sources, flood(sources), flood(sources[:1]), flood(sources[1:])


def test_under_the_box_on_the_twin():
    g, sources, both, high, low = under_the_box()
    assert not g[35, 9, 10] > 0 and both.source_body.tolist() == [0, 0, -1] and len(both.bodies) == 1 and int(both.bodies[0]["n_sources"]) == 2
    assert both.bodies[0]["lo"].tolist()[1] == 2 and int(both.bodies[0]["flags"]) == _lib.WATER_AT_FACE
    assert int(high.bodies[0]["n_sources"]) == 1 and np.array_equal(high.body, both.body) and high.water.tobytes() == both.water.tobytes()
    assert low.source_body.tolist() == [-1, -1] and len(low.bodies) == 0 and (low.water == -1).all() and (low.body == -1).all() and low.vd == both.vd


@pytest.mark.gpu
def test_gpu_a_level_under_the_box():
    g, sources, both, high, low = under_the_box()
    with ws.terrain(g, world=W) as ex:
        for rows, want in ((sources, both), (sources[1:], low), (sources[:1], high), (sources[1:], low)):
            ws.same_result(ex, want, *ex.terrain_flood(twin.sources_of(rows), *ws.bounds_of("interior", W)))


# -- E: box shapes -----------------------------------------------------------------------------------------------------------------------------
E_DIMS, E_SEED = (64, 16, 16), 3                # the seed: chosen on the CPU so that test_box_shapes_on_the_twin holds
# (first sample, samples per axis): the largest first and one sample right after it, for the buffers only ever grow
E_BOXES = [((0, 0, 0), (66, 18, 18)), ((5, 3, 7), (1, 1, 1)), ((1, 2, 3), (65, 11, 10)), ((2, 0, 0), (64, 10, 11)), ((3, 9, 9), (63, 9, 9)), ((0, 5, 0), (66, 1, 18)),
           ((10, 4, 6), (2, 8, 8)), ((7, 1, 2), (1, 11, 9)), ((0, 16, 4), (64, 2, 2)), ((20, 3, 17), (40, 8, 1)), ((64, 0, 0), (2, 18, 18)), ((0, 0, 5), (65, 18, 1))]


@functools.lru_cache(maxsize=None)
def shapes_case(seed=E_SEED):
    """One random terrain and per box (sources, the twin's flood): 16 sources on random open samples of the box, a little off them, on 4
    levels between the plane under the box and the one over it."""
    rng = np.random.default_rng([2630, seed])
    g = ws.random_field(rng, E_DIMS)
    out = []
    for first, ext in E_BOXES:
        inside = np.argwhere(~(g[tuple(slice(first[k], first[k] + ext[k]) for k in range(3))] > 0))
        if not len(inside):
            inside = np.zeros((1, 3), np.int64)
        levels = rng.uniform(ws.height(first[1] - 1, W), ws.height(first[1] + ext[1], W), 4)
        src = rows_on(inside[rng.choice(len(inside), 16)] + np.asarray(first), levels[np.arange(16) % 4], rng)
        out.append((src, twin.flood(g, first, ext, *W, src)))
    return g, out


def test_box_shapes_on_the_twin():
    for axis, sizes in enumerate(((1, 2, 63, 64, 65, 66), (1, 2, 8, 9, 10, 11), (1, 2, 8, 9, 10, 11))):
        assert set(sizes) <= {ext[axis] for _, ext in E_BOXES} and any(first[axis] for first, _ in E_BOXES)
    volume = lambda ext: ext[0] * ext[1] * ext[2]
    assert volume(E_BOXES[0][1]) == max(volume(ext) for _, ext in E_BOXES) and E_BOXES[1][1] == (1, 1, 1)
    assert {twin.volume_dim(d) for _, ext in E_BOXES for d in ext} >= {10, 18, 66} and (twin.volume_dim(10), twin.volume_dim(11)) == (10, 18)
    _, floods = shapes_case()
    assert sum(len(r.bodies) for _, r in floods) >= 20 and sum(r.near for _, r in floods) >= 200
    for (first, ext), (_, r) in zip(E_BOXES, floods):
        assert r.ext == ext and r.vd == tuple(twin.volume_dim(d) for d in ext)
    assert sum(len(r.bodies) for (_, ext), (_, r) in zip(E_BOXES, floods) if ext[1] == 1) >= 1
    assert sum(len(r.bodies) for (_, ext), (_, r) in zip(E_BOXES, floods) if 1 in (ext[0], ext[2])) >= 2


@pytest.mark.gpu
def test_gpu_box_shapes_equal_the_twin():
    g, floods = shapes_case()
    with ws.terrain(g, E_DIMS, W) as ex:
        for (first, ext), (src, want) in zip(E_BOXES, floods):
            ws.same_result(ex, want, *ex.terrain_flood(src, *ws.bounds_of((first, ext), W, E_DIMS)))
            bodies = ex.water_bodies()
            assert ex.water_info()[2] == tuple(twin.volume_dim(d) for d in ext)
            if ext[1] == 1:
                assert (bodies["n_surface"] == 0).all()
            if 1 in (ext[0], ext[2]):
                assert (bodies["flags"] == _lib.WATER_AT_FACE).all()
