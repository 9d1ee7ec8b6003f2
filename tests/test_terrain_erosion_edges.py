"""VTMC_MOD_EROSION (include/vtmc_erosion.h, csrc/terrain_erosion.hip) beyond one parameter set, 40 steps and noise terrain.
test_terrain_erosion.py erodes the noise world with P, whose dt = 0.25 makes dt * Kr, dt * G, 1 / dt and Ke * dt exact scalings, for at
most 40 steps, before the state holds its first subnormal, and on ground that has no two equal neighbouring heights.  Here:
  1   a census in the twin (erosion_twin.step(census=)) counts the columns that took each branch of the rule, and a table of cases -- off
      the dyadic parameters, at the caps, with Ke * dt == 1, with a subnormal rain, with the rates at 0 and at 1, 600, 4096 and 65536 steps,
      and crafted heightfields (terraces of bit-equal heights, a flat floor, a checkerboard of walls, an L-shaped wall, both kinds of
      inactive column side by side) -- is held to conditions on the CPU: every branch is taken somewhere, the state is finite at every
      step (the header's "Why the caps", tested);
  2   seven mutants of the twin, each one operation swapped for a near neighbour (a fused keep, G as a double, 1 / dt of the unrounded dt,
      the two reciprocal forms, subnormals flushed, fmin / fmax): each shows on a case of the table -- fmin / fmax on none, for no NaN
      arises -- and none shows at P in 40 steps, which is the gap;
  3   on the GPU every case equals the twin as raw bytes, four of them through the LDS variant too; a shape matrix around the 64-lane row
      and the 4-row workgroup; boxes one and two samples thick; two erosions in one queue, in both orders; the clamp's read-back.
Every GPU comparison is for EQUALITY (erosion_support.erode_and_compare): the grid as uint32, the five maps as raw bytes, the report,
the dirty list."""
import collections
import contextlib
import fractions
import functools
import time

import numpy as np
import pytest

from volumetricterrain_amd import _lib
import erosion_support as es
import erosion_twin as twin
from erosion_support import P
from terrain_twin import bits, block_list, dirty_ids

f32 = np.float32
TINY = np.finfo(f32).tiny
NX, NY, NZ = es.CRAFT_TOP[0] + 1, es.CRAFT_TOP[1] + 1, es.CRAFT_TOP[2] + 1   # the crafted world's samples: 74 x 26 x 50
CRAFT_WHOLE = ((0, 0, 0), es.CRAFT_TOP)


# -- the crafted heightfields: (h, active) [z, x] of the crafted world, exact in float32 ----------------------------------------------------
def ground(seed):
    rng = np.random.default_rng([2701, seed])
    z, x = np.mgrid[0:NZ, 0:NX]
    return (11 + 3 * np.sin(x * 0.21) * np.cos(z * 0.27) + 0.05 * x + rng.random((NZ, NX))).astype(f32)


def terraces():
    """Terraces 5 columns wide along x and 7 along z of bit-equal heights; the steps between them, 0.125 and 0.75 along x and 0.25 and
    0.75 along z in turn, lie under and over the talus of the case, 0.5."""
    z, x = np.mgrid[0:NZ, 0:NX]
    step_x = np.cumsum(np.where(np.arange(NX // 5 + 1) % 2, 1.5, 0.25))[x // 5]
    step_z = np.cumsum(np.where(np.arange(NZ // 7 + 1) % 2, 0.25, 0.75))[z // 7]
    return (f32(3.3) + step_x.astype(f32) * f32(0.5) + step_z.astype(f32)).astype(f32), np.ones((NZ, NX), bool)


def flat():
    return np.full((NZ, NX), f32(9.3)), np.ones((NZ, NX), bool)


def checkerboard():
    """Rolling ground; on x 8..39, z 6..29 every other column is a wall, which leaves the columns between them without a neighbour."""
    h, active = ground(1), np.ones((NZ, NX), bool)
    z, x = np.mgrid[0:NZ, 0:NX]
    active[(x >= 8) & (x < 40) & (z >= 6) & (z < 30) & ((x + z) % 2 == 0)] = False
    return h, active


def l_wall():
    """An L-shaped wall two columns thick (so it holds both kinds of inactive column side by side: solid to the top of the box and open
    to its bottom), with its re-entrant corner at (30, 20), and a second L inside it, one column thick."""
    h, active = ground(2), np.ones((NZ, NX), bool)
    active[20:22, 30:60] = False
    active[20:42, 30:32] = False
    active[30, 40:50] = False
    active[30:38, 40] = False
    return h, active


TERRAINS = {"terraces": terraces, "flat": flat, "checkerboard": checkerboard, "l_wall": l_wall}


@functools.lru_cache(maxsize=None)
def grid_of(terrain):
    """The samples [x, y, z] of a terrain of the table, read-only: the noise world as terrain_twin.py builds it, or a crafted heightfield
    through craft_grid."""
    g = es.world_grid() if terrain == "noise" else es.craft_grid(*TERRAINS[terrain](), ny=NY)
    g.setflags(write=False)
    return g


# -- the table ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "terrain lo hi params steps")
OFF = twin.Params(0.013, 0.07, 1.3, 0.37, 0.21, 0.3, 0.45, 0.11)
# OFF rounds in every constant, yet a fused keep and a 1 / dt taken from the double 0.3 happen to round to the rule's bits there; at
# dt = 0.58 with Ke = 0.57 all three constants tell the rule from its neighbours (test_the_parameters_of_the_table): the crafted cases use it.
# 1 / dt enters the state only where the speed is capped, which takes a column that drains in one step: d2 is 0 there, so is e, and only
# the deposit q = Kd * (s - C) feels the cap.  Of the table's cases the checkerboard has such columns.
OFF2 = OFF._replace(evaporation=0.57, dt=0.58)
CAPS = twin.Params(256, 1, 65536, 1, 1, 1, 0, 0.125)
KEEP0_DT, KEEP0_KE = 0.3, 3.3333332538604736   # float32 values whose float32 product is exactly 1


def noise(params, steps, lo=es.WHOLE[0], hi=es.WHOLE[1]):
    return Case("noise", lo, hi, params, steps)


def crafted(terrain, params, steps):
    return Case(terrain, *CRAFT_WHOLE, params, steps)


CASES = {
    "off_dyadic": noise(OFF, 300),
    "caps": noise(CAPS, 300),
    "caps_wet": noise(CAPS._replace(evaporation=0), 300),
    "keep0": noise(OFF._replace(evaporation=KEEP0_KE, dt=KEEP0_DT), 60),
    "tiny_rain": noise(OFF._replace(rain=1e-42, dt=0.3), 60),
    "zeros": noise(OFF._replace(dissolve=0, deposit=0), 80),
    "ones": noise(OFF._replace(dissolve=1, deposit=1), 80),
    "dry": noise(OFF._replace(rain=0), 30),
    "long_600": noise(P, 600),
    "long_4096": noise(P, 4096),
    "limit": noise(P, 65536, (10, 0, 10), (17, 33, 15)),
    "terraces": crafted("terraces", OFF2._replace(talus=0.5), 120),
    "flat": crafted("flat", OFF2, 120),
    "checkerboard": crafted("checkerboard", OFF2, 120),
    "l_wall": crafted("l_wall", OFF2, 120),
}

Run = collections.namedtuple("Run", "result census seconds")


@functools.lru_cache(maxsize=None)
def twin_of(name):
    """The twin's erosion of a case, its census, and the seconds it took: computed once, shared by every test of the module."""
    c = CASES[name]
    census = twin.new_census()
    t0 = time.perf_counter()
    r = twin.erode(grid_of(c.terrain), c.lo, c.hi, c.steps, c.params, census)
    seconds = time.perf_counter() - t0
    for a in r:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return Run(r, census, seconds)


def fresh(name):
    """The same erosion computed afresh: what a mutant installed in the twin changes."""
    c = CASES[name]
    return twin.erode(grid_of(c.terrain), c.lo, c.hi, c.steps, c.params)


def differs(a, b):
    """Whether two results differ in the grid or in a map, as raw bytes."""
    return any(np.ascontiguousarray(getattr(a, n)).tobytes() != np.ascontiguousarray(getattr(b, n)).tobytes() for n in ("grid", "before", "after", "water", "sediment", "active"))


def subnormal(a):
    return (a != 0) & (np.abs(a) < TINY)


# -- 1: the conditions of the table, on the CPU ------------------------------------------------------------------------------------------------
def test_the_parameters_of_the_table():
    """off_dyadic rounds where P does not; keep0's product is 1 in float32 and its dt is no power of two; caps sits on every cap; the
    mirror accepts them all (the library's check is the same expression: test_gpu_cases_equal_the_twin runs them)."""
    one = f32(1)
    for p, exact in ((P, True), (OFF, False)):
        dt, ke, kr = f32(p.dt), f32(p.evaporation), f32(p.rain)
        products = [float(dt) * float(kr) == float(f32(dt * kr)), float(dt) * float(f32(twin.G)) == float(f32(dt * f32(twin.G))),
                    fractions.Fraction(1) / fractions.Fraction(float(dt)) == fractions.Fraction(float(one / dt)), float(ke) * float(dt) == float(f32(ke * dt))]
        assert all(products) if exact else not any(products), (p, products)
    dt, ke = f32(OFF2.dt), f32(OFF2.evaporation)
    assert fused_keep(f32, ke, dt) != twin.keep_of(f32, ke, dt) and f32(one / dt) != f32(1.0 / OFF2.dt) and f32(dt * f32(twin.G)) != f32(float(dt) * twin.G)
    dt, ke = f32(OFF.dt), f32(OFF.evaporation)
    assert fused_keep(f32, ke, dt) == twin.keep_of(f32, ke, dt) and f32(one / dt) == f32(1.0 / OFF.dt) and f32(dt * f32(twin.G)) != f32(float(dt) * twin.G)
    dt, ke = f32(KEEP0_DT), f32(KEEP0_KE)
    assert float(ke) == KEEP0_KE and f32(ke * dt) == one and float(ke) * float(dt) != 1.0 and np.frexp(dt)[0] != 0.5
    assert twin.keep_of(f32, ke, dt) == 0
    assert (CAPS.rain, CAPS.capacity, CAPS.thermal_rate) == (_lib.EROSION_MAX_RAIN, _lib.EROSION_MAX_CAPACITY, _lib.EROSION_MAX_THERMAL)
    assert (CAPS.dt, CAPS.evaporation * CAPS.dt, CAPS.talus, CASES["limit"].steps) == (1, 1, 0, _lib.EROSION_MAX_ITERATIONS)
    assert 0 < f32(CASES["tiny_rain"].params.rain) < TINY
    for c in CASES.values():
        es.erosion(c.lo, c.hi, c.steps, c.params)


def test_the_crafted_heightfields_read_back_exactly():
    for name, make in TERRAINS.items():
        h, active = make()
        h0, a0 = twin.heights(grid_of(name), *CRAFT_WHOLE)
        assert np.array_equal(a0, active) and np.array_equal(bits(h0[active]), bits(h[active])), name
    g = grid_of("l_wall")
    _, active = l_wall()
    ix, iz = np.nonzero(~active.T)
    kinds = {(int(x), int(z)): bool(g[x, NY - 1, z] > 0) for x, z in zip(ix, iz)}
    pairs = sum(1 for (x, z), solid in kinds.items() if solid and kinds.get((x + 1, z)) is False)
    assert pairs >= 10   # a column solid to the top of the box next to one open to its bottom
    # re-entrant corners: an active column away from the faces of the box with walls on two sides that meet
    cnt = twin.State(*l_wall()).counts
    inner = active.copy()
    inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
    assert sum(int((inner & ~cnt[kx] & ~cnt[kz]).sum()) for kx in (0, 1) for kz in (2, 3)) >= 2


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_stays_finite_at_every_step(name):
    """The header's "Why the caps", tested: b, d, s and the fluxes are finite after every step, at the caps as anywhere."""
    run = twin_of(name)
    assert run.census["not_finite"] == 0
    r = run.result
    assert all(np.isfinite(a).all() for a in (r.after, r.water, r.sediment)) and r.info["n_active"] > 0
    if name == "flat":   # and a flat floor stays flat
        assert r.info["n_rewritten"] == 0 and (r.sediment == 0).all() and (r.water > 0).all()
    else:
        assert r.info["n_rewritten"] > 0


def test_every_branch_of_the_rule_is_taken_in_some_case():
    total = twin.new_census()
    for name in CASES:
        for key, v in twin_of(name).census.items():
            total[key] += v
    assert set(total) == set(twin.CENSUS_KEYS)
    never = ("not_finite", "subnormal_b")   # a height of the table is never within 1e-38 of 0; water, sediment and the fluxes are
    for key in twin.CENSUS_KEYS:
        assert (total[key] > 0) == (key not in never), (key, total[key])


def test_the_conditions_of_the_named_cases():
    tiny = twin_of("tiny_rain")
    assert subnormal(tiny.result.water).sum() >= 1000 and tiny.census["subnormal_f"] > 0 and tiny.census["subnormal_d"] > 0
    t = twin_of("terraces").census
    assert t["sign_zero"] >= 100 and t["sa_raised"] >= 100 and t["thermal_moves"] > 0 and t["sign_minus"] == t["sign_plus"] > 0
    h, active = terraces()
    first = twin.new_census()
    twin.step(twin.State(h, active), CASES["terraces"].params, first)   # in the first step alone, on the heights as crafted
    assert first["sign_zero"] >= 100 and first["sa_raised"] >= 100
    st = twin.State(*checkerboard())
    alone = st.active & ~(st.counts[0] | st.counts[1] | st.counts[2] | st.counts[3])
    assert alone.sum() >= 20
    caps = twin_of("caps")
    assert caps.result.info["n_clamped"] > 0 and (caps.result.water == 0).all() and twin_of("caps_wet").result.water.max() > 0
    assert (twin_of("keep0").result.water == 0).all() and twin_of("keep0").census["sp_capped"] > 0    # keep == 0 dries every column, every step
    assert twin_of("dry").census["transport_dry"] > 0 and twin_of("dry").census["shallow"] > 0
    assert twin_of("long_600").census["negative_s"] > 0 and twin_of("long_600").census["subnormal_s"] > 0
    for name in ("zeros", "ones"):
        p = CASES[name].params
        assert p.dissolve == p.deposit == (name == "ones") and twin_of(name).census["takes"] > 0 and twin_of(name).census["deposits"] > 0
    assert (twin_of("zeros").result.sediment == 0).all() and twin_of("zeros").result.info["n_rewritten"] > 0      # the thermal half alone moves it
    info = twin_of("limit").result.info
    assert (info["nx"], info["nz"], info["iterations"]) == (8, 6, 65536) and info["n_active"] == 48


# -- 2: mutants of the twin ---------------------------------------------------------------------------------------------------------------
def to_f32(q):
    """The float32 nearest a Fraction, ties to even."""
    c = f32(float(q))
    near = [np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))]
    return min(near, key=lambda v: (abs(fractions.Fraction(float(v)) - q), int(v.view(np.uint32)) & 1))


def fused_keep(t, ke, dt):
    """1 - Ke * dt rounded once, as an fma gives it."""
    return to_f32(1 - fractions.Fraction(float(ke)) * fractions.Fraction(float(dt))) if t is f32 else t(1) - ke * dt


def flushed(a):
    return np.where((a != 0) & (np.abs(a) < np.finfo(np.asarray(a).dtype).tiny), np.copysign(np.zeros_like(a), a), a)


MUTANTS = {
    "keep fused": dict(keep_of=fused_keep),
    "G a double": dict(dt_g_of=lambda t, dt: t(float(dt) * 9.81)),
    "1 / dt of a double": dict(inv_dt_of=lambda t, dt, given_dt: t(1.0 / float(given_dt))),
    "fr by the reciprocal": dict(fraction_of=lambda f, dt, d1: twin.result(f * twin.result(dt / d1))),
    "u by the reciprocal": dict(quotient=lambda a, b: a * twin.result(np.ones_like(b) / b)),
    "subnormals flushed": dict(result=flushed),
    "fmin and fmax": dict(lesser=np.fmin, greater=np.fmax),
}
CONSTANTS = ("keep fused", "G a double", "1 / dt of a double")
# where each mutant is looked for: the first case that shows it ends the search
SHOWS_ON = {"keep fused": ["terraces", "keep0"], "G a double": ["off_dyadic", "terraces"], "1 / dt of a double": ["checkerboard"],
            "fr by the reciprocal": ["off_dyadic"], "u by the reciprocal": ["off_dyadic"], "subnormals flushed": ["tiny_rain"]}


@contextlib.contextmanager
def mutant(name):
    """The twin with one operation of the rule swapped for its neighbour."""
    kept = {n: getattr(twin, n) for n in MUTANTS[name]}
    try:
        for n, f in MUTANTS[name].items():
            setattr(twin, n, f)
        yield
    finally:
        for n, f in kept.items():
            setattr(twin, n, f)


@pytest.mark.parametrize("name", list(SHOWS_ON))
def test_each_mutant_shows_on_a_case_of_the_table(name):
    for case in SHOWS_ON[name]:
        with mutant(name):
            other = fresh(case)
        if differs(other, twin_of(case).result):
            return
    pytest.fail("%s computes the rule's bits on %s" % (name, SHOWS_ON[name]))


@pytest.mark.parametrize("case", list(CASES))
def test_fmin_and_fmax_change_nothing_on_any_case(case):
    """No NaN arises (test_every_case_stays_finite_at_every_step) and no comparison is between zeros of two signs, so the rule may state
    min and max as a < b ? a : b and a > b ? a : b: the library's selects and a fminf / fmaxf would compute the same bytes."""
    with mutant("fmin and fmax"):
        other = fresh(case)
    assert not differs(other, twin_of(case).result)


@functools.lru_cache(maxsize=None)
def at_p():
    """P, 40 steps, the whole noise world: the most the library has been compared on before this file."""
    return twin.erode(es.world_grid(), *es.WHOLE, 40, P)


@pytest.mark.parametrize("name", CONSTANTS + ("subnormals flushed",))
def test_no_such_mutant_shows_at_p_in_40_steps(name):
    """The gap, stated as a test: at dt = 0.25 the constants come out the same however they are made, and in 40 steps nothing is
    subnormal yet."""
    with mutant(name):
        other = twin.erode(es.world_grid(), *es.WHOLE, 40, P)
    assert not differs(other, at_p())


def test_the_flush_shows_in_the_water_of_tiny_rain():
    rule = twin_of("tiny_rain").result
    with mutant("subnormals flushed"):
        other = fresh("tiny_rain")
    assert other.water.tobytes() != rule.water.tobytes() and (other.water == 0).all()


def test_the_twin_is_itself_again_after_a_mutant():
    assert not differs(fresh("dry"), twin_of("dry").result)


# -- 3: the GPU --------------------------------------------------------------------------------------------------------------------------
HISTORY = 1 << 26


@pytest.fixture(scope="module")
def noise_ex():
    with es.World() as ex:
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(es.world_grid()))   # the twins of the table were made from this grid
        yield ex


@pytest.fixture(scope="module")
def craft_ex():
    with es.World(dims=es.CRAFT_DIMS, grid=grid_of("flat")) as ex:
        yield ex


def device_of(name, noise_ex, craft_ex):
    """The module's context that holds the case's kind of world, refilled with the case's samples; and the world's cells."""
    terrain = CASES[name].terrain
    ex, dims = (noise_ex, es.DIMS) if terrain == "noise" else (craft_ex, es.CRAFT_DIMS)
    ex.terrain_write_samples(grid_of(terrain))
    return ex, dims


def run_case(name, noise_ex, craft_ex):
    c = CASES[name]
    ex, dims = device_of(name, noise_ex, craft_ex)
    want = twin_of(name).result
    before, _ = es.erode_and_compare(ex, c.lo, c.hi, c.steps, c.params, dims, want)
    assert np.array_equal(bits(before), bits(grid_of(c.terrain)))
    return ex, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "limit"])
def test_gpu_cases_equal_the_twin(noise_ex, craft_ex, name):
    run_case(name, noise_ex, craft_ex)


@pytest.mark.gpu
def test_gpu_the_limit_of_65536_steps_equals_the_twin(noise_ex, craft_ex):
    """196611 launches queued back to back on an 8 x 6 box; prints the seconds of both sides."""
    want = twin_of("limit")
    c = CASES["limit"]
    ex, _ = device_of("limit", noise_ex, craft_ex)
    t0 = time.perf_counter()
    ex.terrain_update([es.erosion(c.lo, c.hi, c.steps, c.params)])
    info = ex.erosion_info()   # waits for the queue
    seconds = time.perf_counter() - t0
    print("limit: 65536 steps on 8 x 6 columns: device %.2f s, twin %.2f s" % (seconds, want.seconds))
    assert info == want.result.info
    es.same_maps(ex, want.result)
    assert np.array_equal(bits(ex.terrain_read_samples()), bits(want.result.grid))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["off_dyadic", "tiny_rain", "caps", "terraces"])
def test_gpu_cases_staged_in_lds_equal_the_twin(noise_ex, craft_ex, name):
    ex = craft_ex if CASES[name].terrain != "noise" else noise_ex
    assert ex._L.vtmc_debug_erosion_lds(ex._h, 1) == _lib.OK
    try:
        run_case(name, noise_ex, craft_ex)
    finally:
        assert ex._L.vtmc_debug_erosion_lds(ex._h, 0) == _lib.OK


@pytest.mark.gpu
def test_gpu_clamped_columns_read_back_to_their_height(noise_ex, craft_ex):
    ex, want = run_case("caps", noise_ex, craft_ex)
    c = CASES["caps"]
    assert ex.erosion_info()["n_clamped"] == want.info["n_clamped"] > 0
    h, active = twin.heights(ex.terrain_read_samples(), c.lo, c.hi)
    low, high = f32(c.lo[1] + 0.5), f32(c.hi[1] - 1)
    clamped = (want.active > 0) & ((want.after == low) | (want.after == high))
    assert clamped.sum() == want.info["n_clamped"] and (want.after == low).any() and (want.after == high).any()   # both ends of the clamp
    assert active[clamped].all() and np.array_equal(bits(h[clamped]), bits(want.after[clamped]))


# the shape matrix: boxes of one crafted grid 138 samples long, around the 64-lane row and the 4-row workgroup
SHAPE_DIMS = (136, 16, 8)
SHAPE_NX, SHAPE_NZ = (1, 63, 64, 65, 128, 129), (1, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def shape_grid():
    """Rough ground with walls of both kinds scattered over it, one column in 16."""
    nx, ny, nz = (d + 2 for d in SHAPE_DIMS)
    rng = np.random.default_rng(2702)
    z, x = np.mgrid[0:nz, 0:nx]
    h = (8 + 2 * np.sin(x * 0.37) * np.cos(z * 0.9) + 2 * rng.random((nz, nx))).astype(f32)
    g = es.craft_grid(h, rng.random((nz, nx)) >= 1 / 16, ny=ny)
    g.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def shape_ex():
    with es.World(dims=SHAPE_DIMS, grid=shape_grid()) as ex:
        yield ex


@pytest.mark.gpu
@pytest.mark.parametrize("nx", SHAPE_NX)
def test_gpu_shape_matrix_equals_the_twin(shape_ex, nx):
    ex, g = shape_ex, shape_grid()
    try:
        for nz in SHAPE_NZ:
            for x0, z0 in ((0, 0), (138 - nx, 10 - nz), ((138 - nx) // 2 | 1, (10 - nz) // 2)):
                lo, hi = (x0, 0, z0), (x0 + nx - 1, 17, z0 + nz - 1)
                want = twin.erode(g, lo, hi, 5, OFF2)
                assert (want.info["nx"], want.info["nz"]) == (nx, nz)
                for lds in (0, 1):
                    ex.terrain_write_samples(g)
                    assert ex._L.vtmc_debug_erosion_lds(ex._h, lds) == _lib.OK
                    es.erode_and_compare(ex, lo, hi, 5, OFF2, SHAPE_DIMS, want)
    finally:
        assert ex._L.vtmc_debug_erosion_lds(ex._h, 0) == _lib.OK


def test_the_shape_matrix_has_work_in_every_box():
    g = shape_grid()
    _, active = twin.heights(g, (0, 0, 0), (137, 17, 9))
    assert 40 <= (~active).sum() <= 160 and {bool(g[x, 17, z] > 0) for z, x in zip(*np.nonzero(~active))} == {True, False}
    r = twin.erode(g, (0, 0, 0), (128, 17, 4), 5, OFF2)
    assert r.info["n_rewritten"] > 500 and r.water.max() > 0


THIN = ((3, 7, 4), (60, 7, 40))      # one sample thick in y: no column can be active
TWO = ((3, 8, 4), (60, 9, 40))       # two samples thick: the clamp's bounds cross, lo = 8.5 > hi = 8


def test_thin_boxes_on_the_twin():
    g = grid_of("terraces")
    thin, two = twin.erode(g, *THIN, 7, OFF2), twin.erode(g, *TWO, 7, OFF2)
    assert (thin.info["n_active"], thin.info["n_rewritten"], thin.info["n_clamped"]) == (0, 0, 0) and np.array_equal(bits(thin.grid), bits(g))
    assert all((getattr(thin, m) == 0).all() for m in ("before", "after", "water", "sediment", "active"))
    assert two.info["n_active"] >= 100 and two.info["n_clamped"] == two.info["n_active"] and two.info["n_rewritten"] > 0
    assert set(np.unique(two.after[two.active > 0]).tolist()) <= {8.0, 8.5}


@pytest.mark.gpu
def test_gpu_boxes_one_and_two_samples_thick(craft_ex):
    ex, g = craft_ex, grid_of("terraces")
    ex.terrain_write_samples(g)
    ex.terrain_set_history(HISTORY)
    try:
        for box in (THIN, TWO):
            steps = ex.terrain_history()[0]
            before, want = es.erode_and_compare(ex, *box, 7, OFF2, es.CRAFT_DIMS)
            assert ex.terrain_history()[:2] == (steps + 1, 0)
            if box is THIN:
                info = ex.erosion_info()
                assert (info["n_active"], info["n_rewritten"], info["n_clamped"]) == (0, 0, 0) and len(ex.terrain_dirty_blocks()) > 0
                assert np.array_equal(bits(ex.terrain_read_samples()), bits(before))
            after = ex.terrain_read_samples()
            ex.terrain_undo()
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(before)) and ex.terrain_history()[:2] == (steps, 1)
            ex.terrain_redo()
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(after)) and ex.terrain_history()[:2] == (steps + 1, 0)
    finally:
        ex.terrain_set_history(0)


SMALL, LARGE = ((5, 0, 5), (20, 25, 12)), CRAFT_WHOLE      # 16 x 8 columns, and the whole plane of 74 x 50


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["small_then_large", "large_then_small"])
def test_gpu_two_erosions_in_one_queue(order):
    """A fresh context, so that the state buffer is as the first erosion of the queue left it: the second either needs a larger one
    (which waits for the first and reallocates in the middle of the queue) or lays a smaller plane out in the same one."""
    first, second = (SMALL, LARGE) if order == "small_then_large" else (LARGE, SMALL)
    start = grid_of("l_wall")
    middle = twin.erode(start, *first, 9, OFF2)
    want = twin.erode(middle.grid, *second, 6, OFF)
    assert middle.info["n_rewritten"] > 0 and want.info["n_rewritten"] > 0
    nb = tuple(d // 8 for d in es.CRAFT_DIMS)
    with es.World(HISTORY, es.CRAFT_DIMS, start) as ex:
        n_dirty, _ = ex.terrain_update([es.erosion(*first, 9, OFF2), es.erosion(*second, 6, OFF)])
        es.same_maps(ex, want)
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(want.grid))
        dirty = block_list(dirty_ids(*first, nb) | dirty_ids(*second, nb), nb)
        assert np.array_equal(ex.terrain_dirty_blocks(), dirty) and n_dirty == len(dirty) and ex.terrain_history()[:2] == (1, 0)
        ex.terrain_undo()
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(start)) and ex.terrain_history()[:2] == (0, 1)
        ex.terrain_redo()
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(want.grid)) and ex.terrain_history()[:2] == (1, 0)
        es.same_maps(ex, want)      # a redo simulates nothing and keeps the snapshot
        # one of each again, in calls of their own: the buffer both have used gives the same bytes as the twin
        es.erode_and_compare(ex, *first, 9, OFF2, es.CRAFT_DIMS)
        es.erode_and_compare(ex, *second, 6, OFF, es.CRAFT_DIMS)
