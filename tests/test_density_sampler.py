"""The density sampler (volumetricterrain_amd/csrc/density.hip) off its power-of-two parameters, against the float64 twin of
density_twin.py: frequencies, lacunarities and gains that are not dyadic, cells that jump, move backwards or stand still, origins that are
negative, straddle zero, sit near +-2^20 and beyond 2^24, every octave count, the per-sample kernel of 9-16 octaves in both memory orders,
the sign words of fill_keeps_signs against the sample-reading classify and the oracle, and pipelined fills.  Every sample of every volume
is compared; the x-fastest, z-fastest and padded fill of the same points must agree bit for bit.

THE BAR is k * A, A = sum_o |gain|^o + the ramp's largest magnitude (density_twin.amplitude), one k for all cases:
test_fp32_twin_agrees_with_the_float64_twin measures, on the CPU and over the very inputs the GPU tests use, how far the FP32 CPU twin
(oracle/density_ref.c: the definition's own operation order, one rounding per operation) lies from the float64 twin in units of A.  The GPU
sampler reorders the lerps (lane axes first, walk axis last) and contracts to fma, which may cost a few ulp more, not an order of magnitude."""
import collections
import ctypes
import functools

import numpy as np
import pytest

import density_twin
from density_twin import Params
from volumetricterrain_amd._lib import DensityParams

gpu = pytest.mark.gpu

# The largest |vto_density_fill - float64 twin| / A over every case of this file (the test below prints the figure per family and fails
# when one exceeds this constant): 1.099e-6 measured (the random sweep's seed 4: two octaves and a ramp; the families lie between 1.2e-7
# and 7.1e-7), rounded up.
CPU_FP32_DEVIATION = 1.1e-6
MARGIN = 4.0                     # operation order and fma contraction of the GPU sampler: a few ulp, not an order of magnitude
K = MARGIN * CPU_FP32_DEVIATION  # 4.4e-6: the GPU's bar is K * A
BENIGN_BAR = 2e-6                # what test_gpu_parity.py asks of the benchmark parameters: kept where K * A is looser

SENTINEL = 12345.0
GUARD = 37

Case = collections.namedtuple("Case", "family tag prm orgs dims")


def case_id(c):
    p = c.prm
    return "%s-%s-f%.4g-L%.4g-g%.4g-o%d-r%.4g@%.4g-s%d-%dx%dx%d-org%s" % (
        (c.family, c.tag, p.frequency, p.lacunarity, p.gain, p.octaves, p.ramp_scale, p.ramp_center, p.seed) + tuple(c.dims)
        + ("_".join(",".join(str(v) for v in o) for o in c.orgs),))


# planes of 255, 256, 257 and 600 points; walks of 1, 2, 3, 17, 63, 64, 65, 66, 160, 161 and 330 steps (the 64-step ballot chunk, kColSeg = 160, two and
# three equal segments; z-fastest: flushes that are no multiple of 4, 8 or 16 steps)
SHAPES = [(17, 15, 63), (16, 16, 64), (257, 1, 65), (24, 25, 160), (5, 7, 161), (9, 4, 330), (3, 5, 1), (6, 2, 2), (2, 3, 3), (13, 20, 66)]
ORGS = ((7, 100, 3), (512, -40, 77))
NONDYADIC = [(0.0137, 2.17, 0.7), (0.1, 1.9, 0.3), (1.0 / 3.0, 3.0, 1.0), (0.73, 0.5, 0.7)]


def _families():
    out = []

    def add(family, tag, f, lac, gain, dims, octaves=8, orgs=ORGS, rs=0.0, rc=0.0, seed=1337):
        out.append(Case(family, str(tag), Params(seed, f, octaves, lac, gain, rs, rc), tuple(tuple(o) for o in orgs), tuple(dims)))

    for i, (f, lac, g) in enumerate(NONDYADIC):
        for s in range(3):
            add("nondyadic", 3 * i + s, f, lac, g, SHAPES[(3 * i + s) % len(SHAPES)], seed=1337 + i)
    # more than one cell per step at octave 0: every octave jumps at every step, at fractions that are not 0
    for i, (f, lac) in enumerate([(1.37, 2.17), (2.6, 1.9)]):
        for s, dims in enumerate([(16, 16, 64), (5, 7, 161), (9, 4, 330)]):
            add("fast", 3 * i + s, f, lac, 0.7, dims)
    # octaves 0-2 step one cell every few steps (0.1, 0.217, 0.47 cells a step), octave 3 mixes, octaves 4-7 jump: one walk holds all three kinds of step
    for s, dims in enumerate([(5, 7, 161), (9, 4, 330), (16, 16, 64), (24, 25, 160)]):
        add("mixed", s, 0.1, 2.17, 0.7, dims)
    # the cell decreases along the walk; a negative lacunarity alternates the direction per octave
    for s, (f, lac, dims) in enumerate([(-0.0137, 2.17, (9, 4, 330)), (-1.37, 1.9, (17, 15, 63)), (0.1, -1.9, (5, 7, 161)), (-0.3, -2.17, (13, 20, 66))]):
        add("negative", s, f, lac, 0.7, dims)
    for s, (f, g, rs) in enumerate([(0.0, 0.7, 0.0), (0.0137, 0.0, 0.0), (0.0, 0.0, 0.0371), (-0.0, 0.7, 0.0)]):
        add("zero", s, f, 2.17, g, [(5, 7, 161), (17, 15, 63), (13, 20, 66), (16, 16, 64)][s], rs=rs, rc=103.3)
    for o in range(1, 9):   # 17 steps, at most 4 octaves: the 16-step flush of the z-fastest order and its 1-step rest
        for s, dims in enumerate([(5, 7, 161)] + ([(20, 13, 17)] if o <= 4 else [])):
            add("octaves", "%d.%d" % (o, s), 0.3, 2.17, 0.7, dims, octaves=o)
    far = 2 ** 20
    for s, (orgs, (f, lac, g), dims) in enumerate([
            (((-5000, -300, -77), (-9, -20000, -4)), NONDYADIC[0], (13, 20, 66)),
            (((-5000, -300, -77), (-9, -20000, -4)), NONDYADIC[2], (5, 7, 161)),
            (((-3, -2, -5), (-8, -7, -30)), NONDYADIC[0], (13, 20, 66)),        # zero inside the volume on every axis
            (((-3, -2, -5), (-8, -7, -150)), NONDYADIC[1], (9, 4, 330)),
            (((far - 6, -far - 4, far - 30), (-far - 10, far - 10, -far - 1)), (0.0137, 1.9, 0.7), (13, 20, 66)),
            (((far - 2, -far - 3, far - 100), (-far - 2, far - 3, -far - 80)), (0.73, 2.17, 0.7), (5, 7, 161))]):
        add("origins", s, f, lac, g, dims, orgs=orgs)
    # sample indices beyond 2^24, where (float)(index) skips integers: the walk's "previous cell" must be the previous sample's own
    big = 2 ** 25
    for s, (orgs, dims) in enumerate([(((big + 3, -big // 2 - 11, big + 1), (-big - 7, 5, -big // 2 - 300)), (5, 7, 161)),
                                      (((3, 4, big // 2 - 100), (-5, 6, -big - 160)), (9, 4, 330))]):
        add("beyond24", s, 0.13, 1.7, 0.7, dims, octaves=4, orgs=orgs)
    for s, (rs, rc, dims) in enumerate([(0.0371, 103.3, (13, 20, 66)), (-0.0371, 112.0, (13, 20, 66)), (0.73, 100.9, (5, 7, 161))]):
        add("ramp", s, 0.0137, 2.17, 0.7, dims, orgs=((7, 100, 3), (-40, 100, 77)), rs=rs, rc=rc)
    # the benchmark parameters at n = 64 (power-of-two everything): these keep 2e-6 where K * A is looser
    add("benign", "fbm8", 4.0 / 64, 2.0, 0.5, (16, 16, 64), rs=2.0 / 64, rc=32.0, orgs=((0, 0, 0), (30, 28, 5)))
    add("benign", "perlin3d", 8.0 / 64, 2.0, 0.5, (16, 16, 64), octaves=1, orgs=((0, 0, 0), (30, 28, 5)))
    return out


FAMILIES = _families()

# the per-sample kernel (more than 8 octaves): both memory orders, compact and padded, a fast axis of 257 and 600 samples (two and three
# 256-sample workgroups a row), and a square volume whose two orders share their points
GENERIC_PRM = {9: (0.0137, 2.17, 0.7), 12: (0.1, 1.9, 0.5), 16: (1.0 / 3.0, 1.7, 0.9)}
GENERIC = [(Case("generic", "%d.%d" % (o, s), Params(99 + o, GENERIC_PRM[o][0], o, GENERIC_PRM[o][1], GENERIC_PRM[o][2], 0.0371, 3.3),
                 ((-7, 2, 3), (512, -3, -260)), dims), layouts)
           for o in (9, 12, 16)
           for s, (dims, layouts) in enumerate([((257, 3, 5), ("x", "p")), ((5, 3, 257), ("z", "zp")), ((600, 2, 3), ("x", "p")),
                                                ((3, 2, 600), ("z", "zp")), ((40, 3, 40), ("x", "z", "zp"))])]

N_RANDOM = 24
WALKS = [1, 2, 3, 5, 17, 63, 64, 65, 100, 161, 200, 330]


def draw(seed):
    """A random case and its layout: parameters, origins, octave count, dims, number of volumes."""
    rng = np.random.default_rng(7000 + seed)
    octaves = int(rng.integers(1, 9))
    f = float(np.exp(rng.uniform(np.log(0.005), np.log(3.0)))) * (-1.0 if rng.random() < 0.2 else 1.0)
    lac = float(rng.uniform(0.5, 3.0))
    gain = float(rng.uniform(0.2, 1.0))
    dz = int(rng.choice(WALKS))
    dx = int(rng.integers(1, 41))
    dy = int(rng.integers(1, max(2, min(40, 600 // dx) + 1)))
    nv = int(rng.integers(1, 4))
    scale = int(rng.choice([10, 5000, 2 ** 20]))
    orgs = rng.integers(-scale, scale + 1, size=(nv, 3))
    rs, rc = 0.0, 0.0
    if rng.random() < 0.5:
        orgs[:, 1] = orgs[0, 1]   # one ramp centre inside every volume
        rs, rc = float(rng.uniform(-0.05, 0.05)), float(orgs[0, 1] + rng.uniform(0, dy))
    prm = Params(int(rng.integers(0, 2 ** 32)), f, octaves, lac, gain, rs, rc)
    while density_twin.chain_peak(prm, orgs, (dx, dy, dz)) >= 2 ** 30:   # keep the FP32 chain clear of 2^31
        orgs = orgs // 16
        if rs:
            prm = prm._replace(ramp_center=float(orgs[0, 1]) + 0.5 * dy)
    layout = str(rng.choice(["x", "z", "p", "zp"]))
    return Case("random", seed, prm, tuple(tuple(int(v) for v in o) for o in orgs), (dx, dy, dz)), layout


RANDOM = [draw(s) for s in range(N_RANDOM)]

# the sign words: (40, 16, 72) cells, a walk of 74 steps (more than one 64-step chunk of sign words), a plane of 756 points
SIGN_DIMS = (42, 18, 74)


def _sign_cases():
    out = []

    def add(tag, f, lac, gain, octaves=8, orgs=((7, 100, 3), (-40, 100, -50)), rs=0.0, rc=0.0):
        out.append(Case("signs", tag, Params(4242, f, octaves, lac, gain, rs, rc), orgs, SIGN_DIMS))

    add("nondyadic", 0.0137, 2.17, 0.7, rs=0.0371, rc=108.6)
    add("fast", 1.37, 2.17, 0.7)
    add("mixed", 0.1, 2.17, 0.7, rs=-0.01, rc=109.2)
    add("negative", -0.3, 1.9, 0.5, orgs=((-5000, -300, -77), (-30, -310, -4)))
    add("far", 0.0137, 1.9, 0.7, orgs=((2 ** 20 - 6, -2 ** 20 - 4, 2 ** 20 - 30),))
    # exact zeros: an integer frequency is +-0 everywhere (no surface at all); with a ramp whose centre is a sample plane that plane is +-0,
    # on either side of a ramp of either sign; half-integer coordinates leave the even samples +-0
    add("allzero", 1.0, 2.0, 0.5)
    add("zeroplane+", 1.0, 2.0, 0.5, rs=0.0371, rc=109.0)
    add("zeroplane-", 1.0, 2.0, 0.5, rs=-0.0371, rc=109.0)
    add("halfzero", 0.5, 2.0, 0.5, octaves=3)
    add("halfzero-ramp", 0.5, 2.0, 0.5, octaves=3, rs=0.0371, rc=109.0)
    return out


SIGNS = _sign_cases()

# just inside the documented limit: 0.73 * 3^7 = 1596.5 lattice cells per sample at octave 7, the chain's peak within 0.1 % of 2^31
LIMIT_CASE = Case("limit", "inside", Params(7, 0.73, 8, 3.0, 0.7, 0.0, 0.0), ((1345000, -1345000, 1344990),), (8, 4, 6))

ALL_CASES = FAMILIES + [c for c, _ in GENERIC] + [c for c, _ in RANDOM] + SIGNS + [LIMIT_CASE]
FAMILY_NAMES = sorted({c.family for c in ALL_CASES})


@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 twin [n_volumes, dz, dy, dx], A): computed once per case, read-only."""
    perm = density_twin.permutation(case.prm.seed)
    ref = np.stack([density_twin.density(case.prm, o, case.dims, perm) for o in case.orgs])
    ref.setflags(write=False)
    return ref, density_twin.amplitude(case.prm, case.orgs, case.dims)


def bar(case):
    a = reference(case)[1]
    return min(K * a, BENIGN_BAR) if case.family == "benign" else K * a


# ---- on the CPU: the twin itself ----------------------------------------------------------------------------------------------------

def test_permutation_restated(oracle_mod):
    for seed in (0, 1, 1337, 4242, 2 ** 32 - 1, 2 ** 64 - 1):
        assert np.array_equal(density_twin.permutation(seed), oracle_mod.permutation(seed))


def test_gradient_table_is_perlins():
    """GRAD[h] . (x, y, z) is Perlin's grad(h, x, y, z): twelve edge directions, four of them twice."""
    assert sorted(np.abs(density_twin.GRAD).sum(axis=1)) == [2.0] * 16
    assert len({tuple(g) for g in density_twin.GRAD}) == 12


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_fp32_twin_agrees_with_the_float64_twin(oracle_mod, family):
    """vto_density_fill (FP32, the definition's operation order) against the float64 twin on every case of this file: the figure K is
    derived from.  Also: the FP32 coordinate chain of every case stays below 2^31, where (int)floorf ends."""
    worst = 0.0
    for case in (c for c in ALL_CASES if c.family == family):
        assert density_twin.chain_peak(case.prm, case.orgs, case.dims) < 2 ** 31, case_id(case)
        ref, a = reference(case)
        oprm = oracle_mod.DensityParams(*case.prm)
        dx, dy, dz = case.dims
        for v, o in enumerate(case.orgs):
            got = np.empty((dz, dy, dx), np.float32)
            oracle_mod.lib().vto_density_fill(ctypes.byref(oprm), o[0], o[1], o[2], dx, dy, dz, 1, dx, dx * dy, oracle_mod._p(got))
            dev = float(np.abs(got.astype(np.float64) - ref[v]).max()) / a
            worst = max(worst, dev)
            assert dev <= CPU_FP32_DEVIATION, (case_id(case), v, dev)
    print("\nFP32 twin against the float64 twin, family %s: largest deviation %.3g A" % (family, worst))


def test_twin_known_values():
    """Perlin noise is 0 at lattice points and the ramp is exact there; a one-octave field is bounded by 1."""
    prm = Params(5, 1.0, 3, 2.0, 0.5, 0.25, 2.0)
    d = density_twin.density(prm, (-4, -1, 7), (6, 5, 4))
    assert np.array_equal(d, np.broadcast_to((-(np.arange(-1, 4) - 2.0) * 0.25)[None, :, None], d.shape))
    d = density_twin.density(Params(5, 0.37, 1, 2.0, 0.5, 0.0, 0.0), (-40, -10, 7), (50, 40, 30))
    assert 0.5 < np.abs(d).max() <= 1.0


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ex():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import volumetricterrain_amd as vt
    e = vt.Extractor(0)
    yield e
    e.close()


def layout_strides(dims, layout):
    """(element strides, elements a volume spans) of a memory order: x fastest, z fastest (a C# float[,,]), and both with padded rows and slabs."""
    dx, dy, dz = dims
    if layout == "x":
        return (1, dx, dx * dy), dx * dy * dz
    if layout == "z":
        return (dy * dz, dz, 1), dx * dy * dz
    if layout == "p":
        return (1, dx + 3, (dx + 3) * (dy + 5)), (dx + 3) * (dy + 5) * dz
    if layout == "zp":
        return ((dz + 3) * (dy + 2), dz + 3, 1), (dz + 3) * (dy + 2) * dx
    raise ValueError(layout)


def gpu_fill(ex, case, layout):
    """The fill of a case in one memory order as float32 [n_volumes, dz, dy, dx]; every element the volumes do not own -- row and slab
    padding, a guard band behind every volume -- must keep its sentinel."""
    import torch
    import volumetricterrain_amd as vt
    dx, dy, dz = case.dims
    strides, span = layout_strides(case.dims, layout)
    nv, vs = len(case.orgs), span + GUARD
    d = torch.full((nv * vs,), SENTINEL, dtype=torch.float32, device="cuda")
    ex.density_fill_device(DensityParams(*case.prm), case.orgs, case.dims, strides, vs, d.data_ptr())
    host = d.cpu().numpy().reshape(nv, vs)
    idx = (np.arange(dz)[:, None, None] * strides[2] + np.arange(dy)[None, :, None] * strides[1] + np.arange(dx)[None, None, :] * strides[0])
    untouched = np.ones(vs, bool)
    untouched[idx.ravel()] = False
    assert (host[:, untouched] == SENTINEL).all(), "the sampler wrote outside its volumes (%s, layout %s)" % (case_id(case), layout)
    return host[:, idx]


def check_against_twin(case, got, what):
    ref, a = reference(case)
    limit = bar(case)
    dev = np.abs(got.astype(np.float64) - ref).reshape(len(case.orgs), -1).max(axis=1)
    print("\nGPU %s %s %s: %.3f of the bar (%.3g A)" % (case.family, case.tag, what, dev.max() / limit if limit else 0.0, dev.max() / a))
    assert (dev <= limit).all(), (case_id(case), what, dev.tolist(), limit)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("case", FAMILIES, ids=case_id)
def test_sampler_families_against_the_float64_twin(ex, case):
    """Every family in three memory orders (z-fastest also padded): the same bits in all of them, and the x-fastest fill within K * A of
    the twin, every sample of every volume."""
    got = gpu_fill(ex, case, "x")
    check_against_twin(case, got, "x")
    for layout in ("z", "p", "zp"):
        assert same_bits(gpu_fill(ex, case, layout), got), "x-fastest and %r fills differ in their bits: %s" % (layout, case_id(case))


@gpu
@pytest.mark.parametrize("case,layout", RANDOM, ids=lambda v: case_id(v) if isinstance(v, Case) else v)
def test_sampler_random_sweep(ex, case, layout):
    check_against_twin(case, gpu_fill(ex, case, layout), layout)


@gpu
@pytest.mark.parametrize("case,layouts", GENERIC, ids=lambda v: case_id(v) if isinstance(v, Case) else "+".join(v))
def test_per_sample_kernel_against_the_float64_twin(ex, case, layouts):
    """9, 12 and 16 octaves: density_generic_kernel in both memory orders, one to three workgroups along the fast axis, padded strides,
    two volumes.  It is one function of position too: the orders agree in their bits."""
    fills = [gpu_fill(ex, case, layout) for layout in layouts]
    for layout, got in zip(layouts, fills):
        check_against_twin(case, got, layout)
        assert same_bits(got, fills[0]), (layouts[0], layout, case_id(case))


@gpu
@pytest.mark.parametrize("case", SIGNS, ids=case_id)
def test_sign_words_classify_like_the_samples_and_the_oracle(oracle_mod, case):
    """fill_keeps_signs: the extract that classifies from the sampler's sign words and the one that reads the samples leave the same block
    offsets, per-volume counts and output bytes, and those offsets are what the oracle counts on the downloaded field -- on general
    parameters and on fields full of exact zeros of either sign, where `value > 0` must fall the same way in all three.  The field itself
    is compared with the twin as everywhere."""
    import torch
    import volumetricterrain_amd as vt
    dx, dy, dz = case.dims
    n = (dx - 2, dy - 2, dz - 2)
    nv, sv = len(case.orgs), dx * dy * dz
    bpv = (n[0] // 8) * (n[1] // 8) * (n[2] // 8)
    prm = DensityParams(*case.prm)
    d = torch.full((nv * sv,), SENTINEL, dtype=torch.float32, device="cuda")
    with vt.Extractor(0) as e2:
        outs = []
        for keep in (0, 1):
            e2.set_tuning(fill_keeps_signs=keep)
            e2.density_fill_device(prm, case.orgs, case.dims, (1, dx, dx * dy), sv, d.data_ptr())
            T = e2.extract_volumes_device(d.data_ptr(), n, (1, dx, dx * dy), nv, sv)
            if keep:
                assert e2.last_stage_ms()["classify"] > 0
            _, off_ptr, vc_ptr = e2.device_results()
            outs.append((T, e2.copy_u32(off_ptr, nv * bpv + 1).copy(), e2.copy_u32(vc_ptr, 2 * nv).copy(), e2.read_triangles()[0].tobytes()))
    assert outs[0][0] == outs[1][0], case_id(case)
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3], case_id(case)
    host = d.cpu().numpy().reshape(nv, dz, dy, dx)
    check_against_twin(case, host, "x")
    ref = reference(case)[0]
    print("exact zeros: twin %d, GPU +0 %d, GPU -0 %d; T = %d" % ((ref == 0).sum(), ((host == 0) & ~np.signbit(host)).sum(),
                                                                 ((host == 0) & np.signbit(host)).sum(), outs[1][0]))
    assert ((host == 0) | (ref != 0)).all(), "a sample the definition makes exactly 0 (a lattice point on the ramp's centre plane) is not"
    want = [0]
    for v in range(nv):
        _, offs, _ = oracle_mod.extract_grid(np.ascontiguousarray(host[v].transpose(2, 1, 0)), threads=4, count_only=True)
        want.extend((np.asarray(offs[1:], np.int64) + want[-1]).tolist())
    assert np.array_equal(outs[1][1].astype(np.int64), np.asarray(want, np.int64)), case_id(case)


@gpu
@pytest.mark.parametrize("own_queue", [False, True], ids=["torch-stream", "own-queue-stream"])
def test_pipelined_fills_equal_their_blocking_fills(ex, own_queue):
    """Two vtmc_density_fill_device_async calls back to back on one stream that is not the default one, other origins, another seed, other
    buffers, no host wait in between: each buffer holds what its own blocking fill gives, bit for bit (the staged origins, the
    permutation's re-upload and the shared rows buffer are all stream-ordered)."""
    import torch
    import volumetricterrain_amd as vt
    dims, strides = (24, 25, 160), (1, 24, 24 * 25)
    vs = 24 * 25 * 160 + GUARD
    jobs = [(DensityParams(11, 0.0137, 8, 2.17, 0.7, 0.0371, 103.3), [(7, 100, 3), (512, -40, 77)]),
            (DensityParams(12, 0.31, 5, 1.9, 0.5, 0.0, 0.0), [(-5000, -300, -77), (-9, -20000, -4)])]
    side = torch.cuda.Stream() if not own_queue else None
    stream = ex.stream_handle(own_queue=True) if own_queue else side.cuda_stream
    bufs = [torch.full((2 * vs,), SENTINEL, dtype=torch.float32, device="cuda") for _ in jobs]
    torch.cuda.synchronize()
    for (prm, orgs), d in zip(jobs, bufs):
        ex.density_fill_device(prm, orgs, dims, strides, vs, d.data_ptr(), stream=stream, wait=False)
    torch.cuda.synchronize()
    got = [d.cpu().numpy() for d in bufs]
    for (prm, orgs), g in zip(jobs, got):
        d = torch.full((2 * vs,), SENTINEL, dtype=torch.float32, device="cuda")
        ex.density_fill_device(prm, orgs, dims, strides, vs, d.data_ptr())
        want = d.cpu().numpy()
        assert (want.reshape(2, vs)[:, :-GUARD] != SENTINEL).all() and (want.reshape(2, vs)[:, -GUARD:] == SENTINEL).all()
        assert same_bits(g, want)
    assert not same_bits(got[0], got[1])


@gpu
def test_lattice_coordinates_past_the_int_range_are_refused(ex):
    """include/vtmc.h: the chain's reach, |origin + index| * |f| * max(1, |L|)^(octaves - 1), must stay below 2^31; beyond it the fill
    answers VTMC_ERR_INVALID_ARG and writes nothing.  Just inside the limit it fills; the context stays usable."""
    import torch
    import volumetricterrain_amd as vt
    dims, strides = LIMIT_CASE.dims, (1, 8, 32)
    d = torch.full((8 * 4 * 6,), SENTINEL, dtype=torch.float32, device="cuda")

    def refused(prm, org):
        with pytest.raises(vt.VtmcError) as e:
            ex.density_fill_device(prm, [org], dims, strides, 0, d.data_ptr())
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == SENTINEL).all()

    inside = LIMIT_CASE
    prm = DensityParams(*inside.prm)
    assert 2 ** 31 * 0.999 < density_twin.chain_peak(inside.prm, inside.orgs, dims) < 2 ** 31
    refused(prm, (1345200, 0, 0))
    refused(prm, (0, -1345200, 0))
    refused(prm, (0, 0, 1345200))
    refused(prm, (0, 0, 2 ** 31 - 3))                            # origin + dim - 1 leaves int32
    refused(DensityParams(7, float("nan"), 8, 2.0, 0.5, 0.0, 0.0), (0, 0, 0))
    refused(DensityParams(7, 1e-3, 8, float("inf"), 0.5, 0.0, 0.0), (1, 1, 1))
    refused(DensityParams(7, 0.5, 16, 4.5, 0.5, 0.0, 0.0), (3, 3, 3))   # 0.5 * 4.5^15 * 8 cells
    check_against_twin(inside, gpu_fill(ex, inside, "x"), "x")
