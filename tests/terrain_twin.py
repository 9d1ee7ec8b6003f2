"""The one twin of the device-resident terrain: what test_terrain.py, test_terrain_history.py, test_terrain_brushes.py,
test_terrain_noise.py and test_terrain_io.py compare the device against, bit for bit.

A modifier is a spec ("kind", args).  Kinds 0-3 (plane, sphere, cylinder, island) run on the CPU restatement oracle.Terrain
(oracle/terrain_ref.c).  The kinds the oracle lacks run in numpy on its memory, one event number each: the sculpt brushes
(VTMC_MOD_SMOOTH / VTMC_MOD_FLATTEN) and the noise modifier (VTMC_MOD_NOISE: fBm, billow, ridged multifractal), each a FP32 restatement
of include/vtmc.h's rule in its order of operations (numpy's float32 + - * / sqrt floor abs are correctly rounded and never fused, as
the library's are under -ffp-contract=off), with the clamp draws of kinds 0-3 and 8 (terrainfile.terrain_uniform / clamp_drawn).
test_terrain_noise.py checks the noise yardstick on the CPU against the committed oracle, not against the code under test.

Grids are compared as uint32, every sample (NaN payloads, -0); triangles as in test_terrain.py: offsets and `block` exact, floats
within 1e-5.  Each test file keeps its own world (dims, seed, queue) and hands it in."""
import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
from volumetricterrain_amd.terrainfile import terrain_uniform

f32, u64 = np.float32, np.uint64


# -- modifier specs -----------------------------------------------------------------------------------------------------------------------
def gpu_mod(spec):
    """The device's modifier of any spec; a noise spec carries NoiseModifier's keyword arguments."""
    kind, args = spec[0], spec[1]
    if kind == "noise":
        return vt.NoiseModifier(**args)
    return {"plane": vt.PlaneModifier, "sphere": vt.SphereModifier, "cylinder": vt.CylinderModifier, "island": vt.IslandModifier,
            "smooth": vt.SmoothModifier, "flatten": vt.FlattenModifier}[kind](*args)


def with_box(m, spec, keep=None):
    """A spec may carry a third entry (lower, upper): the AABB the struct m gets in place of its modifier's own, set after to_struct()
    (session_twin.py: boxes of exact sample extents).  keep: what the struct borrows memory from (a heightmap) and must outlive."""
    if len(spec) > 2:
        m.lower[:], m.upper[:] = (tuple(float(f32(v)) for v in b) for b in spec[2])
    if keep is not None:
        m._keep = keep
    return m


def gpu_struct(spec, mod_of=gpu_mod):
    """The vtmc_modifier of a spec, its AABB overridden where the spec says so: what the device is handed and the numpy kinds read."""
    mod = mod_of(spec)
    return with_box(mod.to_struct(), spec, mod)


def oracle_mod_of(oracle_mod, spec):
    """The reference's kinds only, through the oracle's own (independent) bound formulas (an overridden AABB apart)."""
    kind, args = spec[0], spec[1]
    return with_box({"plane": oracle_mod.plane_modifier, "sphere": oracle_mod.sphere_modifier,
                     "cylinder": oracle_mod.cylinder_modifier, "island": oracle_mod.heightmap_modifier}[kind](*args), spec)


def island_heightmap(res=(48, 40), height=14.0):
    """A smooth synthetic island, its hill `height` high: what Island.GetElevation would have filled in (IslandModifier.cs:85-91)."""
    u = np.linspace(-1, 1, res[0], dtype=np.float32)[:, None]
    v = np.linspace(-1, 1, res[1], dtype=np.float32)[None, :]
    k = height / 14.0
    return (k * 14.0 * np.exp(-2.5 * (u * u + v * v)) + k * 1.5 * np.sin(5 * u) * np.cos(4 * v) + k * 3.0).astype(np.float32)


# -- index arithmetic (terrain.hip) ---------------------------------------------------------------------------------------------------------
def saturating_int(v):
    return -2 ** 31 if v <= -2147483648.0 else (2 ** 31 - 1 if v >= 2147483648.0 else int(v))


def sample_range(m, dims_s, scale, origin):
    """terrain.hip's sample_range: ([low], [up]) clamped as the dirty rule reads them, and the box (first sample, extent)."""
    low, up, first, ext = [], [], [], []
    for k in range(3):
        top = dims_s[k] - 1
        lo = max(saturating_int(np.floor((f32(m.lower[k]) - f32(origin[k])) / f32(scale))), 0)
        hi = min(saturating_int(np.ceil((f32(m.upper[k]) - f32(origin[k])) / f32(scale))), top)
        e = hi - lo + 1
        low.append(lo)
        up.append(hi)
        first.append(lo)
        ext.append(0 if e <= 0 or lo > top else min(e, top - lo + 1))
    return low, up, first, ext


def dirty_ids(low, up, nb):
    """mark_dirty_blocks: up >= 8b && low <= 8b + 8 on every axis."""
    r = []
    for k in range(3):
        lo, hi = low[k] - 8, up[k]
        f = 0 if lo <= 0 else (lo + 7) // 8
        last = min(-1 if hi < 0 else hi // 8, nb[k] - 1)
        if f > last:
            return set()
        r.append(range(f, last + 1))
    return {bx + nb[0] * (by + nb[1] * bz) for bz in r[2] for by in r[1] for bx in r[0]}


def block_list(ids, nb):
    """Block ids as the dirty list the library returns: (n, 3) int32 (bx, by, bz), ordered by id."""
    ids = np.array(sorted(ids), np.int64)
    return np.stack([ids % nb[0], (ids // nb[0]) % nb[1], ids // (nb[0] * nb[1])], axis=1).astype(np.int32).reshape(-1, 3)


def image_bytes(ext):
    """terrain.hip's image_bytes: what the edit journal keeps of a box, rounded up to 256 bytes."""
    n = ext[0] * ext[1] * ext[2]
    return 0 if min(ext) <= 0 else (4 * n + 255) // 256 * 256


def box_of(ref, m):
    """Modifier struct m on the twin ref: the box it writes (first sample, extent) and the block ids its AABB dirties."""
    low, up, first, ext = sample_range(m, tuple(d + 2 for d in ref.dims), ref.scale, ref.origin)
    return first, ext, dirty_ids(low, up, tuple(d // 8 for d in ref.dims))


def step_bytes(ref, specs):
    """What the journal keeps of one update: the boxes' images, no halo."""
    return sum(image_bytes(box_of(ref, gpu_struct(s))[1]) for s in specs)


# -- the write rule of kinds 0-3 and 8 ------------------------------------------------------------------------------------------------------
def clamp_drawn(v, seed, event, sample, k):
    """Mathf.Clamp(v, void, full), void = draw k - 2, full = draw k + 1 + 1.  Returns (values, clamped low, clamped high)."""
    lo = terrain_uniform(seed, event, sample, k) - f32(2)
    hi = terrain_uniform(seed, event, sample, k + 1) + f32(1)
    low, high = (v < -1) & (v < lo), ~(v < -1) & (v > 1) & (v > hi)
    return np.where(low, lo, np.where(high, hi, v)), low, high


def csg_write(ref, first, ext, q, add):
    """The write of kinds 0-3 and 8 on the twin's memory: q the density of the box [z, y, x]; takes the next event number.  Reads and
    writes only the box slice of ref._mem.  Returns how many samples of q took the low and the high clamp branch."""
    (lx, ly, lz), (dx, dy, dz) = first, ext
    event = ref.events + 1
    taken = (0, 0)
    if min(ext) > 0:
        Dx, Dy = ref.dims[0] + 2, ref.dims[1] + 2
        zz, yy, xx = np.meshgrid(np.arange(lz, lz + dz, dtype=u64), np.arange(ly, ly + dy, dtype=u64), np.arange(lx, lx + dx, dtype=u64),
                                 indexing="ij")
        sample = xx + u64(Dx) * (yy + u64(Dy) * zz)
        md, low, high = clamp_drawn(q, ref.seed, event, sample, 0)
        taken = (int(low.sum()), int(high.sum()))
        S = ref._mem[lz:lz + dz, ly:ly + dy, lx:lx + dx]
        if add:
            r = np.where(S > md, S, md)
        else:
            r, _, _ = clamp_drawn(np.where(S < -md, S, -md), ref.seed, event, sample, 2)
        ref._mem[lz:lz + dz, ly:ly + dy, lx:lx + dx] = r.astype(f32)
    ref.events = event
    return taken


def positions(ref, first, ext):
    return [np.arange(first[k], first[k] + ext[k]).astype(f32) * f32(ref.scale) + f32(ref.origin[k]) for k in range(3)]


# -- the brushes (kinds 4, 5) -----------------------------------------------------------------------------------------------------------------
def brush_values(mem, m, first, ext, scale, origin):
    """New values of the box first..first+ext of mem ([z, y, x], the pre-brush samples) under brush struct m."""
    (lx, ly, lz), (dx, dy, dz) = first, ext
    Dz, Dy, Dx = mem.shape
    c0, c1, c2, r, s = (f32(v) for v in m.p[0:5])
    S = mem[lz:lz + dz, ly:ly + dy, lx:lx + dx]
    px = np.arange(lx, lx + dx).astype(f32) * f32(scale) + f32(origin[0])
    py = np.arange(ly, ly + dy).astype(f32) * f32(scale) + f32(origin[1])
    pz = np.arange(lz, lz + dz).astype(f32) * f32(scale) + f32(origin[2])
    ddx, ddy, ddz = px - c0, py - c1, pz - c2
    d = np.sqrt(((ddx * ddx)[None, None, :] + (ddy * ddy)[None, :, None]) + (ddz * ddz)[:, None, None])
    t = f32(1) - d / r
    t = t + t
    t = np.where(t < 0, f32(0), np.where(t > 1, f32(1), t))
    w = s * t
    if m.kind == _lib.MOD_SMOOTH:
        zi = np.clip(np.arange(lz - 1, lz + dz + 1), 0, Dz - 1)
        yi = np.clip(np.arange(ly - 1, ly + dy + 1), 0, Dy - 1)
        xi = np.clip(np.arange(lx - 1, lx + dx + 1), 0, Dx - 1)
        G = mem[np.ix_(zi, yi, xi)]
        R = (G[:, :, :-2] + G[:, :, 1:-1]) + G[:, :, 2:]
        P = (R[:, :-2] + R[:, 1:-1]) + R[:, 2:]
        T = ((P[:-2] + P[1:-1]) + P[2:]) / f32(27)
    else:
        n0, n1, n2 = (f32(v) for v in m.p[5:8])
        g = ((n0 * (c0 - px)[None, None, :] + n1 * (c1 - py)[None, :, None]) + n2 * (c2 - pz)[:, None, None]) / f32(scale)
        T = np.where(g < -1, f32(-1), np.where(g > 1, f32(1), g))
    out = S + (T - S) * w
    return np.where(w == 0, S, out).astype(f32)


def apply_brush(ref, m):
    """One brush on the twin's memory, one event number; returns the block ids it dirties."""
    first, ext, ids = box_of(ref, m)
    if min(ext) > 0:
        (lx, ly, lz), (dx, dy, dz) = first, ext
        ref._mem[lz:lz + dz, ly:ly + dy, lx:lx + dx] = brush_values(ref._mem, m, first, ext, ref.scale, ref.origin)
    ref.events += 1
    return ids


# -- the noise modifier (kind 8) --------------------------------------------------------------------------------------------------------------
def permutation(seed):
    """density_permutation: Fisher-Yates driven by SplitMix64(seed)."""
    M = (1 << 64) - 1
    perm, s = list(range(256)), seed & M
    for i in range(255, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        j = z % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, np.int64)


def fade(t):
    return t * t * t * (t * (t * f32(6) - f32(15)) + f32(10))


def mix(t, a, b):
    return a + t * (b - a)


def grad(h, x, y, z):
    h = h & 15
    u = np.where(h < 8, x, y)
    v = np.where(h < 4, y, np.where((h == 12) | (h == 14), x, z))
    return np.where((h & 1) == 0, u, -u) + np.where((h & 2) == 0, v, -v)


def noise3(perm, x, y, z):
    """Improved noise on float32 arrays of one shape; lattice coordinates stay far below 2^24 (the library rejects the rest)."""
    fx, fy, fz = np.floor(x), np.floor(y), np.floor(z)
    X, Y, Z = fx.astype(np.int64) & 255, fy.astype(np.int64) & 255, fz.astype(np.int64) & 255
    x, y, z = x - fx, y - fy, z - fz
    u, v, w = fade(x), fade(y), fade(z)
    P = lambda i: perm[i & 255]   # noqa: E731
    A = P(X) + Y
    AA, AB = P(A) + Z, P(A + 1) + Z
    B = P(X + 1) + Y
    BA, BB = P(B) + Z, P(B + 1) + Z
    one = f32(1)
    return mix(w,
               mix(v, mix(u, grad(P(AA), x, y, z), grad(P(BA), x - one, y, z)),
                   mix(u, grad(P(AB), x, y - one, z), grad(P(BB), x - one, y - one, z))),
               mix(v, mix(u, grad(P(AA + 1), x, y, z - one), grad(P(BA + 1), x - one, y, z - one)),
                   mix(u, grad(P(AB + 1), x, y - one, z - one), grad(P(BB + 1), x - one, y - one, z - one))))


def noise_density(perm, px, py, pz, octaves, basis, f, L, g, a=1.0, b=0.0, rs=0.0, rc=0.0, h=1.0):
    """q of include/vtmc.h at world positions px, py, pz (float32, broadcast to one [z, y, x] shape)."""
    f, L, g, a, b, rs, rc, h = (f32(v) for v in (f, L, g, a, b, rs, rc, h))
    px, py, pz = np.broadcast_arrays(px, py, pz)
    x, y, z = px * f, py * f, pz * f
    amp, total, w = f32(1), np.zeros(px.shape, f32), np.ones(px.shape, f32)
    for _ in range(octaves):
        n = noise3(perm, x, y, z)
        if basis == 0:
            total = total + amp * n
        elif basis == 1:
            t = np.abs(n)
            t = t + t
            t = t - f32(1)
            total = total + amp * t
        else:
            r = h - np.abs(n)
            r = r * r
            r = r * w
            w = r + r
            w = np.where(w < 0, f32(0), np.where(w > 1, f32(1), w))
            total = total + amp * r
        x, y, z = x * L, y * L, z * L
        amp = f32(amp * g)
    q = a * total
    q = q + b
    q = q - (py - rc) * rs
    assert q.dtype == f32
    return q


def apply_noise(ref, m):
    """One VTMC_MOD_NOISE struct on the twin's memory, one event number; returns the block ids it dirties and csg_write's clamp-branch
    counts."""
    first, ext, ids = box_of(ref, m)
    q = None
    if min(ext) > 0:
        px, py, pz = positions(ref, first, ext)
        perm = permutation(m.data_dims[0] & 0xFFFFFFFF)
        q = noise_density(perm, px[None, None, :], py[None, :, None], pz[:, None, None], m.data_dims[1] & 255, m.data_dims[1] >> 8, *m.p[0:8])
    return ids, csg_write(ref, first, ext, q, bool(m.add_or_erode))


# -- device / twin plumbing -----------------------------------------------------------------------------------------------------------------
def twin_update(ref, oracle_mod, specs, taken=None):
    """The queue on the twin ref (an oracle.Terrain), one modifier and one event number at a time: kinds 0-3 through
    oracle.Terrain.update, brushes and noise through numpy on its memory.  Returns the dirty list ordered by block id.
    taken: a {"low": n, "high": n} dict of the caller's, to which the noise modifiers' clamp-branch counts are added."""
    nb = tuple(d // 8 for d in ref.dims)
    ids = set()
    for spec in specs:
        if spec[0] == "noise":
            hit, (low, high) = apply_noise(ref, gpu_struct(spec))
            ids |= hit
            if taken is not None:
                taken["low"] += low
                taken["high"] += high
        elif spec[0] in ("smooth", "flatten"):
            ids |= apply_brush(ref, gpu_struct(spec))
        else:
            ids |= {int(bx + nb[0] * (by + nb[1] * bz)) for bx, by, bz in ref.update([oracle_mod_of(oracle_mod, spec)])}
    return block_list(ids, nb)


def both_update(ex, ref, oracle_mod, specs, taken=None):
    """The same queue on the device, in one call, and on the twin; returns the device's (n_dirty, T) and the twin's dirty list."""
    got = ex.terrain_update([gpu_struct(s) for s in specs])
    return got, twin_update(ref, oracle_mod, specs, taken)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_grid(ex, want):
    assert np.array_equal(bits(ex.terrain_read_samples()), bits(want))


def assert_triangles(ex, oracle_mod, grid, dirty, T):
    want, want_offs, _ = oracle_mod.extract_grid(np.ascontiguousarray(grid), dirty, threads=8)
    assert T == len(want)
    if T:
        got, offs = ex.read_triangles()
        assert np.array_equal(offs, want_offs) and np.array_equal(got["block"], want["block"])
        for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
            assert np.abs(got[f] - want[f]).max() <= 1e-5


def assert_update(ex, ref, oracle_mod, specs, taken=None):
    (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, specs, taken)
    assert_grid(ex, ref.grid)
    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
    assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
    return n_dirty, T


def world(oracle_mod, dims, scale, origin, seed, specs, history=0):
    """A device terrain and its twin after the queue specs, alike bit for bit; the history budget is set after the build."""
    ex = vt.Extractor(0)
    ex.terrain_init(*dims, scale, origin, seed)
    ref = oracle_mod.Terrain(*dims, scale, origin, seed)
    both_update(ex, ref, oracle_mod, specs)
    assert_grid(ex, ref.grid)
    if history:
        ex.terrain_set_history(history)
    return ex, ref


def invalid(ex, mods):
    with pytest.raises(vt.VtmcError) as e:
        ex.terrain_update(mods)
    assert e.value.code == _lib.ERR_INVALID_ARG
    return str(e.value)


def no_result(fn):
    with pytest.raises(vt.VtmcError) as e:
        fn()
    assert e.value.code == _lib.ERR_NO_RESULT
