"""The numpy twin of the synthetic density sampler (include/vtmc.h, vtmc_density_params; oracle/density_ref.c states the same definition
in FP32 C): Ken Perlin's 2002 improved noise over the SplitMix64 permutation, summed over octaves, minus a vertical ramp.

One deliberate split.  The COORDINATE CHAIN stays FP32, exactly as the CPU twin and both GPU kernels compute it: x = float32(origin + i) * f,
then x = x * lacunarity per octave, each a single IEEE operation.  It decides the lattice cell floor(x) and the fraction x - floor(x) (an
FP32 subtraction too: a tiny negative x gives the fraction 1.0f in every implementation).  EVERYTHING AFTER THE FRACTION runs in float64:
fade, the eight gradient dot products, the seven lerps, the amplitudes, the octave sum and the ramp.  What an FP32 implementation differs
from this twin by is therefore its own rounding after the fraction -- its operation order, its fma contractions -- and nothing else.

The permutation is restated here (permutation) and checked against vto_density_permutation by test_density_sampler.py.

A parameter set is any object with the fields of vtmc_density_params (vt.DensityParams, oracle.DensityParams, Params below)."""
import collections

import numpy as np

f32, f64 = np.float32, np.float64

Params = collections.namedtuple("Params", "seed frequency octaves lacunarity gain ramp_scale ramp_center")

_M64 = (1 << 64) - 1


def permutation(seed):
    """The 256-entry permutation: a Fisher-Yates shuffle from the top, j = SplitMix64() % (i + 1)."""
    perm = list(range(256))
    s = int(seed) & _M64
    for i in range(255, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & _M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
        j = z % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, np.uint8)


def _grad_table():
    """Perlin's grad(hash, x, y, z) is linear in (x, y, z): row h = its coefficients, taken from the definition on the unit vectors."""
    g = np.zeros((16, 3), f64)
    for h in range(16):
        for a in range(3):
            x, y, z = (1.0 if a == c else 0.0 for c in range(3))
            u = x if h < 8 else y
            v = y if h < 4 else (x if h in (12, 14) else z)
            g[h, a] = (u if (h & 1) == 0 else -u) + (v if (h & 2) == 0 else -v)
    return g


GRAD = _grad_table()


def chain(prm, origin, n):
    """The FP32 coordinate chain of n samples from `origin` along one axis: (cells [octaves, n] int64, fractions [octaves, n] float32,
    the largest |coordinate| any octave reaches).  float32(origin + i) is the int -> float conversion of the int32 sum."""
    p = np.int64(origin) + np.arange(n, dtype=np.int64)
    assert np.abs(p).max() < 2 ** 31
    x = p.astype(f32) * f32(prm.frequency)
    cells, fracs, peak = [], [], 0.0
    for _ in range(prm.octaves):
        assert x.dtype == f32
        fx = np.floor(x)
        peak = max(peak, float(np.abs(x).max()))
        cells.append(fx.astype(np.int64))
        fracs.append(x - fx)
        x = x * f32(prm.lacunarity)
    return np.stack(cells), np.stack(fracs), peak


def chain_peak(prm, origins, dims):
    """The largest |lattice coordinate| of the fill: (int)floorf is defined only below 2^31."""
    return max(chain(prm, o[a], dims[a])[2] for o in np.asarray(origins).reshape(-1, 3) for a in range(3))


def fade(t):
    return t * t * t * (t * (t * 6.0 - 15.0) + 10.0)


def mix(t, a, b):
    return a + t * (b - a)


def noise_octave(P, cx, tx, cy, ty, cz, tz):
    """One octave on the grid of three axes: P = the permutation twice over (int64 [512]: no index of the hash chain exceeds 511), c* the
    lattice cells and t* the FP32 fractions per axis.  float64 [nz, ny, nx]."""
    X, Y, Z = (cx & 255)[None, None, :], (cy & 255)[None, :, None], (cz & 255)[:, None, None]
    x, y, z = tx.astype(f64)[None, None, :], ty.astype(f64)[None, :, None], tz.astype(f64)[:, None, None]
    u, v, w = fade(x), fade(y), fade(z)
    A, B = P[X] + Y, P[X + 1] + Y
    AA, AB, BA, BB = P[A] + Z, P[A + 1] + Z, P[B] + Z, P[B + 1] + Z

    def grad(idx, gx, gy, gz):
        h = P[idx] & 15
        return GRAD[h, 0] * gx + GRAD[h, 1] * gy + GRAD[h, 2] * gz

    return mix(w,
               mix(v, mix(u, grad(AA, x, y, z), grad(BA, x - 1, y, z)),
                   mix(u, grad(AB, x, y - 1, z), grad(BB, x - 1, y - 1, z))),
               mix(v, mix(u, grad(AA + 1, x, y, z - 1), grad(BA + 1, x - 1, y, z - 1)),
                   mix(u, grad(AB + 1, x, y - 1, z - 1), grad(BB + 1, x - 1, y - 1, z - 1))))


def density(prm, origin, dims, perm=None):
    """The density of a (dx, dy, dz) volume whose sample (0, 0, 0) is global sample `origin`: float64 [dz, dy, dx] (x fastest)."""
    dx, dy, dz = dims
    if perm is None:
        perm = permutation(prm.seed)
    P = np.concatenate([perm, perm]).astype(np.int64)
    (cx, tx, _), (cy, ty, _), (cz, tz, _) = (chain(prm, origin[a], dims[a]) for a in range(3))
    total, amp = np.zeros((dz, dy, dx), f64), 1.0
    for o in range(prm.octaves):
        total = total + amp * noise_octave(P, cx[o], tx[o], cy[o], ty[o], cz[o], tz[o])
        amp = amp * f64(f32(prm.gain))
    py = (np.int64(origin[1]) + np.arange(dy, dtype=np.int64)).astype(f32).astype(f64)
    ramp = (py - f64(f32(prm.ramp_center))) * f64(f32(prm.ramp_scale))
    return total - ramp[None, :, None]


def amplitude(prm, origins, dims):
    """A of the bar k * A: sum_o |gain|^o, plus the ramp's largest magnitude over the volumes where a ramp is on."""
    a = float(sum(abs(f64(f32(prm.gain))) ** o for o in range(prm.octaves)))
    if f32(prm.ramp_scale) != 0:
        oy = np.asarray(origins, np.int64).reshape(-1, 3)[:, 1]
        py = np.concatenate([oy, oy + dims[1] - 1]).astype(f32).astype(f64)
        a += float(np.abs((py - f64(f32(prm.ramp_center))) * f64(f32(prm.ramp_scale))).max())
    return a
