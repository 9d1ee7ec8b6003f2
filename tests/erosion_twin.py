"""The rule EROSION of include/vtmc_erosion.h in numpy, vectorised over the plane and following the header operation by operation: every
line below is one IEEE operation per element in `dtype` (float32: the library's arithmetic, held to it bit for bit; float64: the same
rule with less rounding, for the conservation test).  Planes are indexed [z, x] (x fastest in memory, as the library's maps); a grid is
indexed [x, y, z] as Extractor.terrain_read_samples returns it."""
import collections

import numpy as np

G, SIN_MIN, DEPTH_EPS = 9.81, 0.05, 1.0e-4
DIRS = ((0, -1), (0, 1), (-1, 0), (1, 0))   # (dz, dx) of the directions k = 0..3 = [-x, +x, -z, +z]; the opposite of k is k ^ 1

Params = collections.namedtuple("Params", "rain evaporation capacity dissolve deposit dt talus thermal_rate")
DEFAULT = Params(0.01, 0.02, 1.0, 0.3, 0.3, 0.25, 1.0, 0.0)
Result = collections.namedtuple("Result", "grid lo hi before after water sediment active info")


def neighbour(a, k, fill=0):
    """a's value at the neighbour in direction k of every column; `fill` where that neighbour lies outside the plane."""
    dz, dx = DIRS[k]
    out = np.full_like(a, fill)
    nz, nx = a.shape
    dst_z, src_z = (slice(1, nz), slice(0, nz - 1)) if dz < 0 else (slice(0, nz - 1), slice(1, nz)) if dz > 0 else (slice(0, nz), slice(0, nz))
    dst_x, src_x = (slice(1, nx), slice(0, nx - 1)) if dx < 0 else (slice(0, nx - 1), slice(1, nx)) if dx > 0 else (slice(0, nx), slice(0, nx))
    out[dst_z, dst_x] = a[src_z, src_x]
    return out


def sum4(v):
    return (v[0] + v[1]) + (v[2] + v[3])


class State:
    """b, d, s, f[4] and the mask of a plane; every plane holds 0 on an inactive column."""

    def __init__(self, h0, active, dtype=np.float32):
        self.t = np.dtype(dtype).type
        self.active = np.asarray(active, bool)
        self.counts = [self.active & neighbour(self.active, k, False) for k in range(4)]
        zero = np.zeros(self.active.shape, dtype)
        self.b = np.where(self.active, np.asarray(h0, dtype), zero)
        self.d, self.s, self.f = zero.copy(), zero.copy(), [zero.copy() for _ in range(4)]


# -- the operations a test may swap for a near neighbour (test_terrain_erosion_edges.py, "mutants"): as they stand they are the rule's ------
def result(a):
    """Every FP32 result of a step passes through here, unchanged: IEEE keeps subnormals."""
    return a


def keep_of(t, ke, dt):
    """1 - Ke * dt: two operations."""
    return t(t(1) - t(ke * dt))


def dt_g_of(t, dt):
    """dt * G, G rounded to the step's type first."""
    return t(dt * t(G))


def inv_dt_of(t, dt, given_dt):
    """1 / dt of the ROUNDED dt; given_dt is the parameter as the caller wrote it."""
    return t(t(1) / dt)


def quotient(a, b):
    """Speed: wx / db."""
    return a / b


def fraction_of(f, dt, d1):
    """Transport: (f' * dt) / d1."""
    return result(result(f * dt) / d1)


def lesser(a, b):
    """min(a, b) = a < b ? a : b"""
    return np.where(a < b, a, b)


def greater(a, b):
    """max(a, b) = a > b ? a : b"""
    return np.where(a > b, a, b)


CENSUS_KEYS = ("flux_zeroed", "scaled", "not_scaled", "d2_clipped", "deep", "shallow", "sp_capped", "sa_raised", "takes", "deposits", "e_limited",
               "transport_dry", "thermal_moves", "sign_minus", "sign_plus", "sign_zero", "subnormal_b", "subnormal_d", "subnormal_s",
               "subnormal_f", "negative_s", "not_finite")


def new_census():
    return dict.fromkeys(CENSUS_KEYS, 0)


def subnormals(a):
    tiny = np.finfo(a.dtype).tiny
    return int(((a != 0) & (np.abs(a) < tiny)).sum())


def step(st, p, census=None):
    """One step of the rule on st.  census: a dict (new_census()) to which the step adds, per branch of the rule, the number of active
    columns that took it -- for a branch taken per direction (flux_zeroed, thermal_moves, sign_*) the number of column-directions whose
    neighbour counts -- and the number of subnormal values b, d, s and f hold after the step, of negative s, and of values of the state
    that are not finite.  It changes no bit."""
    t, act, cnt = st.t, st.active, st.counts
    R = result
    zero = np.zeros(act.shape, t)
    dt, kr, ke, kc, ks, kd, talus, kt = t(p.dt), t(p.rain), t(p.evaporation), t(p.capacity), t(p.dissolve), t(p.deposit), t(p.talus), t(p.thermal_rate)
    dt_rain, dt_g, inv_dt = R(t(dt * kr)), R(dt_g_of(t, dt)), R(inv_dt_of(t, dt, p.dt))
    keep = R(keep_of(t, ke, dt))
    half, eps, sin_min = t(0.5), t(DEPTH_EPS), t(SIN_MIN)
    b, d, s = st.b, st.d, st.s
    note = {} if census is not None else None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        # flux
        d1 = R(d + dt_rain)
        H = R(b + d1)
        f, dropped = [], 0
        for k in range(4):
            g = R(st.f[k] + R(dt_g * R(H - neighbour(H, k))))
            f.append(np.where(cnt[k] & (g > 0), g, zero))
            if note is not None:
                dropped += int((cnt[k] & ~(g > 0)).sum())
        out = R(sum4r(f))
        vol = R(out * dt)
        scale = vol > d1
        K = R(d1 / vol)
        f = [np.where(scale, R(f[k] * K), f[k]) for k in range(4)]
        out = sum4r(f)
        # water and speed
        fin = [np.where(cnt[k], neighbour(f[k ^ 1], k), zero) for k in range(4)]
        inn = sum4r(fin)
        d2 = R(d1 + R(dt * R(inn - out)))
        wet = d2 > 0
        d2 = np.where(wet, d2, zero)
        wx = R(R(R(fin[0] - f[0]) + R(f[1] - fin[1])) * half)
        wz = R(R(R(fin[2] - f[2]) + R(f[3] - fin[3])) * half)
        db = R(R(d1 + d2) * half)
        deep = db > eps
        u = np.where(deep, R(quotient(wx, db)), zero)
        w = np.where(deep, R(quotient(wz, db)), zero)
        sp_free = R(np.sqrt(R(R(u * u) + R(w * w))))
        sp = lesser(sp_free, inv_dt)
        # erosion and deposition
        bn = [np.where(cnt[k], neighbour(b, k), b) for k in range(4)]
        gx = R(R(bn[1] - bn[0]) * half)
        gz = R(R(bn[3] - bn[2]) * half)
        g2 = R(R(gx * gx) + R(gz * gz))
        sa_free = R(np.sqrt(R(g2 / R(t(1) + g2))))
        sa = greater(sa_free, sin_min)
        C = R(R(kc * sa) * sp)
        take = C > s
        e_free = R(ks * R(C - s))
        e = lesser(e_free, d2)
        q = R(kd * R(s - C))
        b1 = np.where(take, R(b - e), R(b + q))
        s1 = np.where(take, R(s + e), R(s - q))
        # transport
        rained = d1 > 0
        give = [R(s1 * np.where(rained, fraction_of(f[k], dt, d1), zero)) for k in range(4)]
        gin = [np.where(cnt[k], neighbour(give[k ^ 1], k), zero) for k in range(4)]
        s2 = R(R(s1 - sum4r(give)) + sum4r(gin))
        # evaporation
        d3 = R(d2 * keep)
        # thermal
        th, moves, signs = [], 0, [0, 0, 0]
        for k in range(4):
            b1n = neighbour(b1, k)
            hi, lo = greater(b1, b1n), lesser(b1, b1n)
            m = R(kt * R(R(hi - lo) - talus))
            m = np.where(cnt[k] & (m > 0), m, zero)
            sign = np.where(b1 > b1n, t(-1), np.where(b1 < b1n, t(1), t(0)))
            th.append(R(sign * m))
            if note is not None:
                moves += int((m > 0).sum())
                for i, v in enumerate((-1, 1, 0)):
                    signs[i] += int((cnt[k] & (sign == v)).sum())
        b2 = R(b1 + sum4r(th))
    st.b, st.d, st.s = np.where(act, b2, zero), np.where(act, d3, zero), np.where(act, s2, zero)
    st.f = [np.where(act, f[k], zero) for k in range(4)]
    if census is not None:
        n = lambda flag: int((act & flag).sum())   # noqa: E731
        for key, v in (("flux_zeroed", dropped), ("scaled", n(scale)), ("not_scaled", n(~scale)), ("d2_clipped", n(~wet)), ("deep", n(deep)),
                       ("shallow", n(~deep)), ("sp_capped", n(~(sp_free < inv_dt))), ("sa_raised", n(~(sa_free > sin_min))), ("takes", n(take)),
                       ("deposits", n(~take)), ("e_limited", n(take & ~(e_free < d2))), ("transport_dry", n(~rained)), ("thermal_moves", moves),
                       ("sign_minus", signs[0]), ("sign_plus", signs[1]), ("sign_zero", signs[2]), ("subnormal_b", subnormals(st.b)),
                       ("subnormal_d", subnormals(st.d)), ("subnormal_s", subnormals(st.s)), ("subnormal_f", sum(subnormals(a) for a in st.f)),
                       ("negative_s", int((st.s < 0).sum())), ("not_finite", sum(int((~np.isfinite(a)).sum()) for a in (st.b, st.d, st.s, *st.f)))):
            census[key] = census.get(key, 0) + v
    return st


def sum4r(v):
    """sum4 with each of its three results passed through result()."""
    return result(result(v[0] + v[1]) + result(v[2] + v[3]))


def simulate(h0, active, iterations, params=DEFAULT, dtype=np.float32, census=None):
    st = State(h0, active, dtype)
    for _ in range(iterations):
        step(st, params, census)
    return st


def heights(grid, lo, hi):
    """(h0 [z, x] float32, active [z, x] bool) of the inclusive sample box lo..hi of grid[x, y, z], by the rule's Heights."""
    box = np.asarray(grid, np.float32)[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    nx, ny, nz = box.shape
    h0, active = np.zeros((nz, nx), np.float32), np.zeros((nz, nx), bool)
    solid = box > 0
    for ix in range(nx):
        for iz in range(nz):
            if solid[ix, ny - 1, iz]:
                continue
            js = np.nonzero(solid[ix, :ny - 1, iz])[0]
            if len(js):
                j = int(js[-1])
                sj, sa = box[ix, j, iz], box[ix, j + 1, iz]
                with np.errstate(all="ignore"):
                    h0[iz, ix] = np.float32(lo[1] + j) + sj / (sj - sa)
                active[iz, ix] = True
    return h0, active


def clamp_heights(b, active, ly, uy):
    """h1 and the columns the clamp changed."""
    cl, ch = np.float32(np.float32(ly) + np.float32(0.5)), np.float32(uy - 1)
    h1 = np.where(b < cl, cl, np.where(b > ch, ch, b)).astype(np.float32)
    h1 = np.where(active, h1, np.float32(0))
    return h1, active & (h1 != b)


def write_back(grid, lo, hi, h0, h1, active):
    """A copy of grid[x, y, z] with the rule's Write-back applied to the box."""
    out = np.array(grid, np.float32, copy=True)
    one = np.float32(1)
    for iz, ix in zip(*np.nonzero(active & (h1 != h0))):
        a, b = h0[iz, ix], h1[iz, ix]
        low, high = (a if a < b else b) - one, (a if a > b else b) + one
        for y in range(lo[1], hi[1] + 1):
            fy = np.float32(y)
            if low <= fy <= high:
                v = b - fy
                out[lo[0] + ix, y, lo[2] + iz] = -one if v < -one else (one if v > one else v)
    return out


def erode(grid, lo, hi, iterations, params=DEFAULT, census=None):
    """VTMC_MOD_EROSION on the inclusive, already clamped sample box lo..hi of grid[x, y, z]: the new grid, the five maps and the report."""
    h0, active = heights(grid, lo, hi)
    st = simulate(h0, active, iterations, params, census=census)
    h1, clamped = clamp_heights(st.b, active, lo[1], hi[1])
    info = {"lo": tuple(lo), "hi": tuple(hi), "nx": hi[0] - lo[0] + 1, "nz": hi[2] - lo[2] + 1, "iterations": iterations,
            "n_active": int(active.sum()), "n_rewritten": int((active & (h1 != h0)).sum()), "n_clamped": int(clamped.sum())}
    return Result(write_back(grid, lo, hi, h0, h1, active), tuple(lo), tuple(hi), h0, h1, st.d, st.s, active.astype(np.uint8), info)
