"""The twin of the flood (vtmc_terrain_flood and its readers): a numpy restatement of the rule WATER of include/vtmc_water.h.  Integers
and 32-bit copies plus the rule's few FP32 steps, each one IEEE operation in float32, so everything test_terrain_water.py compares with it
must be EQUAL, records and volumes as raw bytes.

Grids are float32 arrays indexed [x, y, z], as Extractor.terrain_read_samples returns them.  A box is (first sample, samples per axis).
The labelling is fragment_twin's min-propagation (every sample of the graph takes the smallest label among itself and its neighbours until
nothing changes), run on the graph of each level: open, under the level, not yet wet."""
import types

import numpy as np

import fragment_twin
from volumetricterrain_amd._lib import WATER_AT_FACE, WATER_BODY_DTYPE, WATER_MAX_LEVELS, WATER_MAX_SOURCES, WATER_SOURCE_DTYPE

f32 = np.float32
DRY = np.int64(2 ** 40)   # "no body" where the smallest body index of a neighbourhood is taken


def bits(v):
    return int(np.asarray(v, f32).view(np.uint32))


def sources_of(rows):
    """A WATER_SOURCE_DTYPE array from rows of (x, y, z, level)."""
    rows = np.asarray(rows, f32).reshape(-1, 4)
    out = np.zeros(len(rows), WATER_SOURCE_DTYPE)
    out["position"], out["level"] = rows[:, :3], rows[:, 3]
    return out


def plane_height(j, scale, origin_y):
    """y_j = (float)j * scale + origin_y, two float32 operations; j may be an array."""
    return f32(np.asarray(j).astype(f32) * f32(scale)) + f32(origin_y) if np.ndim(j) else f32(f32(f32(j) * f32(scale)) + f32(origin_y))


def plane_of(level, scale, origin_y, dim_y):
    """The highest plane of 0..dim_y-1 that is under the level (y_j <= level), or -1: a scan over every plane."""
    under = np.nonzero(plane_height(np.arange(dim_y), scale, origin_y) <= f32(level))[0]
    return int(under.max()) if len(under) else -1


def nearest(p, origin, scale):
    """The nearest sample along one axis: g = (p - origin) / scale; floor(g + 0.5), saturating at the int32 range (None for NaN)."""
    with np.errstate(all="ignore"):
        g = f32(f32(p) - f32(origin))
        g = f32(g / f32(scale))
        g = np.floor(f32(g + f32(0.5)))
    return None if np.isnan(g) else int(min(max(float(g), -2.0 ** 31), 2.0 ** 31 - 1))   # saturating, as the library's conversion


def volume_dim(d):
    return 8 * -(-max(d - 2, 1) // 8) + 2


def levels_of(src):
    """The distinct level bit patterns in the order they are processed: descending value, +0 before -0."""
    seen = {}
    for v in src["level"]:
        seen.setdefault(bits(v), f32(v))
    return sorted(seen.values(), key=lambda v: (-float(v), bits(v)))


def clamped_depth(level, height, scale):
    """t = L - y_j; t = t / scale; t = clamp(t, -1, 1), float32 arrays or scalars."""
    with np.errstate(all="ignore"):
        t = (np.asarray(level, f32) - np.asarray(height, f32)).astype(f32)
        t = (t / f32(scale)).astype(f32)
    return np.clip(t, f32(-1), f32(1)).astype(f32)


def flood(grid, first, ext, scale, origin, sources):
    """The result of vtmc_terrain_flood on that box: a namespace of source_body (int32), bodies (WATER_BODY_DTYPE), first, ext, vd (the
    volume dims), body (int32) and water (float32), both [x, y, z] with the volume dims, and wet."""
    src = sources if getattr(sources, "dtype", None) == WATER_SOURCE_DTYPE else sources_of(sources)
    assert len(src) <= WATER_MAX_SOURCES and len(levels_of(src)) <= WATER_MAX_LEVELS
    res = types.SimpleNamespace(source_body=np.full(len(src), -1, np.int32), bodies=np.zeros(0, WATER_BODY_DTYPE), first=tuple(first), ext=tuple(ext),
                                vd=(0, 0, 0), body=np.zeros((0, 0, 0), np.int32), water=np.zeros((0, 0, 0), f32), wet=0, near=0, refused=0)
    if min(ext) <= 0:
        res.ext = (0, 0, 0)
        return res
    (lx, ly, lz), (dx, dy, dz) = first, ext
    box = grid[lx:lx + dx, ly:ly + dy, lz:lz + dz]
    solid = box > 0
    body = np.full(ext, -1, np.int64)
    place = []
    for s in src:
        c = [nearest(s["position"][k], origin[k], scale) for k in range(3)]
        c = None if None in c else tuple(c[k] - first[k] for k in range(3))
        place.append(c if c is not None and all(0 <= c[k] < ext[k] for k in range(3)) else None)
    recs = []
    for level in levels_of(src):
        mine = [k for k in range(len(src)) if bits(src["level"][k]) == bits(level)]
        plane = plane_of(level, scale, origin[1], grid.shape[1]) - ly
        graph = ~solid & (body < 0)
        graph[:, max(plane + 1, 0):, :] = False
        lab = fragment_twin.label(np.where(graph, f32(1), f32(0)))
        roots = {}
        for k in mine:
            if place[k] is None:
                continue
            if body[place[k]] >= 0:                      # already wet: the source joins
                res.source_body[k] = body[place[k]]
                recs[body[place[k]]]["n_sources"] += 1
            elif lab[place[k]] >= 0:
                roots.setdefault(int(lab[place[k]]), []).append(k)
        for root in sorted(roots):                       # ascending box-linear index = ascending grid index of the seed
            rec = np.zeros((), WATER_BODY_DTYPE)
            rec["seed"] = (lx + root % dx, ly + root // dx % dy, lz + root // (dx * dy))
            rec["level"], rec["n_sources"] = level, len(roots[root])
            body[lab == root] = len(recs)
            res.source_body[roots[root]] = len(recs)
            recs.append(rec)
    wet = body >= 0
    above_dry_open = np.zeros(ext, bool)
    above_dry_open[:, :-1, :] = ~solid[:, 1:, :] & ~wet[:, 1:, :]
    face = np.zeros(ext, bool)
    face[:, 0, :] = face[0, :, :] = face[-1, :, :] = face[:, :, 0] = face[:, :, -1] = True
    for i, rec in enumerate(recs):
        mask = body == i
        where = np.argwhere(mask)
        rec["lo"], rec["hi"] = where.min(axis=0) + first, where.max(axis=0) + first
        rec["n_samples"], rec["n_surface"] = len(where), int((mask & above_dry_open).sum())
        rec["flags"] = WATER_AT_FACE if (mask & face).any() else 0
    res.bodies = np.array(recs, WATER_BODY_DTYPE) if recs else np.zeros(0, WATER_BODY_DTYPE)
    res.wet = int(wet.sum())
    # the volumes
    res.vd = tuple(volume_dim(d) for d in ext)
    res.body = np.full(res.vd, -1, np.int32)
    res.body[:dx, :dy, :dz] = body
    res.water = np.full(res.vd, f32(-1), f32)
    if recs:
        pad = np.full((dx + 2, dy + 2, dz + 2), DRY)
        pad[1:-1, 1:-1, 1:-1] = np.where(wet, body, DRY)
        low = np.full(ext, DRY)                          # the smallest body index of the 27: the largest level
        for ox in range(3):
            for oy in range(3):
                for oz in range(3):
                    low = np.minimum(low, pad[ox:ox + dx, oy:oy + dy, oz:oz + dz])
        has = low < DRY
        chosen = np.where(wet, body, np.where(has, low, 0))
        height = plane_height(np.arange(ly, ly + dy), scale, origin[1]).astype(f32)
        t = clamped_depth(res.bodies["level"][chosen], height[None, :, None], scale)
        res.water[:dx, :dy, :dz] = np.where(has & (wet | solid | (t <= 0)), t, f32(-1))
        res.near, res.refused = int((has & ~wet).sum()), int((has & ~wet & ~solid & ~(t <= 0)).sum())
    return res


def probe(res, positions, scale, origin):
    """(body, depth) of vtmc_water_probe on the result of flood()."""
    p = np.asarray(positions, f32).reshape(-1, 3)
    body, depth = np.full(len(p), -1, np.int32), np.zeros(len(p), f32)
    for i, q in enumerate(p):
        if not np.isfinite(q).all() or min(res.ext) <= 0:
            continue
        c = [nearest(q[k], origin[k], scale) for k in range(3)]
        if None in c:
            continue
        c = tuple(c[k] - res.first[k] for k in range(3))
        if all(0 <= c[k] < res.ext[k] for k in range(3)) and res.body[c] >= 0:
            body[i] = res.body[c]
            depth[i] = f32(res.bodies["level"][body[i]]) - q[1]
    return body, depth


def volume_counts(res):
    """(near, refused, positive, wet zeros) of a result: the near samples, those of them that hold -1 because they are open and under the
    level (diagonal contact only), the values > 0, and the wet samples that hold 0 exactly."""
    dx, dy, dz = res.ext
    wet = res.body[:dx, :dy, :dz] >= 0
    return res.near, res.refused, int((res.water > 0).sum()), int((wet & (res.water[:dx, :dy, :dz] == 0)).sum())
