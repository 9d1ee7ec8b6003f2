"""Ray picking held to float32 precision (surface_twin.tight_check_ray): every marching-cubes case and triangle slot aimed at on
purpose, memory layouts and non-cubic boxes, the max_distance cut-off, the terrain entry point in a scaled and shifted world, and
stream ordering.  The CPU tests show that the tight checker rejects the mistakes a rewrite of the kernel could make, and that the
aimed ray sets reach every (case, slot) pair of the table.

Ambiguous rays (surface_twin's rule), measured with the reference alone: the aimed rays 0 of 6560 (all-cases grid) and 0 of 13120
(64^3 random field); the layout rays 0, 1 and 0 of 1200 (the three box configurations); the terrain rays 0 of 600, one- and
two-sided; the cut-off rays 2 of 240.  Each test's cap is set a little above its own rate.
"""
import numpy as np
import pytest

import fields
from surface_twin import (RAY_HIT_BYTES, DeviceGrid, Surface, _cast, _device, _rays_perlin, check_tight, compare, reference, report,
                          tight_check_ray)


# ---------------------------------------------------------------------------------------------------------------------------------
# rays aimed at chosen triangles
# ---------------------------------------------------------------------------------------------------------------------------------
SHORT = 0.25   # max_distance of the short batches (world units at scale 1): a ray crosses one or two cells, most lanes share them


def _tangents(n):
    a = np.where(np.abs(n[:, :1]) < 0.6, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t1 = np.cross(n, a)
    t1 /= np.linalg.norm(t1, axis=1)[:, None]
    return t1, np.cross(n, t1)


def aimed_batches(surf, targets):
    """Four batches (max_distance, two_sided, origins, directions, target index per ray) of rays at the centroids of the target
    triangles: single-sided from in front (-normal from 1/16 cell, a tilted ray from 1/8 cell, short; -normal from 1/16 cell and
    a tilted ray from 0.3 cell, unbounded), and the same from behind the face, two-sided."""
    P = surf.P[targets]
    c = P.mean(1)
    n = surf.unit_n[targets]
    t1, t2 = _tangents(n)
    s = surf.scale
    out = []
    for two_sided, sign in ((False, -1.0), (True, 1.0)):
        dn = sign * n
        tilt1 = dn + 0.35 * t1 - 0.2 * t2
        tilt2 = dn - 0.3 * t1 + 0.4 * t2
        for md, rays in ((SHORT * s, ((dn, 1 / 16), (tilt1, 1 / 8))), (np.inf, ((dn, 1 / 16), (tilt2, 0.3)))):
            O = np.concatenate([c - L * s * d / np.linalg.norm(d, axis=1)[:, None] for d, L in rays])
            D = np.concatenate([d for d, _ in rays])
            out.append((md, two_sided, O.astype(np.float32), D.astype(np.float32), np.concatenate([targets] * len(rays))))
    return out


def accepted(surf, ref, tgt):
    """Rays the reference answers, non-ambiguously and with the next hit more than 1e-3 cells farther, with their target."""
    ok = np.zeros(len(ref), bool)
    for i, (r, j) in enumerate(zip(ref, tgt)):
        ok[i] = r["hit"] and not r["ambiguous"] and r["gap"] > 1e-3 and surf.lookup(*r["key"]) == j
    return ok


def all_pairs(oracle_mod):
    _, tri_num, _ = oracle_mod.tables()
    return {(c, i) for c in range(256) for i in range(tri_num[c])}


def isolated_targets(surf):
    """The triangles of the all-cases grid's isolated cells (even global coordinates)."""
    g = 8 * surf.block + np.stack([surf.cell % 8, (surf.cell // 8) % 8, surf.cell // 64], 1)
    return np.nonzero(np.all(g % 2 == 0, axis=1))[0]


def random_targets(surf, seed):
    """Two triangles of every (case, slot) pair the surface holds, drawn at random."""
    rng = np.random.default_rng(seed)
    pair = surf.case.astype(np.int64) * 5 + surf.tri
    order = rng.permutation(len(pair))
    _, first = np.unique(pair[order], return_index=True)
    rest = np.setdiff1d(np.arange(len(order)), first)
    _, second = np.unique(pair[order][rest], return_index=True)
    return np.sort(order[np.concatenate([first, rest[second]])])


def aimed_sets(oracle_mod):
    """(label, grid, surface, batches with their references and accepted masks) for the all-cases grid and a 64^3 random field."""
    out = []
    for label, g, pick in (("all-cases grid", fields.all_cases_grid(), isolated_targets),
                           ("random 64^3", fields.random_field((64, 64, 64), 29), lambda s: random_targets(s, 3))):
        surf = Surface.of_grid(oracle_mod, g)
        batches = []
        for md, two_sided, O, D, tgt in aimed_batches(surf, pick(surf)):
            ref = reference(surf, O, D, max_distance=md, two_sided=two_sided)
            batches.append((md, two_sided, O, D, tgt, ref, accepted(surf, ref, tgt)))
        out.append((label, g, surf, batches))
    return out


def covered(surf, batches, two_sided):
    got = set()
    for _, ts, _, _, tgt, _, ok in batches:
        if ts == two_sided:
            got |= set(zip(surf.case[tgt[ok]].tolist(), surf.tri[tgt[ok]].tolist()))
    return got


def test_aimed_rays_reach_every_case_and_slot(oracle_mod):
    """CPU: the aimed ray sets hold, for every (case, slot) of the table, rays the reference answers with exactly that triangle, both
    single-sided from in front and two-sided from behind -- in the all-cases grid alone, and again in the 64^3 random field."""
    pairs = all_pairs(oracle_mod)
    assert len(pairs) == 820
    for label, _, surf, batches in aimed_sets(oracle_mod):
        n = sum(len(b[2]) for b in batches)
        n_amb = sum(r["ambiguous"] for b in batches for r in b[5])
        n_ok = sum(int(b[6].sum()) for b in batches)
        print("%s: %d aimed rays, %d ambiguous, %d accepted" % (label, n, n_amb, n_ok))
        assert n_amb <= 0.002 * n, n_amb
        for two_sided in (False, True):
            missing = pairs - covered(surf, batches, two_sided)
            assert not missing, (label, two_sided, sorted(missing)[:20])


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker has teeth (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def perfect_hits(surf, ref):
    """What a correct kernel returns, built from the reference's float64 answers."""
    import volumetricterrain_amd as vt
    hits = np.zeros(len(ref), vt.RAY_HIT_DTYPE)
    for h, r in zip(hits, ref):
        if not r["hit"]:
            h["distance"], h["block"], h["cell"], h["triangle"] = -1.0, -1, -1, -1
            continue
        (idx, t, u, v, _, hit, _), o, d = r["trace"]
        k = np.nonzero(idx == surf.lookup(*r["key"]))[0][0]
        h["distance"] = np.float32(r["t"])
        h["point"] = (o + r["t"] * d).astype(np.float32)
        h["normal"] = r["normal"].astype(np.float32)
        h["barycentric"] = np.float32([u[k], v[k]])
        h["block"], h["cell"], h["triangle"] = r["key"]
    return hits


def _mutations(h):
    """(name, mutated copy) for the mistakes the checker must catch."""
    out = []
    m = h.copy()
    m["barycentric"] = h["barycentric"][::-1]
    if abs(float(h["barycentric"][0]) - float(h["barycentric"][1])) > 1e-5:
        out.append(("u and v swapped", m))
    m = h.copy()
    d = np.float32(h["distance"])
    for _ in range(4):
        d = np.nextafter(d, np.float32(np.inf))
    m["distance"] = d
    out.append(("distance + 4 ulp", m))
    for k in range(3):
        m = h.copy()
        m["normal"][k] = np.float32(float(h["normal"][k]) + (1e-6 if h["normal"][k] <= 0 else -1e-6))
        out.append(("normal[%d] +- 1e-6" % k, m))
    m = h.copy()
    m["triangle"] = h["triangle"] - 1 if h["triangle"] > 0 else h["triangle"] + 1
    out.append(("triangle slot off by one", m))
    m = h.copy()
    m["cell"] = h["cell"] ^ 1 if h["cell"] % 8 else h["cell"] + 8 * (1 if (h["cell"] // 8) % 8 < 7 else -1)
    out.append(("wrong cell", m))
    return out


def test_tight_checker_catches_single_mistakes(oracle_mod):
    """Hits built from the reference pass tight_check_ray on a plane, a sphere and a small random field; each single mutation of
    every such hit -- u and v swapped, the distance moved by 4 ulps, one normal component moved by 1e-6, the triangle slot off by
    one, a neighbouring cell -- fails it."""
    rng = np.random.default_rng(41)
    cases = []
    surf = Surface.of_grid(oracle_mod, fields.plane((24, 16, 24), 7.375))
    o = np.stack([rng.uniform(0.5, 23.5, 48), np.full(48, 15.5), rng.uniform(0.5, 23.5, 48)], 1)
    d = np.stack([rng.uniform(-0.3, 0.3, 48), -np.ones(48), rng.uniform(-0.3, 0.3, 48)], 1)
    cases.append(("plane", surf, o, d))
    c = np.array([12.3, 11.7, 12.1])
    surf = Surface.of_grid(oracle_mod, fields.sphere((24, 24, 24), c, 7.5))
    u = rng.normal(size=(64, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    cases.append(("sphere", surf, c + 30 * u, -u + 0.1 * rng.normal(size=(64, 3))))
    surf = Surface.of_grid(oracle_mod, fields.random_field((16, 16, 16), 12))
    o = rng.uniform(-2, 18, (256, 3))
    cases.append(("random 16^3", surf, o, rng.uniform(2, 14, (256, 3)) - o))
    n_mut = {}
    for label, surf, o, d in cases:
        o, d = o.astype(np.float32), d.astype(np.float32)
        ref = reference(surf, o, d)
        hits = perfect_hits(surf, ref)
        assert compare(hits, ref, 1.0, label) <= 0.02 * len(o)
        n_chk, n_graze = check_tight(hits, ref, surf, label)
        assert n_chk >= len(o) // 3, (label, n_chk)
        for h, r in zip(hits, ref):
            if r["ambiguous"] or not r["hit"] or tight_check_ray(h, r, surf) < 1e-4:
                continue
            for name, m in _mutations(h):
                with pytest.raises(AssertionError):
                    tight_check_ray(m, r, surf)
                n_mut[name] = n_mut.get(name, 0) + 1
    assert all(n_mut.get(name, 0) >= 100 for name in ("u and v swapped", "distance + 4 ulp", "normal[1] +- 1e-6",
                                                      "triangle slot off by one", "wrong cell")), n_mut


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: every case and slot
# ---------------------------------------------------------------------------------------------------------------------------------
def _strides(g):
    return tuple(int(s) // 4 for s in g.strides)


@pytest.mark.gpu
def test_every_case_and_slot_on_the_device(oracle_mod):
    """The aimed rays through vtmc_raycast_device, on the all-cases grid and a 64^3 random field: every accepted ray returns its
    target's (block, cell, triangle) exactly and passes the tight check; together they cover all 820 (case, slot) pairs,
    single-sided from in front and two-sided from behind."""
    import volumetricterrain_amd as vt
    pairs = all_pairs(oracle_mod)
    with vt.Extractor(0) as ex:
        for label, g, surf, batches in aimed_sets(oracle_mod):
            mem = np.ascontiguousarray(g.transpose(2, 1, 0))
            d_g = _device(mem.ravel())
            n = tuple(s - 2 for s in g.shape)
            st = (1, g.shape[0], g.shape[0] * g.shape[1])
            seen = {False: set(), True: set()}
            n_rays = n_amb = 0
            tight = [0, 0]
            for md, two_sided, O, D, tgt, ref, ok in batches:
                hits = _cast(ex, d_g.data_ptr(), n, st, (0, 0, 0), 1.0, O, D, max_distance=md, two_sided=two_sided)
                lab = "%s md %g two_sided %d" % (label, md, two_sided)
                n_amb += compare(hits, ref, 1.0, lab)
                tight = [a + b for a, b in zip(tight, check_tight(hits, ref, surf, lab))]
                n_rays += len(O)
                for i in np.nonzero(ok)[0]:
                    h = hits[i]
                    assert (tuple(h["block"]), int(h["cell"]), int(h["triangle"])) == ref[i]["key"], (lab, i, h, ref[i]["key"])
                seen[two_sided] |= set(zip(surf.case[tgt[ok]].tolist(), surf.tri[tgt[ok]].tolist()))
            report(label + " aimed", n_rays, n_amb, tight)
            assert n_amb <= 0.002 * n_rays, n_amb
            assert seen[False] == pairs and seen[True] == pairs


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: layouts, boxes, a far origin
# ---------------------------------------------------------------------------------------------------------------------------------
def _layout(dims, order, pad):
    """Element strides (sx, sy, sz) and span for dims samples (x, y, z) in memory order `order` (slowest axis first), the middle
    and slowest pitches padded by pad elements."""
    m = [dims["xyz".index(a)] for a in order]
    p1 = m[2] + pad[0]
    p0 = p1 * m[1] + pad[1]
    st = [0, 0, 0]
    st["xyz".index(order[0])], st["xyz".index(order[1])], st["xyz".index(order[2])] = p0, p1, 1
    return tuple(st), p0 * m[0]


LAYOUTS = (("zyx", (3, 7)), ("zxy", (0, 0)), ("xyz", (5, 2)), ("yzx", (0, 0)))   # x- / y- / z-fastest and (x, z, y)


def _rays_box(n, k, seed):
    """Rays through a box of n cells: from outside at a point of the box, from inside in any direction, and axis-aligned rays
    (off the lattice planes) along each axis."""
    rng = np.random.default_rng(seed)
    n = np.asarray(n, float)
    c = n / 2
    k1, k2 = k // 2, k // 4
    u = rng.normal(size=(k1, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o1 = c + u * rng.uniform(0.6, 0.9, (k1, 1)) * np.linalg.norm(n)
    d1 = rng.uniform(0, 1, (k1, 3)) * n - o1
    o2 = rng.uniform(0, 1, (k2, 3)) * n
    d2 = rng.normal(size=(k2, 3))
    k3 = k - k1 - k2
    o3 = rng.uniform(0.01, 0.99, (k3, 3)) * n
    ax = rng.integers(0, 3, k3)
    o3[np.arange(k3), ax] = np.where(rng.random(k3) < 0.5, -1.5, n[ax] + 1.5)
    d3 = np.zeros((k3, 3))
    d3[np.arange(k3), ax] = np.sign(c[ax] - o3[np.arange(k3), ax])
    return np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])


@pytest.mark.gpu
def test_layouts_and_boxes_give_identical_hits(oracle_mod):
    """One perlin3d field filled on the device in four memory orders (x-fastest padded, y-fastest, z-fastest padded, x-z-y), on a
    40 x 16 x 72 and an 8 x 64 x 8 box, the first also at voxel_scale 0.5 with the origin near 1e4: the four layouts read back the
    same samples and return byte-identical hits, which agree with the reference under the tight check."""
    import torch
    import volumetricterrain_amd as vt
    prm = vt.density_params("perlin3d", 64)
    configs = (((40, 16, 72), 1.0, (0.0, 0.0, 0.0), 51), ((40, 16, 72), 0.5, (10000.0, -2500.0, 9999.5), 52),
               ((8, 64, 8), 1.0, (3.25, -7.5, 1.0), 53))
    with vt.Extractor(0) as ex:
        for n, scale, origin, seed in configs:
            dims = tuple(c + 2 for c in n)
            O, D = _rays_box(n, 1200, seed)
            o = (np.float32(origin) + O.astype(np.float32) * np.float32(scale)).astype(np.float32)
            D = D.astype(np.float32)
            first, grid = None, None
            for order, pad in LAYOUTS:
                st, span = _layout(dims, order, pad)
                buf = torch.full((span,), float("nan"), dtype=torch.float32, device="cuda")
                ex.density_fill_device(prm, [[0, 0, 0]], dims, st, 0, buf.data_ptr())
                host = buf.cpu().numpy()
                view = np.lib.stride_tricks.as_strided(host, shape=dims, strides=tuple(4 * s for s in st))
                if grid is None:
                    grid = np.ascontiguousarray(view.transpose(2, 1, 0)).transpose(2, 1, 0)
                assert np.array_equal(view.view(np.uint32), grid.view(np.uint32)), order
                hits = _cast(ex, buf.data_ptr(), n, st, origin, scale, o, D)
                if first is None:
                    first = hits
                assert hits.tobytes() == first.tobytes(), ("layout %s gives different hits" % order, n, scale)
            surf = Surface.of_grid(oracle_mod, grid, origin, scale)
            ref = reference(surf, o, D)
            label = "box %s scale %g origin %s" % (n, scale, origin)
            n_amb = compare(first, ref, scale, label)
            report(label, len(o), n_amb, check_tight(first, ref, surf, label))
            assert n_amb <= 0.005 * len(o), n_amb
            assert (first["triangle"] >= 0).sum() > len(o) // 3


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: max_distance
# ---------------------------------------------------------------------------------------------------------------------------------
def _cast_each(ex, d_g, n, st, origin, scale, o, d, mds, two_sided=False):
    """Ray i alone with max_distance mds[i]: one launch per ray, all queued on the context's stream, one read-back."""
    import torch
    import volumetricterrain_amd as vt
    d_o, d_d = _device(o), _device(d)
    d_h = torch.zeros(len(o) * RAY_HIT_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i, md in enumerate(mds):
        ex.raycast_device(d_g, n, st, origin, scale, d_o.data_ptr() + 12 * i, d_d.data_ptr() + 12 * i, 1, d_h.data_ptr() + RAY_HIT_BYTES * i,
                          float(md), two_sided)
    return ex.copy_to_host(d_h.data_ptr(), len(o) * RAY_HIT_BYTES).view(vt.RAY_HIT_DTYPE)


@pytest.mark.gpu
def test_max_distance_cut_off_moves_no_hit(oracle_mod):
    """Rays with a non-ambiguous hit at distance d on a 64^3 perlin3d field: with max_distance d, d (1 + 2^-10), 1.5 d, 4 d and inf
    (each of which cuts the clipped interval, and so every lane's sub-interval, differently) the hit is byte-identical to the
    unbounded one, and with max_distance nextafter(d, 0) the ray misses.  Two calls with the same arguments return the same bytes.
    A plane at an integer height (samples exactly 0, triangles on the cells' top faces): a vertical ray from y = 40 returns the
    exact distance, point and normal (0, 1, 0), also with max_distance equal to that distance."""
    import torch
    import volumetricterrain_amd as vt
    n, dim = 64, 66
    st = (1, dim, dim * dim)
    with vt.Extractor(0) as ex:
        g = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
        ex.density_fill_device(vt.density_params("perlin3d", n), [[0, 0, 0]], (dim,) * 3, st, 0, g.data_ptr())
        grid = g.cpu().numpy().reshape(dim, dim, dim).transpose(2, 1, 0)
        O, D = _rays_perlin(n, 4096, 23)
        rng = np.random.default_rng(4)
        sel = rng.permutation(len(O))[:240]
        O, D = O[sel], D[sel]
        base = _cast(ex, g.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, O, D)
        again = _cast(ex, g.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, O, D)
        assert base.tobytes() == again.tobytes()
        surf = Surface.of_grid(oracle_mod, grid)
        ref = reference(surf, O, D)
        n_amb = compare(base, ref, 1.0, "cut-off rays")
        report("cut-off rays", len(O), n_amb, check_tight(base, ref, surf, "cut-off rays"))
        assert n_amb <= 0.02 * len(O), n_amb
        keep = np.array([r["hit"] and not r["ambiguous"] for r in ref]) & (base["triangle"] >= 0)
        assert keep.sum() >= 96, keep.sum()
        O, D, want = O[keep], D[keep], base[keep]
        d = want["distance"].astype(np.float32)
        for label, mds in (("d", d), ("d(1+2^-10)", d * np.float32(1 + 2.0 ** -10)), ("1.5d", d * np.float32(1.5)), ("4d", 4 * d),
                           ("inf", np.full(len(d), np.inf, np.float32))):
            got = _cast_each(ex, g.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, O, D, mds)
            bad = [i for i in range(len(O)) if got[i].tobytes() != want[i].tobytes()]
            assert not bad, (label, bad[:5], got[bad[:2]], want[bad[:2]])
        got = _cast_each(ex, g.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, O, D, np.nextafter(d, np.float32(0)))
        assert (got["triangle"] == -1).all() and (got["distance"] == -1.0).all(), np.nonzero(got["triangle"] >= 0)[0][:5]
        # exact answers on a plane at an integer height
        h, np_ = 21, (32, 48, 32)
        pg = fields.plane(np_, h)
        d_p = _device(np.ascontiguousarray(pg.transpose(2, 1, 0)).ravel())
        pst = (1, 34, 34 * 50)
        k = 64
        xz = (rng.integers(0, 32, (k, 2)) + np.array([0.3, 0.6])).astype(np.float32)
        O = np.stack([xz[:, 0], np.full(k, 40.0, np.float32), xz[:, 1]], 1).astype(np.float32)
        D = np.tile(np.float32([0, -1, 0]), (k, 1))
        for md in (np.inf, 40.0 - h, 100.0):
            hits = _cast(ex, d_p.data_ptr(), np_, pst, (0, 0, 0), 1.0, O, D, max_distance=md)
            assert (hits["triangle"] >= 0).all(), md
            assert (hits["distance"] == np.float32(40 - h)).all(), (md, hits["distance"])
            assert np.array_equal(hits["point"], np.stack([O[:, 0], np.full(k, h, np.float32), O[:, 2]], 1)), md
            assert np.array_equal(hits["normal"], np.tile(np.float32([0, 1, 0]), (k, 1))), md
        miss = _cast(ex, d_p.data_ptr(), np_, pst, (0, 0, 0), 1.0, O, D, max_distance=float(np.nextafter(np.float32(40 - h), np.float32(0))))
        assert (miss["triangle"] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the terrain entry point in a scaled, shifted world
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_terrain_raycast_in_a_scaled_shifted_world(oracle_mod):
    """terrain_init(64, 32, 48, voxel_scale 0.5, origin (-3.25, 1.5, 7)), a plane at world height 9.3 and sphere edits:
    vtmc_terrain_raycast agrees with the reference on terrain_read_samples() placed at that origin and scale (tight check), is
    byte-identical to vtmc_raycast_device on vtmc_terrain_device_grid, one- and two-sided; a ray straight down onto the plane, away
    from the spheres, hits at world y = 9.3 within float32 rounding (the vertex's block-local position, 0.5 ulp(8) grid units,
    and the point's own rounding, 0.5 ulp(9.3)) with normal (0, 1, 0)."""
    import volumetricterrain_amd as vt
    scale, origin, hgt = 0.5, (-3.25, 1.5, 7.0), 9.3
    rng = np.random.default_rng(61)
    mods = [vt.PlaneModifier(hgt, (-100.0, -100.0), (100.0, 100.0), True), vt.SphereModifier((5.0, 9.0, 15.0), 3.0, True),
            vt.SphereModifier((10.0, 9.5, 25.0), 2.5, False), vt.SphereModifier((12.0, 13.0, 20.0), 2.0, True)]
    k = 600
    cam = np.stack([rng.uniform(-8, 34, k), rng.uniform(14, 30, k), rng.uniform(2, 36, k)], 1)
    tgt = np.stack([rng.uniform(-3, 28, k), rng.uniform(2, 16, k), rng.uniform(7, 31, k)], 1)
    cam[:100] = tgt[:100] + rng.normal(size=(100, 3))   # short rays near the surface and in the spheres
    O, D = cam.astype(np.float32), (tgt - cam).astype(np.float32)
    with vt.Extractor(0) as ex:
        ex.terrain_init(64, 32, 48, scale, origin, 5)
        ex.terrain_update(mods)
        surf = Surface.of_grid(oracle_mod, ex.terrain_read_samples(), origin, scale)
        dg = DeviceGrid.of_terrain(ex)
        assert dg.n == (64, 32, 48)
        for two_sided in (False, True):
            hits = ex.terrain_raycast(O, D, two_sided=two_sided)
            dev = _cast(ex, dg.ptr, dg.n, dg.strides, origin, scale, O, D, two_sided=two_sided)
            assert hits.tobytes() == dev.tobytes(), two_sided
            ref = reference(surf, O, D, two_sided=two_sided)
            label = "scaled terrain two_sided %d" % two_sided
            n_amb = compare(hits, ref, scale, label)
            report(label, k, n_amb, check_tight(hits, ref, surf, label))
            assert n_amb <= 0.005 * k, n_amb
            assert (hits["triangle"] >= 0).sum() > k // 2
        # straight down onto the plane, x in [20, 26], z in [9, 14]: no sphere above or near it
        m = 64
        Ov = np.stack([rng.uniform(20, 26, m), np.full(m, 25.0), rng.uniform(9, 14, m)], 1).astype(np.float32)
        Dv = np.tile(np.float32([0, -1, 0]), (m, 1))
        hits = ex.terrain_raycast(Ov, Dv)
        h32 = np.float32(hgt)
        tol = float(np.spacing(np.float32(8))) * scale + float(np.spacing(h32))
        assert (hits["triangle"] >= 0).all()
        assert np.abs(hits["point"][:, 1].astype(np.float64) - float(h32)).max() <= tol, hits["point"][:, 1]
        assert np.abs(hits["distance"].astype(np.float64) - (25.0 - float(h32))).max() <= tol + float(np.spacing(np.float32(16)))
        assert np.array_equal(hits["point"][:, [0, 2]], Ov[:, [0, 2]])
        assert np.array_equal(hits["normal"], np.tile(np.float32([0, 1, 0]), (m, 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: stream ordering
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fill_then_raycast_on_one_stream_without_a_host_sync():
    """vtmc_density_fill_device_async and vtmc_raycast_device queued back to back on one non-default torch stream, the grid NaN
    before the fill: the hits equal those of the synchronous fill and cast."""
    import torch
    import volumetricterrain_amd as vt
    n, dim = 256, 258
    st = (1, dim, dim * dim)
    prm = vt.density_params("perlin3d", n)
    O, D = _rays_perlin(n, 4096, 71)
    with vt.Extractor(0) as ex:
        g = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
        ex.density_fill_device(prm, [[0, 0, 0]], (dim,) * 3, st, 0, g.data_ptr())
        want = _cast(ex, g.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, O, D)
        assert (want["triangle"] >= 0).sum() > len(O) // 3
        g2 = torch.full((dim ** 3,), float("nan"), dtype=torch.float32, device="cuda")
        d_o, d_d = _device(O), _device(D)
        d_h = torch.zeros(len(O) * RAY_HIT_BYTES, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        ex.density_fill_device(prm, [[0, 0, 0]], (dim,) * 3, st, 0, g2.data_ptr(), stream=s.cuda_stream, wait=False)
        ex.raycast_device(g2.data_ptr(), (n,) * 3, st, (0, 0, 0), 1.0, d_o.data_ptr(), d_d.data_ptr(), len(O), d_h.data_ptr(),
                          stream=s.cuda_stream)
        got = ex.copy_to_host(d_h.data_ptr(), len(O) * RAY_HIT_BYTES, stream=s.cuda_stream).view(vt.RAY_HIT_DTYPE)
        s.synchronize()
        assert got.tobytes() == want.tobytes()
        del s
