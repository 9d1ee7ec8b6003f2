"""The twin of the surface scatter (csrc/terrain_scatter.hip): a numpy restatement of include/vtmc.h's rule, operation by operation.
Every float operand is np.float32 and every line one IEEE operation (numpy's float32 + - * / sqrt floor are correctly rounded and never
fused, as the library's are under -ffp-contract=off); the hash runs in np.uint64, whose array arithmetic wraps.  So
test_terrain_scatter.py compares bytes.

The twin works from 76-byte records (a TRI_DTYPE array, `block` an index into block_xyz) and the per-block triangle offsets; an indexed
result is first turned into records with oracle.deindex's gather (records_of_indexed).  The material byte comes from
material_twin.vertex_weights."""
import numpy as np

import material_twin
from volumetricterrain_amd._lib import INSTANCE_DTYPE, TRI_DTYPE

f32, u64, u32 = np.float32, np.uint64, np.uint32
MAX_DENSITY_CELLS, MAX_PER_TRIANGLE = 8.0, 8
G = u64(0x9E3779B97F4A7C15)


def fin(z):
    z = np.asarray(z, u64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        z = z ^ (z >> u64(31))
    return z


def step(k, w):
    with np.errstate(over="ignore"):
        return fin((np.asarray(k, u64) ^ np.asarray(w, u64)) + G)


def word(k, i, d):
    return step(k, u64((int(i) << 8) | int(d)))


def uniform(k, i, d):
    return (word(k, i, d) >> u64(40)).astype(u32).astype(f32) * f32(2.0 ** -24)


def records_of_indexed(verts, idx, voffs, toffs):
    """An indexed mesh as 76-byte records in the result's triangle order: oracle.deindex's gather."""
    out = np.zeros(len(idx), TRI_DTYPE)
    block = np.repeat(np.arange(len(toffs) - 1, dtype=np.int32), np.diff(toffs))
    g = idx + np.asarray(voffs)[block][:, None]
    for c in range(3):
        out["p%d" % c] = verts["position"][g[:, c]]
        out["n%d" % c] = verts["normal"][g[:, c]]
    out["block"] = block
    return out


def triangle_keys(tris, blocks, seed):
    """k of every triangle: fin(seed + G), then the bits of g[c][a] = ((float)(8 b_a) + p[c][a]) + 0.0f, corner by corner."""
    with np.errstate(over="ignore"):
        k = np.broadcast_to(fin(np.array([seed], u64) + G), (len(tris),)).copy()
    base = (8 * blocks).astype(f32)
    for c in range(3):
        p = tris["p%d" % c]
        for a in range(3):
            g = base[:, a] + p[:, a]
            g = g + f32(0.0)
            k = step(k, np.ascontiguousarray(g).view(u32).astype(u64))
    return k


def scatter(tris, toffs, block_xyz, scale, origin, density, min_up=-1.0, max_up=1.0, min_y=-np.inf, max_y=np.inf, material_channel=-1, seed=0,
            layer=None, dims=None):
    """(instances, block_offsets, info) of a result: tris its records, toffs the B + 1 per-block triangle offsets, block_xyz the (bx, by,
    bz) of its blocks; layer / dims = (W, E, H) the material layer when material_channel >= 0.  info: per triangle L, lam (0 where the
    triangle yields nothing), n (candidates) and kept (survivors), and `weights`, the material byte of every instance (or None)."""
    block_xyz = np.asarray(block_xyz, np.int64).reshape(-1, 3)
    T = len(tris)
    blocks = block_xyz[tris["block"]] if T else np.zeros((0, 3), np.int64)
    p0, p1, p2 = tris["p0"], tris["p1"], tris["p2"]
    n0, n1, n2 = tris["n0"], tris["n1"], tris["n2"]
    scale = f32(scale)
    origin = np.asarray(origin, f32)
    with np.errstate(all="ignore"):
        e1 = p1 - p0
        e2 = p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        L = cx * cx + cy * cy
        L = L + cz * cz
        L = np.sqrt(L)
        good = (L > f32(0)) & (L < f32(np.inf))
        up = cy / L
        good &= (f32(min_up) <= up) & (up <= f32(max_up))
        s2 = scale * scale
        dc = f32(density) * s2
        lam = f32(0.5) * L
        lam = lam * dc
        fl = np.floor(lam)
        k = triangle_keys(tris, blocks, seed)
        frac = lam - fl
        n = np.minimum(fl, f32(MAX_PER_TRIANGLE)).astype(np.int64) + (uniform(k, 0, 0) < frac)
    assert L.dtype == f32 and lam.dtype == f32 and frac.dtype == f32 and dc.dtype == f32
    n = np.where(good, np.minimum(n, MAX_PER_TRIANGLE), 0)
    lam = np.where(good, lam, f32(0))
    d1, d2 = n1 - n0, n2 - n0
    base = (8 * blocks).astype(f32)
    parts, weights = [], []
    for i in range(MAX_PER_TRIANGLE):
        sel = np.nonzero(n > i)[0]
        if not len(sel):
            break
        ks = k[sel]
        u, v = uniform(ks, i, 1), uniform(ks, i, 2)
        flip = u + v > f32(1.0)
        u = np.where(flip, f32(1.0) - u, u)
        v = np.where(flip, f32(1.0) - v, v)
        with np.errstate(all="ignore"):
            q = p0[sel] + e1[sel] * u[:, None]
            q = q + e2[sel] * v[:, None]
            nrm = n0[sel] + d1[sel] * u[:, None]
            nrm = nrm + d2[sel] * v[:, None]
            g = base[sel] + q
            g = g * scale
            pos = origin[None, :] + g
        assert q.dtype == f32 and nrm.dtype == f32 and pos.dtype == f32
        keep = (f32(min_y) <= pos[:, 1]) & (pos[:, 1] <= f32(max_y))
        w = None
        if material_channel >= 0:
            w = material_twin.vertex_weights(layer, dims, blocks[sel], q)[:, material_channel]
            keep &= uniform(ks, i, 3) * f32(255.0) < w.astype(f32)
        part = np.zeros(int(keep.sum()), INSTANCE_DTYPE)
        part["position"], part["normal"] = pos[keep], nrm[keep]
        part["triangle"] = sel[keep]
        part["rnd"] = (word(ks[keep], i, 4) >> u64(32)).astype(u32)
        parts.append((part, np.full(len(part), i)))
        weights.append(w[keep] if w is not None else None)
    if parts:
        inst = np.concatenate([p for p, _ in parts])
        order = np.argsort(inst["triangle"].astype(np.int64) * MAX_PER_TRIANGLE + np.concatenate([i for _, i in parts]), kind="stable")
        inst = inst[order]
        weights = np.concatenate(weights)[order] if material_channel >= 0 else None
    else:
        inst, weights = np.zeros(0, INSTANCE_DTYPE), (np.zeros(0, np.uint8) if material_channel >= 0 else None)
    offsets = np.searchsorted(inst["triangle"], np.asarray(toffs, np.int64), side="left").astype(np.int32)
    kept = np.bincount(inst["triangle"], minlength=T) if T else np.zeros(0, np.int64)
    return inst, offsets, dict(L=L, lam=lam, n=n, kept=kept, weights=weights)
