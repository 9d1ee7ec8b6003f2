"""The twin of the per-vertex ambient occlusion (csrc/terrain_ao.hip): a numpy FP32 restatement of include/vtmc.h's rule, operation by
operation.  Every operand is np.float32 and every line one IEEE operation (numpy's float32 + - * / sqrt floor rint are correctly rounded and
never fused, as the library's are under -ffp-contract=off; np.rint rounds ties to even as rintf does), sums are written in the rule's
association, so test_terrain_ao.py compares bytes.

The grid is indexed [x, y, z] with shape (W+2, E+2, H+2), what Extractor.terrain_read_samples returns.  Vertices are given by their
block (bx, by, bz), their block-local position and their normal, all as the device returned them."""
import numpy as np

f32 = np.float32
MAX_STEPS, MAX_RADIUS_CELLS = 8, 6
LEN = {1: f32(1.0), 2: f32(0.70710678), 3: f32(0.57735027)}


def directions():
    """The 26 (i, j, k, len) in the rule's order: ascending (i+1) + 3*(j+1) + 9*(k+1), the centre left out."""
    out = []
    for code in range(27):
        i, j, k = code % 3 - 1, (code // 3) % 3 - 1, code // 9 - 1
        nz = (i != 0) + (j != 0) + (k != 0)
        if nz:
            out.append((i, j, k, LEN[nz]))
    return out


def tables(radius, voxel_scale, steps):
    """(Rg, h[1..S], fall[1..S]) as the host computes them, entry s - 1 for step s."""
    S = int(steps)
    rg = f32(radius) / f32(voxel_scale)
    h, fall = [], []
    for s in range(1, S + 1):
        frac = f32(s) / f32(S)
        h.append(rg * frac)
        back = f32(s - 1) / f32(S)
        fall.append(f32(1.0) - back)
    return rg, h, fall


def _axis(q, n):
    """(i0, f) of one axis of fetch(): t = clamp(q, 0, n-1) as the rule's two comparisons; i0 = floor(t) capped at n-2; f = t - i0."""
    top = f32(n - 1)
    t = np.where(q < f32(0), f32(0), np.where(q > top, top, q)).astype(f32)
    i0 = np.floor(t).astype(np.int64)
    i0 = np.minimum(i0, n - 2)
    f = t - i0.astype(f32)
    assert f.dtype == f32
    return i0, f


def _lerp(a, b, f):
    d = b - a
    d = d * f
    return a + d


def fetch(grid, qx, qy, qz):
    """The clamp-to-edge trilinear sample of the rule at grid coordinates (qx, qy, qz), arrays of float32."""
    assert grid.dtype == f32
    i0, fx = _axis(qx, grid.shape[0])
    j0, fy = _axis(qy, grid.shape[1])
    k0, fz = _axis(qz, grid.shape[2])
    i1, j1, k1 = i0 + 1, j0 + 1, k0 + 1
    a00 = _lerp(grid[i0, j0, k0], grid[i1, j0, k0], fx)
    a10 = _lerp(grid[i0, j1, k0], grid[i1, j1, k0], fx)
    a01 = _lerp(grid[i0, j0, k1], grid[i1, j0, k1], fx)
    a11 = _lerp(grid[i0, j1, k1], grid[i1, j1, k1], fx)
    b0 = _lerp(a00, a10, fy)
    b1 = _lerp(a01, a11, fy)
    r = _lerp(b0, b1, fz)
    assert r.dtype == f32
    return r


def vertex_ao(grid, blocks, positions, normals, radius, voxel_scale, strength=1.0, steps=4):
    """The occlusion byte of n vertices: blocks (n, 3) their (bx, by, bz), positions and normals (n, 3) float32 as the records hold them."""
    grid = np.asarray(grid)
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    p = np.asarray(positions, f32).reshape(-1, 3)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    n = len(p)
    out = np.full(n, 255, np.uint8)
    if n == 0:
        return out
    _, h, fall = tables(radius, voxel_scale, steps)
    strength = f32(strength)
    g = [(8 * blocks[:, k]).astype(f32) + p[:, k] for k in range(3)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xx = nrm[:, 0] * nrm[:, 0]
        yy = nrm[:, 1] * nrm[:, 1]
        zz = nrm[:, 2] * nrm[:, 2]
        l = xx + yy
        l = l + zz
        l = np.sqrt(l)
        good = (l > f32(0)) & (l < f32(np.inf))
        N = [nrm[:, k] / l for k in range(3)]
        num = np.zeros(n, f32)
        den = np.zeros(n, f32)
        for i, j, k, ln in directions():
            d = (f32(i) * ln, f32(j) * ln, f32(k) * ln)
            c = N[0] * d[0]
            c = c + N[1] * d[1]
            c = c + N[2] * d[2]
            use = good & (c > f32(0))
            if not use.any():
                continue
            sel = np.nonzero(use)[0]
            o = np.zeros(len(sel), f32)
            for s in range(len(h)):
                qx = g[0][sel] + d[0] * h[s]
                qy = g[1][sel] + d[1] * h[s]
                qz = g[2][sel] + d[2] * h[s]
                r = fetch(grid, qx, qy, qz)
                r = np.where(r > f32(0), np.where(r < f32(1), r, f32(1)), f32(0)).astype(f32)
                r = r * fall[s]
                o = np.where(r > o, r, o)
            t = c[sel] * o
            num[sel] = num[sel] + t
            den[sel] = den[sel] + c[sel]
        a = num / den
        a = strength * a
        a = f32(1.0) - a
        a = np.where(a > f32(0), np.where(a < f32(1), a, f32(1)), f32(0)).astype(f32)
        a = a * f32(255.0)
        a = np.rint(a)
    assert a.dtype == f32 and num.dtype == f32 and den.dtype == f32
    out[good] = a[good].astype(np.uint8)
    return out


def soup_vertices(tris, block_xyz):
    """(blocks, positions, normals) of the 3 T vertices of a soup result in the order 3 t + v; tris a TRI_DTYPE array, block_xyz the
    (bx, by, bz) of every block of the dirty list."""
    block_xyz = np.asarray(block_xyz).reshape(-1, 3)
    pos = np.stack([tris["p0"], tris["p1"], tris["p2"]], axis=1).reshape(-1, 3)
    nrm = np.stack([tris["n0"], tris["n1"], tris["n2"]], axis=1).reshape(-1, 3)
    blocks = np.repeat(block_xyz[tris["block"]], 3, axis=0) if len(tris) else np.zeros((0, 3), np.int64)
    return blocks, pos, nrm


def indexed_vertices(verts, vertex_offsets, block_xyz):
    """(blocks, positions, normals) of the V vertices of an indexed result; vertex_offsets the n_blocks + 1 per-block vertex offsets."""
    block_xyz = np.asarray(block_xyz).reshape(-1, 3)
    counts = np.diff(np.asarray(vertex_offsets, np.int64))
    blocks = np.repeat(block_xyz, counts, axis=0) if len(block_xyz) else np.zeros((0, 3), np.int64)
    return blocks, verts["position"], verts["normal"]
