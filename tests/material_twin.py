"""The twin of the material layer (csrc/terrain_material.hip): a numpy FP32 restatement of include/vtmc.h's rule, operation by operation.
Every operand is np.float32, every line one IEEE operation (numpy's float32 + - * / sqrt floor rint are correctly rounded and never fused,
as the library's are under -ffp-contract=off; np.rint rounds ties to even as rintf does), so test_terrain_material.py compares bytes.

A layer is a (C, C, C, 8) uint8 array indexed [k, j, i, channel], what Extractor.material_read returns.  A stroke is the tuple
(center, radius, channel, strength), the arguments of vt.MaterialStroke in their order."""
import numpy as np

f32 = np.float32
CHANNELS = 8


def initial(C):
    """The layer after material_init: every texel (255,0,0,0, 0,0,0,0)."""
    layer = np.zeros((C, C, C, CHANNELS), np.uint8)
    layer[..., 0] = 255
    return layer


def quantise(colors):
    """(uint8)rintf(clamp(c, 0, 1) * 255.0f) of every float of `colors`, any shape."""
    c = np.asarray(colors, f32)
    c = np.maximum(c, f32(0))
    c = np.minimum(c, f32(1))
    v = c * f32(255)
    v = np.rint(v)
    return v.astype(np.uint8)


def set_control_map(layer, colors, group):
    """The layer with `colors` (C^3 x 4 floats, x fastest) quantised into the four bytes of group 1 or 2."""
    C = layer.shape[0]
    out = layer.copy()
    out[..., 4 * (group - 1):4 * group] = quantise(np.asarray(colors, f32).reshape(C, C, C, 4))
    return out


def texel_centres(C, dims, scale, origin):
    """World position of the texel centres per axis: ((float)i + 0.5f) * ts + origin, ts = ((float)cells * scale) / (float)C."""
    p = []
    for k in range(3):
        world = f32(dims[k]) * f32(scale)
        ts = world / f32(C)
        i = np.arange(C).astype(f32)
        i = i + f32(0.5)
        i = i * ts
        p.append(i + f32(origin[k]))
    return p


def stroke_weights(C, stroke, dims, scale, origin):
    """w of every texel [k, j, i] under one stroke."""
    c, r, _, s = stroke
    c, r, s = np.asarray(c, f32), f32(r), f32(s)
    px, py, pz = texel_centres(C, dims, scale, origin)
    with np.errstate(over="ignore"):
        dx = px[None, None, :] - c[0]
        dy = py[None, :, None] - c[1]
        dz = pz[:, None, None] - c[2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        q = xx + yy
        q = q + zz
        d = np.sqrt(q)
        t = d / r
        t = f32(1) - t
        t = t + t
        t = np.maximum(t, f32(0))
        t = np.minimum(t, f32(1))
        w = s * t
    assert w.dtype == f32
    return w


def paint(layer, strokes, dims, scale, origin):
    """The layer after the strokes, applied in order; dims = (W, E, H) cells."""
    C = layer.shape[0]
    out = layer.copy()
    for stroke in strokes:
        w = stroke_weights(C, stroke, dims, scale, origin)
        T = np.zeros(CHANNELS, f32)
        T[stroke[2]] = f32(255)
        v = out.astype(f32)
        g = T - v
        g = g * w[..., None]
        v = v + g
        v = np.rint(v)
        assert v.dtype == f32 and v.min() >= 0 and v.max() <= 255
        out = np.where((w != 0)[..., None], v.astype(np.uint8), out)
    return out


def _axis(block, position, cells, C):
    """(i0, i1, f) of one axis: g = (float)(8 * b) + p; t = g * s - 0.5; the texel below, wrapped (Repeat), the next one, the weight."""
    s = f32(C) / f32(cells)
    g = (8 * np.asarray(block, np.int64)).astype(f32)
    g = g + np.asarray(position, f32)
    t = g * s
    t = t - f32(0.5)
    fl = np.floor(t)
    i0 = fl.astype(np.int64)
    f = t - i0.astype(f32)
    i0 = np.mod(i0, C)          # ((i0 % C) + C) % C of C's truncating %
    i1 = np.mod(i0 + 1, C)
    assert f.dtype == f32
    return i0, i1, f


def _lerp(a, b, f):
    d = b - a
    d = d * f[:, None]
    return a + d


def vertex_weights(layer, dims, blocks, positions):
    """The (n, 8) weights of n vertices: blocks (n, 3) their (bx, by, bz), positions (n, 3) float32 block-local, dims = (W, E, H)."""
    C = layer.shape[0]
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    positions = np.asarray(positions, f32).reshape(-1, 3)
    i0, i1, fx = _axis(blocks[:, 0], positions[:, 0], dims[0], C)
    j0, j1, fy = _axis(blocks[:, 1], positions[:, 1], dims[1], C)
    k0, k1, fz = _axis(blocks[:, 2], positions[:, 2], dims[2], C)
    m = layer.astype(f32)
    a00 = _lerp(m[k0, j0, i0], m[k0, j0, i1], fx)
    a10 = _lerp(m[k0, j1, i0], m[k0, j1, i1], fx)
    a01 = _lerp(m[k1, j0, i0], m[k1, j0, i1], fx)
    a11 = _lerp(m[k1, j1, i0], m[k1, j1, i1], fx)
    b0 = _lerp(a00, a10, fy)
    b1 = _lerp(a01, a11, fy)
    q = _lerp(b0, b1, fz)
    q = np.rint(q)
    assert q.dtype == f32
    return q.astype(np.uint8)
