"""The twin of the level-of-detail extract (vtmc_terrain_extract_lod): a numpy restatement of include/vtmc.h's rule.

select_nodes is the selection descent in float64 (numpy's float64 + - * / are correctly rounded and never fused); node_tiles builds
every node's 10x10x10 tile from a sample grid by the clamp rule.  The tiles feed oracle.extract_tiles, so the CPU oracle stays the
yardstick for the mesh: the twin restates only the front end.  tests/test_terrain_lod.py compares the device against both."""
import numpy as np

f32, f64 = np.float32, np.float64
MAX_LEVEL = 7


def node_cells(level):
    return 8 << level


def viewer_cells(origin, scale, viewer):
    """c of the rule: the viewer in cells, from the float32 values the library is handed, in double."""
    return [(f64(f32(viewer[k])) - f64(f32(origin[k]))) / f64(f32(scale)) for k in range(3)]


def distance(c, o, n):
    """d of the rule: the Chebyshev distance from c to the box [o, o + n], 0 inside."""
    d = f64(0.0)
    for k in range(3):
        below, above = f64(o[k]) - c[k], c[k] - (f64(o[k]) + f64(n))
        if below > d:
            d = below
        if above > d:
            d = above
    return d


def select_nodes(dims, origin, scale, viewer, max_level, split):
    """The node list: an (n, 4) int32 array of (origin x, y, z in cells, level) in the depth-first order of the descent.  dims = (W, E, H)
    cells, each a multiple of 8 * 2^max_level."""
    n_root = node_cells(max_level)
    assert 0 <= max_level <= MAX_LEVEL and all(d > 0 and d % n_root == 0 for d in dims)
    c, split = viewer_cells(origin, scale, viewer), f64(f32(split))
    out = []

    def descend(o, level):
        n = node_cells(level)
        if level > 0 and distance(c, o, n) < split * f64(n):
            h = n // 2
            for k in range(8):
                descend((o[0] + h * (k & 1), o[1] + h * ((k >> 1) & 1), o[2] + h * ((k >> 2) & 1)), level - 1)
        else:
            out.append((o[0], o[1], o[2], level))

    for rz in range(dims[2] // n_root):
        for ry in range(dims[1] // n_root):
            for rx in range(dims[0] // n_root):
                descend((rx * n_root, ry * n_root, rz * n_root), max_level)
    return np.array(out, np.int32).reshape(-1, 4)


def node_tiles(S, nodes, clamp=True):
    """The tiles of the nodes, (n, 1000) float32, x fastest: T[i, j, k] = S[min(o + (i, j, k) * 2^level, dim - 1)] for the grid S indexed
    [x, y, z].  clamp=False is the twin that clamps nothing, for tests that must be able to fail: past the grid it reads the linear
    extrapolation of the last two sample planes instead of the last plane again."""
    S = np.asarray(S, f32)
    if not clamp:
        for axis in range(3):
            last, before = np.take(S, [-1], axis=axis), np.take(S, [-2], axis=axis)
            S = np.concatenate([S] + [last + (last - before) * f32(m) for m in range(1, 129)], axis=axis)
    dim = S.shape
    out = np.empty((len(nodes), 1000), f32)
    for n, (ox, oy, oz, level) in enumerate(np.asarray(nodes, np.int64)):
        s = 1 << int(level)
        ix, iy, iz = (np.minimum(o + np.arange(10) * s, d - 1) for o, d in ((ox, dim[0]), (oy, dim[1]), (oz, dim[2])))
        out[n] = S[np.ix_(ix, iy, iz)].transpose(2, 1, 0).ravel()      # [k, j, i] in memory: i + 10 j + 100 k
    return out


def coverage(dims, nodes):
    """How many nodes cover each 8^3-cell block of the terrain: an array of shape (W/8, E/8, H/8); all ones when the nodes tile it."""
    count = np.zeros(tuple(d // 8 for d in dims), np.int64)
    for ox, oy, oz, level in np.asarray(nodes, np.int64):
        b = 1 << int(level)
        assert ox >= 0 and oy >= 0 and oz >= 0 and ox + 8 * b <= dims[0] and oy + 8 * b <= dims[1] and oz + 8 * b <= dims[2]
        count[ox // 8:ox // 8 + b, oy // 8:oy // 8 + b, oz // 8:oz // 8 + b] += 1
    return count


def level_map(dims, nodes):
    """The level of the node covering each 8^3-cell block (the nodes must tile the terrain)."""
    level = np.full(tuple(d // 8 for d in dims), -1, np.int64)
    for ox, oy, oz, lv in np.asarray(nodes, np.int64):
        b = 1 << int(lv)
        level[ox // 8:ox // 8 + b, oy // 8:oy // 8 + b, oz // 8:oz // 8 + b] = lv
    return level


def max_face_level_step(dims, nodes):
    """The largest difference in level between two nodes that share (part of) a face."""
    lv = level_map(dims, nodes)
    assert (lv >= 0).all()
    return max(int(np.abs(np.diff(lv, axis=a)).max(initial=0)) for a in range(3))


def world_positions(origin, scale, nodes, block, local_positions):
    """terrain origin + (o + p * 2^level) * voxel scale in float64, (o, level) = nodes[block]; local_positions (n, 3)."""
    nodes = np.asarray(nodes, np.int64)
    o, s = nodes[block, :3].astype(f64), np.ldexp(1.0, nodes[block, 3])[:, None]
    return np.array([f64(f32(v)) for v in origin]) + (o + np.asarray(local_positions, f64) * s) * f64(f32(scale))
