"""The numpy twin of vtmc_stamp_from_mesh: a restatement of include/vtmc.h's rule in its order of operations -- float32 for the distance,
float64 for the sign -- written from the header, not from the kernel.  It takes every triangle at every sample, guided by nothing but the rule's
own comparisons: no tiles, no chunks, no survivor lists, so a stamp that equals it bit for bit shows that the kernel's pruning is exact.

Also the mesh builders the tests use: a box of 12 triangles, an icosphere by subdivision with welded indices, a torus, and the
concatenation of several meshes.  A mesh is (vertices float32 (n, 3), triangles int32 (m, 3))."""
import numpy as np

f32, f64 = np.float32, np.float64
BAND = f32(3.0)


# -- mesh builders ------------------------------------------------------------------------------------------------------------------------
def box(lo, hi):
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    v = np.array([[(hi if i & 1 else lo)[0], (hi if i & 2 else lo)[1], (hi if i & 4 else lo)[2]] for i in range(8)], f32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # -z, +z, -y, +y, -x, +x
    t = [tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))]
    return v, np.array(t, np.int32)


def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 * 4^subdivisions triangles; a midpoint is made once per edge, so the indices are welded and the mesh is closed."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, f64) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        t = [tri for a, b, c in t for ab, bc, ca in [(midpoint(a, b), midpoint(b, c), midpoint(c, a))]
             for tri in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))]
    return (np.array(v) * radius + np.asarray(centre, f64)).astype(f32), np.array(t, np.int32)


def torus(major, minor, n_major=16, n_minor=8, centre=(0.0, 0.0, 0.0)):
    """About the y axis: 2 * n_major * n_minor triangles."""
    u = 2 * np.pi * np.arange(n_major) / n_major
    w = 2 * np.pi * np.arange(n_minor) / n_minor
    ring = major + minor * np.cos(w)
    v = np.stack([np.outer(np.cos(u), ring), np.broadcast_to(minor * np.sin(w), (n_major, n_minor)), np.outer(np.sin(u), ring)], axis=-1).reshape(-1, 3)
    t = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b = i * n_minor + j, ((i + 1) % n_major) * n_minor + j
            c, d = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor, i * n_minor + (j + 1) % n_minor
            t += [(a, b, c), (a, c, d)]
    return (v + np.asarray(centre, f64)).astype(f32), np.array(t, np.int32)


def concat(*meshes):
    v, t, base = [], [], 0
    for mv, mt in meshes:
        v.append(mv)
        t.append(mt + base)
        base += len(mv)
    return np.concatenate(v).astype(f32), np.concatenate(t).astype(np.int32)


def is_closed(triangles):
    """The header's closed-mesh rule: without the triangles that repeat an index, every undirected index pair is used exactly twice."""
    t = np.asarray(triangles)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all())


# -- the rule -----------------------------------------------------------------------------------------------------------------------------
def positions(first, pitch, dims):
    """px [nx], py [ny], pz [nz]: (float)i * h + first[k], float32."""
    h = f32(pitch)
    return tuple(np.arange(n).astype(f32) * h + f32(first[k]) for k, n in enumerate(dims))


def reach_box_grow(tri_v, first, pitch, dims):
    """g of the header: 3.0f * h + 1e-4f * reach, float32."""
    h = f32(pitch)
    reach = max([h] + [abs(f32(first[k])) for k in range(3)] + [abs(f32(dims[k] - 1) * h + f32(first[k])) for k in range(3)] + [np.abs(tri_v).max()])
    g = f32(3.0) * h + f32(1e-4) * f32(reach)
    assert g.dtype == f32
    return g


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _distance(p, a, b, c, lo, hi, g):
    """d of the rule for one triangle at the samples p (three float32 arrays that broadcast); +inf where the triangle does not bid (outside
    its reach box, or NaN)."""
    ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    ap, bp, cp = [p[k] - a[k] for k in range(3)], [p[k] - b[k] for k in range(3)], [p[k] - c[k] for k in range(3)]
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    r_a = (d1 <= 0) & (d2 <= 0)
    r_b = (d3 >= 0) & (d4 <= d3)
    r_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    r_c = (d6 >= 0) & (d5 <= d6)
    r_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    r_bc = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    zero, one = f32(0), f32(1)
    den = one / ((va + vb) + vc)
    wb = np.where(r_a, zero, np.where(r_b, one, np.where(r_ab, d1 / (d1 - d3), np.where(r_c | r_ac, zero, vb * den))))
    wc = np.where(r_a | r_b | r_ab, zero, np.where(r_c, one, np.where(r_ac, d2 / (d2 - d6), vc * den)))
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    on_bc = r_bc & ~(r_a | r_b | r_ab | r_c | r_ac)
    q = [np.where(on_bc, b[k] + w * (c[k] - b[k]), (a[k] + ab[k] * wb) + ac[k] * wc) for k in range(3)]
    cx, cy, cz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    d = np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert d.dtype == f32
    bids = np.ones(np.broadcast(*p).shape, bool)
    for k in range(3):
        bids &= (p[k] >= lo[k] - g) & (p[k] <= hi[k] + g)
    return np.where(bids & ~np.isnan(d), d, f32(np.inf))


def _counts(p, v, lo, hi):
    """True where the triangle covers the sample and lies in front of it; float64 from the float32 inputs."""
    px, py, pz = p
    pxd, pyd, pzd = (x.astype(f64) for x in p)
    odd = np.zeros(np.broadcast(px, py, pz).shape, bool)
    for e in range(3):
        s, t = v[e], v[(e + 1) % 3]
        swap = (t[2] < s[2]) | ((t[2] == s[2]) & (t[1] < s[1]))
        lo_y, lo_z, hi_y, hi_z = np.where(swap, t[1], s[1]), np.where(swap, t[2], s[2]), np.where(swap, s[1], t[1]), np.where(swap, s[2], t[2])
        straddles = (lo_z <= pz) & (pz < hi_z)
        lo_y, lo_z, hi_y, hi_z = (x.astype(f64) for x in (lo_y, lo_z, hi_y, hi_z))
        det = (hi_y - lo_y) * (pzd - lo_z) - (pyd - lo_y) * (hi_z - lo_z)
        odd ^= straddles & (det > 0)
    covers = odd & (lo[1] <= py) & (py <= hi[1])
    v0, v1, v2 = ([x.astype(f64) for x in vv] for vv in v)
    u, w = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
    nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
    t = (nx * (pxd - v0[0]) + ny * (pyd - v0[1])) + nz * (pzd - v0[2])
    front = np.where(px >= hi[0], False, np.where(px < lo[0], True, ((t < 0) & (nx > 0)) | ((t > 0) & (nx < 0))))
    return covers & front


def _span(mask):
    """The index range [i0, i1) that holds every True of a 1-D mask (positions are monotonic, so the Trues are contiguous anyway)."""
    i = np.flatnonzero(mask)
    return (int(i[0]), int(i[-1]) + 1) if len(i) else (0, 0)


def distance_and_sign(vertices, triangles, first, pitch, dims):
    """(dmin float32, inside bool), both indexed [x, y, z].  Every triangle is taken at every sample, one triangle at a time, in index
    order.  The rule's own float comparisons -- the reach box, the straddle of an edge, the y extremes, px < max_x -- are separable per axis,
    so they are evaluated on the three axis vectors, and the arithmetic runs on the box of samples they leave (with the comparisons applied
    again inside it).  No tiles, no chunks, no bound but the rule's."""
    tv = np.asarray(vertices, f32)[np.asarray(triangles)]   # [m, 3 vertices, 3 coordinates]
    tv = np.stack([t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))] for t in tv])   # v0, v1, v2: ascending by (x, then y, then z)
    g = reach_box_grow(tv, first, pitch, dims)
    P = positions(first, pitch, dims)
    dmin = np.full(dims, np.inf, f32)
    inside = np.zeros(dims, bool)
    with np.errstate(all="ignore"):
        for tri in tv:
            v = [[tri[j, k] for k in range(3)] for j in range(3)]
            lo, hi = [tri[:, k].min() for k in range(3)], [tri[:, k].max() for k in range(3)]
            # distance: the samples inside the reach box
            r = [_span((P[k] >= lo[k] - g) & (P[k] <= hi[k] + g)) for k in range(3)]
            if all(b > a for a, b in r):
                sub = tuple(slice(a, b) for a, b in r)
                p = [P[0][sub[0], None, None], P[1][None, sub[1], None], P[2][None, None, sub[2]]]
                dmin[sub] = np.minimum(dmin[sub], _distance(p, v[0], v[1], v[2], lo, hi, g))
            # sign: the samples with px < max_x, py within the y extremes and pz straddled by some edge
            zs = np.zeros(dims[2], bool)
            for e in range(3):
                z0, z1 = sorted((v[e][2], v[(e + 1) % 3][2]))
                zs |= (z0 <= P[2]) & (P[2] < z1)
            r = [_span(P[0] < hi[0]), _span((lo[1] <= P[1]) & (P[1] <= hi[1])), _span(zs)]
            if all(b > a for a, b in r):
                sub = tuple(slice(a, b) for a, b in r)
                p = [P[0][sub[0], None, None], P[1][None, sub[1], None], P[2][None, None, sub[2]]]
                inside[sub] ^= _counts(p, v, lo, hi)
    return dmin, inside


def voxelize(vertices, triangles, first, pitch, dims):
    """The stamp of the rule, float32 indexed [x, y, z]: s = sigma * min(dmin / h, 3)."""
    dmin, inside = distance_and_sign(vertices, triangles, first, pitch, dims)
    with np.errstate(all="ignore"):
        r = dmin / f32(pitch)
    m = np.where(r < BAND, r, BAND).astype(f32)
    return np.where(inside, m, -m).astype(f32)
