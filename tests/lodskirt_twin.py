"""The twin of the level-of-detail skirts (vtmc_lod_skirts): a numpy restatement of the rule LODSKIRT of include/vtmc_lodskirt.h.

face_masks is Flagged over a set of (origin, level); skirts is Quads, Displacement, Records and Offsets over the records of a result, in
float32 (numpy's float32 * + / and sqrt are correctly rounded and never fused).  closure_walk is the check the feature is for: between the
boundary curves of a fine and a coarse node on their shared face, is every point inside a skirt triangle of one of them?
tests/test_terrain_lodskirt.py compares the device against all of it."""
import numpy as np

from volumetricterrain_amd import TRI_DTYPE

f32, f64 = np.float32, np.float64
ALL_FACES = 1
ZERO, EIGHT = 0x00000000, 0x41000000          # the bits of 0.0f and 8.0f


def face_masks(dims, nodes, all_faces=False):
    """The mask byte of every node: bit f (0..5 = -x, +x, -y, +y, -z, +z) when the same-size box beyond face f lies inside the terrain of
    dims = (W, E, H) cells and (unless all_faces) the list holds no node with that origin at the node's level."""
    nodes = np.asarray(nodes, np.int64).reshape(-1, 4)
    have = set(map(tuple, nodes.tolist()))
    out = np.zeros(len(nodes), np.uint8)
    for i, (ox, oy, oz, level) in enumerate(nodes.tolist()):
        n = 8 << level
        for f in range(6):
            o = [ox, oy, oz]
            o[f >> 1] += n if f & 1 else -n
            if o[f >> 1] < 0 or o[f >> 1] + n > dims[f >> 1]:
                continue
            if all_faces or (o[0], o[1], o[2], level) not in have:
                out[i] |= 1 << f
    return out


def corners(records):
    """(positions, normals) of TRI_DTYPE records as (T, 3, 3) float32 arrays [triangle, corner, component]."""
    P = np.stack([records["p0"], records["p1"], records["p2"]], axis=1).astype(f32)
    N = np.stack([records["n0"], records["n1"], records["n2"]], axis=1).astype(f32)
    return P, N


def triangle_masks(records, masks):
    """The face-mask byte of every triangle: bit f when face f of its node is flagged and exactly two positions lie on its plane."""
    P, _ = corners(records)
    bits = np.ascontiguousarray(P).view(np.uint32)
    node_mask = np.asarray(masks, np.uint8)[records["block"]]
    out = np.zeros(len(records), np.uint8)
    for f in range(6):
        on = (bits[:, :, f >> 1] == (EIGHT if f & 1 else ZERO)).sum(axis=1)
        out |= (((node_mask >> f) & 1).astype(bool) & (on == 2)).astype(np.uint8) << f
    return out


def displace(P, N, axis, depth):
    """p' of the vertices (P, N), (n, 3) float32 each, for a face of the axis: depth along -n without its axis component, normalised."""
    u, v = [k for k in range(3) if k != axis]
    depth = f32(depth)
    Q = P.copy()
    with np.errstate(all="ignore"):
        du, dv = -N[:, u], -N[:, v]
        l2 = du * du + dv * dv
        ok = (l2 > 0) & ~np.isinf(l2)
        l = np.sqrt(l2)
        Q[ok, u] = (P[:, u] + (depth * du) / l)[ok]
        Q[ok, v] = (P[:, v] + (depth * dv) / l)[ok]
    return Q


def skirts(records, masks, depth, n_nodes=None):
    """The skirt records of `records` (TRI_DTYPE, result order) for the nodes' face masks: (skirt records, node_offsets, faces), faces[q]
    the face of quad q, whose records are 2 q and 2 q + 1."""
    n_nodes = len(masks) if n_nodes is None else n_nodes
    P, N = corners(records)
    bits = np.ascontiguousarray(P).view(np.uint32)
    tmask = triangle_masks(records, masks)
    tri, face = np.nonzero((tmask[:, None] >> np.arange(6)[None, :]) & 1)        # row-major: triangles in order, faces ascending
    out = np.zeros(2 * len(tri), TRI_DTYPE)
    for f in range(6):
        sel = np.nonzero(face == f)[0]
        if not len(sel):
            continue
        t, axis = tri[sel], f >> 1
        c = np.argmin(bits[t, :, axis] == (EIGHT if f & 1 else ZERO), axis=1)    # the corner off the plane
        a, b = (c + 1) % 3, (c + 2) % 3
        Pa, Na, Pb, Nb = P[t, a], N[t, a], P[t, b], N[t, b]
        Qa, Qb = displace(Pa, Na, axis, depth), displace(Pb, Nb, axis, depth)
        first, second = out[2 * sel], out[2 * sel + 1]
        first["p0"], first["p1"], first["p2"], first["n0"], first["n1"], first["n2"] = Pb, Pa, Qa, Nb, Na, Na
        second["p0"], second["p1"], second["p2"], second["n0"], second["n1"], second["n2"] = Pb, Qa, Qb, Nb, Na, Nb
        first["block"] = second["block"] = records["block"][t]
        out[2 * sel], out[2 * sel + 1] = first, second
    per_node = np.bincount(records["block"][tri], minlength=n_nodes) * 2
    offsets = np.concatenate([[0], np.cumsum(per_node)]).astype(np.int32)
    return out, offsets, face.astype(np.int64)


def quad_faces(skirt_records):
    """The face of every quad of a skirt list, from the records alone: the axis on which all six positions of the quad agree bitwise with
    0.0f or 8.0f; -1 where none or more than one does (a quad along an edge of the node's box)."""
    first, second = skirt_records[0::2], skirt_records[1::2]
    bits = np.stack([first["p0"], first["p1"], first["p2"], second["p0"], second["p1"], second["p2"]], axis=1).astype(f32).view(np.uint32)
    hit = np.stack([(bits[:, :, f >> 1] == (EIGHT if f & 1 else ZERO)).all(axis=1) for f in range(6)], axis=1)
    return np.where(hit.sum(axis=1) == 1, np.argmax(hit, axis=1), -1)


# -- closure: the points between the fine and the coarse boundary curve of a shared face ------------------------------------------------------
def node_cells(nodes, block, P):
    """Node-local positions in the terrain's cells: o + p * 2^level, float64."""
    nodes = np.asarray(nodes, np.int64)
    return nodes[block, :3].astype(f64) + np.asarray(P, f64) * np.ldexp(1.0, nodes[block, 3])[:, None]


def boundary_edges(records, masks):
    """The edges the quads hang from: (triangle, face, a, b) with a, b node-local (n, 3) float32 positions, in the rule's order."""
    P, _ = corners(records)
    bits = np.ascontiguousarray(P).view(np.uint32)
    tri, face = np.nonzero((triangle_masks(records, masks)[:, None] >> np.arange(6)[None, :]) & 1)
    c = np.array([np.argmin(bits[t, :, f >> 1] == (EIGHT if f & 1 else ZERO)) for t, f in zip(tri, face)], np.int64).reshape(-1)
    return tri, face, P[tri, (c + 1) % 3], P[tri, (c + 2) % 3]


def point_segment(p, a, b):
    """The nearest point of each segment a[i]..b[i] to p, 2-D float64: (points, distances)."""
    ab, ap = b - a, p - a
    den = (ab * ab).sum(axis=1)
    t = np.clip(np.where(den > 0, (ap * ab).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
    q = a + t[:, None] * ab
    return q, np.sqrt(((q - p) ** 2).sum(axis=1))


def inside_any(points, tris, eps=1e-6):
    """Is each 2-D point inside one of the 2-D triangles (k, 3, 2), barycentric coordinates >= -eps?  Triangles without area hold nothing."""
    if not len(tris) or not len(points):
        return np.zeros(len(points), bool)
    a, b, c = tris[:, 0][None], tris[:, 1][None], tris[:, 2][None]
    p = points[:, None, :]

    def cross(u, v):
        return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]

    area = cross(b - a, c - a)
    with np.errstate(all="ignore"):
        w0, w1, w2 = cross(b - p, c - p) / area, cross(c - p, a - p) / area, cross(a - p, b - p) / area
        ok = (area != 0) & (w0 >= -eps) & (w1 >= -eps) & (w2 >= -eps)
    return ok.any(axis=1)


def closure_walk(nodes, records, masks, skirt_records, depth, samples=5):
    """In every world face plane that holds boundary edges (the edges quads hang from) of nodes of two adjacent levels L and L + 1:
    `samples` points on every boundary edge of the level-L nodes there; for each its nearest point on the boundary edges of the
    level-(L + 1) nodes in that plane; where that gap is at most depth / 2 coarse cells, `samples` points along the connecting segment,
    each of which must lie inside a skirt triangle, in that plane, of a node of either level (2-D, eps 1e-6).  Returns
    dict(fine_points, skipped, points, uncovered, max_gap): counts, and the largest gap walked, in coarse cells."""
    nodes = np.asarray(nodes, np.int64)
    tri, face, A, B = boundary_edges(records, masks)
    node = records["block"][tri].astype(np.int64)
    A, B = node_cells(nodes, node, A), node_cells(nodes, node, B)                # the terrain's cells
    e_axis, e_level = face >> 1, nodes[node, 3]
    e_plane = A[np.arange(len(A)), e_axis] if len(A) else np.zeros(0)
    sk_tris = (np.stack([node_cells(nodes, skirt_records["block"], skirt_records[k]) for k in ("p0", "p1", "p2")], axis=1)
               if len(skirt_records) else np.zeros((0, 3, 3)))
    sk_level = nodes[skirt_records["block"], 3]
    out = dict(fine_points=0, skipped=0, points=0, uncovered=0, max_gap=0.0)
    ts = (np.arange(samples) + 0.5) / samples
    for axis, plane in sorted(set(zip(e_axis.tolist(), e_plane.tolist()))):
        here = (e_axis == axis) & (e_plane == plane)
        uv = [k for k in range(3) if k != axis]
        for level in sorted(set(e_level[here].tolist())):
            fine, coarse = here & (e_level == level), here & (e_level == level + 1)
            if not coarse.any():
                continue
            scale = float(2 << level)                                            # a coarse cell in the terrain's cells
            Ca, Cb = A[coarse][:, uv], B[coarse][:, uv]
            cover = sk_tris[(sk_tris[:, :, axis] == plane).all(axis=1) & ((sk_level == level) | (sk_level == level + 1))][:, :, uv]
            for a, b in zip(A[fine][:, uv], B[fine][:, uv]):
                for t in ts:
                    p = a + t * (b - a)
                    out["fine_points"] += 1
                    q, d = point_segment(p, Ca, Cb)
                    k = int(np.argmin(d))
                    gap = d[k] / scale
                    if gap > depth / 2:
                        out["skipped"] += 1
                        continue
                    out["max_gap"] = max(out["max_gap"], float(gap))
                    walk = p[None, :] + np.linspace(0.0, 1.0, samples)[:, None] * (q[k] - p)[None, :]
                    out["points"] += samples
                    out["uncovered"] += int((~inside_any(walk, cover)).sum())
    return out
