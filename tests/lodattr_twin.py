"""The twin of the per-vertex materials and occlusion of a level-of-detail result (csrc/terrain_lodattr.hip): the rule LODATTR of
include/vtmc_lodattr.h, restated by COMPOSING the twins of the two full-resolution rules without touching them.

  Materials   material_twin.vertex_weights with blocks = o // 8 and positions = p * s: its g = (float)(8 * block) + position is then
              (float)o + p * (float)s, the product exact in float32.
  Occlusion   ao_twin.vertex_ao on the node's own sample lattice S_L = S[min(i * s, dim - 1)] with blocks = o // (8 s) and positions = p:
              its g is (float)(o / s) + p, its fetch clamps to the edge of S_L's n_L samples, and Rg stays radius / voxel_scale.
  Skirts      the source map: quad q, records 2q = (b, a, a') and 2q + 1 = (b, a', b'), gets attr(b), attr(a), attr(a), attr(b), attr(a),
              attr(b), with b and a corners 0 and 1 of record 2q and the node its `block`.

Nodes are an (n, 4) array of (origin x, y, z in cells, level); vertices are given by their node index, node-local position and normal as
the device returned them.  tests/test_terrain_lodattr.py compares bytes."""
import numpy as np

import ao_twin
import material_twin

f32 = np.float32
MATERIAL, AO = 0, 1
MESH, SKIRTS = 0, 1
SKIRT_SOURCE = (0, 1, 1, 0, 1, 0)       # corner c of a quad's six takes corner SKIRT_SOURCE[c] of record 2q: 0 is b, 1 is a


def lattice_samples(dim, s):
    """n_L of an axis of dim = cells + 2 samples."""
    return (dim - 2) // s + 2


def lattice(S, level):
    """S_L: the grid S, indexed [x, y, z], subsampled at stride 2^level with the last index on the replicated plane dim - 1."""
    s = 1 << int(level)
    return np.ascontiguousarray(S[np.ix_(*(np.minimum(np.arange(lattice_samples(d, s)) * s, d - 1) for d in S.shape))])


def vertex_materials(layer, dims, nodes, block, positions):
    """The (n, 8) weights of n vertices of nodes[block] at node-local `positions`."""
    nodes = np.asarray(nodes, np.int64).reshape(-1, 4)
    block = np.asarray(block, np.int64)
    p = np.asarray(positions, f32).reshape(-1, 3)
    s = (1 << nodes[block, 3]).astype(f32)
    scaled = p * s[:, None]
    assert scaled.dtype == f32
    return material_twin.vertex_weights(layer, dims, nodes[block, :3] // 8, scaled)


def vertex_ao(S, nodes, block, positions, normals, radius, voxel_scale, strength=1.0, steps=4):
    """The occlusion byte of n vertices of nodes[block]; S the grid indexed [x, y, z]."""
    nodes = np.asarray(nodes, np.int64).reshape(-1, 4)
    block = np.asarray(block, np.int64)
    p = np.asarray(positions, f32).reshape(-1, 3)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    out = np.full(len(p), 255, np.uint8)
    level = nodes[block, 3]
    for lv in sorted(set(level.tolist())):
        sel = np.nonzero(level == lv)[0]
        s = 1 << lv
        out[sel] = ao_twin.vertex_ao(lattice(S, lv), nodes[block[sel], :3] // (8 * s), p[sel], nrm[sel], radius, voxel_scale, strength, steps)
    return out


def soup_vertices(tris):
    """(block, positions, normals) of the 3 T vertices of soup records in the order 3 t + v."""
    pos = np.stack([tris["p0"], tris["p1"], tris["p2"]], axis=1).reshape(-1, 3)
    nrm = np.stack([tris["n0"], tris["n1"], tris["n2"]], axis=1).reshape(-1, 3)
    return np.repeat(tris["block"].astype(np.int64), 3), pos, nrm


def indexed_vertices(verts, vertex_offsets):
    """(block, positions, normals) of the V vertices of an indexed result with its n_nodes + 1 vertex offsets."""
    counts = np.diff(np.asarray(vertex_offsets, np.int64))
    return np.repeat(np.arange(len(counts), dtype=np.int64), counts), verts["position"], verts["normal"]


def skirt_sources(skirt_records):
    """(block, positions, normals) of the two source vertices of every quad, 2 q + c for corner c of record 2q: b, then a."""
    first = skirt_records[0::2]
    pos = np.stack([first["p0"], first["p1"]], axis=1).reshape(-1, 3)
    nrm = np.stack([first["n0"], first["n1"]], axis=1).reshape(-1, 3)
    return np.repeat(first["block"].astype(np.int64), 2), pos, nrm


def spread_to_corners(source_values):
    """The values of the 3 n skirt corners from those of the 2 per quad that skirt_sources lists: the source map."""
    v = np.asarray(source_values)
    per_quad = v.reshape((-1, 2) + v.shape[1:])
    return per_quad[:, list(SKIRT_SOURCE)].reshape((-1,) + v.shape[1:])


def skirt_materials(layer, dims, nodes, skirt_records):
    return spread_to_corners(vertex_materials(layer, dims, nodes, *skirt_sources(skirt_records)[:2]))


def skirt_ao(S, nodes, skirt_records, radius, voxel_scale, strength=1.0, steps=4):
    return spread_to_corners(vertex_ao(S, nodes, *skirt_sources(skirt_records), radius, voxel_scale, strength, steps))
