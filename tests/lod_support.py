"""What the level-of-detail tests share (test_terrain_lod.py, test_terrain_lodskirt.py, test_terrain_lod_edges.py): the debug read of the
gathered tiles, the oracle's welded form of a tile list, the brute-force restatements of the face masks, the properties of a skirt list, the
closure walk with its caps, the comparison of the device's skirts with the twin, and the poisoning of the device's skirt buffers between
two runs.  The helpers that need a world take its dims as an argument and read no module constant.  No tests here."""
import ctypes

import numpy as np

from volumetricterrain_amd import _lib
import lod_twin
import lodskirt_twin as twin

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lod_tiles(ex, n_nodes):
    out = np.zeros((n_nodes, 1000), f32)
    assert ex._L.vtmc_debug_lod_tiles(ex._h, out.ctypes.data, out.size) == _lib.OK
    return out


def oracle_indexed_soup(oracle_mod, tiles):
    """The oracle's welded mesh of every tile (a tile is a grid of one block), de-indexed into records in list order."""
    out = []
    for n, t in enumerate(tiles):
        soup = oracle_mod.deindex(*oracle_mod.extract_grid_indexed(np.ascontiguousarray(t.reshape(10, 10, 10).transpose(2, 1, 0))))
        soup["block"] = n
        out.append(soup)
    return np.concatenate(out)


def brute_masks(dims, nodes, all_faces=False):
    """Flagged, restated over the level of every 8^3-cell block: the same-size box beyond a face lies inside the terrain and (unless
    all_faces) is not one node of the node's own level -- a box aligned to its size whose blocks all have level L is a node of level L."""
    lv = lod_twin.level_map(dims, nodes)
    out = np.zeros(len(nodes), np.uint8)
    for i, (ox, oy, oz, level) in enumerate(np.asarray(nodes, np.int64).tolist()):
        n = 8 << level
        for f in range(6):
            lo = [ox, oy, oz]
            lo[f >> 1] += n if f & 1 else -n
            if lo[f >> 1] < 0 or lo[f >> 1] + n > dims[f >> 1]:
                continue
            box = lv[tuple(slice(lo[k] // 8, (lo[k] + n) // 8) for k in range(3))]
            if all_faces or not (box == level).all():
                out[i] |= 1 << f
    return out


def interior_masks(dims, nodes):
    nodes = np.asarray(nodes, np.int64)
    out = np.zeros(len(nodes), np.uint8)
    for k in range(3):
        size = 8 << nodes[:, 3]
        out |= ((nodes[:, k] > 0).astype(np.uint8) << (2 * k)) | ((nodes[:, k] + size < dims[k]).astype(np.uint8) << (2 * k + 1))
    return out


def check_skirt_properties(skirt, faces, depth):
    """The properties of a skirt list, of the twin or of the device; returns (quads, quads with a source edge, second triangles inwards)."""
    assert len(skirt) == 2 * len(faces) and len(faces) > 50
    first, second = skirt[0::2], skirt[1::2]
    axis = faces >> 1
    want = np.where(faces & 1, twin.EIGHT, twin.ZERO).astype(np.uint32)
    rows = np.arange(len(faces))
    for rec in (first, second):
        for k in ("p0", "p1", "p2"):
            assert np.array_equal(bits(rec[k].astype(f32))[rows, axis], want), k                 # the face-axis coordinate is bitwise 0 or 8
    assert np.array_equal(twin.quad_faces(skirt), faces)
    # every displaced vertex lies `depth` from its source within 1e-5, or on it
    for moved, source in ((first["p2"], first["p1"]), (second["p2"], second["p0"])):
        d = np.sqrt(((moved.astype(np.float64) - source.astype(np.float64)) ** 2).sum(axis=1))
        assert ((np.abs(d - depth) <= 1e-5) | (d == 0)).all(), np.abs(d - depth)[d != 0].max()
    assert first["p2"].tobytes() == second["p1"].tobytes()                                       # a' is one vertex
    # orientation: (b, a, a') faces out of the node through the face wherever the source edge has a length
    outward = np.where(faces & 1, 1.0, -1.0)

    def normal_out(rec):
        p0, p1, p2 = (rec[k].astype(np.float64) for k in ("p0", "p1", "p2"))
        return np.cross(p1 - p0, p2 - p0)[rows, axis] * outward

    with_edge = (first["p0"] != first["p1"]).any(axis=1)
    assert (normal_out(first)[with_edge] > 0).all()
    inwards = int((normal_out(second)[with_edge] <= 0).sum())
    assert inwards <= 0.10 * with_edge.sum(), (inwards, int(with_edge.sum()))                  # a cap, not a measurement
    return len(faces), int(with_edge.sum()), inwards


def check_closure(nodes, records, masks, skirt, depth, min_fine_points=200, min_points=1000):
    """The closure walk and its caps.  The floors say that the walk had something to walk on: a world with fewer seam edges states its own."""
    walk = twin.closure_walk(nodes, records, masks, skirt, depth)
    print("closure at depth %g: %s" % (depth, walk))
    assert walk["fine_points"] > min_fine_points and walk["points"] > min_points
    assert walk["skipped"] <= 0.05 * walk["fine_points"], walk                                  # a cap
    assert walk["uncovered"] == 0, walk
    empty = twin.closure_walk(nodes, records, masks, skirt[:0], depth)
    assert empty["points"] == walk["points"] and empty["uncovered"] > 0.2 * empty["points"], empty   # the walk can fail
    return walk


def device_records(ex, oracle_mod, indexed):
    """The records of the result the context holds (indexed: de-indexed in order)."""
    if not indexed:
        return ex.read_triangles()[0]
    return oracle_mod.deindex(*ex.read_indexed_mesh())


def assert_skirts_match_the_twin(ex, oracle_mod, dims, nodes, indexed, depth, all_faces=False):
    """lod_skirts on the result the context holds against the twin fed with the device's own records.  Returns (records, device skirts,
    masks, the number of displaced components whose bits differ from the twin's)."""
    records = device_records(ex, oracle_mod, indexed)
    masks = twin.face_masks(dims, nodes, all_faces)
    want, want_offsets, faces = twin.skirts(records, masks, depth)
    n = ex.lod_skirts(depth, all_faces)
    assert n == len(want) and ex.lodskirt_info() == (len(nodes), int((masks != 0).sum()), n)
    assert np.array_equal(ex.lodskirt_masks(), masks)
    got, offsets = ex.lodskirt_read()
    assert offsets.dtype == np.int32 and np.array_equal(offsets, want_offsets) and np.array_equal(got["block"], want["block"])
    for k in ("n0", "n1", "n2"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k                                    # all normals: bitwise
    first, second = (got[0::2], want[0::2]), (got[1::2], want[1::2])
    for (g, w), k in ((first, "p0"), (first, "p1"), (second, "p0")):
        assert np.array_equal(bits(g[k]), bits(w[k])), k                                         # the copied positions: bitwise
    differ = 0
    for (g, w), k in ((first, "p2"), (second, "p1"), (second, "p2")):
        assert np.array_equal(np.isnan(g[k]), np.isnan(w[k])) and np.allclose(g[k], w[k], rtol=0.0, atol=1e-5, equal_nan=True), k
        differ += int((bits(g[k]) != bits(w[k])).sum())
        rows = np.arange(len(faces))
        assert np.array_equal(bits(g[k])[rows, faces >> 1], bits(w[k])[rows, faces >> 1])       # the face-axis component is copied
    return records, got, masks, differ


POISON = 0xA5


def poison_skirts(ex):
    """Overwrites the skirt records and the node offsets the context holds (the skirts must be current) with POISON bytes on the device.
    The record buffer only ever grows and a later lod_skirts writes into it again, so without this a pass that leaves records unwritten
    reads back the bytes an earlier, correct pass left there.  Poisons as many records as the context has ever held at once: the buffer
    is at least that large.  The skirts of the context are garbage afterwards; run lod_skirts again before reading them."""
    d_tris, d_offsets, n = ex.device_lodskirts()
    nodes = ex.lodskirt_info()[0]
    seen = ex._poisoned_records = max(getattr(ex, "_poisoned_records", 0), n)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    if seen and d_tris:
        assert hip.hipMemset(d_tris, POISON, 76 * seen) == 0
    assert hip.hipMemset(d_offsets, POISON, 4 * (nodes + 1)) == 0
    assert hip.hipDeviceSynchronize() == 0
    got, offsets = ex.lodskirt_read()
    assert (got.view(np.uint8) == POISON).all() and (offsets.view(np.uint8) == POISON).all()    # the poison is where the next run writes
