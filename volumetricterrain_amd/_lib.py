"""ctypes binding of libvtmc.so -- the same C ABI a C# host binds with [DllImport].

There is no CPU fallback: if the library is missing it is built with hipcc; if that fails, or the
library cannot be loaded, importing raises.  Creating a context without a HIP device fails with
VtmcError (vtmc_create returns VTMC_ERR_DEVICE).
"""
import ctypes
import os
import sys

import numpy as np

from . import build as _build

TRI_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("p2", "<f4", 3),
                      ("n0", "<f4", 3), ("n1", "<f4", 3), ("n2", "<f4", 3),
                      ("block", "<i4")])
assert TRI_DTYPE.itemsize == 76  # CSTriangle.stride, VoxelTerrain.cs:36

VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3)])   # vtmc_vertex
assert VERTEX_DTYPE.itemsize == 24
# vtmc_ray_hit: one answer of vtmc_terrain_raycast / vtmc_raycast_device
RAY_HIT_DTYPE = np.dtype([("distance", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("barycentric", "<f4", 2),
                          ("block", "<i4", 3), ("cell", "<i4"), ("triangle", "<i4")])
assert RAY_HIT_DTYPE.itemsize == 56
RAY_TWO_SIDED = 1
TERRAIN_SAVE_EXACT, TERRAIN_LOAD_NO_EXTRACT = 1, 1
# vtmc_sphere_hit: one answer of vtmc_terrain_spherecast / _closest_point and their _device forms
SPHERE_HIT_DTYPE = np.dtype([("distance", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("block", "<i4", 3), ("cell", "<i4"),
                             ("triangle", "<i4")])
assert SPHERE_HIT_DTYPE.itemsize == 48
SPHERE_MAX_RADIUS_CELLS = 16
# vtmc_instance: one instance of vtmc_scatter_surface
INSTANCE_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("triangle", "<u4"), ("rnd", "<u4")])
assert INSTANCE_DTYPE.itemsize == 32
# vtmc_fragment: one record of vtmc_terrain_fragments
FRAGMENT_DTYPE = np.dtype([("seed", "<i4", 3), ("lo", "<i4", 3), ("hi", "<i4", 3), ("n_samples", "<i4"), ("stamp_id", "<i4"), ("reserved", "<i4")])
assert FRAGMENT_DTYPE.itemsize == 48
OUTPUT_SOUP, OUTPUT_INDEXED = 0, 1

OK = 0
ERR_INVALID_ARG, ERR_DIMS, ERR_CAPACITY, ERR_DEVICE, ERR_NO_RESULT, ERR_TOO_LARGE = -1, -2, -3, -4, -5, -6
FLAG_WANT_CASES, FLAG_NO_DENSE_PATH = 1, 2

# every symbol include/vtmc.h declares (tests/test_abi_symbols.py checks the header against this)
SYMBOLS = [
    "vtmc_version", "vtmc_create", "vtmc_destroy", "vtmc_last_error", "vtmc_extract_blocks",
    "vtmc_extract_grid", "vtmc_extract_grid_sharded", "vtmc_read_triangles", "vtmc_read_cases",
    "vtmc_last_counts", "vtmc_extract_volumes_device", "vtmc_device_results",
    "vtmc_reserve_triangles", "vtmc_last_stage_ms", "vtmc_set_tuning", "vtmc_density_fill_device",
    "vtmc_terrain_init", "vtmc_terrain_update", "vtmc_terrain_dirty_blocks", "vtmc_terrain_read_samples",
    "vtmc_terrain_device_grid", "vtmc_copy_volume_counts_device", "vtmc_density_fill_device_async",
    "vtmc_set_output_mode", "vtmc_last_vertex_count", "vtmc_read_indexed_mesh", "vtmc_device_indexed_results",
    "vtmc_comm_unique_id", "vtmc_comm_init_rank", "vtmc_comm_destroy", "vtmc_comm_share", "vtmc_allgather_volume_counts",
    "vtmc_copy_to_host", "vtmc_chunk_write", "vtmc_chunk_read",
    "vtmc_extract_volumes_device_async", "vtmc_extract_finish", "vtmc_last_fill_ms", "vtmc_context_stream", "vtmc_release_streams", "vtmc_last_placement",
    "vtmc_terrain_raycast", "vtmc_raycast_device",
    "vtmc_terrain_set_history", "vtmc_terrain_undo", "vtmc_terrain_redo", "vtmc_terrain_history",
    "vtmc_terrain_spherecast", "vtmc_terrain_closest_point", "vtmc_spherecast_device", "vtmc_closest_point_device",
    "vtmc_terrain_save", "vtmc_terrain_load", "vtmc_terrain_write_samples",
    "vtmc_stamp_create", "vtmc_stamp_capture", "vtmc_stamp_info", "vtmc_stamp_read", "vtmc_stamp_destroy",
    "vtmc_stamp_from_mesh",
    "vtmc_material_init", "vtmc_material_set_control_map", "vtmc_material_write", "vtmc_material_read", "vtmc_material_paint",
    "vtmc_material_vertices", "vtmc_material_read_vertices", "vtmc_material_device_results",
    "vtmc_ao_vertices", "vtmc_ao_read_vertices", "vtmc_ao_device_results",
    "vtmc_scatter_surface", "vtmc_scatter_read", "vtmc_scatter_device_results",
    "vtmc_terrain_extract_lod", "vtmc_terrain_lod_nodes",
    "vtmc_terrain_fragments",
]
COMM_ID_BYTES = 128

MOD_PLANE, MOD_SPHERE, MOD_CYLINDER, MOD_HEIGHTMAP = 0, 1, 2, 3
MOD_SMOOTH, MOD_FLATTEN = 4, 5   # sculpt brushes (not in the reference)
MOD_STAMP = 9                     # pastes a stamp (vtmc_stamp_*) through a rotation and a pitch
STAMP_MIN_DIM, STAMP_MAX_DIM, STAMP_MAX_SAMPLES = 2, 1026, 1 << 27
MESH_MAX_TRIANGLES, MESH_BAND, MESH_TRUST_CLOSED = 1 << 20, 3.0, 1   # vtmc_stamp_from_mesh: the most triangles, the band in stamp samples, the flag
MOD_PATH = 10                     # union of tapered capsules over a segment soup: rivers, tunnels, roads in one pass
PATH_CHUNK, PATH_MAX_SEGMENTS = 256, 65536   # csrc/terrain_path.h: segments a workgroup prunes at a time; the most a modifier may hold
MATERIAL_CHANNELS, MATERIAL_MAX_STROKES = 8, 4096   # the material layer: bytes per texel and per vertex; the most strokes of one paint call
AO_MAX_STEPS, AO_MAX_RADIUS_CELLS = 8, 6   # vtmc_ao_vertices: the most steps of a march; the largest radius in cells (radius / voxel_scale)
SCATTER_MAX_DENSITY_CELLS, SCATTER_MAX_PER_TRIANGLE = 8.0, 8   # vtmc_scatter_surface: the largest density * voxel_scale^2; the most instances of a triangle
LOD_MAX_LEVEL = 7                 # vtmc_terrain_extract_lod: the coarsest level of a node (128 fine cells per node cell)
MOD_DETACH = 11                   # removes the floating fragments of its box; data_dims[0] = max_samples (0: no limit)
MOD_NOISE = 8                     # fBm / billow / ridged noise (RidgedMultifractalModifier's device form); 6 and 7 are not defined


class Modifier(ctypes.Structure):
    """vtmc_modifier: one queued TerrainModifier (TerrainModifier.cs:19-33), bounds as the C#
    LowerBound / UpperBound properties return them."""
    _fields_ = [("kind", ctypes.c_int32), ("add_or_erode", ctypes.c_int32), ("lower", ctypes.c_float * 3),
                ("upper", ctypes.c_float * 3), ("p", ctypes.c_float * 8), ("data", ctypes.c_void_p),
                ("data_dims", ctypes.c_int32 * 2)]


class MaterialStroke(ctypes.Structure):
    """vtmc_material_stroke: one paint stroke on the material layer, centre in world space."""
    _fields_ = [("center", ctypes.c_float * 3), ("radius", ctypes.c_float), ("strength", ctypes.c_float), ("channel", ctypes.c_int32)]


class AoParams(ctypes.Structure):
    """vtmc_ao_params: radius in world units, strength in [0, 1], steps 1..AO_MAX_STEPS, flags 0."""
    _fields_ = [("radius", ctypes.c_float), ("strength", ctypes.c_float), ("steps", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class ScatterParams(ctypes.Structure):
    """vtmc_scatter_params: density per world unit^2, the slope band on the face normal's y, the world height band, the material channel
    (-1: none), the seed, the most instances the call may make, flags 0."""
    _fields_ = [("density", ctypes.c_float), ("min_up", ctypes.c_float), ("max_up", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("material_channel", ctypes.c_int32), ("seed", ctypes.c_uint32), ("max_instances", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


class Instance(ctypes.Structure):
    """vtmc_instance: world position, interpolated record normal, the triangle's index in the result, 32 random bits."""
    _fields_ = [("position", ctypes.c_float * 3), ("normal", ctypes.c_float * 3), ("triangle", ctypes.c_uint32), ("rnd", ctypes.c_uint32)]


class LodParams(ctypes.Structure):
    """vtmc_lod_params: viewer in world space, split >= 1, max_level 0..LOD_MAX_LEVEL, max_nodes > 0."""
    _fields_ = [("viewer", ctypes.c_float * 3), ("split", ctypes.c_float), ("max_level", ctypes.c_int32), ("max_nodes", ctypes.c_int32)]


class Fragment(ctypes.Structure):
    """vtmc_fragment: seed (the sample of smallest grid index), tight inclusive bounds, solid sample count, the stamp's id (0: not captured)."""
    _fields_ = [("seed", ctypes.c_int32 * 3), ("lo", ctypes.c_int32 * 3), ("hi", ctypes.c_int32 * 3), ("n_samples", ctypes.c_int32),
                ("stamp_id", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LodNode(ctypes.Structure):
    """vtmc_lod_node: cell origin (multiples of 8 * 2^level) and level of one node of a level-of-detail extract."""
    _fields_ = [("origin", ctypes.c_int32 * 3), ("level", ctypes.c_int32)]


class VolumeBatch(ctypes.Structure):
    _fields_ = [("d_samples", ctypes.c_void_p), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32),
                ("nz", ctypes.c_int32), ("stride_x", ctypes.c_int64), ("stride_y", ctypes.c_int64),
                ("stride_z", ctypes.c_int64), ("n_volumes", ctypes.c_int32),
                ("volume_stride", ctypes.c_int64)]


class ChunkView(ctypes.Structure):
    """vtmc_chunk_view: device pointers into an uploaded chunk-file image."""
    _fields_ = [("origin", ctypes.c_int32 * 3), ("cells", ctypes.c_int32 * 3), ("flags", ctypes.c_uint32),
                ("n_blocks", ctypes.c_uint32), ("n_triangles", ctypes.c_uint32), ("n_vertices", ctypes.c_uint32),
                ("d_samples", ctypes.c_void_p), ("d_tri_offsets", ctypes.c_void_p), ("d_triangles", ctypes.c_void_p),
                ("d_vert_offsets", ctypes.c_void_p), ("d_vertices", ctypes.c_void_p), ("d_indices", ctypes.c_void_p)]


class DensityParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("frequency", ctypes.c_float), ("octaves", ctypes.c_int32),
                ("lacunarity", ctypes.c_float), ("gain", ctypes.c_float),
                ("ramp_scale", ctypes.c_float), ("ramp_center", ctypes.c_float)]


class VtmcError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("vtmc error %d: %s" % (code, text))
        self.code = code


_lib = None


def load(path=None):
    """Load (building if stale) libvtmc.so and declare the prototypes.  `path`: another build of the library, loaded beside the product's
    and not cached (tools/ab_two_libs.py: two builds alternating in ONE process -- boxes of the pool drift by several percent between
    processes)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    explicit = path is not None
    path = path or os.environ.get("VTMC_LIB") or _build.build()   # VTMC_LIB: A/B of two builds on one box (tools/ab_bench.py)
    # PyTorch wheels bundle their own libamdhip64; if this process is going to use torch as well
    # (device memory, streams, torch.distributed), torch must load first so both bind to ONE HIP
    # runtime -- loaded the other way round torch.cuda reports no device.
    if "torch" not in sys.modules and os.environ.get("VTMC_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(path)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    P = ctypes.POINTER
    L.vtmc_version.restype = ctypes.c_char_p
    L.vtmc_create.argtypes = [i32, P(vp)]
    L.vtmc_destroy.argtypes = [vp]
    L.vtmc_last_error.argtypes = [vp]
    L.vtmc_last_error.restype = ctypes.c_char_p
    L.vtmc_extract_blocks.argtypes = [vp, vp, i32, P(i32)]
    L.vtmc_extract_grid.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, vp, i32, P(i32)]
    L.vtmc_extract_grid_sharded.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, i32, i32, i32,
                                            vp, i32, P(i32), P(i32)]
    L.vtmc_read_triangles.argtypes = [vp, vp, i64, vp]
    L.vtmc_read_cases.argtypes = [vp, vp, i64]
    L.vtmc_last_counts.argtypes = [vp, P(i32), P(i32)]
    L.vtmc_extract_volumes_device.argtypes = [vp, P(VolumeBatch), vp, u32, P(i64)]
    L.vtmc_extract_volumes_device_async.argtypes = [vp, P(VolumeBatch), vp, u32]
    L.vtmc_extract_finish.argtypes = [vp, P(i64)]
    L.vtmc_last_fill_ms.argtypes = [vp, P(ctypes.c_float)]
    if not explicit or hasattr(L, "vtmc_context_stream"):   # an older build loaded beside the product's (A/B tools) may lack the newest entry points
        L.vtmc_context_stream.argtypes = [vp, i32, P(vp)]
    if not explicit or hasattr(L, "vtmc_release_streams"):
        L.vtmc_release_streams.argtypes = []
    if not explicit or hasattr(L, "vtmc_last_placement"):
        L.vtmc_last_placement.argtypes = [vp, P(ctypes.c_float * 16), P(i32), P(i32)]
    L.vtmc_device_results.argtypes = [vp, P(vp), P(vp), P(vp)]
    L.vtmc_reserve_triangles.argtypes = [vp, i64]
    L.vtmc_copy_volume_counts_device.argtypes = [vp, vp, i32, vp]
    L.vtmc_last_stage_ms.argtypes = [vp, P(ctypes.c_float * 4)]
    L.vtmc_set_tuning.argtypes = [vp, ctypes.c_char_p, i32]
    L.vtmc_density_fill_device.argtypes = [vp, P(DensityParams), vp, i32, i32, i32, i32,
                                           i64, i64, i64, i64, vp, vp]
    L.vtmc_density_fill_device_async.argtypes = L.vtmc_density_fill_device.argtypes
    L.vtmc_set_output_mode.argtypes = [vp, i32]
    L.vtmc_last_vertex_count.argtypes = [vp, P(i32)]
    L.vtmc_read_indexed_mesh.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.vtmc_device_indexed_results.argtypes = [vp, P(vp), P(vp), P(vp), P(vp)]
    L.vtmc_terrain_init.argtypes = [vp, i32, i32, i32, ctypes.c_float, P(ctypes.c_float * 3), ctypes.c_uint64]
    L.vtmc_terrain_update.argtypes = [vp, vp, i32, P(i32), P(i32)]
    L.vtmc_terrain_dirty_blocks.argtypes = [vp, vp, i32, P(i32)]
    L.vtmc_terrain_read_samples.argtypes = [vp, vp, i64, i64, i64]
    L.vtmc_terrain_device_grid.argtypes = [vp, P(vp), P(i64 * 3), P(i32 * 3)]
    if not explicit or hasattr(L, "vtmc_terrain_set_history"):
        L.vtmc_terrain_set_history.argtypes = [vp, i64]
        L.vtmc_terrain_undo.argtypes = [vp, P(i32), P(i32)]
        L.vtmc_terrain_redo.argtypes = [vp, P(i32), P(i32)]
        L.vtmc_terrain_history.argtypes = [vp, P(i32), P(i32), P(i64)]
    if not explicit or hasattr(L, "vtmc_terrain_raycast"):
        L.vtmc_terrain_raycast.argtypes = [vp, vp, vp, i32, ctypes.c_float, u32, vp]
        L.vtmc_raycast_device.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, P(ctypes.c_float * 3), ctypes.c_float,
                                          vp, vp, i32, ctypes.c_float, u32, vp, vp]
    if not explicit or hasattr(L, "vtmc_terrain_spherecast"):
        L.vtmc_terrain_spherecast.argtypes = [vp, vp, vp, vp, i32, ctypes.c_float, u32, vp]
        L.vtmc_terrain_closest_point.argtypes = [vp, vp, vp, i32, u32, vp]
        L.vtmc_spherecast_device.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, P(ctypes.c_float * 3), ctypes.c_float,
                                             vp, vp, vp, i32, ctypes.c_float, u32, vp, vp]
        L.vtmc_closest_point_device.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, P(ctypes.c_float * 3), ctypes.c_float,
                                                vp, vp, i32, u32, vp, vp]
    if not explicit or hasattr(L, "vtmc_terrain_save"):
        L.vtmc_terrain_save.argtypes = [vp, ctypes.c_char_p, u32, P(i64)]
        L.vtmc_terrain_load.argtypes = [vp, ctypes.c_char_p, u32, P(i32), P(i32)]
        L.vtmc_terrain_write_samples.argtypes = [vp, vp, i64, i64, i64]
    if not explicit or hasattr(L, "vtmc_stamp_create"):
        L.vtmc_stamp_create.argtypes = [vp, vp, i32, i32, i32, i64, i64, i64, P(i32)]
        L.vtmc_stamp_capture.argtypes = [vp, P(i32 * 3), i32, i32, i32, P(i32)]
        L.vtmc_stamp_info.argtypes = [vp, i32, P(i32 * 3)]
        L.vtmc_stamp_read.argtypes = [vp, i32, vp, i64, i64, i64]
        L.vtmc_stamp_destroy.argtypes = [vp, i32]
    if not explicit or hasattr(L, "vtmc_stamp_from_mesh"):
        L.vtmc_stamp_from_mesh.argtypes = [vp, vp, i32, vp, i32, P(ctypes.c_float * 3), ctypes.c_float, i32, i32, i32, u32, P(i32)]
    if not explicit or hasattr(L, "vtmc_material_init"):
        L.vtmc_material_init.argtypes = [vp, i32]
        L.vtmc_material_set_control_map.argtypes = [vp, vp, i32]
        L.vtmc_material_write.argtypes = [vp, vp]
        L.vtmc_material_read.argtypes = [vp, vp, P(i32)]
        L.vtmc_material_paint.argtypes = [vp, vp, i32]
        L.vtmc_material_vertices.argtypes = [vp, P(i64)]
        L.vtmc_material_read_vertices.argtypes = [vp, vp, i64]
        L.vtmc_material_device_results.argtypes = [vp, P(vp), P(i64)]
    if not explicit or hasattr(L, "vtmc_ao_vertices"):
        L.vtmc_ao_vertices.argtypes = [vp, P(AoParams), P(i64)]
        L.vtmc_ao_read_vertices.argtypes = [vp, vp, i64]
        L.vtmc_ao_device_results.argtypes = [vp, P(vp), P(i64)]
        L.vtmc_debug_ao_routes.argtypes = [vp, P(u32 * 2), i32]   # not in the header: the route counters of the last vtmc_ao_vertices
        L.vtmc_debug_ao_routes.restype = i32
    if not explicit or hasattr(L, "vtmc_scatter_surface"):
        L.vtmc_scatter_surface.argtypes = [vp, P(ScatterParams), P(i64)]
        L.vtmc_scatter_read.argtypes = [vp, vp, i64, vp]
        L.vtmc_scatter_device_results.argtypes = [vp, P(vp), P(vp), P(i64)]
        L.vtmc_debug_scatter_ms.argtypes = [vp, P(ctypes.c_float * 4)]   # not in the header: device time of the last scatter's four kernels
        L.vtmc_debug_scatter_ms.restype = i32
    if not explicit or hasattr(L, "vtmc_terrain_extract_lod"):
        L.vtmc_terrain_extract_lod.argtypes = [vp, P(LodParams), P(i32), P(i32)]
        L.vtmc_terrain_lod_nodes.argtypes = [vp, vp, i32, P(i32)]
        L.vtmc_debug_lod_gather_ms.argtypes = [vp, P(ctypes.c_float)]   # not in the header: device time of the last gather launch
        L.vtmc_debug_lod_gather_ms.restype = i32
        L.vtmc_debug_lod_tiles.argtypes = [vp, vp, i64]                 # not in the header: the gathered tiles of the last level-of-detail extract
        L.vtmc_debug_lod_tiles.restype = i32
    if not explicit or hasattr(L, "vtmc_terrain_fragments"):
        L.vtmc_terrain_fragments.argtypes = [vp, P(ctypes.c_float * 3), P(ctypes.c_float * 3), i32, i32, vp, i32, P(i32)]
    L.vtmc_comm_unique_id.argtypes = [vp]
    L.vtmc_comm_init_rank.argtypes = [vp, vp, i32, i32]
    L.vtmc_comm_destroy.argtypes = [vp]
    L.vtmc_comm_share.argtypes = [vp, vp]
    L.vtmc_allgather_volume_counts.argtypes = [vp, vp, i32, vp]
    L.vtmc_copy_to_host.argtypes = [vp, vp, vp, i64, vp]
    L.vtmc_chunk_write.argtypes = [vp, ctypes.c_char_p, i32, P(i32 * 3), i32]
    L.vtmc_chunk_read.argtypes = [vp, ctypes.c_char_p, P(ChunkView)]
    for name in SYMBOLS:
        if explicit and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int:
            fn.restype = i32
    if not explicit:
        _lib = L
    return L


def release_streams():
    """vtmc_release_streams: destroys the streams the library keeps parked for contexts that are gone.  Call it once nothing of the host's
    (events, stream wrappers, pinned tensors copied on them) refers to a handle of a closed Extractor any more -- the tools that run under
    rocprofv3 do, before they exit."""
    return _lib.vtmc_release_streams() if _lib is not None else 0


def library_path():
    return _build.LIB if os.path.exists(_build.LIB) else None
