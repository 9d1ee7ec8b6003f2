"""ctypes binding of libvtmc.so -- the same C ABI a C# host binds with [DllImport].

Constants, structs, record dtypes and prototypes are read from include/vtmc.h (_header.py); nothing of the header is retyped here.

There is no CPU fallback: if the library is missing it is built with hipcc; if that fails, or the
library cannot be loaded, importing raises.  Creating a context without a HIP device fails with
VtmcError (vtmc_create returns VTMC_ERR_DEVICE).
"""
import ctypes
import os
import sys

from . import build as _build
from ._header import HEADER, LAYERS

# every #define VTMC_<NAME> of every layer's header as <NAME>.  include/vtmc.h: OK and the ERR_* codes, FLAG_*, OUTPUT_*, MOD_*, TERRAIN_SAVE_EXACT,
# TERRAIN_LOAD_NO_EXTRACT, MESH_*, MATERIAL_*, AO_*, SCATTER_*, LOD_MAX_LEVEL, RAY_TWO_SIDED, SPHERE_MAX_RADIUS_CELLS, COMM_ID_BYTES ...
# The optional layers' headers: NAV_OPEN, NAVFIELD_UNIT, NAVERODE_MAX_RADIUS, NAVSIGHT_ANY_COST, NAVCROWD_ANY_DETOUR, WATER_AT_FACE, LODSKIRT_ALL_FACES, LODATTR_AO, MOD_EROSION, EROSION_G, LIGHT_MAX_ROUNDS ...
for _layer in LAYERS.values():
    globals().update((name[len("VTMC_"):], value) for name, value in _layer.constants.items())
STAMP_MIN_DIM, STAMP_MAX_DIM, STAMP_MAX_SAMPLES = 2, 1026, 1 << 27   # vtmc_stamp_create: the limits of a stamp's dims (the header states them in prose)
PATH_CHUNK, PATH_MAX_SEGMENTS = 256, 65536   # csrc/terrain_path.h: segments a workgroup prunes at a time; the most a modifier may hold

LAYER_SYMBOLS = {name: list(header.prototypes) for name, header in LAYERS.items()}   # per layer, every symbol its header declares
SYMBOLS = LAYER_SYMBOLS["core"]   # every symbol include/vtmc.h declares (tests/test_abi_symbols.py finds them with a regex of its own)

# the wire record (CSTriangle.stride = 76, VoxelTerrain.cs:36) under the short names the package uses
TRI_DTYPE = HEADER.dtype("vtmc_triangle", ("p0", "p1", "p2", "n0", "n1", "n2", "block"))
VERTEX_DTYPE = HEADER.dtype("vtmc_vertex")
RAY_HIT_DTYPE = HEADER.dtype("vtmc_ray_hit")         # one answer of vtmc_terrain_raycast / vtmc_raycast_device
SPHERE_HIT_DTYPE = HEADER.dtype("vtmc_sphere_hit")   # one answer of vtmc_terrain_spherecast / _closest_point and their _device forms
INSTANCE_DTYPE = HEADER.dtype("vtmc_instance")       # one instance of vtmc_scatter_surface
FRAGMENT_DTYPE = HEADER.dtype("vtmc_fragment")       # one record of vtmc_terrain_fragments
NAV_SPAN_DTYPE = LAYERS["nav"].dtype("vtmc_nav_span")       # one span of vtmc_terrain_nav_build
NAVFIELD_CELL_DTYPE = LAYERS["navfield"].dtype("vtmc_navfield_cell")   # one cell of vtmc_navfield_build: cost and next
NAVFIELD_GOAL_DTYPE = LAYERS["navfield"].dtype("vtmc_navfield_goal")   # one goal of vtmc_navfield_build: span and cost
NAVSIGHT_HIT_DTYPE = LAYERS["navsight"].dtype("vtmc_navsight_hit")     # one answer of vtmc_nav_sight: the span the walk ended on and its steps
NAVCROWD_AGENT_DTYPE = LAYERS["navcrowd"].dtype("vtmc_navcrowd_agent")   # one agent of vtmc_navcrowd_spawn: span, budget, speed, state
WATER_SOURCE_DTYPE = LAYERS["water"].dtype("vtmc_water_source")   # one source of vtmc_terrain_flood: world position and level
WATER_BODY_DTYPE = LAYERS["water"].dtype("vtmc_water_body")       # one body of vtmc_water_bodies: seed, bounds, level, counts, flags
LIGHT_SOURCE_DTYPE = LAYERS["light"].dtype("vtmc_light_source")   # one source of vtmc_terrain_light: world position and level 1..255
LIGHT_SAMPLE_DTYPE = LAYERS["light"].dtype("vtmc_light_sample")   # one sample of the light volume, one vertex of vtmc_light_vertices: sky, torch

Modifier = HEADER.structure("vtmc_modifier", "Modifier", """vtmc_modifier: one queued TerrainModifier (TerrainModifier.cs:19-33), bounds as the C#
    LowerBound / UpperBound properties return them.""")
MaterialStroke = HEADER.structure("vtmc_material_stroke", "MaterialStroke", "vtmc_material_stroke: one paint stroke on the material layer, centre in world space.")
AoParams = HEADER.structure("vtmc_ao_params", "AoParams", "vtmc_ao_params: radius in world units, strength in [0, 1], steps 1..AO_MAX_STEPS, flags 0.")
ScatterParams = HEADER.structure("vtmc_scatter_params", "ScatterParams", """vtmc_scatter_params: density per world unit^2, the slope band on the face normal's y,
    the world height band, the material channel (-1: none), the seed, the most instances the call may make, flags 0.""")
Instance = HEADER.structure("vtmc_instance", "Instance", "vtmc_instance: world position, interpolated record normal, the triangle's index in the result, 32 random bits.")
LodParams = HEADER.structure("vtmc_lod_params", "LodParams", "vtmc_lod_params: viewer in world space, split >= 1, max_level 0..LOD_MAX_LEVEL, max_nodes > 0.")
Fragment = HEADER.structure("vtmc_fragment", "Fragment", """vtmc_fragment: seed (the sample of smallest grid index), tight inclusive bounds, solid sample count,
    the stamp's id (0: not captured).""")
NavParamsStruct = LAYERS["nav"].structure("vtmc_nav_params", "NavParamsStruct", "vtmc_nav_params: agent_height in samples, max_step in grid units, max_spans > 0, flags 0.")
NavSpan = LAYERS["nav"].structure("vtmc_nav_span", "NavSpan", "vtmc_nav_span: floor height (grid units), floor sample y, clearance, four links, region.")
NavFieldParamsStruct = LAYERS["navfield"].structure("vtmc_navfield_params", "NavFieldParamsStruct", "vtmc_navfield_params: climb and drop cost per grid unit in [0, 1024], max_cost 1..0x7fffffff, flags 0.")
NavErodeParamsStruct = LAYERS["naverode"].structure("vtmc_naverode_params", "NavErodeParamsStruct", "vtmc_naverode_params: radius in columns, 0..NAVERODE_MAX_RADIUS, flags NAVERODE_OPEN_BOX_FACES or 0, two reserved words, 0.")
NavSightParamsStruct = LAYERS["navsight"].structure("vtmc_navsight_params", "NavSightParamsStruct", "vtmc_navsight_params: max_look 1..NAVSIGHT_MAX_LOOK, max_extra_cost or NAVSIGHT_ANY_COST, flags 0, reserved 0.")
NavCrowdParamsStruct = LAYERS["navcrowd"].structure("vtmc_navcrowd_params", "NavCrowdParamsStruct", "vtmc_navcrowd_params: max_detour or NAVCROWD_ANY_DETOUR, flags NAVCROWD_LEAVE_ON_ARRIVAL or 0, two reserved words, 0.")
LodSkirtParamsStruct = LAYERS["lodskirt"].structure("vtmc_lodskirt_params", "LodSkirtParamsStruct", "vtmc_lodskirt_params: depth in the node's own cells, in (0, LODSKIRT_MAX_DEPTH]; flags LODSKIRT_ALL_FACES or 0.")
ErosionReport = LAYERS["erosion"].structure("vtmc_erosion_report", "ErosionReport", "vtmc_erosion_report: the clamped box lo..hi, nx, nz, iterations, and the active, rewritten and clamped column counts.")
LightParamsStruct = LAYERS["light"].structure("vtmc_light_params", "LightParamsStruct", "vtmc_light_params: sky_level 0..255, sky_falloff and torch_falloff 1..255, flags 0.")
LodNode = HEADER.structure("vtmc_lod_node", "LodNode", "vtmc_lod_node: cell origin (multiples of 8 * 2^level) and level of one node of a level-of-detail extract.")
VolumeBatch = HEADER.structure("vtmc_volume_batch", "VolumeBatch")
ChunkView = HEADER.structure("vtmc_chunk_view", "ChunkView", "vtmc_chunk_view: device pointers into an uploaded chunk-file image.")
DensityParams = HEADER.structure("vtmc_density_params", "DensityParams")

_vp, _i32, _i64, _P = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER
DEBUG_ARGTYPES = {   # entry points that are deliberately not in the header; all return int32_t
    "vtmc_debug_ao_routes": [_vp, _P(ctypes.c_uint32 * 2), _i32],   # the route counters of the last vtmc_ao_vertices
    "vtmc_debug_scatter_ms": [_vp, _P(ctypes.c_float * 4)],         # device time of the last scatter's four kernels
    "vtmc_debug_lod_gather_ms": [_vp, _P(ctypes.c_float)],          # device time of the last gather launch
    "vtmc_debug_lod_tiles": [_vp, _vp, _i64],                       # the gathered tiles of the last level-of-detail extract
    "vtmc_debug_nav_ms": [_vp, _P(ctypes.c_float * 8)],             # device time of the last nav build's seven stages, and its rounds
    "vtmc_debug_nav_box_read_ms": [_vp, _vp, _vp, _i32, _P(ctypes.c_float)],   # device time of a plain read of a box in the nav walk's layout
    "vtmc_debug_navfield_ms": [_vp, _P(ctypes.c_float * 4)],        # device time of the last field build's three stages, and its rounds
    "vtmc_debug_naverode_ms": [_vp, _P(ctypes.c_float * 5)],        # device time of the last distance build's or erode's four stages, and its rounds
    "vtmc_debug_navsight_ms": [_vp, _P(ctypes.c_float * 2)],        # device time of the last sight query's or smoothed trace's row fill and kernel
    "vtmc_debug_navcrowd_ms": [_vp, _P(ctypes.c_float * 1)],        # device time of the ticks of the last crowd step
    "vtmc_debug_water_ms": [_vp, _P(ctypes.c_float * 3)],           # device time of the last flood's levels, statistics and volume kernel
    "vtmc_debug_erosion_lds": [_vp, _i32],                          # the step's variant of later erosions: 0 neighbour loads through the caches (the default), 1 staged in LDS
    "vtmc_debug_erosion_ms": [_vp, _P(ctypes.c_float * 3)],         # device time of the last erosion's height pass, steps, and finish with write-back
    "vtmc_debug_erosion_step_ms": [_vp, _i32, _i32, _P(ctypes.c_float)],   # device time of more steps on the last erosion's state: variant 0 direct, 1 LDS, 2 empty launches
    "vtmc_debug_light_variant": [_vp, _i32, _i32],                  # the relaxation of later light calls: 0 tiled rounds (the default), 1 plain one-hop rounds, -1 as it is; rounds per read-back
    "vtmc_debug_light_ms": [_vp, _P(ctypes.c_float * 3)],           # device time of the last light call's seeds, relaxation (with its read-backs) and count
    "vtmc_debug_lodskirt_ms": [_vp, _P(ctypes.c_float * 4)],        # device time of the last skirt pass's four kernels
    "vtmc_debug_lodskirt_store": [_vp, _i32],                       # the emit kernel's store variant of later skirt passes: 0 direct, 1 staged in LDS
    "vtmc_debug_lodskirt_read_ms": [_vp, _i32, _P(ctypes.c_float)],  # median device time of a plain read of the result's records
    "vtmc_debug_lodattr_routes": [_vp, _P(ctypes.c_uint32 * 2), _i32],   # the route counters of the last vtmc_lod_ao_vertices
    "vtmc_debug_lodattr_skirts_in_node": [_vp, _i32],               # later occlusion calls: a node's skirt quads in its own workgroup (1, the default) or a pass of their own (0)
    "vtmc_debug_lodattr_ms": [_vp, _P(ctypes.c_float * 2)],         # device time of the last occlusion call's nodes' kernel and skirts' pass
}


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
    signatures = [(p.name, p.restype, p.argtypes) for h in LAYERS.values() for p in h.prototypes.values()] + [(n, _i32, a) for n, a in DEBUG_ARGTYPES.items()]
    for name, restype, argtypes in signatures:
        if explicit and not hasattr(L, name):   # an older build loaded beside the product's (A/B tools) may lack the newest entry points;
            continue                            # in the product's own library a missing name is an error
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
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
