"""volumetricterrain_amd -- MI355X-native marching-cubes extraction path of
MangoSister/VolumetricTerrain (VoxelTerrain.BatchUpdate + its three compute kernels) as
hand-written HIP for gfx950 behind the C ABI of include/vtmc.h.

Only the hot path lives here: csrc/ (HIP kernels + C ABI), the ctypes binding,
the host-side mirror of the reference's VoxelTerrain chunk API, and chunk sharding helpers.
"""
from ._lib import FRAGMENT_DTYPE, INSTANCE_DTYPE, LIGHT_SAMPLE_DTYPE, LIGHT_SOURCE_DTYPE, NAV_SPAN_DTYPE, NAVFIELD_CELL_DTYPE, NAVCROWD_AGENT_DTYPE, NAVFIELD_GOAL_DTYPE, NAVSIGHT_HIT_DTYPE, RAY_HIT_DTYPE, SPHERE_HIT_DTYPE, TRI_DTYPE, VERTEX_DTYPE, WATER_BODY_DTYPE, WATER_SOURCE_DTYPE, VtmcError, load, library_path, release_streams  # noqa: F401
from .extractor import Extractor, density_params, elem_strides, nav_world_positions  # noqa: F401
from .terrainfile import classify_bricks, read_terrain, write_terrain  # noqa: F401
from .modifiers import AmbientOcclusion, CylinderModifier, DetachModifier, ErosionModifier, FlattenModifier, IslandModifier, LightParams, LodParams, LodSkirtParams, MaterialStroke, NavCrowdParams, NavErodeParams, NavFieldParams, NavParams, NavSightParams, NoiseModifier, PathModifier, PlaneModifier, ScatterParams, SmoothModifier, SphereModifier, StampModifier, mesh_stamp_box  # noqa: F401

__all__ = ["AmbientOcclusion", "CylinderModifier", "DetachModifier", "ErosionModifier", "FlattenModifier", "IslandModifier", "LightParams", "LodParams", "LodSkirtParams", "MaterialStroke", "NavCrowdParams", "NavErodeParams", "NavFieldParams", "NavParams", "NavSightParams", "NoiseModifier", "PathModifier", "PlaneModifier", "ScatterParams", "SmoothModifier", "SphereModifier", "StampModifier", "mesh_stamp_box", "Extractor", "FRAGMENT_DTYPE", "INSTANCE_DTYPE", "LIGHT_SAMPLE_DTYPE", "LIGHT_SOURCE_DTYPE", "NAV_SPAN_DTYPE", "NAVFIELD_CELL_DTYPE", "NAVFIELD_GOAL_DTYPE", "NAVCROWD_AGENT_DTYPE", "NAVSIGHT_HIT_DTYPE", "RAY_HIT_DTYPE", "SPHERE_HIT_DTYPE", "TRI_DTYPE", "VERTEX_DTYPE", "WATER_BODY_DTYPE", "WATER_SOURCE_DTYPE", "VtmcError", "classify_bricks", "density_params", "elem_strides", "nav_world_positions", "read_terrain", "write_terrain", "load", "library_path", "release_streams"]
