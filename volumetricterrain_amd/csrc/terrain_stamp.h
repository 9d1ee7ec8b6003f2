// terrain_stamp.h -- what terrain.hip, terrain_stamp.hip and stamp_mesh.hip need of each other: the check and the launch of a VTMC_MOD_STAMP modifier
// (terrain_stamp.hip, called from vtmc_terrain_update's queue walk), and the box copy of the resident grid (terrain.hip, called by
// vtmc_stamp_capture).  The stamp table itself is part of the context (vtmc_ctx.h).
#ifndef VTMC_TERRAIN_STAMP_H
#define VTMC_TERRAIN_STAMP_H
#include "vtmc_ctx.h"

namespace vtmc {
// VTMC_OK, or VTMC_ERR_INVALID_ARG with the modifier's index in the error text (include/vtmc.h, VTMC_MOD_STAMP)
int check_stamp_modifier(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
// the paste of a checked modifier on its non-empty clamped sample box (a: lx..dz and the event); image: the box's journal image or null
hipError_t launch_stamp_paste(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image, hipStream_t stream);
// terrain.hip: the box b of the grid to dst (b.dx * b.dy * b.dz samples, x fastest), 32-bit copies
hipError_t launch_terrain_copy_box(const float *grid, float *dst, const TerrainShape &sh, const TerrainBox &b, hipStream_t stream);
// terrain_stamp.hip, for stamp_mesh.hip (vtmc_stamp_from_mesh): the dims check of every stamp; a new stamp of checked dims with its device
// memory allocated; and its entry into the context's table, which takes the id -- only once nothing can fail any more
int check_stamp_dims(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz);
int new_stamp(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz, VtmcStamp &st);
int32_t keep_stamp(vtmc_ctx *ctx, VtmcStamp &st);
}  // namespace vtmc
#endif
