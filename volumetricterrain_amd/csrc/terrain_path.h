// terrain_path.h -- what terrain.hip needs of terrain_path.hip: the check and the launch of a VTMC_MOD_PATH modifier, called from
// vtmc_terrain_update's queue walk.  The segment buffer is part of the context (vtmc_ctx.h).
#ifndef VTMC_TERRAIN_PATH_H
#define VTMC_TERRAIN_PATH_H
#include "vtmc_ctx.h"

namespace vtmc {
constexpr int kPathChunk = 256;         // segments a workgroup tests at a time: one per thread
constexpr int kPathMaxSegments = 65536;
// VTMC_OK, or VTMC_ERR_INVALID_ARG with the modifier's index in the error text (include/vtmc.h, VTMC_MOD_PATH)
int check_path_modifier(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
// A checked modifier on its non-empty clamped sample box (a: lx..dz and the event): stages its segments in the context's buffer and
// queues the kernel; image: the box's journal image or null.  VTMC_OK or an error code with the context's error text set.
int launch_path(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image, hipStream_t stream);
}  // namespace vtmc
#endif
