// terrain_stamp.h -- what terrain_stamp.hip, stamp_mesh.hip and terrain.hip need of each other outside the modifier table (terrain_edit.h): the
// making of a stamp, and the box copy of the resident grid.  The stamp table itself is part of the context (vtmc_ctx.h).
#ifndef VTMC_TERRAIN_STAMP_H
#define VTMC_TERRAIN_STAMP_H
#include "vtmc_ctx.h"

namespace vtmc {
// terrain.hip: the box b of the grid to dst (b.dx * b.dy * b.dz samples, x fastest), 32-bit copies
hipError_t launch_terrain_copy_box(const float *grid, float *dst, const TerrainShape &sh, const TerrainBox &b, hipStream_t stream);
// terrain_stamp.hip, for stamp_mesh.hip (vtmc_stamp_from_mesh): the dims check of every stamp; a new stamp of checked dims with its device
// memory allocated; and its entry into the context's table, which takes the id -- only once nothing can fail any more
int check_stamp_dims(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz);
int new_stamp(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz, VtmcStamp &st);
int32_t keep_stamp(vtmc_ctx *ctx, VtmcStamp &st);
}  // namespace vtmc
#endif
