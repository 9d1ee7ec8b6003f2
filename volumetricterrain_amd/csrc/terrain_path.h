// terrain_path.h -- the limits of a VTMC_MOD_PATH modifier (terrain_path.hip; its check and apply are entries of the modifier table,
// terrain_edit.h).  The segment buffer is part of the context (vtmc_ctx.h).
#ifndef VTMC_TERRAIN_PATH_H
#define VTMC_TERRAIN_PATH_H

namespace vtmc {
constexpr int kPathChunk = 256;         // segments a workgroup tests at a time: one per thread
constexpr int kPathMaxSegments = 65536;
}  // namespace vtmc
#endif
