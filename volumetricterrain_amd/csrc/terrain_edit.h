// terrain_edit.h -- what terrain.hip (vtmc_terrain_update's queue walk and the table of modifier kinds) and the files of the kinds
// (terrain_brush.hip, terrain_noise.hip, terrain_stamp.hip, terrain_path.hip, terrain_fragments.hip, terrain_erosion.hip) need of each other.  Host side only.
#ifndef VTMC_TERRAIN_EDIT_H
#define VTMC_TERRAIN_EDIT_H
#include "terrain_box.h"

namespace vtmc {

// One kind of vtmc_modifier: a new kind is one entry of the table in terrain.hip.
struct ModifierKind {
    int32_t kind;
    // VTMC_OK, or fail(...) with the modifier's index i in the error text
    int (*check)(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
    // A checked modifier on its non-empty clamped sample box (a: sample_range's, with the event): queues its kernels on ctx->stream; image:
    // the box's journal image or null.  VTMC_OK or an error code with the context's error text set.
    int (*apply)(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
};
const ModifierKind *find_modifier_kind(int32_t kind);  // null: unknown

// the entries that live outside terrain.hip, in the file of their name; check_brush serves VTMC_MOD_SMOOTH and VTMC_MOD_FLATTEN
int check_brush(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int check_noise(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int check_stamp(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int check_path(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int check_detach(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int check_erosion(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i);
int apply_smooth(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_flatten(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_noise(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_stamp(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_path(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_detach(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);
int apply_erosion(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image);

static TerrainBox box_of(const TerrainModifierArgs &m) { return TerrainBox{m.lx, m.ly, m.lz, m.dx, m.dy, m.dz}; }
// terrain.hip: a modifier's kernel arguments: its AABB in sample indices, [low, up] clamped to the grid (up[] is also what the dirty blocks
// are found from)
TerrainModifierArgs sample_range(const TerrainShape &sh, const vtmc_modifier &md, int low[3], int up[3]);
// terrain.hip: the clamped sample box of the world bounds lower..upper, as sample_range finds a modifier's (the queries that take a box)
TerrainBox bounds_box(const TerrainShape &sh, const float lower[3], const float upper[3]);
// terrain.hip: `bytes` of host data into a grow-only buffer of the context that the modifier's kernel reads (the heightmap, a path's
// segments); drains ctx->stream first, and the copy blocks
int stage_for_queue(vtmc_ctx *ctx, VtmcDevBuf &buf, const void *host, size_t bytes);

}  // namespace vtmc
#endif
