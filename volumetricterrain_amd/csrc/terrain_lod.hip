// terrain_lod.hip -- level-of-detail extraction of the resident terrain (include/vtmc.h, "Level of detail"): the host chooses an octree of
// nodes around a viewer (terrain_lod.h), lod_gather_kernel gathers every node's 10x10x10 tile from the resident grid at stride 2^level,
// and the packed tiles go through the ordinary classify -> scan -> emit path as the batch of one-block volumes vtmc_extract_blocks submits.
// Nothing of the extraction kernels is touched: the front end is all there is.
//
// The kernel.  One 256-thread workgroup per node; thread t takes the tile elements e = t, t + 256, t + 512, t + 768 (e = i + 10 j + 100 k),
// so a wave's 64 lanes cover a run of 6.4 consecutive tile rows and neighbouring lanes walk x.  At level 0 a row's 10 samples are 40
// contiguous bytes of the grid, one or two 64-byte lines; at level L the row spans 9 * 2^L + 1 samples and the useful bytes per line fall as
// 2^-L -- a property of the subsample, not of the schedule: the lines of one row are still fetched by neighbouring lanes of one
// instruction.  The four loads of a thread are issued before the first store; the stores are the packed tile, consecutive lanes on
// consecutive dwords.  The node record is the same for the whole workgroup (scalar loads).  The index is clamped with min, not a branch;
// element offsets are 64-bit.  No LDS: nothing is reused inside a workgroup (neighbouring nodes share two of ten sample planes per axis,
// which the caches serve).
//
// Bounds.  Every grid index is min(o + i s, dim - 1) with o >= 0: inside the grid.  Every store is tile element e < VTMC_TILE_SAMPLES of
// node blockIdx.x < n_nodes, and the tile buffer holds n_nodes * VTMC_TILE_SAMPLES floats.  The node list is the host's own (lod_select),
// never the caller's.
#include "vtmc_ctx.h"
#include "terrain_lod.h"

#include <cstring>
#include <new>

namespace vtmc {

constexpr int kLodThreads = 256;
constexpr int kLodRounds = (VTMC_TILE_SAMPLES + kLodThreads - 1) / kLodThreads;   // 4

__global__ __launch_bounds__(kLodThreads) void lod_gather_kernel(const float *__restrict__ grid, int dim_x, int dim_y, int dim_z,
                                                                  const vtmc_lod_node *__restrict__ nodes, float *__restrict__ tiles)
{
    const vtmc_lod_node nd = nodes[blockIdx.x];
    const int ox = nd.origin[0], oy = nd.origin[1], oz = nd.origin[2], level = nd.level;
    const long long sy = dim_x, sz = (long long)dim_x * dim_y;
    float v[kLodRounds];
#pragma unroll
    for (int r = 0; r < kLodRounds; ++r) {
        // the lanes past the tile's end in the last round read its last sample again and store nothing
        const unsigned e = min(threadIdx.x + (unsigned)(kLodThreads * r), (unsigned)(VTMC_TILE_SAMPLES - 1));
        const unsigned k = e / 100u, jr = e - 100u * k, j = jr / 10u, i = jr - 10u * j;
        const int x = min(ox + (int)(i << level), dim_x - 1);
        const int y = min(oy + (int)(j << level), dim_y - 1);
        const int z = min(oz + (int)(k << level), dim_z - 1);
        v[r] = grid[(long long)x + sy * (long long)y + sz * (long long)z];
    }
    float *tile = tiles + (size_t)blockIdx.x * VTMC_TILE_SAMPLES;
#pragma unroll
    for (int r = 0; r < kLodRounds; ++r) {
        const unsigned e = threadIdx.x + (unsigned)(kLodThreads * r);
        if (e < (unsigned)VTMC_TILE_SAMPLES) tile[e] = v[r];
    }
}

static bool lod_current(const vtmc_ctx *ctx) { return ctx->result.valid && ctx->result.source == ResultSource::TerrainLod; }

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_extract_lod(vtmc_ctx *ctx, const vtmc_lod_params *params, int32_t *n_nodes, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!params) return fail(ctx, VTMC_ERR_INVALID_ARG, "params is null");
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_extract_lod before terrain_init");
    if (const char *fault = lod_params_fault(*params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_extract_lod: %s", fault);
    const TerrainShape &sh = ctx->tshape;
    const int32_t cells[3] = {sh.dim_x - 2, sh.dim_y - 2, sh.dim_z - 2};
    if (!lod_dims_fit(cells, params->max_level))
        return fail(ctx, VTMC_ERR_DIMS, "terrain_extract_lod: a root of level %d (%d cells) does not divide the terrain (%dx%dx%d)", params->max_level,
                    lod_node_cells(params->max_level), cells[0], cells[1], cells[2]);
    // the selection, before anything of the context is touched: a refused call leaves the previous result as it was
    std::vector<vtmc_lod_node> nodes;
    try {
        if (!lod_select(cells, sh.origin, sh.scale, *params, nodes))
            return fail(ctx, VTMC_ERR_TOO_LARGE, "terrain_extract_lod: the selection holds more than max_nodes = %d nodes", params->max_nodes);
    } catch (const std::bad_alloc &) {
        return fail(ctx, VTMC_ERR_DEVICE, "terrain_extract_lod: out of host memory for the node list");
    }
    const size_t n = nodes.size();
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->result.valid = false;   // from here on the tiles of an earlier level-of-detail result are overwritten
    if (int rc = ensure(ctx, ctx->lod_nodes_dev, n * sizeof(vtmc_lod_node))) return rc;
    if (int rc = ensure(ctx, ctx->lod_tiles, n * VTMC_TILE_SAMPLES * sizeof(float))) return rc;
    int rc = VTMC_OK;
    {
        hipError_t e = hipMemcpyAsync(ctx->lod_nodes_dev.p, nodes.data(), n * sizeof(vtmc_lod_node), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = ctx->lod_clock.begin();
        if (e == hipSuccess) e = ctx->lod_clock.mark(0, ctx->stream);
        if (e == hipSuccess)
            e = launch(lod_gather_kernel, dim3((unsigned)n), dim3(kLodThreads), 0, ctx->stream, (const float *)ctx->terrain.p, sh.dim_x, sh.dim_y, sh.dim_z,
                       (const vtmc_lod_node *)ctx->lod_nodes_dev.p, (float *)ctx->lod_tiles.p);
        if (e == hipSuccess) e = ctx->lod_clock.mark(1, ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, VTMC_ERR_DEVICE, "terrain_extract_lod: %s", hipGetErrorString(e));
    }
    if (rc == VTMC_OK) {
        // the tile buffer is a batch of n volumes of one 8^3 block each, as vtmc_extract_blocks submits it
        const BlockSpace sp = dense_space((const float *)ctx->lod_tiles.p, 8, 8, 8, 1, 10, 100, (int)n, VTMC_TILE_SAMPLES);
        rc = extract_core(ctx, sp, 0, ResultSource::TerrainLod, tri_count);
    }
    if (rc) {   // `nodes` is only borrowed by the upload: a failure must not return while the copy may still read it
        quiet(hipStreamSynchronize(ctx->stream));
        return rc;
    }
    ctx->lod_nodes.swap(nodes);
    ctx->lod_clock.arm();
    if (n_nodes) *n_nodes = (int32_t)n;
    return VTMC_OK;
}

int32_t vtmc_terrain_lod_nodes(vtmc_ctx *ctx, vtmc_lod_node *dst, int32_t capacity_nodes, int32_t *n_nodes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lod_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_lod_nodes: the context holds no level-of-detail result");
    const size_t n = ctx->lod_nodes.size();
    if (n_nodes) *n_nodes = (int32_t)n;
    if (!dst) return VTMC_OK;   // size query
    if ((size_t)(capacity_nodes > 0 ? capacity_nodes : 0) < n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %zu nodes", capacity_nodes, n);
    memcpy(dst, ctx->lod_nodes.data(), n * sizeof(vtmc_lod_node));
    return VTMC_OK;
}

// Not part of the ABI (tests, tools/lod_bench.py): device time in milliseconds of the last lod_gather_kernel launch.
int32_t vtmc_debug_lod_gather_ms(vtmc_ctx *ctx, float *ms)
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->lod_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_lod_gather_ms before any level-of-detail extract");
    if (int rc = ctx->lod_clock.sync_last(ctx)) return rc;
    return ctx->lod_clock.elapsed(ctx, 0, 1, ms);
}

// Not part of the ABI (tests): the gathered tiles of the level-of-detail result the context holds, VTMC_TILE_SAMPLES floats per node.
int32_t vtmc_debug_lod_tiles(vtmc_ctx *ctx, float *dst, int64_t capacity_floats)
{
    if (!ctx || !dst) return VTMC_ERR_INVALID_ARG;
    if (!lod_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_lod_tiles: the context holds no level-of-detail result");
    const size_t n = ctx->lod_nodes.size() * VTMC_TILE_SAMPLES;
    if (capacity_floats < 0 || (size_t)capacity_floats < n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %zu floats", (long long)capacity_floats, n);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipMemcpy(dst, ctx->lod_tiles.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

}  // extern "C"
