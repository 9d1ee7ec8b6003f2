// terrain_ao.hip -- per-vertex ambient occlusion of a terrain extract (vtmc_ao_*): one byte per vertex from a clamped-density march along
// the 26 lattice directions through the resident grid.  The rule, operation by operation, is in include/vtmc.h; the kernels follow it bit
// for bit (library built with -ffp-contract=off).  The host half -- argument checks, Rg, the h[] / fall[] tables -- is terrain_ao.h.
//
// A vertex makes up to 26 x steps trilinear fetches, 8 samples each, so the samples must not come from global memory one by one.  The work
// unit is a NON-EMPTY BLOCK of the result: the scan of the extract has left one BlockDesc per such block (`active`, in list order) with the
// block's first triangle / vertex and their counts, vertices arrive in canonical order, so a block's vertices are one contiguous range of
// the records, and every fetch of theirs lies in the samples 8b - R .. 8b + 9 + R per axis, R = ceil(Rg) <= 6.  A workgroup stages that
// box once in LDS -- (10 + 2R)^3 floats, 42.6 KB at R = 6, 11 KB at R = 2, loaded as runs along x, indices clamped to the grid -- and every
// fetch then reads LDS.  fetch()'s clamp-to-edge needs no special case: the kernel evaluates the rule's own clamped index i0 in grid
// coordinates and subtracts the tile's origin, and a clamped i0 names a sample that is inside both the grid and the tile.
// Empty blocks have no BlockDesc and launch nothing.  A block with at most kAoDirectMax vertices is not worth a tile (10648 loads at R = 6):
// its workgroup fetches from global memory with the same code (route counters: vtmc_debug_ao_routes).
// The march itself and the pass of a workgroup over its block's records (the record loader, the chunks, the dword-assembled byte output)
// are ao_march.h's, shared with the level-of-detail pass of terrain_lodattr.hip.
#include "ao_march.h"
#include "material_filter.h"
#include "vtmc_ctx.h"

namespace vtmc {

struct AoArgs {
    const float *grid;  // the terrain's samples, x fastest
    int n[3];           // samples per axis
    const BlockDesc *active;
    BlockMap map;       // material_filter.h
    int reach, extent;  // R and 10 + 2R
    FastDiv d_extent;
    AoMarch march;      // ao_march.h
    uint32_t direct_max;
    uint32_t *stats;  // [0] workgroups that staged a tile, [1] workgroups on the direct route
    uint8_t *out;
};

// One workgroup per non-empty block; the march and the pass over the block's records are ao_march.h's.
template <bool INDEXED>
__global__ __launch_bounds__(256) void ao_kernel(const uint32_t *__restrict__ recs, AoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ __attribute__((aligned(16))) uint32_t rec[AoChunkLds<INDEXED>::REC_WORDS];
    __shared__ uint32_t outw[AoChunkLds<INDEXED>::OUT_WORDS];
    const BlockDesc d = a.active[blockIdx.x];
    const uint32_t first = INDEXED ? d.vert_base : d.tri_base;
    const uint32_t count = INDEXED ? d.vert_cnt : (d.cnt_mask & kCountMask);
    if (count == 0u) return;
    const uint32_t vpr = INDEXED ? 1u : 3u;
    int b[3];
    material_block(a.map, d.b, b[0], b[1], b[2]);
    AoField F;
    F.tile = tile;
    F.grid = a.grid;
    F.E = a.extent;
    F.stride = 1;
    for (int k = 0; k < 3; ++k) F.n[k] = F.dim[k] = a.n[k], F.o[k] = 8 * b[k] - a.reach;
    const bool direct = count * vpr <= a.direct_max;
    if (threadIdx.x == 0) atomicAdd(a.stats + (direct ? 1 : 0), 1u);
    if (!direct) {
        // the box, row by row along x; an index outside the grid takes the edge sample (never fetched: see the file comment)
        const uint32_t E = (uint32_t)a.extent, E3 = E * E * E;
        for (uint32_t i = threadIdx.x; i < E3; i += 256u) {
            const uint32_t row = a.d_extent.quot(i), x = i - row * E;
            const uint32_t z = a.d_extent.quot(row), y = row - z * E;
            int gx = F.o[0] + (int)x, gy = F.o[1] + (int)y, gz = F.o[2] + (int)z;
            gx = gx < 0 ? 0 : (gx > F.n[0] - 1 ? F.n[0] - 1 : gx);
            gy = gy < 0 ? 0 : (gy > F.n[1] - 1 ? F.n[1] - 1 : gy);
            gz = gz < 0 ? 0 : (gz > F.n[2] - 1 ? F.n[2] - 1 : gz);
            tile[i] = F.grid[(size_t)gx + (size_t)F.n[0] * ((size_t)gy + (size_t)F.n[1] * (size_t)gz)];
        }
    }
    const float base[3] = {(float)(8 * b[0]), (float)(8 * b[1]), (float)(8 * b[2])};
    ao_chunks<INDEXED, kAoGrid>(recs, first, count, direct, base, a.march, F, a.out, rec, outw);
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_ao_vertices(vtmc_ctx *ctx, const vtmc_ao_params *params, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!params) return fail(ctx, VTMC_ERR_INVALID_ARG, "params is null");
    if (int rc = attr_gate(ctx, "ao_vertices")) return rc;
    if (const char *fault = ao_params_fault(*params, ctx->tshape.scale)) return fail(ctx, VTMC_ERR_INVALID_ARG, "ao_vertices: %s", fault);
    const VtmcResult &res = ctx->result;
    const int64_t n = res.vertices();
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, ctx->ao_stats, 2 * sizeof(uint32_t))) return rc;
    VTMC_HIP(ctx, hipMemsetAsync(ctx->ao_stats.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    if (n > 0 && res.active > 0) {
        if (int rc = ensure(ctx, ctx->ao.values, ((size_t)n + 3) & ~(size_t)3)) return rc;
        const AoTables tb = ao_tables(*params, ctx->tshape.scale);
        AoArgs a{};
        a.grid = (const float *)ctx->terrain.p;
        a.n[0] = ctx->tshape.dim_x, a.n[1] = ctx->tshape.dim_y, a.n[2] = ctx->tshape.dim_z;
        a.active = (const BlockDesc *)ctx->active.p;
        a.map = block_map(res.space, res.blocks);
        a.reach = tb.reach, a.extent = tb.extent;
        a.d_extent = FastDiv((unsigned)tb.extent);
        a.march = ao_march(*params, tb);
        a.direct_max = (uint32_t)(ctx->ao_direct_max >= 0 ? ctx->ao_direct_max : kAoDirectMax);
        a.stats = (uint32_t *)ctx->ao_stats.p;
        a.out = (uint8_t *)ctx->ao.values.p;
        const size_t lds = ao_tile_bytes(tb.extent);
        if (res.indexed) VTMC_HIP(ctx, launch(ao_kernel<true>, dim3(res.active), dim3(256), lds, ctx->stream, (const uint32_t *)ctx->verts.p, a));
        else VTMC_HIP(ctx, launch(ao_kernel<false>, dim3(res.active), dim3(256), lds, ctx->stream, (const uint32_t *)ctx->tris.p, a));
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->ao.n = n;
    ctx->ao.epoch = res.epoch;
    if (n_vertices) *n_vertices = n;
    return VTMC_OK;
}

int32_t vtmc_ao_read_vertices(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    return attr_read(ctx, ctx->ao, "ao_read_vertices: no occlusion values of the current result (call vtmc_ao_vertices)", 1, dst, capacity_vertices);
}

int32_t vtmc_ao_device_results(vtmc_ctx *ctx, const uint8_t **d_ao, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    return attr_device_results(ctx, ctx->ao, "ao_device_results: no occlusion values of the current result (call vtmc_ao_vertices)", d_ao, n_vertices);
}

// Not part of the ABI (tests, tools/ao_bench.py): counts[0] = workgroups of the last vtmc_ao_vertices that staged a tile, counts[1] = those
// that took the direct route; direct_max >= 0 sets the vertex count up to which a block goes direct, -1 restores the default, -2 leaves it.
int32_t vtmc_debug_ao_routes(vtmc_ctx *ctx, uint32_t counts[2], int32_t direct_max)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (direct_max >= -1) ctx->ao_direct_max = direct_max;
    if (counts) {
        counts[0] = counts[1] = 0u;
        if (ctx->ao_stats.p) {
            VTMC_HIP(ctx, hipSetDevice(ctx->device));
            VTMC_HIP(ctx, hipMemcpy(counts, ctx->ao_stats.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    }
    return VTMC_OK;
}

}  // extern "C"
