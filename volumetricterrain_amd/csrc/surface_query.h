// surface_query.h -- the host side the surface queries share (raycast.hip, spherequery.hip): how a caller's grid or the resident terrain
// becomes a SurfaceGrid (mc_cell.h), the argument rules of a batch, and the staging of a host batch through ctx->rays / ctx->h_rays.
#ifndef VTMC_SURFACE_QUERY_H
#define VTMC_SURFACE_QUERY_H
#include "vtmc_ctx.h"
#include "mc_cell.h"
#include <cmath>
#include <cstring>

namespace vtmc {

// a caller's device grid of nx x ny x nz cells: the checks of the _device entry points, then the fill
static inline int surface_of_grid(vtmc_ctx *ctx, const float *d_grid, int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz, const float origin[3],
                           float scale, SurfaceGrid *g)
{
    if (int rc = check_dims(ctx, nx, ny, nz)) return rc;
    if (!(scale > 0.0f) || !std::isfinite(scale)) return fail(ctx, VTMC_ERR_INVALID_ARG, "voxel_scale must be positive and finite");
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return fail(ctx, VTMC_ERR_INVALID_ARG, "origin is not finite");
    *g = SurfaceGrid{d_grid, sx, sy, sz, {nx, ny, nz}, {origin[0], origin[1], origin[2]}, scale, ctx->tables.vert_packed};
    return VTMC_OK;
}

// the resident terrain: dim samples per axis carry a 1-sample border, so dim - 2 cells are meshed (as extract_dirty's dense_space); x fastest
static inline SurfaceGrid surface_of_terrain(const vtmc_ctx *ctx)
{
    const TerrainShape &sh = ctx->tshape;
    return SurfaceGrid{(const float *)ctx->terrain.p, 1, sh.dim_x, (long long)sh.dim_x * sh.dim_y, {sh.dim_x - 2, sh.dim_y - 2, sh.dim_z - 2},
                       {sh.origin[0], sh.origin[1], sh.origin[2]}, sh.scale, ctx->tables.vert_packed};
}

// the rules every batch shares; `count` names the count in the error text
static inline int check_batch(vtmc_ctx *ctx, int32_t n, const char *count, bool null_arg)
{
    if (n < 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "%s < 0", count);
    if (n > 0 && null_arg) return fail(ctx, VTMC_ERR_INVALID_ARG, "null argument");
    return VTMC_OK;
}
// ... and the one every cast adds
static inline int check_max_distance(vtmc_ctx *ctx, float max_distance)
{
    if (!(max_distance > 0.0f)) return fail(ctx, VTMC_ERR_INVALID_ARG, "max_distance must be positive (+inf allowed)");
    return VTMC_OK;
}

// A host batch on its way through the device: ctx->rays holds  input 0 | input 1 | input 2 | pad | hits  (absent inputs take no room, the
// hit records start at a 16-byte boundary), ctx->h_rays the same bytes in pinned memory.
struct QueryStage {
    const float *in[3];  // device; null where the input is absent
    void *hits;          // device
    size_t hit_off, hit_bytes;
};

// grows both buffers, packs the host inputs (src[i] of bytes[i] bytes, or null) and queues their upload on the context's stream
static inline int stage_queries(vtmc_ctx *ctx, const float *const src[3], const size_t bytes[3], size_t hit_bytes, QueryStage *st)
{
    size_t off[3], end = 0;
    for (int i = 0; i < 3; ++i) {
        off[i] = end;
        if (src[i]) end += bytes[i];
    }
    st->hit_off = (end + 15) & ~(size_t)15;
    st->hit_bytes = hit_bytes;
    const size_t total = st->hit_off + hit_bytes;
    if (int rc = ensure(ctx, ctx->rays, total)) return rc;
    if (ctx->h_rays.bytes < total) VTMC_HIP(ctx, pin(ctx->h_rays, total));
    unsigned char *h = ctx->h_rays.p, *dv = (unsigned char *)ctx->rays.p;
    for (int i = 0; i < 3; ++i) {
        st->in[i] = src[i] ? (const float *)(dv + off[i]) : nullptr;
        if (src[i]) memcpy(h + off[i], src[i], bytes[i]);
    }
    st->hits = dv + st->hit_off;
    VTMC_HIP(ctx, hipMemcpyAsync(dv, h, end, hipMemcpyHostToDevice, ctx->stream));
    return VTMC_OK;
}

// behind the kernel: the hit records come back, the stream is drained, and they go to the caller
static inline int fetch_hits(vtmc_ctx *ctx, const QueryStage &st, void *hits)
{
    unsigned char *h = ctx->h_rays.p + st.hit_off;
    VTMC_HIP(ctx, hipMemcpyAsync(h, st.hits, st.hit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(hits, h, st.hit_bytes);
    return VTMC_OK;
}

}  // namespace vtmc
#endif
