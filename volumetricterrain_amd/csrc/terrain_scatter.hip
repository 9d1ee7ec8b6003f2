// terrain_scatter.hip -- instances scattered over the surface of a terrain extract (vtmc_scatter_*): area-weighted points on the triangles
// of the result, filtered by slope, world height and one channel of the material layer.  The rule, operation by operation, is in
// include/vtmc.h; the kernels follow it bit for bit (library built with -ffp-contract=off).  The host half -- argument checks, dc, the
// hash -- is terrain_scatter.h; the material filter and the block mapping are material_filter.h, the code the vertex weights use.
//
// The pass is the stream over the result's triangles of tri_stream_kernels.h: the scheme, its traffic and the bounds of every access are
// written down there, and the view of the result, the tiles, the loader (which clamps what it gathers: the scatter rests on the same
// bounds argument as the skirts), the offsets kernel and the host glue come from there.  The scatter's own: scatter_count_kernel
// evaluates every candidate of its triangle and writes one SURVIVOR MASK byte per triangle (bit i: candidate i survives; n <= 8); the
// host checks the grand total against max_instances; scatter_emit_kernel hashes only triangles with a set bit again and skips the
// filters, which the mask has already answered; an instance leaves as two 16-byte stores to its 32-byte slot, so a wave's stores fall
// into one contiguous run of the output.  One record per set bit.
#include "terrain_scatter.h"
#include "terrain_material.h"
#include "tri_stream_kernels.h"
#include <cmath>

namespace vtmc {

struct ScatterArgs {
    TriView v;
    MaterialVertexArgs m;      // the block mapping, and the layer when channel >= 0
    int channel;
    uint64_t k0;               // fin(seed + G)
    float dc, min_up, max_up, min_y, max_y;
    float scale, origin[3];
};

// a triangle as the rule reads it: block-local positions, record normals, the block
struct ScatterTri {
    float p[3][3], n[3][3];
    int b[3];
};

template <bool INDEXED>
__device__ __forceinline__ void scatter_load(const ScatterArgs &a, const uint32_t *rec, const uint32_t *range, uint32_t t, ScatterTri &tri)
{
    const uint32_t b = tri_block_of<INDEXED>(a.v, rec, range, t);
    material_block(a.m.map, b, tri.b[0], tri.b[1], tri.b[2]);   // before the gather: the list entry's load goes out first
    TriWords w;
    tri_load<INDEXED>(a.v, rec, t, b, w);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) tri.p[c][k] = __uint_as_float(w.p[c][k]), tri.n[c][k] = __uint_as_float(w.n[c][k]);
}

// the triangle's key: the seed, then the nine grid coordinates of its corners (+ 0.0f: -0 becomes +0)
__device__ __forceinline__ uint64_t scatter_key(const ScatterArgs &a, const ScatterTri &t)
{
    uint64_t k = a.k0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            float g = (float)(8 * t.b[x]) + t.p[c][x];
            g = g + 0.0f;
            k = scatter_step(k, (uint64_t)__float_as_uint(g));
        }
    return k;
}

// candidates of the triangle: 0 when it is degenerate or outside the slope band; the key is hashed only for a triangle that passes
__device__ __forceinline__ int scatter_candidates(const ScatterArgs &a, const ScatterTri &t, uint64_t &k)
{
    const float e1x = t.p[1][0] - t.p[0][0], e1y = t.p[1][1] - t.p[0][1], e1z = t.p[1][2] - t.p[0][2];
    const float e2x = t.p[2][0] - t.p[0][0], e2y = t.p[2][1] - t.p[0][1], e2z = t.p[2][2] - t.p[0][2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float L = sqrtf((cx * cx + cy * cy) + cz * cz);
    if (!(L > 0.0f) || !(L < INFINITY)) return 0;
    const float up = cy / L;
    if (!(a.min_up <= up && up <= a.max_up)) return 0;
    const float lam = (0.5f * L) * a.dc;
    const float fl = floorf(lam);
    k = scatter_key(a, t);
    if (fl >= (float)VTMC_SCATTER_MAX_PER_TRIANGLE) return VTMC_SCATTER_MAX_PER_TRIANGLE;   // the cap, before (int) can overflow
    const int n = (int)fl + (scatter_uniform(k, 0u, 0u) < lam - fl ? 1 : 0);
    return n < VTMC_SCATTER_MAX_PER_TRIANGLE ? n : VTMC_SCATTER_MAX_PER_TRIANGLE;
}

// Candidate i of the triangle.  FILTER: apply the height band and the material filter and report whether the candidate survives;
// otherwise (the mask has answered that) compute the instance.
template <bool FILTER>
__device__ __forceinline__ bool scatter_candidate(const ScatterArgs &a, const ScatterTri &t, uint64_t k, uint32_t i, float pos[3], float nrm[3])
{
    float u = scatter_uniform(k, i, 1u), v = scatter_uniform(k, i, 2u);
    if (u + v > 1.0f) u = 1.0f - u, v = 1.0f - v;
    float q[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const float e1 = t.p[1][x] - t.p[0][x], e2 = t.p[2][x] - t.p[0][x];
        q[x] = (t.p[0][x] + e1 * u) + e2 * v;
        pos[x] = a.origin[x] + ((float)(8 * t.b[x]) + q[x]) * a.scale;
    }
    if (FILTER) {
        if (!(a.min_y <= pos[1] && pos[1] <= a.max_y)) return false;
        if (a.channel >= 0) {
            const MaterialTaps taps = material_taps(a.m, t.b[0], t.b[1], t.b[2], q[0], q[1], q[2]);
            const float w = (float)material_filter_channel(taps, a.channel);
            if (!(scatter_uniform(k, i, 3u) * 255.0f < w)) return false;
        }
    } else {
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const float d1 = t.n[1][x] - t.n[0][x], d2 = t.n[2][x] - t.n[0][x];
            nrm[x] = (t.n[0][x] + d1 * u) + d2 * v;
        }
    }
    return true;
}

template <bool INDEXED>
__global__ __launch_bounds__(256) void scatter_count_kernel(ScatterArgs a, uint8_t *__restrict__ masks, uint32_t *__restrict__ tile_totals)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kTriTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    uint32_t t0, nt;
    tri_tile_bounds(a.v, t0, nt);
    if (INDEXED) tri_tile_bracket(a.v, range, t0, nt);
    else tri_tile_stage(a.v, rec, t0, nt);
    uint32_t mask = 0u;
    if (threadIdx.x < nt) {
        ScatterTri tri;
        scatter_load<INDEXED>(a, rec, range, t0 + threadIdx.x, tri);
        uint64_t k = 0;
        const int n = scatter_candidates(a, tri, k);
        float pos[3], nrm[3];
        for (int i = 0; i < n; ++i)
            if (scatter_candidate<true>(a, tri, k, (uint32_t)i, pos, nrm)) mask |= 1u << i;
    }
    masks[(size_t)t0 + threadIdx.x] = (uint8_t)mask;   // the buffer holds whole tiles: the ragged tile's tail is written as zeros
    uint32_t total;
    block_scan<4>((uint32_t)__popc(mask), wave_sums, total);
    if (threadIdx.x == 0) tile_totals[blockIdx.x] = total;
}

template <bool INDEXED>
__global__ __launch_bounds__(256) void scatter_emit_kernel(ScatterArgs a, const uint8_t *__restrict__ masks, const uint32_t *__restrict__ tile_offsets,
                                                           const uint32_t *__restrict__ group_offsets, uint32_t capacity, float4 *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kTriTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    uint32_t t0, nt;
    tri_tile_bounds(a.v, t0, nt);
    uint32_t mask = masks[(size_t)t0 + threadIdx.x];
    uint32_t total;
    const uint32_t before = block_scan<4>((uint32_t)__popc(mask), wave_sums, total);
    if (total == 0u) return;   // a tile without survivors reads no record (uniform across the workgroup)
    if (INDEXED) tri_tile_bracket(a.v, range, t0, nt);
    else tri_tile_stage(a.v, rec, t0, nt);
    if (mask == 0u || threadIdx.x >= nt) return;
    ScatterTri tri;
    scatter_load<INDEXED>(a, rec, range, t0 + threadIdx.x, tri);
    const uint64_t k = scatter_key(a, tri);
    uint32_t slot = group_offsets[blockIdx.x / (uint32_t)kScanThreads] + tile_offsets[blockIdx.x] + before;
    while (mask) {
        const uint32_t i = (uint32_t)__ffs(mask) - 1u;
        mask &= mask - 1u;
        float pos[3], nrm[3];
        scatter_candidate<false>(a, tri, k, i, pos, nrm);
        if (slot < capacity) {   // holds for the masks of this call; keeps a store inside the buffer whatever the masks say
            out[2 * (size_t)slot] = make_float4(pos[0], pos[1], pos[2], nrm[0]);
            out[2 * (size_t)slot + 1] = make_float4(nrm[1], nrm[2], __uint_as_float(t0 + threadIdx.x), __uint_as_float((uint32_t)(scatter_word(k, i, 4u) >> 32)));
        }
        ++slot;
    }
}

static bool scatter_current(const vtmc_ctx *ctx) { return ctx->result.valid && ctx->scatter.epoch == ctx->result.epoch; }

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_scatter_surface(vtmc_ctx *ctx, const vtmc_scatter_params *params, int64_t *n_instances)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!params) return fail(ctx, VTMC_ERR_INVALID_ARG, "params is null");
    if (int rc = attr_gate(ctx, "scatter_surface")) return rc;
    if (const char *fault = scatter_params_fault(*params, ctx->tshape.scale)) return fail(ctx, VTMC_ERR_INVALID_ARG, "scatter_surface: %s", fault);
    if (params->material_channel >= 0 && !ctx->mat_c)
        return fail(ctx, VTMC_ERR_NO_RESULT, "scatter_surface: material_channel %d before material_init", params->material_channel);
    const VtmcResult &res = ctx->result;
    VtmcTriStream &sc = ctx->scatter;
    const int64_t T = res.tris;
    const int B = res.blocks;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, sc.block_offsets, sizeof(int32_t) * ((size_t)B + 1))) return rc;
    sc.epoch = 0;   // from here on the buffers no longer hold the previous scatter
    StageClock<6> &clock = ctx->scatter_clock;
    VTMC_HIP(ctx, clock.begin());   // disarmed: a result without triangles leaves it so
    unsigned long long total = 0;
    if (T == 0 || B == 0) {
        VTMC_HIP(ctx, hipMemsetAsync(sc.block_offsets.p, 0, sizeof(int32_t) * ((size_t)B + 1), ctx->stream));
    } else {
        const uint32_t tiles = tri_tiles(T);
        ScanLayout scan(tiles);
        if (int rc = tri_stream_scratch(ctx, sc, T, &scan)) return rc;
        ScatterArgs a{};
        if (int rc = tri_view(ctx, "scatter_surface", &a.v)) return rc;   // refuses indexed triangles without vertices; the scatter is gone by now
        a.m.map = block_map(res.space, B);
        a.channel = params->material_channel;
        if (a.channel >= 0) {
            const int cells[3] = {ctx->tshape.dim_x - 2, ctx->tshape.dim_y - 2, ctx->tshape.dim_z - 2};
            a.m.layer = (const uint2 *)ctx->material.p;
            a.m.C = ctx->mat_c;
            material_vertex_scale(cells, a.m.C, a.m.s);
        }
        a.k0 = scatter_seed_key(params->seed);
        a.dc = scatter_density_cells(params->density, ctx->tshape.scale);
        a.min_up = params->min_up, a.max_up = params->max_up;
        a.min_y = params->min_y, a.max_y = params->max_y;
        a.scale = ctx->tshape.scale;
        for (int k = 0; k < 3; ++k) a.origin[k] = ctx->tshape.origin[k];
        uint8_t *masks = (uint8_t *)sc.masks.p;
        VTMC_HIP(ctx, clock.mark(0, ctx->stream));
        VTMC_HIP(ctx, launch(res.indexed ? scatter_count_kernel<true> : scatter_count_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a, masks, scan.tile_totals()));
        if (int rc = tri_scan_total(ctx, scan, clock, &total)) return rc;
        if (total > (unsigned long long)params->max_instances)
            return fail(ctx, VTMC_ERR_TOO_LARGE, "scatter_surface: %llu instances exceed max_instances %d", total, params->max_instances);
        if (total > 0)
            if (int rc = ensure(ctx, sc.records, sizeof(vtmc_instance) * (size_t)total)) return rc;
        VTMC_HIP(ctx, clock.mark(3, ctx->stream));
        if (total > 0)
            VTMC_HIP(ctx, launch(res.indexed ? scatter_emit_kernel<true> : scatter_emit_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a, masks, scan.tile_offsets(),
                                 scan.group_offsets(), (uint32_t)total, (float4 *)sc.records.p));
        if (int rc = tri_launch_offsets(ctx, a.v, sc, scan, 1u, clock)) return rc;
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sc.n = (int64_t)total;
    sc.blocks = B;
    sc.epoch = res.epoch;
    if (n_instances) *n_instances = sc.n;
    return VTMC_OK;
}

int32_t vtmc_scatter_read(vtmc_ctx *ctx, vtmc_instance *dst, int64_t capacity, int32_t *block_instance_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!scatter_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "scatter_read: no instances of the current result (call vtmc_scatter_surface)");
    return tri_stream_read(ctx, ctx->scatter, sizeof(vtmc_instance), "instances", VTMC_ERR_INVALID_ARG, dst, capacity, block_instance_offsets);
}

int32_t vtmc_scatter_device_results(vtmc_ctx *ctx, const vtmc_instance **d_instances, const int32_t **d_block_offsets, int64_t *n_instances)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!scatter_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "scatter_device_results: no instances of the current result (call vtmc_scatter_surface)");
    tri_stream_device_results(ctx->scatter, d_instances, d_block_offsets, n_instances);
    return VTMC_OK;
}

// Not part of the ABI (tools/scatter_bench.py): device time of the last vtmc_scatter_surface that launched kernels, ms[0..3] = the count
// kernel, the scan, the emit kernel, the block offsets.
int32_t vtmc_debug_scatter_ms(vtmc_ctx *ctx, float ms[4])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    return tri_stream_ms(ctx, ctx->scatter_clock, "debug_scatter_ms before a scatter that launched kernels", ms);
}

}  // extern "C"
