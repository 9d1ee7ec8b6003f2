// terrain_scatter.hip -- instances scattered over the surface of a terrain extract (vtmc_scatter_*): area-weighted points on the triangles
// of the result, filtered by slope, world height and one channel of the material layer.  The rule, operation by operation, is in
// include/vtmc.h; the kernels follow it bit for bit (library built with -ffp-contract=off).  The host half -- argument checks, dc, the
// tile count, the hash -- is terrain_scatter.h; the material filter and the block mapping are material_filter.h, the code the vertex
// weights use.
//
// The pass is a stream over the records, in tiles of kScatterTile = 256 triangles, one lane per triangle, and no atomic decides where an
// instance goes: the order is a function of the result alone.
//   1. scatter_count_kernel  evaluates every candidate of its triangle and writes one SURVIVOR MASK byte per triangle (bit i: candidate i
//      survives; n <= 8) and the tile's survivor total.
//   2. the scan of the tile totals, in two levels: scan_tiles_kernel gives every tile its prefix inside its group of 1024 tiles
//      and every group its total; scan_groups_kernel, one workgroup, scans the group totals (at most 8192 of them) and leaves the
//      grand total, which goes to the host for the max_instances check and the growth of the instance buffer.  A tile's offset is the sum
//      of the two prefixes.  (One workgroup over all the tile totals took 0.19 ms of the pass's 0.88 at 1024^3: profiles/r19/scatter.)
//   3. scatter_emit_kernel   the same tiling; a workgroup scan of the masks' popcounts gives every lane its slot; only triangles with a
//      set bit are loaded into registers and hashed again, only set bits are recomputed, and the filters, which the mask has already
//      answered, are skipped.  An instance leaves as two 16-byte stores to its 32-byte slot; a lane's instances are consecutive slots and
//      consecutive lanes continue each other, so a wave's stores fall into one contiguous run of the output.
//   4. scatter_block_offsets_kernel  a thread per block of the result: the tile offset of the block's first triangle plus the popcounts
//      of the mask bytes of the tile before it, read as dwords.
// Soup records come into LDS as consecutive 16-byte pieces (record_tile.h), never at a 76-byte lane stride; a lane then reads its record
// at a stride of 19 dwords, which is odd, so the LDS banks do not collide.  In indexed mode a lane finds its block in the triangle offsets
// (two lanes bracket the tile's blocks first), reads its index triple and gathers its three vtmc_vertex through the block's vertex offset;
// the vertices of a block are shared by about six triangles and come from L2.
// Traffic that must reach HBM, soup: 76 T (count) + T (masks out) + T (masks in) + 76 T' (emit: the tiles with a survivor) + 32 N.
#include "terrain_scatter.h"
#include "material_filter.h"
#include "record_tile.h"
#include "scan_kernels.h"
#include "terrain_material.h"
#include "vtmc_ctx.h"
#include <cmath>

namespace vtmc {

struct ScatterArgs {
    const uint32_t *recs;      // soup: T records of 19 dwords (vtmc_triangle); indexed: V records of 6 dwords (vtmc_vertex)
    const int32_t *indices;    // indexed: 3 T block-local indices
    const uint32_t *toffsets;  // the n_blocks + 1 per-block triangle offsets
    const uint32_t *voffsets;  // indexed: the n_blocks + 1 per-block vertex offsets
    uint32_t n_tris;
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
    if (INDEXED) {
        const uint32_t b = material_block_of(a.toffsets, range[0], range[1], t);
        material_block(a.m, b, tri.b[0], tri.b[1], tri.b[2]);
        const uint32_t vb = a.voffsets[b];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // a vtmc_vertex is 24 bytes at a multiple of 24: three 8-byte loads
            const uint2 *r = reinterpret_cast<const uint2 *>(a.recs + 6 * ((size_t)vb + (uint32_t)a.indices[3 * (size_t)t + c]));
            const uint2 r0 = r[0], r1 = r[1], r2 = r[2];
            tri.p[c][0] = __uint_as_float(r0.x), tri.p[c][1] = __uint_as_float(r0.y), tri.p[c][2] = __uint_as_float(r1.x);
            tri.n[c][0] = __uint_as_float(r1.y), tri.n[c][1] = __uint_as_float(r2.x), tri.n[c][2] = __uint_as_float(r2.y);
        }
    } else {
        const uint32_t *r = rec + 19u * (t % (uint32_t)kScatterTile);
        material_block(a.m, r[18], tri.b[0], tri.b[1], tri.b[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) tri.p[c][k] = __uint_as_float(r[3 * c + k]), tri.n[c][k] = __uint_as_float(r[9 + 3 * c + k]);
    }
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

// the tile of a workgroup: soup records into LDS; indexed, the blocks of the tile's first and last triangle
template <bool INDEXED>
__device__ __forceinline__ void scatter_stage(const ScatterArgs &a, uint32_t *rec, uint32_t *range, uint32_t t0, uint32_t nt)
{
    if (INDEXED) {
        if (threadIdx.x < 2) range[threadIdx.x] = material_block_of(a.toffsets, 0u, a.m.n_blocks - 1, threadIdx.x ? t0 + nt - 1 : t0);
    } else {
        load_record_tile(rec, a.recs + (size_t)t0 * 19, nt * 19);  // tile base: 256 * 76 bytes per tile, 16-byte aligned
    }
    __syncthreads();
}

template <bool INDEXED>
__global__ __launch_bounds__(256) void scatter_count_kernel(ScatterArgs a, uint8_t *__restrict__ masks, uint32_t *__restrict__ tile_totals)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kScatterTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    const uint32_t t0 = blockIdx.x * (uint32_t)kScatterTile;
    const uint32_t nt = a.n_tris - t0 < (uint32_t)kScatterTile ? a.n_tris - t0 : (uint32_t)kScatterTile;
    scatter_stage<INDEXED>(a, rec, range, t0, nt);
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
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kScatterTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    const uint32_t t0 = blockIdx.x * (uint32_t)kScatterTile;
    const uint32_t nt = a.n_tris - t0 < (uint32_t)kScatterTile ? a.n_tris - t0 : (uint32_t)kScatterTile;
    uint32_t mask = masks[(size_t)t0 + threadIdx.x];
    uint32_t total;
    const uint32_t before = block_scan<4>((uint32_t)__popc(mask), wave_sums, total);
    if (total == 0u) return;   // a tile without survivors reads no record (uniform across the workgroup)
    scatter_stage<INDEXED>(a, rec, range, t0, nt);
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

// out[b], b = 0..n_blocks: the instances on triangles before the block's first one
__global__ __launch_bounds__(256) void scatter_block_offsets_kernel(const uint32_t *__restrict__ toffsets, uint32_t n_blocks, uint32_t n_tris,
                                                                    const uint32_t *__restrict__ mask_words, const uint32_t *__restrict__ tile_offsets,
                                                                    const uint32_t *__restrict__ group_offsets, const unsigned long long *__restrict__ total,
                                                                    int32_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > n_blocks) return;
    const uint32_t t = toffsets[b];
    if (t >= n_tris) {
        out[b] = (int32_t)*total;
        return;
    }
    const uint32_t tile = t / (uint32_t)kScatterTile, r = t % (uint32_t)kScatterTile;
    const uint32_t *w = mask_words + (size_t)tile * (kScatterTile / 4);
    uint32_t sum = group_offsets[tile / (uint32_t)kScanThreads] + tile_offsets[tile];
    for (uint32_t j = 0; j < r / 4u; ++j) sum += (uint32_t)__popc(w[j]);
    if (r & 3u) sum += (uint32_t)__popc(w[r / 4u] & ((1u << (8u * (r & 3u))) - 1u));
    out[b] = (int32_t)sum;
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
    VtmcScatter &sc = ctx->scatter;
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
        const uint32_t tiles = scatter_tiles(T);
        if (int rc = ensure(ctx, sc.masks, scatter_mask_bytes(T))) return rc;
        if (int rc = ensure(ctx, sc.tiles, ScanLayout(tiles).bytes())) return rc;
        const ScanLayout scan(tiles, sc.tiles.p);
        ScatterArgs a{};
        a.recs = (const uint32_t *)(res.indexed ? ctx->verts.p : ctx->tris.p);
        a.indices = (const int32_t *)ctx->indices.p;
        a.toffsets = (const uint32_t *)ctx->offsets.p;
        a.voffsets = (const uint32_t *)ctx->voffsets.p;
        a.n_tris = (uint32_t)T;
        const BlockSpace &sp = res.space;
        a.m.list = sp.list;
        a.m.n_blocks = (uint32_t)B;
        a.m.nbx = sp.nbx, a.m.nby = sp.nby;
        a.m.d_nbx = sp.d_nbx, a.m.d_nby = sp.d_nby;
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
        VTMC_HIP(ctx, clock.mark(1, ctx->stream));
        VTMC_HIP(ctx, launch_scan(scan, ctx->stream));
        VTMC_HIP(ctx, clock.mark(2, ctx->stream));
        VTMC_HIP(ctx, hipMemcpyAsync(&total, scan.total(), sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (total > (unsigned long long)params->max_instances)
            return fail(ctx, VTMC_ERR_TOO_LARGE, "scatter_surface: %llu instances exceed max_instances %d", total, params->max_instances);
        if (total > 0)
            if (int rc = ensure(ctx, sc.instances, sizeof(vtmc_instance) * (size_t)total)) return rc;
        VTMC_HIP(ctx, clock.mark(3, ctx->stream));
        if (total > 0)
            VTMC_HIP(ctx, launch(res.indexed ? scatter_emit_kernel<true> : scatter_emit_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a, masks, scan.tile_offsets(),
                                 scan.group_offsets(), (uint32_t)total, (float4 *)sc.instances.p));
        VTMC_HIP(ctx, clock.mark(4, ctx->stream));
        VTMC_HIP(ctx, launch(scatter_block_offsets_kernel, lanes256((int64_t)B + 1), dim3(256), 0, ctx->stream, a.toffsets, (uint32_t)B, (uint32_t)T,
                             (const uint32_t *)sc.masks.p, scan.tile_offsets(), scan.group_offsets(), scan.total(), (int32_t *)sc.block_offsets.p));
        VTMC_HIP(ctx, clock.mark(5, ctx->stream));
        clock.arm();
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
    const VtmcScatter &sc = ctx->scatter;
    if (capacity < sc.n) return fail(ctx, VTMC_ERR_INVALID_ARG, "capacity %lld < %lld instances", (long long)capacity, (long long)sc.n);
    if (sc.n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (sc.n > 0) VTMC_HIP(ctx, hipMemcpy(dst, sc.instances.p, sizeof(vtmc_instance) * (size_t)sc.n, hipMemcpyDeviceToHost));
    if (block_instance_offsets)
        VTMC_HIP(ctx, hipMemcpy(block_instance_offsets, sc.block_offsets.p, sizeof(int32_t) * ((size_t)sc.blocks + 1), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_scatter_device_results(vtmc_ctx *ctx, const vtmc_instance **d_instances, const int32_t **d_block_offsets, int64_t *n_instances)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!scatter_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "scatter_device_results: no instances of the current result (call vtmc_scatter_surface)");
    if (d_instances) *d_instances = (const vtmc_instance *)ctx->scatter.instances.p;
    if (d_block_offsets) *d_block_offsets = (const int32_t *)ctx->scatter.block_offsets.p;
    if (n_instances) *n_instances = ctx->scatter.n;
    return VTMC_OK;
}

// Not part of the ABI (tools/scatter_bench.py): device time of the last vtmc_scatter_surface that launched kernels, ms[0..3] = the count
// kernel, the scan, the emit kernel, the block offsets.
int32_t vtmc_debug_scatter_ms(vtmc_ctx *ctx, float ms[4])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->scatter_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_scatter_ms before a scatter that launched kernels");
    if (int rc = ctx->scatter_clock.sync_last(ctx)) return rc;
    static const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
    for (int i = 0; i < 4; ++i)
        if (int rc = ctx->scatter_clock.elapsed(ctx, pairs[i][0], pairs[i][1], &ms[i])) return rc;
    return VTMC_OK;
}

}  // extern "C"
