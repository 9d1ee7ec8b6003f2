// terrain_material.hip -- the material layer: the device form of VoxelTerrain.SetControlMap (VoxelTerrain.cs:186-209), a paint brush on it
// and the material weights of every vertex of an extracted mesh (vtmc_material_*).  The rule, operation by operation, is in
// include/vtmc.h; the kernels follow it bit for bit (library built with -ffp-contract=off).  The host half -- argument checks, the
// per-axis factors, the texel box of a paint call -- is terrain_material.h.
//
// The vertex pass is the hot one: one pass over the result of an extract.  A soup record is 19 dwords, so a lane that reads "its" record
// walks memory at a 76-byte stride; instead a workgroup loads a tile of kMatTile records as consecutive 16-byte pieces into LDS (every
// 128-byte line arrives whole either way, and only once), then each VERTEX gets a lane: vertex 3t + v reads dwords 3v..3v+2 and 18 of
// record t from LDS.  Consecutive lanes own consecutive vertices, so their 8-byte results are consecutive in memory and the store is
// coalesced as it stands: no LDS stage on the way out.  Per vertex the kernel fetches 8 texels, each as one 8-byte load; the cube is at
// most 128^3 x 8 B = 16 MB, read-shared by every wave, and lives in L2 and the Infinity Cache.  Traffic that must reach HBM:
// 76 T read + 24 T written (soup), 24 V + 8 V (indexed).
#include "terrain_material.h"
#include "material_filter.h"
#include "record_tile.h"
#include "vtmc_ctx.h"
#include <cmath>

namespace vtmc {

struct MaterialPaintArgs {
    float ts[3], origin[3];
    int C;
    int lo[3], n[3];  // the texel box the launch walks
    int n_strokes;
};

// soup: out[3t + v] = the weights of corner v of triangle t
__global__ __launch_bounds__(256) void material_soup_kernel(const uint32_t *__restrict__ tris, uint32_t n_tris, uint2 *__restrict__ out, MaterialVertexArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 19];
    material_soup_tile(tris, n_tris, out, a, MaterialOfBlocks{}, rec);
}

// indexed: out[v] = the weights of vertex v, its block found through the n_blocks + 1 per-block vertex offsets
__global__ __launch_bounds__(256) void material_indexed_kernel(const uint32_t *__restrict__ verts, uint32_t n_verts, const uint32_t *__restrict__ voffsets,
                                                               uint2 *__restrict__ out, MaterialVertexArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 6];
    __shared__ uint32_t range[2];
    material_indexed_tile(verts, n_verts, voffsets, out, a, MaterialOfBlocks{}, rec, range);
}

// every texel (255,0,0,0, 0,0,0,0): TerrainSample starts with _matComponents[0] = 1
__global__ __launch_bounds__(256) void material_fill_kernel(uint2 *__restrict__ layer, uint32_t n)
{
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id < n) layer[id] = make_uint2(255u, 0u);
}

__device__ __forceinline__ uint32_t material_quantise(float c)
{
    c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    return (uint32_t)rintf(c * 255.0f);
}

// set_control_map: the Color of every texel into the four bytes of its group (half 0: group 1, half 1: group 2), the other four kept
__global__ __launch_bounds__(256) void material_quantise_kernel(uint32_t *__restrict__ layer, const float4 *__restrict__ img, uint32_t n, int half)
{
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n) return;
    const float4 c = img[id];
    layer[2 * (size_t)id + half] = material_quantise(c.x) | material_quantise(c.y) << 8 | material_quantise(c.z) << 16 | material_quantise(c.w) << 24;
}

// paint: a thread per texel of the box, every stroke of the call in order; the strokes are read at a wave-uniform index
__global__ __launch_bounds__(256) void material_paint_kernel(uint2 *__restrict__ layer, const vtmc_material_stroke *__restrict__ strokes, MaterialPaintArgs a)
{
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= (uint32_t)a.n[0] * (uint32_t)a.n[1] * (uint32_t)a.n[2]) return;
    const uint32_t row = id / (uint32_t)a.n[0];
    const int i = a.lo[0] + (int)(id - row * (uint32_t)a.n[0]);
    const int j = a.lo[1] + (int)(row % (uint32_t)a.n[1]), k = a.lo[2] + (int)(row / (uint32_t)a.n[1]);
    const float px = ((float)i + 0.5f) * a.ts[0] + a.origin[0];
    const float py = ((float)j + 0.5f) * a.ts[1] + a.origin[1];
    const float pz = ((float)k + 0.5f) * a.ts[2] + a.origin[2];
    uint2 *texel = layer + (i + a.C * (j + a.C * k));
    const uint2 old = *texel;
    float v[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) v[ch] = material_channel(old, ch);
    bool touched = false;
    for (int s = 0; s < a.n_strokes; ++s) {
        const vtmc_material_stroke st = strokes[s];
        const float dx = px - st.center[0], dy = py - st.center[1], dz = pz - st.center[2];
        const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
        float t = 1.0f - d / st.radius;
        t = t + t;
        t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
        const float w = st.strength * t;
        if (w == 0.0f) continue;
        touched = true;
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            const float T = ch == st.channel ? 255.0f : 0.0f;
            v[ch] = rintf(v[ch] + (T - v[ch]) * w);  // the byte the stroke leaves, as the float the next stroke reads
        }
    }
    if (!touched) return;
    uint32_t out[2] = {0u, 0u};
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) out[ch >> 2] |= ((uint32_t)v[ch] & 0xffu) << (8 * (ch & 3));
    *texel = make_uint2(out[0], out[1]);
}

void material_drop(vtmc_ctx *ctx)
{
    ctx->mat_c = 0;
    ctx->mat_weights.n = 0;
    ctx->mat_weights.epoch = 0;
    release(ctx->material);
    release(ctx->mat_image);
}

static size_t material_texels(const vtmc_ctx *ctx) { return (size_t)ctx->mat_c * ctx->mat_c * ctx->mat_c; }

static int need_layer(vtmc_ctx *ctx, const char *who)
{
    if (!ctx->mat_c) return fail(ctx, VTMC_ERR_NO_RESULT, "%s before material_init", who);
    return VTMC_OK;
}

static void terrain_cells(const vtmc_ctx *ctx, int cells[3])
{
    cells[0] = ctx->tshape.dim_x - 2, cells[1] = ctx->tshape.dim_y - 2, cells[2] = ctx->tshape.dim_z - 2;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_material_init(vtmc_ctx *ctx, int32_t fineness)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "material_init before terrain_init");
    const int C = material_size(fineness);
    if (!C) return fail(ctx, VTMC_ERR_INVALID_ARG, "fineness %d not in %d..%d", fineness, kMaterialMinFineness, kMaterialMaxFineness);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    material_drop(ctx);
    const size_t n = (size_t)C * C * C;
    if (int rc = ensure(ctx, ctx->material, n * VTMC_MATERIAL_CHANNELS)) return rc;
    VTMC_HIP(ctx, launch(material_fill_kernel, lanes256(n), dim3(256), 0, ctx->stream, (uint2 *)ctx->material.p, (uint32_t)n));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mat_c = C;
    return VTMC_OK;
}

int32_t vtmc_material_set_control_map(vtmc_ctx *ctx, const float *rgba, int32_t group)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = need_layer(ctx, "material_set_control_map")) return rc;
    if (!rgba) return fail(ctx, VTMC_ERR_INVALID_ARG, "rgba is null");
    if (group != 1 && group != 2) return fail(ctx, VTMC_ERR_INVALID_ARG, "invalid group %d: expected 1 or 2", group);  // VoxelTerrain.cs:188-189
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = material_texels(ctx), bytes = n * 4 * sizeof(float);
    // the image goes through the pinned stage, checked on the way in; without one, from where it lies
    float *stage = pinned_stage(ctx, bytes);
    const long long bad = stage ? material_copy_checked(stage, rgba, n * 4) : material_first_nan(rgba, n * 4);
    if (bad >= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "set_control_map: channel %lld of texel %lld is NaN", bad % 4, bad / 4);
    if (int rc = ensure(ctx, ctx->mat_image, bytes)) return rc;
    VTMC_HIP(ctx, hipMemcpyAsync(ctx->mat_image.p, stage ? stage : rgba, bytes, hipMemcpyHostToDevice, ctx->stream));
    VTMC_HIP(ctx, launch(material_quantise_kernel, lanes256(n), dim3(256), 0, ctx->stream, (uint32_t *)ctx->material.p, (const float4 *)ctx->mat_image.p, (uint32_t)n,
                         group - 1));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the stage and rgba are free again
    return VTMC_OK;
}

int32_t vtmc_material_write(vtmc_ctx *ctx, const uint8_t *src)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = need_layer(ctx, "material_write")) return rc;
    if (!src) return fail(ctx, VTMC_ERR_INVALID_ARG, "src is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VTMC_HIP(ctx, hipMemcpy(ctx->material.p, src, material_texels(ctx) * VTMC_MATERIAL_CHANNELS, hipMemcpyHostToDevice));
    return VTMC_OK;
}

int32_t vtmc_material_read(vtmc_ctx *ctx, uint8_t *dst, int32_t *size)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = need_layer(ctx, "material_read")) return rc;
    if (size) *size = ctx->mat_c;
    if (!dst) return VTMC_OK;  // size query
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VTMC_HIP(ctx, hipMemcpy(dst, ctx->material.p, material_texels(ctx) * VTMC_MATERIAL_CHANNELS, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_material_paint(vtmc_ctx *ctx, const vtmc_material_stroke *strokes, int32_t n_strokes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = need_layer(ctx, "material_paint")) return rc;
    if (n_strokes < 0 || n_strokes > VTMC_MATERIAL_MAX_STROKES)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "n_strokes %d not in 0..%d", n_strokes, VTMC_MATERIAL_MAX_STROKES);
    if (n_strokes > 0 && !strokes) return fail(ctx, VTMC_ERR_INVALID_ARG, "strokes is null");
    const char *fault = nullptr;
    const int32_t bad = material_check_strokes(strokes, n_strokes, &fault);
    if (bad >= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "stroke %d: %s", bad, fault);
    if (n_strokes == 0) return VTMC_OK;
    MaterialPaintArgs a{};
    int cells[3];
    terrain_cells(ctx, cells);
    a.C = ctx->mat_c;
    material_texel_size(cells, ctx->tshape.scale, a.C, a.ts);
    for (int k = 0; k < 3; ++k) a.origin[k] = ctx->tshape.origin[k];
    const MaterialBox box = material_paint_box(strokes, n_strokes, a.ts, a.origin, a.C);
    const size_t n = (size_t)box.n[0] * box.n[1] * box.n[2];
    if (n == 0) return VTMC_OK;  // no stroke reaches a texel
    for (int k = 0; k < 3; ++k) a.lo[k] = box.lo[k], a.n[k] = box.n[k];
    a.n_strokes = n_strokes;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, ctx->mat_strokes, sizeof(vtmc_material_stroke) * VTMC_MATERIAL_MAX_STROKES)) return rc;
    VTMC_HIP(ctx, hipMemcpyAsync(ctx->mat_strokes.p, strokes, sizeof(vtmc_material_stroke) * (size_t)n_strokes, hipMemcpyHostToDevice, ctx->stream));
    VTMC_HIP(ctx, launch(material_paint_kernel, lanes256(n), dim3(256), 0, ctx->stream, (uint2 *)ctx->material.p, (const vtmc_material_stroke *)ctx->mat_strokes.p, a));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // strokes is borrowed for the call; the next call may overwrite mat_strokes
    return VTMC_OK;
}

int32_t vtmc_material_vertices(vtmc_ctx *ctx, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = need_layer(ctx, "material_vertices")) return rc;
    if (int rc = attr_gate(ctx, "material_vertices")) return rc;
    const VtmcResult &res = ctx->result;
    const int64_t n = res.vertices();
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        if (int rc = ensure(ctx, ctx->mat_weights.values, (size_t)n * VTMC_MATERIAL_CHANNELS)) return rc;
        MaterialVertexArgs a{};
        int cells[3];
        terrain_cells(ctx, cells);
        a.layer = (const uint2 *)ctx->material.p;
        a.C = ctx->mat_c;
        material_vertex_scale(cells, a.C, a.s);
        a.map = block_map(res.space, res.blocks);
        if (res.indexed) {
            const uint32_t V = (uint32_t)res.verts;
            VTMC_HIP(ctx, launch(material_indexed_kernel, dim3((V + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->verts.p, V,
                                 (const uint32_t *)ctx->voffsets.p, (uint2 *)ctx->mat_weights.values.p, a));
        } else {
            const uint32_t T = (uint32_t)res.tris;
            VTMC_HIP(ctx, launch(material_soup_kernel, dim3((T + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->tris.p, T,
                                 (uint2 *)ctx->mat_weights.values.p, a));
        }
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->mat_weights.n = n;
    ctx->mat_weights.epoch = res.epoch;
    if (n_vertices) *n_vertices = n;
    return VTMC_OK;
}

int32_t vtmc_material_read_vertices(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    return attr_read(ctx, ctx->mat_weights, "material_read_vertices: no vertex weights of the current result (call vtmc_material_vertices)",
                     VTMC_MATERIAL_CHANNELS, dst, capacity_vertices);
}

int32_t vtmc_material_device_results(vtmc_ctx *ctx, const uint8_t **d_weights, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    return attr_device_results(ctx, ctx->mat_weights, "material_device_results: no vertex weights of the current result (call vtmc_material_vertices)",
                               d_weights, n_vertices);
}

}  // extern "C"
