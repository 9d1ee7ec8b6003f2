// terrain.hip -- device-resident density grid with the reference's CSG write semantics: the
// "density-field sampler" stage of the path (hand-written gfx950 / CDNA4).
//
// Replaces (paths relative to /root/reference/Unity-Project/Assets/Scripts/):
//   VoxelTerrain.cs:145-149  Init: grid filled with "void" values            -> terrain_fill_kernel
//   VoxelTerrain.cs:284-305  Update: per-sample QueryDensity + clamp + max / min -> terrain_modify_kernel
//   TerrainModifier.cs:59-62 (plane), :79-82 (sphere), :143-149 (cylinder),
//   IslandModifier.cs:45-73 (bilinear heightmap, the modifier of the world build TerrainEngine.cs:87) -> query_density
// One lane per sample of the modifier's AABB, x fastest (the grid is x fastest), so a wave reads and
// writes contiguous 256-byte row segments.  HBM-bound: 8 bytes per touched sample, a handful of
// FP32 operations in the reference's order (library built with -ffp-contract=off; sqrt is the
// correctly rounded one, as Mathf.Sqrt = (float)Math.Sqrt is).
//
// voidDensity / fullDensity (VoxelTerrain.cs:50-51) are FRESH random numbers in [-2,-1] / [1,2] on
// every read in the reference (UnityEngine.Random: a stream nobody can replay).  Here they are a
// counter-based hash of (seed, event, sample index, draw index) -- same ranges, same number of
// draws per sample (2 per add, 4 per erode, 1 per Init sample), deterministic; the CPU oracle
// restates the same hash (oracle/terrain_ref.c).
#include "terrain_edit.h"
#include "terrain_stamp.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

namespace vtmc {

__device__ __forceinline__ float clampf(float v, float lo, float hi)  // Mathf.Clamp
{
    if (v < lo) v = lo;
    else if (v > hi) v = hi;
    return v;
}

__device__ __forceinline__ float lerp_unity(float a, float b, float t)  // Mathf.Lerp: a + (b - a) * Clamp01(t)
{
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    return a + (b - a) * t;
}

__device__ __forceinline__ float query_density(const TerrainModifierArgs &m, float px, float py, float pz)
{
    if (m.kind == 0) return m.p[0] - py;  // PlaneModifier: _height - pos.y
    if (m.kind == 1) {                    // SphereModifier: _radius - (pos - _center).magnitude
        const float dx = px - m.p[0], dy = py - m.p[1], dz = pz - m.p[2];
        return m.p[3] - __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    }
    // CylinderModifier: Min(projLength, _axisLength - projLength, _radius - Sqrt(|start2pos|^2 - projLength^2))
    const float sx = px - m.p[0], sy = py - m.p[1], sz = pz - m.p[2];
    const float proj = sx * m.p[3] + sy * m.p[4] + sz * m.p[5];
    const float sq = sx * sx + sy * sy + sz * sz;
    const float c = m.p[7] - __builtin_sqrtf(sq - proj * proj);
    float r = proj;  // Mathf.Min(params): `if (v < min) min = v`, so a NaN candidate is skipped
    const float b = m.p[6] - proj;
    if (b < r) r = b;
    if (c < r) r = c;
    return r;
}

__global__ __launch_bounds__(256) void terrain_fill_kernel(float *__restrict__ grid, long long n, uint64_t seed)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        grid[i] = terrain_uniform(seed, 0u, (uint64_t)i, 0u) - 2.0f;  // voidDensity
}

// What of a modifier's density does not depend on y (the heightmap's bilinear fetch): evaluated once
// per (x, z) column and reused for the kYRun samples a thread walks.
__device__ __forceinline__ float column_term(const TerrainModifierArgs &m, float px, float pz)
{
    if (m.kind != 3) return 0.0f;
    // IslandModifier.cs:45-73: bilinear interpolation of _heightmap[u, v]
    const float wm1 = (float)(m.dims0 - 1), hm1 = (float)(m.dims1 - 1);
    float u = clampf(px, 0.0f, m.p[0]);
    u = u / m.p[0] * wm1;
    u = clampf(u, 0.0f, wm1);
    float v = clampf(pz, 0.0f, m.p[1]);
    v = v / m.p[1] * hm1;
    v = clampf(v, 0.0f, hm1);
    const int u0 = (int)floorf(u), u1 = (int)ceilf(u), v0 = (int)floorf(v), v1 = (int)ceilf(v);
    const float h00 = m.data[(size_t)u0 * m.dims1 + v0], h10 = m.data[(size_t)u1 * m.dims1 + v0];
    const float h01 = m.data[(size_t)u0 * m.dims1 + v1], h11 = m.data[(size_t)u1 * m.dims1 + v1];
    const float h0 = lerp_unity(h00, h01, v - (float)v0);
    const float h1 = lerp_unity(h10, h11, v - (float)v0);
    return lerp_unity(h0, h1, u - (float)u0);
}

// kJournal (history on): the sample it replaces also goes to the box's image (12 bytes per touched sample instead of 8).  History off
// runs the instruction sequence the kernel had before it was a template (profiles/r10/edit_refactor/README.md).
template <bool kJournal>
__global__ __launch_bounds__(256) void terrain_modify_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainModifierArgs m)
{
    const BoxThread t;
    if (!t.inside(m)) return;
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    // worldPos = new Vector3(x, y, z) * _voxelScale + TerrainOrigin (VoxelTerrain.cs:290)
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    const float col = column_term(m, px, pz);
    const uint64_t row = box_index(m, t.ix, 0, t.iz);  // image index of (ix, 0, iz); sample iy lies iy rows of dx further
    for (int iy = t.iy0, iy1 = t.iy1(m); iy < iy1; ++iy) {
        const int y = m.ly + iy;
        const float py = (float)y * sh.scale + sh.origin[1];
        const uint64_t sample = grid_index(sh, x, y, z);
        const float q = m.kind == 3 ? col - py : query_density(m, px, py, pz);  // IslandModifier: elevation - pos.y
        const float md = clamp_drawn(q, sh.seed, m.event, sample, 0u);
        const float s = grid[sample];
        if (kJournal) image[row + (uint64_t)m.dx * (uint64_t)iy] = s;
        grid[sample] = csg_combine(sh, m.event, sample, m.add_or_erode, md, s);
    }
}

// Undo / redo of one box: grid box <-> its journal image, 32-bit copies (NaN payloads and -0 survive), 16 bytes per sample.
__global__ __launch_bounds__(256) void terrain_swap_kernel(uint32_t *__restrict__ grid, uint32_t *__restrict__ image, TerrainShape sh, TerrainBox b)
{
    const BoxThread t;
    if (!t.inside(b)) return;
    const uint64_t s0 = grid_index(sh, b.lx + t.ix, b.ly + t.iy0, b.lz + t.iz), j0 = box_index(b, t.ix, t.iy0, t.iz);
    const int iy1 = t.iy1(b);
    // every load of the run is issued before the first store: 2 * kYRun loads in flight per lane, not 2
    uint32_t g[kYRun], h[kYRun];
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) {
            g[k] = grid[s0 + (uint64_t)sh.dim_x * k];
            h[k] = image[j0 + (uint64_t)b.dx * k];
        }
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) {
            grid[s0 + (uint64_t)sh.dim_x * k] = h[k];
            image[j0 + (uint64_t)b.dx * k] = g[k];
        }
}

// A box h of the grid, copied to `stage`: pass 1 of a smooth (terrain_brush.hip: the brush's box plus a one-sample halo, intersected with
// the grid) and a stamp's capture.  Load-before-store order of terrain_swap_kernel.
__global__ __launch_bounds__(256) void terrain_stage_kernel(const float *__restrict__ grid, float *__restrict__ stage, TerrainShape sh, TerrainBox h)
{
    const BoxThread t;
    if (!t.inside(h)) return;
    const int iy1 = t.iy1(h);
    const uint64_t s0 = grid_index(sh, h.lx + t.ix, h.ly + t.iy0, h.lz + t.iz), j0 = box_index(h, t.ix, t.iy0, t.iz);
    float v[kYRun];
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) v[k] = grid[s0 + (uint64_t)sh.dim_x * k];
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) stage[j0 + (uint64_t)h.dx * k] = v[k];
}

hipError_t launch_terrain_fill(float *grid, long long n, uint64_t seed, int n_cus, hipStream_t stream)
{
    long long wgs = (n + 255) / 256;
    if (wgs > (long long)n_cus * 16) wgs = (long long)n_cus * 16;
    if (wgs < 1) wgs = 1;
    return launch(terrain_fill_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, grid, n, seed);
}

// declared by vtmc_internal.h, whose text the traffic constant of the extract path is tied to: kept for that declaration, vtmc_terrain_update
// goes through launch_box itself
hipError_t launch_terrain_modify(float *grid, const TerrainShape &sh, const TerrainModifierArgs &m, hipStream_t stream)
{
    return box_empty(box_of(m)) ? hipSuccess : launch_box(terrain_modify_kernel<false>, box_of(m), stream, grid, (float *)nullptr, sh, m);
}

// terrain_stamp.h: a box of the grid as 32-bit copies, for vtmc_stamp_capture and the stage of a smooth (terrain_brush.hip)
hipError_t launch_terrain_copy_box(const float *grid, float *dst, const TerrainShape &sh, const TerrainBox &b, hipStream_t stream)
{
    return launch_box(terrain_stage_kernel, b, stream, grid, dst, sh, b);
}

static int saturating_int(float f)   // of a floor / ceil: Mathf.FloorToInt / CeilToInt, saturating
{
    return f <= -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f);
}

// the terrain's blocks per axis, and f(bx, by, bz) for every block in block-id order (x fastest)
static std::array<int, 3> block_counts(const TerrainShape &sh) { return {(sh.dim_x - 2) / 8, (sh.dim_y - 2) / 8, (sh.dim_z - 2) / 8}; }
template <class F>
static void for_each_block(const std::array<int, 3> &nb, F f)
{
    for (int bz = 0; bz < nb[2]; ++bz)
        for (int by = 0; by < nb[1]; ++by)
            for (int bx = 0; bx < nb[0]; ++bx) f(bx, by, bz);
}

TerrainModifierArgs sample_range(const TerrainShape &sh, const vtmc_modifier &md, int low[3], int up[3])
{
    TerrainModifierArgs a{};
    a.kind = md.kind;
    a.add_or_erode = md.add_or_erode ? 1 : 0;
    memcpy(a.p, md.p, sizeof a.p);
    const int top[3] = {sh.dim_x - 1, sh.dim_y - 1, sh.dim_z - 1};
    int ext[3];
    for (int k = 0; k < 3; ++k) {
        // world -> sample index: (world - TerrainOrigin) / _voxelScale, floor / ceil, clamp (VoxelTerrain.cs:273-281)
        low[k] = std::max(saturating_int(std::floor((md.lower[k] - sh.origin[k]) / sh.scale)), 0);
        up[k] = std::min(saturating_int(std::ceil((md.upper[k] - sh.origin[k]) / sh.scale)), top[k]);
        // extents in 64 bits: floor/ceil saturate at INT32_MIN/MAX, so an inverted or far-away AABB must
        // come out as an empty range (the reference's loops simply do not execute, VoxelTerrain.cs:284-286),
        // never as a wrapped positive size; low >= 0 and up <= top bound a valid extent by the grid
        const long long e = (long long)up[k] - (long long)low[k] + 1;
        ext[k] = e <= 0 || low[k] > top[k] ? 0 : (int)std::min<long long>(e, (long long)top[k] - low[k] + 1);
    }
    a.lx = low[0], a.ly = low[1], a.lz = low[2];
    a.dx = ext[0], a.dy = ext[1], a.dz = ext[2];
    return a;
}

TerrainBox bounds_box(const TerrainShape &sh, const float lower[3], const float upper[3])
{
    vtmc_modifier md{};
    for (int k = 0; k < 3; ++k) md.lower[k] = lower[k], md.upper[k] = upper[k];
    int low[3], up[3];
    return box_of(sample_range(sh, md, low, up));
}

// dirty blocks: up >= 8b && low <= 8b + 8 on every axis (VoxelTerrain.cs:307-317), as index ranges; returns how many were newly marked
static size_t mark_dirty_blocks(const int low[3], const int up[3], const std::array<int, 3> &nb, std::vector<uint8_t> &mark)
{
    int b0[3], b1[3];
    for (int k = 0; k < 3; ++k) {
        // b <= up / 8 and b >= (low - 8) / 8 rounded up; the reference's loops leave an empty
        // (low > up) AABB with its block tests, so the same arithmetic is used for it
        const long long lo = (long long)low[k] - 8, hi = up[k];
        const long long f = lo <= 0 ? 0 : (lo + 7) / 8;
        const long long l = std::min<long long>(hi < 0 ? -1 : hi / 8, nb[k] - 1);
        if (f > l) return 0;
        b0[k] = (int)f;
        b1[k] = (int)l;
    }
    size_t n_new = 0;
    for (int bz = b0[2]; bz <= b1[2]; ++bz)
        for (int by = b0[1]; by <= b1[1]; ++by) {
            uint8_t *row = &mark[(size_t)nb[0] * ((size_t)by + (size_t)nb[1] * bz)];
            for (int bx = b0[0]; bx <= b1[0]; ++bx) {
                n_new += !row[bx];
                row[bx] = 1;
            }
        }
    return n_new;
}

// An earlier modifier of the same queue may still be reading what the buffer held, hence the drain before the buffer is grown or written.
int stage_for_queue(vtmc_ctx *ctx, VtmcDevBuf &buf, const void *host, size_t bytes)
{
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = ensure(ctx, buf, bytes)) return rc;
    VTMC_HIP(ctx, hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
    return VTMC_OK;
}

// the reference's modifiers, kinds 0-3
static int check_reference(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    if (md.kind == VTMC_MOD_HEIGHTMAP && (!md.data || md.data_dims[0] < 1 || md.data_dims[1] < 1))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: heightmap data / dims missing", i);
    return VTMC_OK;
}

static int apply_reference(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &args, float *grid, float *image)
{
    TerrainModifierArgs a = args;
    if (md.kind == VTMC_MOD_HEIGHTMAP) {  // _heightmap (IslandModifier.cs:36) goes to the device
        if (int rc = stage_for_queue(ctx, ctx->heightmap, md.data, sizeof(float) * (size_t)md.data_dims[0] * (size_t)md.data_dims[1])) return rc;
        a.data = (const float *)ctx->heightmap.p;
        a.dims0 = md.data_dims[0];
        a.dims1 = md.data_dims[1];
    }
    VTMC_HIP(ctx, launch_box(image ? terrain_modify_kernel<true> : terrain_modify_kernel<false>, box_of(a), ctx->stream, grid, image, ctx->tshape, a));
    return VTMC_OK;
}

// every kind of vtmc_modifier (terrain_edit.h)
static const ModifierKind kModifierKinds[] = {
    {VTMC_MOD_PLANE, check_reference, apply_reference},
    {VTMC_MOD_SPHERE, check_reference, apply_reference},
    {VTMC_MOD_CYLINDER, check_reference, apply_reference},
    {VTMC_MOD_HEIGHTMAP, check_reference, apply_reference},
    {VTMC_MOD_SMOOTH, check_brush, apply_smooth},
    {VTMC_MOD_FLATTEN, check_brush, apply_flatten},
    {VTMC_MOD_NOISE, check_noise, apply_noise},
    {VTMC_MOD_STAMP, check_stamp, apply_stamp},
    {VTMC_MOD_PATH, check_path, apply_path},
    {VTMC_MOD_DETACH, check_detach, apply_detach},
    {VTMC_MOD_EROSION, check_erosion, apply_erosion},
};

const ModifierKind *find_modifier_kind(int32_t kind)
{
    for (const ModifierKind &k : kModifierKinds)
        if (k.kind == kind) return &k;
    return nullptr;
}

static int check_modifier(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    const ModifierKind *k = find_modifier_kind(md.kind);
    return k ? k->check(ctx, md, i) : fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: unknown kind %d", i, md.kind);
}

// _nextUpdateblocks (VoxelTerrain.cs:321) from the marks, ordered by block id (a full rebuild needs no list), then BatchUpdate
// (VoxelTerrain.cs:322-323) on the resident grid
static int extract_dirty(vtmc_ctx *ctx, const std::vector<uint8_t> &mark, size_t n_marked, int32_t *n_dirty_blocks, int32_t *tri_count)
{
    const TerrainShape &sh = ctx->tshape;
    const auto nb = block_counts(sh);
    ctx->dirty.clear();
    ctx->dirty_is_all = n_marked == mark.size();
    if (!ctx->dirty_is_all) {
        ctx->dirty.reserve(n_marked * 3);
        size_t id = 0;
        for_each_block(nb, [&](int bx, int by, int bz) {
            if (mark[id++]) ctx->dirty.insert(ctx->dirty.end(), {bx, by, bz});
        });
    }
    if (n_dirty_blocks) *n_dirty_blocks = (int32_t)n_marked;
    BlockSpace sp = dense_space((const float *)ctx->terrain.p, sh.dim_x - 2, sh.dim_y - 2, sh.dim_z - 2, 1, sh.dim_x, (int64_t)sh.dim_x * sh.dim_y, 1, 0);
    int n_volumes = 1;
    if (!ctx->dirty_is_all) {  // a proper subset: device block list; every block: the dense streaming path
        if (int rc = upload_block_list(ctx, ctx->dirty.data(), (int)n_marked, sp)) return rc;
        n_volumes = 0;
    }
    return extract_core(ctx, sp, n_volumes, ResultSource::TerrainDirty, tri_count);
}

void history_clear(vtmc_ctx *ctx)   // vtmc_ctx.h: terrain_io.hip clears the history too
{
    ctx->hist.clear();
    ctx->hist_done = 0;
}

// vtmc_terrain_load: every block is dirty, as after a world build (vtmc_ctx.h)
int terrain_extract_all(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count)
{
    const auto nb = block_counts(ctx->tshape);
    const std::vector<uint8_t> mark((size_t)nb[0] * nb[1] * nb[2], 1);
    return extract_dirty(ctx, mark, mark.size(), n_dirty_blocks, tri_count);
}

// journal bytes of a box image: 4 per sample, rounded up to 256
static size_t image_bytes(const TerrainBox &b) { return box_empty(b) ? 0 : ((size_t)4 * b.dx * b.dy * b.dz + 255) / 256 * 256; }

// Places the step of a (validated) queue in the arena before anything is written: the boxes and dirty-rule bounds of every modifier,
// back to back.  A step that writes no sample comes back empty and changes nothing; one larger than the arena comes back empty and
// clears the history.  Otherwise every undone step is dropped, and then the oldest steps until the step's range of the ring is free.
static VtmcHistoryStep plan_step(vtmc_ctx *ctx, const vtmc_modifier *mods, int32_t n_mods)
{
    VtmcHistoryStep st;
    st.boxes.resize((size_t)n_mods);
    for (int32_t i = 0; i < n_mods; ++i) {
        VtmcHistoryBox &hb = st.boxes[i];
        const TerrainModifierArgs a = sample_range(ctx->tshape, mods[i], hb.low, hb.up);
        hb.box = box_of(a);
        hb.off = st.bytes;
        st.bytes += image_bytes(hb.box);
    }
    const size_t cap = ctx->journal.bytes;
    if (st.bytes == 0 || st.bytes > cap) {
        if (st.bytes) history_clear(ctx);
        st.boxes.clear();
        return st;
    }
    ctx->hist.resize(ctx->hist_done);  // a new step discards redo
    const size_t head = ctx->hist.empty() ? 0 : ctx->hist.back().off + ctx->hist.back().bytes;
    st.off = head + st.bytes <= cap ? head : 0;
    if (st.off == 0)  // wrapped: the steps between head and the arena's end are the oldest ones, and the ring wraps only once
        while (!ctx->hist.empty() && ctx->hist.front().off >= head) ctx->hist.pop_front();
    while (!ctx->hist.empty() && ctx->hist.front().off < st.off + st.bytes && st.off < ctx->hist.front().off + ctx->hist.front().bytes)
        ctx->hist.pop_front();
    ctx->hist_done = ctx->hist.size();
    for (VtmcHistoryBox &hb : st.boxes) hb.off += st.off;
    return st;
}

// vtmc_terrain_undo / _redo: swaps the step's boxes with their images (undo newest-first in reverse queue order, redo in queue order),
// then extracts the step's dirty set as its update did
static int32_t history_step(vtmc_ctx *ctx, bool undo, int32_t *n_dirty_blocks, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_%s before terrain_init", undo ? "undo" : "redo");
    if (undo ? ctx->hist_done == 0 : ctx->hist_done == ctx->hist.size())
        return fail(ctx, VTMC_ERR_NO_RESULT, "nothing to %s", undo ? "undo" : "redo");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t k = undo ? ctx->hist_done - 1 : ctx->hist_done;
    const VtmcHistoryStep &st = ctx->hist[k];
    const auto nb = block_counts(ctx->tshape);
    std::vector<uint8_t> mark((size_t)nb[0] * nb[1] * nb[2], 0);
    size_t n_marked = 0;
    const size_t n = st.boxes.size();
    for (size_t i = 0; i < n; ++i) {
        const VtmcHistoryBox &hb = st.boxes[undo ? n - 1 - i : i];
        if (!box_empty(hb.box))
            if (hipError_t e = launch_box(terrain_swap_kernel, hb.box, ctx->stream, (uint32_t *)ctx->terrain.p,
                                          (uint32_t *)((char *)ctx->journal.p + hb.off), ctx->tshape, hb.box)) {
                history_clear(ctx);  // some boxes swapped, some not: no image is what its step says any more
                VTMC_HIP(ctx, e);
            }
        if (n_marked < mark.size()) n_marked += mark_dirty_blocks(hb.low, hb.up, nb, mark);
    }
    ctx->hist_done = undo ? k : k + 1;
    return extract_dirty(ctx, mark, n_marked, n_dirty_blocks, tri_count);
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_init(vtmc_ctx *ctx, int32_t width, int32_t elevation, int32_t height, float voxel_scale,
                          const float terrain_origin[3], uint64_t seed)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!terrain_origin) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_origin is null");
    if (int rc = check_dims(ctx, width, elevation, height)) return rc;
    // VoxelTerrain.cs:141-142
    if (width + 1 > 1025 || elevation + 1 > 1025 || height + 1 > 1025)
        return fail(ctx, VTMC_ERR_DIMS, "too high resolution (exceeds 1025)");
    if (!(voxel_scale > 0.0f)) return fail(ctx, VTMC_ERR_INVALID_ARG, "voxel_scale must be positive");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->has_terrain = false;
    ctx->result.valid = false;
    history_clear(ctx);
    material_drop(ctx);
    nav_drop(ctx);
    water_drop(ctx);
    erosion_drop(ctx);
    light_drop(ctx);
    TerrainShape sh{};
    sh.dim_x = width + 2;
    sh.dim_y = elevation + 2;
    sh.dim_z = height + 2;
    sh.scale = voxel_scale;
    memcpy(sh.origin, terrain_origin, sizeof sh.origin);
    sh.seed = seed;
    const long long n = (long long)sh.dim_x * sh.dim_y * sh.dim_z;
    if (int rc = ensure(ctx, ctx->terrain, sizeof(float) * (size_t)n)) return rc;
    VTMC_HIP(ctx, launch_terrain_fill((float *)ctx->terrain.p, n, seed, ctx->n_cus, ctx->stream));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tshape = sh;
    ctx->terrain_events = 0;
    ctx->dirty.clear();
    ctx->dirty_is_all = false;
    ctx->has_terrain = true;
    return VTMC_OK;
}

int32_t vtmc_terrain_update(vtmc_ctx *ctx, const vtmc_modifier *mods, int32_t n_mods, int32_t *n_dirty_blocks, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_update before terrain_init");
    if (n_mods < 0 || (n_mods > 0 && !mods)) return fail(ctx, VTMC_ERR_INVALID_ARG, "mods is null or n_mods < 0");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const TerrainShape &sh = ctx->tshape;
    const auto nb = block_counts(sh);
    std::vector<uint8_t> mark((size_t)nb[0] * nb[1] * nb[2], 0);
    size_t n_marked = 0;
    // history on: the whole queue is checked and its step placed before the first write (history off: a bad modifier fails where it stands)
    VtmcHistoryStep step;
    if (ctx->journal.p) {
        for (int32_t i = 0; i < n_mods; ++i)
            if (int rc = check_modifier(ctx, mods[i], i)) return rc;
        step = plan_step(ctx, mods, n_mods);
    }
    const bool journaled = !step.boxes.empty();
    struct ClearOnFailure {   // an update that fails after its first write leaves no image its step would claim
        vtmc_ctx *ctx;
        bool armed;
        ~ClearOnFailure()
        {
            if (armed) history_clear(ctx);
        }
    } guard{ctx, journaled};
    for (int32_t i = 0; i < n_mods; ++i) {
        const vtmc_modifier &md = mods[i];
        if (int rc = check_modifier(ctx, md, i)) return rc;
        int low[3], up[3];
        TerrainModifierArgs a = sample_range(sh, md, low, up);
        a.event = ++ctx->terrain_events;
        if (!box_empty(box_of(a))) {
            float *image = journaled ? (float *)((char *)ctx->journal.p + step.boxes[i].off) : nullptr;
            if (int rc = find_modifier_kind(md.kind)->apply(ctx, md, a, (float *)ctx->terrain.p, image)) return rc;
        }
        if (n_marked < mark.size()) n_marked += mark_dirty_blocks(low, up, nb, mark);
    }
    if (journaled) {
        ctx->hist.push_back(std::move(step));
        ctx->hist_done = ctx->hist.size();
    }
    const int rc = extract_dirty(ctx, mark, n_marked, n_dirty_blocks, tri_count);
    guard.armed = rc != VTMC_OK && journaled;
    return rc;
}

int32_t vtmc_terrain_set_history(vtmc_ctx *ctx, int64_t max_bytes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (max_bytes < 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "max_bytes < 0");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    history_clear(ctx);
    // the only place the arena is allocated or freed: hipMalloc / hipFree synchronise, an update or undo must not
    if (ctx->journal.bytes != (size_t)max_bytes) {
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // a journaled write or a swap may still be using the old arena
        ctx->journal.release();
        if (max_bytes > 0) {
            VTMC_HIP(ctx, hipMalloc(&ctx->journal.p, (size_t)max_bytes));
            ctx->journal.bytes = (size_t)max_bytes;
        }
    }
    return VTMC_OK;
}

int32_t vtmc_terrain_undo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count) { return history_step(ctx, true, n_dirty_blocks, tri_count); }

int32_t vtmc_terrain_redo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count) { return history_step(ctx, false, n_dirty_blocks, tri_count); }

int32_t vtmc_terrain_history(const vtmc_ctx *ctx, int32_t *n_undo, int32_t *n_redo, int64_t *bytes_used)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_undo) *n_undo = (int32_t)ctx->hist_done;
    if (n_redo) *n_redo = (int32_t)(ctx->hist.size() - ctx->hist_done);
    if (bytes_used) {
        int64_t b = 0;
        for (const VtmcHistoryStep &st : ctx->hist) b += (int64_t)st.bytes;
        *bytes_used = b;
    }
    return VTMC_OK;
}

int32_t vtmc_terrain_dirty_blocks(vtmc_ctx *ctx, int32_t *dst, int32_t capacity_blocks, int32_t *n_blocks)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_dirty_blocks before terrain_init");
    const auto nb = block_counts(ctx->tshape);
    const size_t n = ctx->dirty_is_all ? (size_t)nb[0] * nb[1] * nb[2] : ctx->dirty.size() / 3;
    if (n_blocks) *n_blocks = (int32_t)n;
    if (!dst) return VTMC_OK;  // size query
    if ((size_t)std::max(capacity_blocks, 0) < n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %zu dirty blocks", capacity_blocks, n);
    if (ctx->dirty_is_all)
        for_each_block(nb, [&](int bx, int by, int bz) {
            *dst++ = bx;
            *dst++ = by;
            *dst++ = bz;
        });
    else if (n)
        memcpy(dst, ctx->dirty.data(), n * 3 * sizeof(int32_t));
    return VTMC_OK;
}

int32_t vtmc_terrain_read_samples(vtmc_ctx *ctx, float *dst, int64_t stride_x, int64_t stride_y, int64_t stride_z)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_read_samples before terrain_init");
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    if (stride_x <= 0 || stride_y <= 0 || stride_z <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const TerrainShape &sh = ctx->tshape;
    const size_t n = (size_t)sh.dim_x * sh.dim_y * sh.dim_z;
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stride_x == 1 && stride_y == sh.dim_x && stride_z == (int64_t)sh.dim_x * sh.dim_y) {
        VTMC_HIP(ctx, hipMemcpy(dst, ctx->terrain.p, n * sizeof(float), hipMemcpyDeviceToHost));
        return VTMC_OK;
    }
    std::vector<float> tmp(n);
    VTMC_HIP(ctx, hipMemcpy(tmp.data(), ctx->terrain.p, n * sizeof(float), hipMemcpyDeviceToHost));
    size_t i = 0;
    for (int z = 0; z < sh.dim_z; ++z)
        for (int y = 0; y < sh.dim_y; ++y)
            for (int x = 0; x < sh.dim_x; ++x) dst[x * stride_x + y * stride_y + z * stride_z] = tmp[i++];
    return VTMC_OK;
}

int32_t vtmc_terrain_device_grid(vtmc_ctx *ctx, const float **d_samples, int64_t strides[3], int32_t dims[3])
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_device_grid before terrain_init");
    const TerrainShape &sh = ctx->tshape;
    if (d_samples) *d_samples = (const float *)ctx->terrain.p;
    if (strides) {
        strides[0] = 1;
        strides[1] = sh.dim_x;
        strides[2] = (int64_t)sh.dim_x * sh.dim_y;
    }
    if (dims) {
        dims[0] = sh.dim_x;
        dims[1] = sh.dim_y;
        dims[2] = sh.dim_z;
    }
    return VTMC_OK;
}

}  // extern "C"
