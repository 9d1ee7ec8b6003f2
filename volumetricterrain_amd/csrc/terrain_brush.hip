// terrain_brush.hip -- the sculpt brushes of the resident terrain (VTMC_MOD_SMOOTH / VTMC_MOD_FLATTEN; not in the reference): their kernels,
// check and applies, entries of the modifier table (terrain_edit.h).
// Both blend a sample towards a target T by w = s * clamp01(2 * (1 - |p - c| / r)): full strength inside r/2, linear to 0 at r.  A
// sample of weight 0 keeps its 32 bits (it is not rewritten); any other becomes S + (T - S) * w (Mathf.Lerp's form).
#include "terrain_edit.h"
#include "terrain_stamp.h"  // launch_terrain_copy_box: the stage of a smooth
#include <algorithm>
#include <cmath>

namespace vtmc {

__device__ __forceinline__ float brush_weight(const TerrainModifierArgs &m, float px, float py, float pz)
{
    const float dx = px - m.p[0], dy = py - m.p[1], dz = pz - m.p[2];
    const float d = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);  // as SphereModifier in terrain.hip
    float t = 1.0f - d / m.p[3];
    t = t + t;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    return m.p[4] * t;
}

// Flatten: T = clamp((n . (c - p)) / scale, -1, 1), solid below the plane through c, air above it, linear in grid units within one
// sample of it.  Pointwise; kJournal also stores every sample of the box into its image.
template <bool kJournal>
__global__ __launch_bounds__(256) void terrain_flatten_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainModifierArgs m)
{
    const BoxThread t;
    if (!t.inside(m)) return;
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    const uint64_t row = box_index(m, t.ix, 0, t.iz);  // image index of (ix, 0, iz); sample iy lies iy rows of dx further
    for (int iy = t.iy0, iy1 = t.iy1(m); iy < iy1; ++iy) {
        const int y = m.ly + iy;
        const float py = (float)y * sh.scale + sh.origin[1];
        const uint64_t sample = grid_index(sh, x, y, z);
        const float w = brush_weight(m, px, py, pz);
        if (!kJournal && w == 0.0f) continue;
        const float s = grid[sample];
        if (kJournal) image[row + (uint64_t)m.dx * (uint64_t)iy] = s;
        if (w == 0.0f) continue;
        float g = (m.p[5] * (m.p[0] - px) + m.p[6] * (m.p[1] - py) + m.p[7] * (m.p[2] - pz)) / sh.scale;
        g = g < -1.0f ? -1.0f : (g > 1.0f ? 1.0f : g);
        grid[sample] = s + (g - s) * w;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Smooth, pass 2: T = the 27-point box mean of the staged (pre-brush) samples, neighbour indices clamped to the grid, summed as
//   R(y, z) = (s[x-1] + s[x]) + s[x+1],  P(z) = (R(y-1, z) + R(y, z)) + R(y+1, z),  T = ((P(z-1) + P(z)) + P(z+1)) / 27.
// A workgroup owns 64 x 4 samples of (x, z) and walks kYRun of y.  Per y-plane of the stage it puts a 66 x 6 tile (the samples and
// their x / z neighbours) in LDS, and each lane keeps the row sums R of the last two planes in registers, so a staged sample is read
// from memory (66 * 6) / (64 * 4) * (kYRun + 2) / kYRun = 1.74 times per workgroup, not 27.  Clamping a tile coordinate to the stage
// is clamping it to the grid: the stage is the box plus whatever of its halo lies in the grid.  Every staged load of the run is
// issued before the first LDS store.  The old value of each box sample comes from the stage, so kJournal's image costs no grid read.
constexpr int kTileX = 66, kTileZ = 6, kTile = kTileX * kTileZ;
template <bool kJournal>
__global__ __launch_bounds__(256) void terrain_smooth_kernel(float *__restrict__ grid, float *__restrict__ image, const float *__restrict__ stage,
                                                             TerrainShape sh, TerrainModifierArgs m, TerrainBox h)
{
    __shared__ float tile[2][kTile];
    const BoxThread bt;
    const int tx = threadIdx.x, tz = threadIdx.y, t = tz * 64 + tx;
    const int ox = m.lx - h.lx, oy = m.ly - h.ly, oz = m.lz - h.lz;  // the box's first sample in the stage (0 or 1 per axis)
    const int n_planes = bt.iy1(m) - bt.iy0 + 2;                          // uniform over the workgroup
    const uint64_t plane = (uint64_t)h.dx * (uint64_t)h.dy;
    // this lane's tile entries t and t + 256 (the second for t < kTile - 256 only)
    const bool two = t + 256 < kTile;
    const uint64_t c0 = (uint64_t)clampi(blockIdx.x * 64 + ox - 1 + t % kTileX, 0, h.dx - 1) +
                        plane * (uint64_t)clampi(blockIdx.y * 4 + oz - 1 + t / kTileX, 0, h.dz - 1);
    const uint64_t c1 = two ? (uint64_t)clampi(blockIdx.x * 64 + ox - 1 + (t + 256) % kTileX, 0, h.dx - 1) +
                                  plane * (uint64_t)clampi(blockIdx.y * 4 + oz - 1 + (t + 256) / kTileX, 0, h.dz - 1)
                            : 0;
    float v0[kYRun + 2], v1[kYRun + 2];
#pragma unroll
    for (int k = 0; k < kYRun + 2; ++k)
        if (k < n_planes) {
            const uint64_t sy = (uint64_t)h.dx * (uint64_t)clampi(bt.iy0 + oy - 1 + k, 0, h.dy - 1);
            v0[k] = stage[c0 + sy];
            if (two) v1[k] = stage[c1 + sy];
        }
    // BoxThread::inside, written out: through the call the compiler nests the 15 unrolled write-backs in two branches instead of one mask
    const bool live = bt.ix < m.dx && bt.iz < m.dz;
    const int x = m.lx + bt.ix, z = m.lz + bt.iz;
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    const uint64_t row = box_index(m, bt.ix, 0, bt.iz);
    float ra[3] = {0.0f, 0.0f, 0.0f}, rb[3] = {0.0f, 0.0f, 0.0f}, sb = 0.0f;  // R of planes k-2 and k-1 at z-1, z, z+1; S of plane k-1
#pragma unroll
    for (int k = 0; k < kYRun + 2; ++k) {
        if (k < n_planes) {  // uniform over the workgroup, as the barrier needs
            // double-buffered: the buffer written here was last read before the previous iteration's barrier
            float *tl = tile[k & 1];
            tl[t] = v0[k];
            if (two) tl[t + 256] = v1[k];
            __syncthreads();
            float r[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float *q = tl + (tz + j) * kTileX + tx;
                r[j] = (q[0] + q[1]) + q[2];
            }
            const float sc = tl[(tz + 1) * kTileX + tx + 1];
            if (k >= 2 && live) {
                const int iy = bt.iy0 + k - 2, y = m.ly + iy;
                const float py = (float)y * sh.scale + sh.origin[1];
                const uint64_t sample = grid_index(sh, x, y, z);
                if (kJournal) image[row + (uint64_t)m.dx * (uint64_t)iy] = sb;
                const float w = brush_weight(m, px, py, pz);
                if (w != 0.0f) {
                    const float p0 = (ra[0] + rb[0]) + r[0], p1 = (ra[1] + rb[1]) + r[1], p2 = (ra[2] + rb[2]) + r[2];
                    const float target = ((p0 + p1) + p2) / 27.0f;
                    grid[sample] = sb + (target - sb) * w;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ra[j] = rb[j];
                rb[j] = r[j];
            }
            sb = sc;
        }
    }
}

// the stage box of a smooth: its (non-empty) box grown by one sample per side, intersected with the grid
static TerrainBox smooth_stage_box(const TerrainShape &sh, const TerrainModifierArgs &m)
{
    const int lx = std::max(m.lx - 1, 0), ly = std::max(m.ly - 1, 0), lz = std::max(m.lz - 1, 0);
    const int ux = std::min(m.lx + m.dx, sh.dim_x - 1), uy = std::min(m.ly + m.dy, sh.dim_y - 1), uz = std::min(m.lz + m.dz, sh.dim_z - 1);
    return TerrainBox{lx, ly, lz, ux - lx + 1, uy - ly + 1, uz - lz + 1};
}

int check_brush(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    const float *p = md.p;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: brush centre not finite", i);
    if (!std::isfinite(p[3]) || !(p[3] > 0.0f)) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: brush radius %g not finite and > 0", i, p[3]);
    if (!std::isfinite(p[4]) || !(p[4] >= 0.0f && p[4] <= 1.0f))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: brush strength %g not in [0, 1]", i, p[4]);
    if (md.kind == VTMC_MOD_FLATTEN &&
        (!std::isfinite(p[5]) || !std::isfinite(p[6]) || !std::isfinite(p[7]) || p[5] * p[5] + p[6] * p[6] + p[7] * p[7] == 0.0f))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: flatten normal not finite or zero", i);
    return VTMC_OK;
}

int apply_smooth(vtmc_ctx *ctx, const vtmc_modifier &, const TerrainModifierArgs &a, float *grid, float *image)
{
    const TerrainShape &sh = ctx->tshape;
    const TerrainBox h = smooth_stage_box(sh, a);
    const size_t bytes = sizeof(float) * (size_t)h.dx * (size_t)h.dy * (size_t)h.dz;
    if (ctx->brush.bytes < bytes) {  // an earlier smooth of this queue may still be reading the stage
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (int rc = ensure(ctx, ctx->brush, bytes)) return rc;
    }
    // h contains the box (sample_range clips it to the grid, smooth_stage_box only grows it), so a box too large to launch fails
    // here, before anything is written
    float *stage = (float *)ctx->brush.p;
    VTMC_HIP(ctx, launch_terrain_copy_box(grid, stage, sh, h, ctx->stream));
    VTMC_HIP(ctx, launch_box(image ? terrain_smooth_kernel<true> : terrain_smooth_kernel<false>, box_of(a), ctx->stream, grid, image, stage, sh, a, h));
    return VTMC_OK;
}

int apply_flatten(vtmc_ctx *ctx, const vtmc_modifier &, const TerrainModifierArgs &a, float *grid, float *image)
{
    VTMC_HIP(ctx, launch_box(image ? terrain_flatten_kernel<true> : terrain_flatten_kernel<false>, box_of(a), ctx->stream, grid, image, ctx->tshape, a));
    return VTMC_OK;
}

}  // namespace vtmc
