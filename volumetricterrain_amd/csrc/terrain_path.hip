// terrain_path.hip -- the path modifier (VTMC_MOD_PATH; not in the reference, which queues one eroding CylinderModifier per river segment,
// RiverRenderer.cs:151-170): the union of tapered capsules over a segment soup, written into the resident terrain with the CSG write of
// kinds 0-3 in one pass over the modifier's box.  The rule, operation by operation, is in include/vtmc.h; the kernel follows it bit for
// bit (library built with -ffp-contract=off).
//
// Unlike the pointwise kinds the work is samples x segments, so a workgroup prunes before it evaluates.  It owns a tile of the shared box
// walk (terrain_box.h: 64 x kYRun x 4 samples) and takes the segments in chunks of kPathChunk.  A chunk whose bounds miss the tile is
// skipped whole; otherwise each thread tests one segment's bounds against the tile, the survivors are compacted into LDS in index order
// (wave ballot, prefix over the four waves), and every thread evaluates that list for the kYRun samples of its run: the running maxima
// stay in registers, and all lanes read the same LDS record at a time (a broadcast, no bank conflict).  About 35 FP32 operations per
// (sample, surviving segment) against 8-12 bytes per sample: VALU-bound where segments are dense, HBM-bound elsewhere.
//
// Pruning is exact, not approximate: a segment whose f stays below -2 on every sample of a tile cannot change md there, since any
// q < -2 -- the initial -inf included -- clamps to the same drawn void value.  A tile with no surviving segment still writes.
#include "terrain_edit.h"
#include "terrain_path.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace vtmc {

// The segments on the device, three arrays in one buffer:
//   seg   2 float4 per segment: (ax, ay, az, ra), (ex, ey, ez, dr)       -- what a sample's evaluation reads
//   bound 2 float4 per segment: (lo.x, lo.y, lo.z, il), (hi.x, hi.y, hi.z, 0): the segment's AABB grown by its pruning reach
//   chunk 2 float4 per chunk of kPathChunk segments: the union of its segments' bounds
struct TerrainPathArgs {
    const float4 *seg, *bound, *chunk;
    int n_seg, add_or_erode;
    int lx, ly, lz, dx, dy, dz;  // the clamped sample box, as TerrainModifierArgs
    uint32_t event;
};

// true when the boxes [lo, hi] and [tlo, thi] are apart on some axis (false for a NaN: the segment is then kept)
__device__ __forceinline__ bool path_apart(const float4 &lo, const float4 &hi, const float tlo[3], const float thi[3])
{
    return thi[0] < lo.x || tlo[0] > hi.x || thi[1] < lo.y || tlo[1] > hi.y || thi[2] < lo.z || tlo[2] > hi.z;
}

// kJournal as terrain_modify_kernel.  A thread outside the box (the tile's x / z tail) takes part in the pruning and evaluates nothing;
// a run's tail past the box along y is evaluated and never loaded or stored, as in terrain_noise_kernel.
template <bool kJournal>
__global__ __launch_bounds__(256) void terrain_path_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainPathArgs m)
{
    __shared__ float4 s_a[kPathChunk], s_e[kPathChunk];  // the surviving segments of the chunk, in index order
    __shared__ float s_il[kPathChunk];
    __shared__ int s_cnt[4];                             // survivors per wave
    const BoxThread t;
    const bool live = t.inside(m);
    const int lane = threadIdx.x, wave = threadIdx.y;    // 64 x 4 threads: a wave is a row of the workgroup
    // The tile's world AABB.  Positions are monotonic in the index (scale > 0, one multiply and one add), so the positions of the tile's
    // first and last sample per axis, computed as the samples' own are, bound every sample of it exactly.
    const int first[3] = {m.lx + (int)blockIdx.x * 64, m.ly + (int)blockIdx.z * kYRun, m.lz + (int)blockIdx.y * 4};
    const int last[3] = {min(first[0] + 63, m.lx + m.dx - 1), min(first[1] + kYRun - 1, m.ly + m.dy - 1), min(first[2] + 3, m.lz + m.dz - 1)};
    float tlo[3], thi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tlo[k] = (float)first[k] * sh.scale + sh.origin[k];
        thi[k] = (float)last[k] * sh.scale + sh.origin[k];
    }
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    float py[kYRun], q[kYRun];
#pragma unroll
    for (int k = 0; k < kYRun; ++k) {
        py[k] = (float)(m.ly + t.iy0 + k) * sh.scale + sh.origin[1];
        q[k] = -INFINITY;
    }
    for (int c0 = 0; c0 < m.n_seg; c0 += kPathChunk) {
        // A segment is skipped only when, on some axis, the gap between the tile's AABB and the segment's exceeds max(ra, rb) + 2 + slack
        // (the host grew the bounds by exactly that, path_records): then d > max(ra, rb) + 2 + slack >= r + 2 on every sample of the
        // tile, whatever t in [0, 1] came out, and f < -2.  slack = max(0.01, 1e-4 * the largest |coordinate| of the grid and of the
        // segment): the roundings of px, of c, of d and of r are each below 1e-6 of that.
        const float4 *cb = m.chunk + 2 * (c0 / kPathChunk);
        if (path_apart(cb[0], cb[1], tlo, thi)) continue;  // uniform over the workgroup, as the barriers below need
        const int i = c0 + wave * 64 + lane;
        bool keep = false;
        float il = 0.0f;
        if (i < m.n_seg) {
            const float4 lo = m.bound[2 * i], hi = m.bound[2 * i + 1];
            keep = !path_apart(lo, hi, tlo, thi);
            il = lo.w;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();  // also: every wave has left the previous chunk's list
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = s_cnt[w];
            if (w < wave) base += c;
            total += c;
        }
        if (keep) {
            const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
            s_a[at] = m.seg[2 * i];
            s_e[at] = m.seg[2 * i + 1];
            s_il[at] = il;
        }
        __syncthreads();
        if (!live) continue;
        const int n_live = __builtin_amdgcn_readfirstlane(total);
        for (int j = 0; j < n_live; ++j) {
            const float4 a = s_a[j], e = s_e[j];
            const float sil = s_il[j];
            const float dx = px - a.x, dz = pz - a.z;
            const float dxex = dx * e.x, dzez = dz * e.z;  // the products of the run's samples that do not depend on y; the sums keep the header's order
#pragma unroll
            for (int k = 0; k < kYRun; ++k) {
                const float dy = py[k] - a.y;
                float tt = ((dxex + dy * e.y) + dzez) * sil;
                tt = tt < 0.0f ? 0.0f : (tt > 1.0f ? 1.0f : tt);
                const float cx = dx - e.x * tt, cy = dy - e.y * tt, cz = dz - e.z * tt;
                const float d = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
                const float r = a.w + e.w * tt;
                const float f = r - d;
                if (f > q[k]) q[k] = f;
            }
        }
    }
    if (!live) return;
    const int iy1 = t.iy1(m);
    const uint64_t s0 = grid_index(sh, x, m.ly + t.iy0, z), j0 = box_index(m, t.ix, t.iy0, t.iz);  // sample k of the run: k rows further
    float old[kYRun];  // every load of the run is issued before the first store, as terrain_swap_kernel
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) old[k] = grid[s0 + (uint64_t)sh.dim_x * k];
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) {
            const uint64_t sample = s0 + (uint64_t)sh.dim_x * k;
            if (kJournal) image[j0 + (uint64_t)m.dx * k] = old[k];
            const float md = clamp_drawn(q[k], sh.seed, m.event, sample, 0u);
            grid[sample] = csg_combine(sh, m.event, sample, m.add_or_erode, md, old[k]);
        }
}

int check_path(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    if (!md.data) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path data is null", i);
    const int n = md.data_dims[0];
    if (n < 1 || n > kPathMaxSegments) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path segment count %d not in 1..%d", i, n, kPathMaxSegments);
    if (md.data_dims[1] != 8) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path data_dims[1] is %d, a segment is 8 floats", i, md.data_dims[1]);
    for (int s = 0; s < n; ++s)
        for (int k = 0; k < 8; ++k) {
            const float v = md.data[(size_t)8 * s + k];
            if (!std::isfinite(v)) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path segment %d: value %d not finite", i, s, k);
            if ((k == 3 || k == 7) && v < 0.0f) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path segment %d: radius %g below 0", i, s, v);
            if (std::fabs(v) > 1048576.0f)
                return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: path segment %d: value %d is %g, above 2^20 in magnitude", i, s, k, v);
        }
    return VTMC_OK;
}

// The device records of a checked modifier: the host half of the header's rule (FP32, one operation per step) and the pruning bounds.
static std::vector<float> path_records(const TerrainShape &sh, const vtmc_modifier &md)
{
    const int n = md.data_dims[0], n_chunks = (n + kPathChunk - 1) / kPathChunk;
    std::vector<float> rec((size_t)16 * n + (size_t)8 * n_chunks, 0.0f);
    float *seg = rec.data(), *bound = seg + (size_t)8 * n, *chunk = bound + (size_t)8 * n;
    float grid_reach = 0.0f;  // the largest |world coordinate| of the grid
    const int dims[3] = {sh.dim_x, sh.dim_y, sh.dim_z};
    for (int k = 0; k < 3; ++k) grid_reach = std::max({grid_reach, std::fabs(sh.origin[k]), std::fabs((float)(dims[k] - 1) * sh.scale + sh.origin[k])});
    for (int c = 0; c < n_chunks; ++c)
        for (int k = 0; k < 3; ++k) chunk[8 * c + k] = INFINITY, chunk[8 * c + 4 + k] = -INFINITY;
    for (int s = 0; s < n; ++s) {
        const float *v = md.data + (size_t)8 * s;
        float *o = seg + (size_t)8 * s, *b = bound + (size_t)8 * s, *cb = chunk + 8 * (s / kPathChunk);
        const float ex = v[4] - v[0], ey = v[5] - v[1], ez = v[6] - v[2];
        const float ll = (ex * ex + ey * ey) + ez * ez;
        o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
        o[4] = ex, o[5] = ey, o[6] = ez, o[7] = v[7] - v[3];
        b[3] = ll >= 1e-30f ? 1.0f / ll : 0.0f;
        // the pruning reach (terrain_path_kernel): max(ra, rb) + 2 + slack, slack = max(0.01, 1e-4 * the largest |coordinate| involved)
        float reach = grid_reach;
        for (int k = 0; k < 8; ++k) reach = std::max(reach, std::fabs(v[k]));
        const float grow = std::max(v[3], v[7]) + 2.0f + std::max(0.01f, 1e-4f * reach);
        for (int k = 0; k < 3; ++k) {
            b[k] = std::min(v[k], v[4 + k]) - grow;
            b[4 + k] = std::max(v[k], v[4 + k]) + grow;
            cb[k] = std::min(cb[k], b[k]);
            cb[4 + k] = std::max(cb[4 + k], b[4 + k]);
        }
    }
    return rec;
}

int apply_path(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image)
{
    const std::vector<float> rec = path_records(ctx->tshape, md);
    const int n = md.data_dims[0];
    if (int rc = stage_for_queue(ctx, ctx->path, rec.data(), rec.size() * sizeof(float))) return rc;
    TerrainPathArgs p{};
    p.seg = (const float4 *)ctx->path.p;
    p.bound = p.seg + (size_t)2 * n;
    p.chunk = p.bound + (size_t)2 * n;
    p.n_seg = n;
    p.add_or_erode = a.add_or_erode;
    p.lx = a.lx, p.ly = a.ly, p.lz = a.lz, p.dx = a.dx, p.dy = a.dy, p.dz = a.dz;
    p.event = a.event;
    VTMC_HIP(ctx, launch_box(image ? terrain_path_kernel<true> : terrain_path_kernel<false>, box_of(a), ctx->stream, grid, image, ctx->tshape, p));
    return VTMC_OK;
}

}  // namespace vtmc
