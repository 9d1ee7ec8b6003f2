// terrain_water.hip -- standing water: floods a box of the resident grid from sources to their levels (vtmc_terrain_flood and the readers
// of its result, include/vtmc_water.h).  Not in the reference.  The rule WATER is in the header; everything here is integers and 32-bit
// copies but the volume kernel's three FP32 steps and the probe's one.  Hand-written for gfx950 / CDNA4.
//
// The levels are processed from the highest to the lowest, everything queued on the context's stream with no read-back in between (the
// body count stays in a control word on the device; a body is at most a source, so the record list has a fixed size).  Per level:
//   1. water_local_kernel    tile_label.h's phase 1 on the predicate "open, plane <= the level's plane, body < 0": one read of the grid
//                            and of the body volume.
//   2. water_merge_kernel    tile_label.h's phase 2.
//   3. water_flatten_kernel  every sample of the graph to its root.
//   4. water_number_kernel   ONE workgroup over the level's sources (at most 4096): a source on a wet sample joins that body; the others
//                            look up their root, and the distinct roots are numbered by RANK -- a root's body index is the body count so
//                            far plus the number of distinct smaller roots of this level -- so no atomic decides an index.  A numbered
//                            root's parent word becomes -2 - body.
//   5. water_assign_kernel   every sample whose root was numbered takes the body index in the body volume.
// After the last level water_stats_kernel counts samples and surface, reduces bounds and face flags (a run of a wave along x shares one
// set of atomics: sums, minima, maxima and ors, whose order does not matter), and water_volume_kernel stages a tile of body indices with a
// halo of 1 in LDS, takes the 27-neighbour minimum there (bodies are ordered by descending level: the smallest index is the largest
// level), reads the grid once for the solid test of a near sample and writes the floats coalesced along x.
//
// EVERY LOOP IS BOUNDED: the labelling's as in terrain_fragments.hip (union_find.h); the number kernel's by the source count.  A
// violation sets the flag word and the call answers VTMC_ERR_DEVICE ("labelling did not converge") with no result left.
#include "terrain_edit.h"
#include "terrain_water.h"
#include "tile_label.h"
#include <climits>
#include <cstring>
#include <vector>

namespace vtmc {

enum { kWaterFlag = 0, kWaterBodies = 1, kWaterCtlWords = 4 };

// the flood's box and its volumes as the kernels take them
struct WaterShape {
    TerrainBox b;
    int vx, vy, vz;   // samples per axis of the volumes
};
__device__ __forceinline__ int volume_index(const WaterShape &w, int ix, int iy, int iz) { return ix + w.vx * (iy + w.vy * iz); }

// Phase 1 on the open, dry samples of the box at or under box plane `plane`.
__global__ __launch_bounds__(256) void water_local_kernel(const float *__restrict__ grid, const int *__restrict__ body, int *__restrict__ P,
                                                          int *__restrict__ flag, TerrainShape sh, WaterShape w, int plane)
{
    label_local(flag, w.b,
                [=](int ix, int iy, int iz) {
                    return iy <= plane && body[volume_index(w, ix, iy, iz)] < 0 && !(grid[grid_index(sh, w.b.lx + ix, w.b.ly + iy, w.b.lz + iz)] > 0.0f);
                },
                [=](int j, int label) { P[j] = label; });
}

__global__ __launch_bounds__(256) void water_merge_kernel(int *__restrict__ P, int *__restrict__ flag, TerrainBox b, int n) { label_merge(P, flag, b, n); }

__global__ __launch_bounds__(256) void water_flatten_kernel(int *__restrict__ P, int *__restrict__ flag, TerrainBox b, int n, int plane)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const RowThread t;
    if (!t.inside(b) || t.iy > plane) return;
    const int j = frag_index(b, t.ix, t.iy, t.iz);
    if (uf_load<kScope>(P, j) < 0) return;
    const int root = uf_find<kScope>(P, j, n, flag);
    if (root >= 0) P[j] = root;
}

// Step 4: one workgroup of 1024 lanes over the m <= VTMC_WATER_MAX_SOURCES sources of a level.  R[i]: the root of source i when it is a
// seed of the graph, -1 otherwise; F[i]: it is the first source of its root.
__global__ __launch_bounds__(1024) void water_number_kernel(const WaterSeed *__restrict__ seeds, int m, float level, int *__restrict__ P,
                                                            const int *__restrict__ body, vtmc_water_body *__restrict__ recs,
                                                            int *__restrict__ source_body, int *__restrict__ ctl, TerrainBox b)
{
    __shared__ int R[VTMC_WATER_MAX_SOURCES];
    __shared__ unsigned char F[VTMC_WATER_MAX_SOURCES];
    __shared__ int fresh;
    const int tid = threadIdx.x;
    if (tid == 0) fresh = 0;
    const int base = ctl[kWaterBodies];
    for (int i = tid; i < m; i += 1024) {
        const WaterSeed s = seeds[i];
        int r = -1;
        if (s.box_index >= 0) {
            const int wet = body[s.volume_index];
            if (wet >= 0) {   // a joiner: the body is of a higher level, numbered by an earlier launch
                source_body[s.source] = wet;
                atomicAdd(&recs[wet].n_sources, 1);
            } else {
                const int p = P[s.box_index];
                if (p >= 0) r = p;
            }
        }
        R[i] = r;
    }
    __syncthreads();
    for (int i = tid; i < m; i += 1024) {
        const int r = R[i];
        bool first = r >= 0;
        for (int j = 0; j < i && first; ++j) first = R[j] != r;
        F[i] = first;
    }
    __syncthreads();
    for (int i = tid; i < m; i += 1024) {
        const int r = R[i];
        if (r < 0) continue;
        int rank = 0, sharing = 0;
        for (int j = 0; j < m; ++j) {
            rank += F[j] && R[j] < r;
            sharing += R[j] == r;
        }
        const int index = base + rank;
        source_body[seeds[i].source] = index;
        if (!F[i]) continue;
        vtmc_water_body rec;
        rec.seed[0] = b.lx + r % b.dx, rec.seed[1] = b.ly + r / b.dx % b.dy, rec.seed[2] = b.lz + r / b.dx / b.dy;
        rec.lo[0] = rec.lo[1] = rec.lo[2] = INT_MAX;
        rec.hi[0] = rec.hi[1] = rec.hi[2] = INT_MIN;
        rec.level = level;
        rec.n_samples = rec.n_surface = 0;
        rec.flags = 0u;
        rec.n_sources = sharing;
        rec.reserved[0] = rec.reserved[1] = 0u;
        recs[index] = rec;
        P[r] = -2 - index;
        atomicAdd(&fresh, 1);
    }
    __syncthreads();
    if (tid == 0) ctl[kWaterBodies] = base + fresh;
}

// Step 5: a sample's parent word is -1 (not in the graph), a root's index, or -2 - body on a numbered root.
__global__ __launch_bounds__(256) void water_assign_kernel(const int *__restrict__ P, int *__restrict__ body, WaterShape w, int n, int plane)
{
    const RowThread t;
    if (!t.inside(w.b) || t.iy > plane) return;
    int v = P[frag_index(w.b, t.ix, t.iy, t.iz)];
    if (v >= 0 && v < n) v = P[v];
    if (v <= -2) body[volume_index(w, t.ix, t.iy, t.iz)] = -2 - v;
}

template <class T>
__device__ __forceinline__ T peek(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Counts, bounds, surface and face flags, one lane per sample of the box: the first lane of a run along x of one body reduces for the run.
__global__ __launch_bounds__(256) void water_stats_kernel(const float *__restrict__ grid, const int *__restrict__ body, vtmc_water_body *recs,
                                                          TerrainShape sh, WaterShape w)
{
    const RowThread t;
    const TerrainBox &b = w.b;
    int key = -1;
    bool surface = false, face = false;
    if (t.inside(b)) {
        const int v = volume_index(w, t.ix, t.iy, t.iz);
        key = body[v];
        if (key >= 0) {
            face = t.iy == 0 || t.ix == 0 || t.ix == b.dx - 1 || t.iz == 0 || t.iz == b.dz - 1;
            if (t.iy + 1 < b.dy && body[v + w.vx] < 0) surface = !(grid[grid_index(sh, b.lx + t.ix, b.ly + t.iy + 1, b.lz + t.iz)] > 0.0f);
        }
    }
    const unsigned long long surfaces = __ballot(surface), faces = __ballot(face);
    const int len = run_length(key);
    if (len > 0) {
        const int lane = __lane_id();
        const unsigned long long run = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
        vtmc_water_body *r = recs + key;
        const int x = b.lx + t.ix, y = b.ly + t.iy, z = b.lz + t.iz;
        atomicAdd(&r->n_samples, len);
        if (surfaces & run) atomicAdd(&r->n_surface, __popcll(surfaces & run));
        // A bound or the flag is touched only where this run would change it: what the load sees is the current value or an older one, and
        // a bound only ever tightens towards its end, so an old value can cost an atomic that changes nothing, never skip one that would.
        // Inside a large body almost every run skips all seven.
        if ((faces & run) && !(peek(&r->flags) & VTMC_WATER_AT_FACE)) atomicOr(&r->flags, (uint32_t)VTMC_WATER_AT_FACE);
        if (x < peek(&r->lo[0])) atomicMin(&r->lo[0], x);
        if (x + len - 1 > peek(&r->hi[0])) atomicMax(&r->hi[0], x + len - 1);
        if (y < peek(&r->lo[1])) atomicMin(&r->lo[1], y);
        if (y > peek(&r->hi[1])) atomicMax(&r->hi[1], y);
        if (z < peek(&r->lo[2])) atomicMin(&r->lo[2], z);
        if (z > peek(&r->hi[2])) atomicMax(&r->hi[2], z);
    }
}

// The water volume.  A workgroup of 64 x 4 lanes makes a tile of 64 x 4 x 4 samples of the volume; the body indices of the tile and of a
// halo of 1 lie in LDS as unsigned words (-1, dry, is the largest), so the smallest body index of the 27 is one min chain.
constexpr int kVolX = 64, kVolY = 4, kVolZ = 4, kHaloX = kVolX + 2, kHaloY = kVolY + 2, kHaloZ = kVolZ + 2;

__global__ __launch_bounds__(256) void water_volume_kernel(const float *__restrict__ grid, const int *__restrict__ body, const vtmc_water_body *__restrict__ recs,
                                                           float *__restrict__ water, TerrainShape sh, WaterShape w)
{
    __shared__ unsigned B[kHaloX * kHaloY * kHaloZ];
    const int x0 = blockIdx.x * kVolX, y0 = blockIdx.y * kVolY, z0 = blockIdx.z * kVolZ;
    const int tid = threadIdx.x + 64 * threadIdx.y;
    for (int i = tid; i < kHaloX * kHaloY * kHaloZ; i += 256) {
        const int hx = i % kHaloX, hy = i / kHaloX % kHaloY, hz = i / (kHaloX * kHaloY);
        const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
        unsigned v = 0xffffffffu;
        if (x >= 0 && x < w.vx && y >= 0 && y < w.vy && z >= 0 && z < w.vz) v = (unsigned)body[volume_index(w, x, y, z)];
        B[i] = v;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= w.vx || y >= w.vy) return;
    const bool row_in_box = x < w.b.dx && y < w.b.dy;
    const float height = (float)(w.b.ly + y) * sh.scale + sh.origin[1];   // y_j of this lane's plane
    for (int lz = 0; lz < kVolZ; ++lz) {
        const int z = z0 + lz;
        if (z >= w.vz) break;
        float value = -1.0f;
        if (row_in_box && z < w.b.dz) {
            const int c = (int)threadIdx.x + 1 + kHaloX * ((int)threadIdx.y + 1 + kHaloY * (lz + 1));
            const unsigned own = B[c];
            unsigned nearest = 0xffffffffu;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) nearest = min(nearest, B[c + dx + kHaloX * (dy + kHaloY * dz)]);
            if (nearest != 0xffffffffu) {
                float tt = recs[own != 0xffffffffu ? own : nearest].level - height;
                tt = tt / sh.scale;
                tt = tt < -1.0f ? -1.0f : (tt > 1.0f ? 1.0f : tt);
                if (own != 0xffffffffu || tt <= 0.0f || grid[grid_index(sh, w.b.lx + x, w.b.ly + y, w.b.lz + z)] > 0.0f) value = tt;
            }
        }
        water[volume_index(w, x, y, z)] = value;
    }
}

// One lane per query: the nearest sample by the source rule, its body and the depth under the level.
__global__ __launch_bounds__(256) void water_probe_kernel(const float *__restrict__ positions, int n, const int *__restrict__ body,
                                                          const vtmc_water_body *__restrict__ recs, int *__restrict__ body_out, float *__restrict__ depth_out,
                                                          TerrainShape sh, WaterShape w)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]};
    int c[3];
    bool in = true;
    for (int k = 0; k < 3; ++k) {
        float g = p[k] - sh.origin[k];
        g = g / sh.scale;
        g = floorf(g + 0.5f);
        in = in && g >= -1.0f && g <= 2048.0f;   // a grid index is below 1026: anything else, NaN included, is outside every box
        c[k] = in ? (int)g : -1;
    }
    in = in && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    const int ix = c[0] - w.b.lx, iy = c[1] - w.b.ly, iz = c[2] - w.b.lz;
    int found = -1;
    float depth = 0.0f;
    if (in && ix >= 0 && ix < w.b.dx && iy >= 0 && iy < w.b.dy && iz >= 0 && iz < w.b.dz) {
        found = body[volume_index(w, ix, iy, iz)];
        if (found >= 0) depth = recs[found].level - p[1];
    }
    body_out[i] = found;
    depth_out[i] = depth;
}

static WaterShape water_shape(const VtmcWater &r) { return WaterShape{TerrainBox{r.lo[0], r.lo[1], r.lo[2], r.d[0], r.d[1], r.d[2]}, r.vd[0], r.vd[1], r.vd[2]}; }
static size_t volume_samples(const VtmcWater &r) { return (size_t)r.vd[0] * r.vd[1] * r.vd[2]; }

static int water_gate(const vtmc_ctx *ctx, const char *who)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->water.valid) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_NO_RESULT, "%s before terrain_flood", who);
    return VTMC_OK;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_flood(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_water_source *sources, int32_t n_sources,
                           uint32_t flags, int32_t *source_body, int32_t *n_bodies)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_bodies) *n_bodies = 0;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_flood before terrain_init");
    if (const char *what = flood_args_fault(lower, upper, sources, n_sources, flags)) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_flood: %s", what);
    const TerrainShape &sh = ctx->tshape;
    const TerrainBox b = bounds_box(sh, lower, upper);
    VtmcWater &r = ctx->water;
    for (int32_t i = 0; source_body && i < n_sources; ++i) source_body[i] = -1;
    if (box_empty(b)) {   // a success with no bodies and dims (0, 0, 0)
        r.valid = true, r.wet = 0, r.bodies.clear();
        for (int k = 0; k < 3; ++k) r.lo[k] = r.d[k] = r.vd[k] = 0;
        r.lo[0] = b.lx, r.lo[1] = b.ly, r.lo[2] = b.lz;
        return VTMC_OK;
    }
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t box_lo[3] = {b.lx, b.ly, b.lz}, box_d[3] = {b.dx, b.dy, b.dz};
    const int32_t vd[3] = {water_volume_dim(b.dx), water_volume_dim(b.dy), water_volume_dim(b.dz)};
    const size_t n = (size_t)b.dx * b.dy * b.dz, vn = (size_t)vd[0] * vd[1] * vd[2];
    // the sources level by level, and each level's plane in the box
    const std::vector<float> levels = water_levels(sources, n_sources);
    std::vector<WaterSeed> seeds;
    std::vector<size_t> first(levels.size() + 1, 0);
    for (size_t l = 0; l < levels.size(); ++l) {
        water_level_seeds(sources, n_sources, levels[l], sh.origin, sh.scale, box_lo, box_d, vd, seeds);
        first[l + 1] = seeds.size();
    }
    // the buffers hold the previous result: grown and written only after the stream has drained, and from here on it is gone
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    r.valid = false;
    if (int rc = ensure(ctx, r.water, 4 * vn)) return rc;
    if (int rc = ensure(ctx, r.body, 4 * vn)) return rc;
    if (int rc = ensure(ctx, r.labels, 4 * n)) return rc;
    if (int rc = ensure(ctx, r.records, sizeof(vtmc_water_body) * VTMC_WATER_MAX_SOURCES)) return rc;
    if (int rc = ensure(ctx, r.seeds, sizeof(WaterSeed) * VTMC_WATER_MAX_SOURCES)) return rc;
    if (int rc = ensure(ctx, r.source_body, 4 * VTMC_WATER_MAX_SOURCES)) return rc;
    if (int rc = ensure(ctx, r.ctl, kWaterCtlWords * sizeof(int))) return rc;
    hipStream_t s = ctx->stream;
    const float *grid = (const float *)ctx->terrain.p;
    float *water = (float *)r.water.p;
    int *body = (int *)r.body.p, *P = (int *)r.labels.p, *d_source_body = (int *)r.source_body.p, *ctl = (int *)r.ctl.p;
    vtmc_water_body *recs = (vtmc_water_body *)r.records.p;
    WaterSeed *d_seeds = (WaterSeed *)r.seeds.p;
    const WaterShape w{b, vd[0], vd[1], vd[2]};
    VTMC_HIP(ctx, ctx->water_clock.begin());
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kWaterCtlWords * sizeof(int), s));
    VTMC_HIP(ctx, hipMemsetAsync(body, 0xff, 4 * vn, s));
    VTMC_HIP(ctx, hipMemsetAsync(d_source_body, 0xff, 4 * VTMC_WATER_MAX_SOURCES, s));
    VTMC_HIP(ctx, hipMemsetAsync(recs, 0, sizeof(vtmc_water_body) * VTMC_WATER_MAX_SOURCES, s));
    if (!seeds.empty()) VTMC_HIP(ctx, hipMemcpyAsync(d_seeds, seeds.data(), sizeof(WaterSeed) * seeds.size(), hipMemcpyHostToDevice, s));
    VTMC_HIP(ctx, ctx->water_clock.mark(0, s));
    for (size_t l = 0; l < levels.size(); ++l) {
        const int m = (int)(first[l + 1] - first[l]);
        bool any = false;
        for (size_t i = first[l]; i < first[l + 1]; ++i) any = any || seeds[i].box_index >= 0;
        if (!any) continue;   // every source of the level lies outside the box: all dry
        const int plane = std::min(water_plane(levels[l], sh.scale, sh.origin[1], sh.dim_y) - b.ly, b.dy - 1);
        if (plane >= 0) {
            VTMC_HIP(ctx, launch(water_local_kernel, tile_grid(b), dim3(64, 4, 1), 0, s, grid, (const int *)body, P, ctl + kWaterFlag, sh, w, plane));
            VTMC_HIP(ctx, launch_rows(water_merge_kernel, b, s, P, ctl + kWaterFlag, b, (int)n));
            VTMC_HIP(ctx, launch_rows(water_flatten_kernel, b, s, P, ctl + kWaterFlag, b, (int)n, plane));
        } else {   // nothing of the box is under the level: no graph, but a source may still join
            VTMC_HIP(ctx, hipMemsetAsync(P, 0xff, 4 * n, s));
        }
        VTMC_HIP(ctx, launch(water_number_kernel, dim3(1), dim3(1024), 0, s, (const WaterSeed *)(d_seeds + first[l]), m, levels[l], P, (const int *)body, recs,
                             d_source_body, ctl, b));
        if (plane >= 0) VTMC_HIP(ctx, launch_rows(water_assign_kernel, b, s, (const int *)P, body, w, (int)n, plane));
    }
    VTMC_HIP(ctx, ctx->water_clock.mark(1, s));
    VTMC_HIP(ctx, launch_rows(water_stats_kernel, b, s, grid, (const int *)body, recs, sh, w));
    VTMC_HIP(ctx, ctx->water_clock.mark(2, s));
    VTMC_HIP(ctx, launch(water_volume_kernel, dim3((unsigned)((vd[0] + kVolX - 1) / kVolX), (unsigned)((vd[1] + kVolY - 1) / kVolY), (unsigned)((vd[2] + kVolZ - 1) / kVolZ)),
                         dim3(64, 4, 1), 0, s, grid, (const int *)body, (const vtmc_water_body *)recs, water, sh, w));
    VTMC_HIP(ctx, ctx->water_clock.mark(3, s));
    int h_ctl[kWaterCtlWords];
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    VTMC_HIP(ctx, hipMemcpy(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost));
    if (h_ctl[kWaterFlag]) return fail(ctx, VTMC_ERR_DEVICE, "terrain_flood: labelling did not converge (flag %d)", h_ctl[kWaterFlag]);
    const int32_t nb = h_ctl[kWaterBodies];
    if (nb < 0 || nb > n_sources) return fail(ctx, VTMC_ERR_DEVICE, "terrain_flood: %d bodies of %d sources", nb, n_sources);
    r.bodies.assign((size_t)nb, vtmc_water_body{});
    if (nb) VTMC_HIP(ctx, hipMemcpy(r.bodies.data(), recs, sizeof(vtmc_water_body) * (size_t)nb, hipMemcpyDeviceToHost));
    if (source_body && n_sources) VTMC_HIP(ctx, hipMemcpy(source_body, d_source_body, 4 * (size_t)n_sources, hipMemcpyDeviceToHost));
    r.wet = 0;
    for (const vtmc_water_body &body_rec : r.bodies) r.wet += body_rec.n_samples;
    for (int k = 0; k < 3; ++k) r.lo[k] = box_lo[k], r.d[k] = box_d[k], r.vd[k] = vd[k];
    ctx->water_clock.arm();
    r.valid = true;
    if (n_bodies) *n_bodies = nb;
    return VTMC_OK;
}

int32_t vtmc_water_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int32_t volume_dims[3], int32_t *n_bodies, int64_t *n_wet)
{
    if (int rc = water_gate(ctx, "water_info")) return rc;
    const VtmcWater &r = ctx->water;
    for (int k = 0; k < 3; ++k) {
        if (box_lo) box_lo[k] = r.lo[k];
        if (box_dims) box_dims[k] = r.d[k];
        if (volume_dims) volume_dims[k] = r.vd[k];
    }
    if (n_bodies) *n_bodies = (int32_t)r.bodies.size();
    if (n_wet) *n_wet = r.wet;
    return VTMC_OK;
}

int32_t vtmc_water_bodies(vtmc_ctx *ctx, vtmc_water_body *dst, int32_t capacity)
{
    if (int rc = water_gate(ctx, "water_bodies")) return rc;
    const VtmcWater &r = ctx->water;
    if (capacity < 0 || (!dst && !r.bodies.empty())) return fail(ctx, VTMC_ERR_INVALID_ARG, "water_bodies: dst is null or capacity < 0");
    if ((size_t)capacity < r.bodies.size()) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %zu bodies", capacity, r.bodies.size());
    if (!r.bodies.empty()) memcpy(dst, r.bodies.data(), sizeof(vtmc_water_body) * r.bodies.size());
    return VTMC_OK;
}

int32_t vtmc_water_read(vtmc_ctx *ctx, float *water_dst, int32_t *body_dst, int64_t capacity_samples)
{
    if (int rc = water_gate(ctx, "water_read")) return rc;
    const VtmcWater &r = ctx->water;
    const size_t vn = volume_samples(r);
    if (capacity_samples < 0 || (uint64_t)capacity_samples < vn) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %zu samples", (long long)capacity_samples, vn);
    if (vn == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (water_dst) VTMC_HIP(ctx, hipMemcpy(water_dst, r.water.p, 4 * vn, hipMemcpyDeviceToHost));
    if (body_dst) VTMC_HIP(ctx, hipMemcpy(body_dst, r.body.p, 4 * vn, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_water_device_results(vtmc_ctx *ctx, const float **d_water, const int32_t **d_body, int32_t volume_dims[3])
{
    if (int rc = water_gate(ctx, "water_device_results")) return rc;
    const VtmcWater &r = ctx->water;
    const bool any = volume_samples(r) != 0;
    if (d_water) *d_water = any ? (const float *)r.water.p : nullptr;
    if (d_body) *d_body = any ? (const int32_t *)r.body.p : nullptr;
    for (int k = 0; volume_dims && k < 3; ++k) volume_dims[k] = r.vd[k];
    return VTMC_OK;
}

int32_t vtmc_water_probe(vtmc_ctx *ctx, const float *positions, int32_t n, int32_t *body_out, float *depth_out)
{
    if (int rc = water_gate(ctx, "water_probe")) return rc;
    if (n < 0 || (n > 0 && !positions)) return fail(ctx, VTMC_ERR_INVALID_ARG, "water_probe: positions is null or n < 0");
    if (n == 0) return VTMC_OK;
    VtmcWater &r = ctx->water;
    if (volume_samples(r) == 0) {   // an empty box: nothing is wet
        for (int32_t i = 0; i < n; ++i) {
            if (body_out) body_out[i] = -1;
            if (depth_out) depth_out[i] = 0.0f;
        }
        return VTMC_OK;
    }
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = 12 * (size_t)n, out_bytes = 4 * (size_t)n;
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier probe may still be reading the stage
    if (int rc = ensure(ctx, r.probe, in_bytes + 2 * out_bytes)) return rc;
    float *d_pos = (float *)r.probe.p, *d_depth = (float *)((char *)r.probe.p + in_bytes + out_bytes);
    int *d_body = (int *)((char *)r.probe.p + in_bytes);
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipMemcpyAsync(d_pos, positions, in_bytes, hipMemcpyHostToDevice, s));
    VTMC_HIP(ctx, launch(water_probe_kernel, lanes256(n), dim3(256), 0, s, (const float *)d_pos, (int)n, (const int *)r.body.p, (const vtmc_water_body *)r.records.p,
                         d_body, d_depth, ctx->tshape, water_shape(r)));
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    if (body_out) VTMC_HIP(ctx, hipMemcpy(body_out, d_body, out_bytes, hipMemcpyDeviceToHost));
    if (depth_out) VTMC_HIP(ctx, hipMemcpy(depth_out, d_depth, out_bytes, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

// device time of the last flood's three phases: the levels, the statistics, the volume (not in the header)
int32_t vtmc_debug_water_ms(vtmc_ctx *ctx, float ms[3])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->water_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "no flood has run its kernels");
    if (int rc = ctx->water_clock.sync_last(ctx)) return rc;
    for (int i = 0; i < 3; ++i)
        if (int rc = ctx->water_clock.elapsed(ctx, i, i + 1, ms + i)) return rc;
    return VTMC_OK;
}

}  // extern "C"
