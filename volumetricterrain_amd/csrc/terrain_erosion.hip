// terrain_erosion.hip -- VTMC_MOD_EROSION: hydraulic and thermal erosion of the heightfield of a box of the resident grid (not in the
// reference), an entry of the modifier table (terrain_edit.h), and the readers of the maps it leaves (include/vtmc_erosion.h, where the
// rule EROSION is written operation by operation; tests/erosion_twin.py is the same rule in numpy and is held to these kernels bit for
// bit).  Host half: terrain_erosion.h.
//
//   erosion_heights_kernel    one lane per column, lanes along x, so every y step of a wave is one coalesced row of the grid; walks from the
//                             top of the box down to the topmost solid sample; fills the state and counts the active columns.
//   the step, three kernels   split where a lane needs a value its neighbour has just computed -- a launch boundary is the barrier:
//     erosion_flux_kernel       f' from b and d of the column and its four neighbours; f is the lane's own, updated in place.
//     erosion_water_kernel      d2, the speed, erosion and deposition: reads f' and b of the neighbours; writes b1 to the second b plane,
//                               s1 over s (only the lane itself read it) and d2 to the second d plane (the neighbours' d1 is still needed).
//     erosion_transport_kernel  transport, evaporation, thermal: reads s1, d and f' of the neighbours and b1; writes s2 and d3 to the second
//                               s and d planes and b2 back to the first b plane.
//                             So b is in its first plane at every step boundary, and d and s change planes once a step.  Each kernel is
//                             a radius-1 stencil over a few planes, 64 x 4 columns per workgroup, neighbour loads served by the caches.
//                             Each also has a variant that stages the planes it reads at a neighbour in LDS (template <kLds>); it was
//                             measured slower (profiles/r28/erosion/README.md) and runs only behind vtmc_debug_erosion_lds.
//   erosion_finish_kernel     the clamp of the final heights and the two counts that depend on it.
//   erosion_writeback_kernel  the box walk of terrain_box.h: the journal image of every sample of the box when history is on, and the band.
// All 3 * iterations + 3 launches are queued back to back on ctx->stream, with no read-back and no flag between them
// (vtmc_nav_distance_build queues its rounds the same way); the counts are read when vtmc_erosion_info asks for them.
#include "terrain_edit.h"
#include "terrain_erosion.h"

namespace vtmc {

struct ErosionPlanes {
    float *before, *b[2], *s[2], *d[2], *f[4];
    uint8_t *mask;
    int32_t *ctl;   // n_active, n_rewritten, n_clamped
};

static ErosionPlanes erosion_planes(void *state, const ErosionLayout &l)
{
    float *base = (float *)state;
    auto plane = [&](int k) { return base + (size_t)k * (size_t)l.stride; };
    ErosionPlanes p;
    p.before = plane(kBefore);
    p.b[0] = plane(kB0), p.b[1] = plane(kB1);
    p.s[0] = plane(kS0), p.s[1] = plane(kS1);
    p.d[0] = plane(kD0), p.d[1] = plane(kD1);
    for (int k = 0; k < 4; ++k) p.f[k] = plane(kF0 + k);
    p.mask = (uint8_t *)state + l.mask_off;
    p.ctl = (int32_t *)((char *)state + l.ctl_off);
    return p;
}

__device__ __forceinline__ float sum4(const float v[4]) { return (v[0] + v[1]) + (v[2] + v[3]); }

// The LDS variant of a step kernel stages, for every plane it reads at a neighbour, the 64 x 4 columns of its workgroup with a halo of one
// column: a tile of 66 x 6 floats.  A column outside the box reads 0 there; nothing reads it, since such a neighbour does not count.
constexpr int kErosionTileW = 66, kErosionTileH = 6, kErosionTile = kErosionTileW * kErosionTileH;

__device__ __forceinline__ void erosion_stage(const float *__restrict__ plane, float *tile, int nx, int nz)
{
    const int x0 = blockIdx.x * 64 - 1, z0 = blockIdx.y * 4 - 1;
    for (int i = threadIdx.y * 64 + threadIdx.x; i < kErosionTile; i += 256) {
        const int x = x0 + i % kErosionTileW, z = z0 + i / kErosionTileW;
        tile[i] = x >= 0 && x < nx && z >= 0 && z < nz ? plane[x + nx * z] : 0.0f;
    }
}

// This lane's column of the nx x nz plane, its four neighbours [-x, +x, -z, +z] and whether each counts; the same places in a tile.
// find() is false where there is no active column.
struct ErosionColumn {
    int c, n[4], tc, tn[4];
    bool v[4];
    __device__ __forceinline__ bool find(int nx, int nz, const uint8_t *__restrict__ mask)
    {
        const int x = blockIdx.x * 64 + threadIdx.x, z = blockIdx.y * 4 + threadIdx.y;
        if (x >= nx || z >= nz) return false;
        c = x + nx * z;
        if (!mask[c]) return false;
        n[0] = c - 1, n[1] = c + 1, n[2] = c - nx, n[3] = c + nx;
        tc = (threadIdx.y + 1) * kErosionTileW + threadIdx.x + 1;
        tn[0] = tc - 1, tn[1] = tc + 1, tn[2] = tc - kErosionTileW, tn[3] = tc + kErosionTileW;
        v[0] = x > 0 && mask[c - 1];
        v[1] = x + 1 < nx && mask[c + 1];
        v[2] = z > 0 && mask[c - nx];
        v[3] = z + 1 < nz && mask[c + nx];
        return true;
    }
};
// a plane's value at a place: from the staged tile, or from memory
template <bool kLds>
__device__ __forceinline__ float erosion_at(const float *__restrict__ plane, const float *tile, int global_index, int tile_index)
{
    return kLds ? tile[tile_index] : plane[global_index];
}

// adds the number of lanes of this wave for which `flag` holds to *counter: one atomic per wave (a wave is one row of 64 columns)
__device__ __forceinline__ void count_lanes(bool flag, int32_t *counter)
{
    const unsigned long long votes = __ballot(flag);
    if (threadIdx.x == 0 && votes) atomicAdd(counter, (int32_t)__popcll(votes));
}

__global__ __launch_bounds__(256) void erosion_heights_kernel(const float *__restrict__ grid, TerrainShape sh, TerrainBox box, ErosionPlanes p)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iz = blockIdx.y * 4 + threadIdx.y;
    const bool inside = ix < box.dx && iz < box.dz;
    bool active = false;
    float h0 = 0.0f;
    if (inside) {
        const int x = box.lx + ix, z = box.lz + iz, uy = box.ly + box.dy - 1;
        float above = grid[grid_index(sh, x, uy, z)];
        if (!(above > 0.0f))
            for (int j = uy - 1; j >= box.ly; --j) {
                const float s = grid[grid_index(sh, x, j, z)];
                if (s > 0.0f) {
                    h0 = (float)j + s / (s - above);
                    active = true;
                    break;
                }
                above = s;
            }
        const int c = ix + box.dx * iz;
        p.before[c] = h0;
        p.b[0][c] = h0;
        p.b[1][c] = 0.0f;
        p.s[0][c] = 0.0f, p.s[1][c] = 0.0f;
        p.d[0][c] = 0.0f, p.d[1][c] = 0.0f;
        for (int k = 0; k < 4; ++k) p.f[k][c] = 0.0f;
        p.mask[c] = active ? 1 : 0;
    }
    count_lanes(active, p.ctl + 0);
}

template <bool kLds>
__global__ __launch_bounds__(256) void erosion_flux_kernel(ErosionPlanes p, int nx, int nz, int cur, ErosionStep e)
{
    __shared__ float tile[kLds ? 2 : 1][kLds ? kErosionTile : 1];
    ErosionColumn col;
    const bool live = col.find(nx, nz, p.mask);
    const float *__restrict__ b = p.b[0], *__restrict__ d = p.d[cur];
    if (kLds) {
        erosion_stage(b, tile[0], nx, nz);
        erosion_stage(d, tile[1], nx, nz);
        __syncthreads();
    }
    if (!live) return;
    const float *tb = tile[0], *td = tile[kLds ? 1 : 0];
    const int c = col.c;
    const float d1 = erosion_at<kLds>(d, td, c, col.tc) + e.dt_rain;
    const float H = erosion_at<kLds>(b, tb, c, col.tc) + d1;
    float f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = 0.0f;
        if (col.v[k]) {
            const float dn = erosion_at<kLds>(d, td, col.n[k], col.tn[k]) + e.dt_rain;
            const float Hn = erosion_at<kLds>(b, tb, col.n[k], col.tn[k]) + dn;
            const float t = e.dt_g * (H - Hn);
            const float g = p.f[k][c] + t;
            f[k] = g > 0.0f ? g : 0.0f;
        }
    }
    const float out = sum4(f);
    const float vol = out * e.dt;
    if (vol > d1) {
        const float K = d1 / vol;
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = f[k] * K;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) p.f[k][c] = f[k];
}

template <bool kLds>
__global__ __launch_bounds__(256) void erosion_water_kernel(ErosionPlanes p, int nx, int nz, int cur, ErosionStep e)
{
    __shared__ float tile[kLds ? 5 : 1][kLds ? kErosionTile : 1];
    ErosionColumn col;
    const bool live = col.find(nx, nz, p.mask);
    const float *__restrict__ b0 = p.b[0];
    if (kLds) {
#pragma unroll
        for (int k = 0; k < 4; ++k) erosion_stage(p.f[k], tile[k], nx, nz);
        erosion_stage(b0, tile[4], nx, nz);
        __syncthreads();
    }
    if (!live) return;
    const int c = col.c;
    const float *tb = tile[kLds ? 4 : 0];
    float f[4], in[4], bn[4];
    const float b = erosion_at<kLds>(b0, tb, c, col.tc);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = erosion_at<kLds>(p.f[k], tile[kLds ? k : 0], c, col.tc);
        in[k] = col.v[k] ? erosion_at<kLds>(p.f[k ^ 1], tile[kLds ? k ^ 1 : 0], col.n[k], col.tn[k]) : 0.0f;
        bn[k] = col.v[k] ? erosion_at<kLds>(b0, tb, col.n[k], col.tn[k]) : b;
    }
    const float out = sum4(f), inn = sum4(in);
    const float d1 = p.d[cur][c] + e.dt_rain;
    float d2 = d1 + e.dt * (inn - out);
    d2 = d2 > 0.0f ? d2 : 0.0f;
    const float wx = ((in[0] - f[0]) + (f[1] - in[1])) * 0.5f;
    const float wz = ((in[2] - f[2]) + (f[3] - in[3])) * 0.5f;
    const float db = (d1 + d2) * 0.5f;
    const bool deep = db > VTMC_EROSION_DEPTH_EPS;
    const float u = deep ? wx / db : 0.0f;
    const float w = deep ? wz / db : 0.0f;
    float sp = __builtin_sqrtf(u * u + w * w);
    sp = sp < e.inv_dt ? sp : e.inv_dt;
    const float gx = (bn[1] - bn[0]) * 0.5f;
    const float gz = (bn[3] - bn[2]) * 0.5f;
    const float g2 = gx * gx + gz * gz;
    float sa = __builtin_sqrtf(g2 / (1.0f + g2));
    sa = sa > VTMC_EROSION_SIN_MIN ? sa : VTMC_EROSION_SIN_MIN;
    const float C = e.kc * sa * sp;
    const float s = p.s[cur][c];
    float b1, s1;
    if (C > s) {
        float er = e.ks * (C - s);
        er = er < d2 ? er : d2;
        b1 = b - er;
        s1 = s + er;
    } else {
        const float q = e.kd * (s - C);
        b1 = b + q;
        s1 = s - q;
    }
    p.b[1][c] = b1;
    p.s[cur][c] = s1;
    p.d[cur ^ 1][c] = d2;
}

template <bool kLds>
__global__ __launch_bounds__(256) void erosion_transport_kernel(ErosionPlanes p, int nx, int nz, int cur, ErosionStep e)
{
    __shared__ float tile[kLds ? 7 : 1][kLds ? kErosionTile : 1];
    ErosionColumn col;
    const bool live = col.find(nx, nz, p.mask);
    const float *__restrict__ s = p.s[cur], *__restrict__ d = p.d[cur], *__restrict__ bb = p.b[1];
    if (kLds) {
#pragma unroll
        for (int k = 0; k < 4; ++k) erosion_stage(p.f[k], tile[k], nx, nz);
        erosion_stage(s, tile[4], nx, nz);
        erosion_stage(d, tile[5], nx, nz);
        erosion_stage(bb, tile[6], nx, nz);
        __syncthreads();
    }
    if (!live) return;
    const int c = col.c;
    const float *ts = tile[kLds ? 4 : 0], *td = tile[kLds ? 5 : 0], *tb = tile[kLds ? 6 : 0];
    const float s1 = erosion_at<kLds>(s, ts, c, col.tc);
    const float d1 = erosion_at<kLds>(d, td, c, col.tc) + e.dt_rain;
    const float b1 = erosion_at<kLds>(bb, tb, c, col.tc);
    float give[4], gin[4], t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fr = d1 > 0.0f ? (erosion_at<kLds>(p.f[k], tile[kLds ? k : 0], c, col.tc) * e.dt) / d1 : 0.0f;
        give[k] = s1 * fr;
        gin[k] = 0.0f;
        t[k] = 0.0f;
        if (col.v[k]) {
            const int n = col.n[k], tn = col.tn[k];
            const float d1n = erosion_at<kLds>(d, td, n, tn) + e.dt_rain;
            const float frn = d1n > 0.0f ? (erosion_at<kLds>(p.f[k ^ 1], tile[kLds ? k ^ 1 : 0], n, tn) * e.dt) / d1n : 0.0f;
            gin[k] = erosion_at<kLds>(s, ts, n, tn) * frn;
            const float bn = erosion_at<kLds>(bb, tb, n, tn);
            const float hi = b1 > bn ? b1 : bn, lo = b1 < bn ? b1 : bn;
            float m = e.kt * ((hi - lo) - e.talus);
            m = m > 0.0f ? m : 0.0f;
            const float sign = b1 > bn ? -1.0f : (b1 < bn ? 1.0f : 0.0f);
            t[k] = sign * m;
        }
    }
    p.s[cur ^ 1][c] = (s1 - sum4(give)) + sum4(gin);
    p.d[cur ^ 1][c] = p.d[cur ^ 1][c] * e.keep;
    p.b[0][c] = b1 + sum4(t);
}

__global__ __launch_bounds__(256) void erosion_finish_kernel(ErosionPlanes p, int nx, int nz, float lo, float hi)
{
    const int x = blockIdx.x * 64 + threadIdx.x, z = blockIdx.y * 4 + threadIdx.y;
    bool rewritten = false, clamped = false;
    if (x < nx && z < nz) {
        const int c = x + nx * z;
        if (p.mask[c]) {
            const float b = p.b[0][c];
            float h1 = b;
            if (h1 < lo) h1 = lo;
            else if (h1 > hi) h1 = hi;
            clamped = h1 != b;
            rewritten = h1 != p.before[c];
            p.b[0][c] = h1;
        }
    }
    count_lanes(rewritten, p.ctl + 1);
    count_lanes(clamped, p.ctl + 2);
}

// An active column with h1 != h0 is rewritten on min(h0, h1) - 1 <= y <= max(h0, h1) + 1 with the flatten brush's profile around h1; every
// other sample keeps its bits (it is not stored).  kJournal: every sample of the box also goes to the box's image.
template <bool kJournal>
__global__ __launch_bounds__(256) void erosion_writeback_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainBox m,
                                                                const float *__restrict__ before, const float *__restrict__ after,
                                                                const uint8_t *__restrict__ mask)
{
    const BoxThread t;
    if (!t.inside(m)) return;
    const int c = t.ix + m.dx * t.iz;
    const float h0 = before[c], h1 = after[c];
    const bool rewrite = mask[c] && h1 != h0;
    if (!kJournal && !rewrite) return;
    const float lo = (h0 < h1 ? h0 : h1) - 1.0f, hi = (h0 > h1 ? h0 : h1) + 1.0f;
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    const uint64_t row = box_index(m, t.ix, 0, t.iz);
    for (int iy = t.iy0, iy1 = t.iy1(m); iy < iy1; ++iy) {
        const int y = m.ly + iy;
        const float fy = (float)y;
        const bool band = rewrite && lo <= fy && fy <= hi;
        if (!kJournal && !band) continue;
        const uint64_t sample = grid_index(sh, x, y, z);
        if (kJournal) image[row + (uint64_t)m.dx * (uint64_t)iy] = grid[sample];
        if (band) {
            float v = h1 - fy;
            v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
            grid[sample] = v;
        }
    }
}

__global__ void erosion_empty_kernel() {}

// The three launches of one step.  variant 0: neighbour loads from memory, through the caches; 1: the planes a kernel reads at a neighbour
// staged in LDS; 2: three empty launches of the same shape (what the launches alone cost: vtmc_debug_erosion_step_ms).
static hipError_t erosion_launch_step(int variant, const ErosionPlanes &p, int nx, int nz, int cur, const ErosionStep &e, hipStream_t st)
{
    const dim3 tiles((unsigned)((nx + 63) / 64), (unsigned)((nz + 3) / 4)), lanes(64, 4, 1);
    if (variant == 2) {
        for (int k = 0; k < 3; ++k)
            if (hipError_t rc = launch(erosion_empty_kernel, tiles, lanes, 0, st)) return rc;
        return hipSuccess;
    }
    if (hipError_t rc = launch(variant ? erosion_flux_kernel<true> : erosion_flux_kernel<false>, tiles, lanes, 0, st, p, nx, nz, cur, e)) return rc;
    if (hipError_t rc = launch(variant ? erosion_water_kernel<true> : erosion_water_kernel<false>, tiles, lanes, 0, st, p, nx, nz, cur, e)) return rc;
    return launch(variant ? erosion_transport_kernel<true> : erosion_transport_kernel<false>, tiles, lanes, 0, st, p, nx, nz, cur, e);
}

int check_erosion(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    const char *fault = erosion_args_fault(md);
    return fault ? fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: erosion %s", i, fault) : VTMC_OK;
}

int apply_erosion(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image)
{
    VtmcErosion &er = ctx->erosion;
    const TerrainBox box = box_of(a);
    const ErosionLayout l = erosion_layout(box.dx, box.dz);
    er.valid = er.has_state = false;
    if (er.state.bytes < l.bytes) {   // the previous erosion of this queue may still be running on the buffer
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (int rc = ensure(ctx, er.state, l.bytes)) return rc;
    }
    const ErosionPlanes p = erosion_planes(er.state.p, l);
    const ErosionStep e = erosion_step(md.p);
    const int32_t iterations = md.data_dims[0];
    const dim3 tiles((unsigned)((box.dx + 63) / 64), (unsigned)((box.dz + 3) / 4)), lanes(64, 4, 1);
    hipStream_t st = ctx->stream;
    if (!box_launchable(box)) return fail(ctx, VTMC_ERR_INVALID_ARG, "erosion box too large to launch");
    VTMC_HIP(ctx, ctx->erosion_clock.begin());
    VTMC_HIP(ctx, hipMemsetAsync(p.ctl, 0, 16, st));
    VTMC_HIP(ctx, ctx->erosion_clock.mark(0, st));
    VTMC_HIP(ctx, launch(erosion_heights_kernel, tiles, lanes, 0, st, (const float *)grid, ctx->tshape, box, p));
    VTMC_HIP(ctx, ctx->erosion_clock.mark(1, st));
    for (int32_t i = 0; i < iterations; ++i)
        VTMC_HIP(ctx, erosion_launch_step(er.lds ? 1 : 0, p, box.dx, box.dz, i & 1, e, st));
    VTMC_HIP(ctx, ctx->erosion_clock.mark(2, st));
    VTMC_HIP(ctx, launch(erosion_finish_kernel, tiles, lanes, 0, st, p, box.dx, box.dz, erosion_clamp_lo(box.ly), erosion_clamp_hi(box.ly + box.dy - 1)));
    VTMC_HIP(ctx, launch_box(image ? erosion_writeback_kernel<true> : erosion_writeback_kernel<false>, box, st, grid, image, ctx->tshape, box,
                             (const float *)p.before, (const float *)p.b[0], (const uint8_t *)p.mask));
    VTMC_HIP(ctx, ctx->erosion_clock.mark(3, st));
    ctx->erosion_clock.arm();
    vtmc_erosion_report &r = er.info;
    r.lo[0] = box.lx, r.lo[1] = box.ly, r.lo[2] = box.lz;
    r.hi[0] = box.lx + box.dx - 1, r.hi[1] = box.ly + box.dy - 1, r.hi[2] = box.lz + box.dz - 1;
    r.nx = box.dx, r.nz = box.dz, r.iterations = iterations;
    r.n_active = r.n_rewritten = r.n_clamped = 0;
    er.counts_pending = true;
    er.valid = er.has_state = true;
    return VTMC_OK;
}

// the five maps of the snapshot as they lie in the state buffer
struct ErosionMaps {
    const void *map[5];
    int64_t columns;
};
static ErosionMaps erosion_maps(const VtmcErosion &er)
{
    const ErosionLayout l = erosion_layout(er.info.nx, er.info.nz);
    const ErosionPlanes p = erosion_planes(er.state.p, l);
    const int par = erosion_final_parity(er.info.iterations);
    return ErosionMaps{{p.before, p.b[0], p.d[par], p.s[par], p.mask}, l.columns};
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_erosion_info(vtmc_ctx *ctx, vtmc_erosion_report *info)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!info) return fail(ctx, VTMC_ERR_INVALID_ARG, "info is null");
    VtmcErosion &er = ctx->erosion;
    if (!er.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "erosion_info before an erosion");
    if (er.counts_pending) {
        VTMC_HIP(ctx, hipSetDevice(ctx->device));
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        int32_t counts[3];
        const ErosionLayout l = erosion_layout(er.info.nx, er.info.nz);
        VTMC_HIP(ctx, hipMemcpy(counts, (const char *)er.state.p + l.ctl_off, sizeof counts, hipMemcpyDeviceToHost));
        er.info.n_active = counts[0], er.info.n_rewritten = counts[1], er.info.n_clamped = counts[2];
        er.counts_pending = false;
    }
    *info = er.info;
    return VTMC_OK;
}

int32_t vtmc_erosion_read(vtmc_ctx *ctx, int32_t map, void *dst, int64_t capacity_bytes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->erosion.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "erosion_read before an erosion");
    const ErosionMaps maps = erosion_maps(ctx->erosion);
    const int64_t bytes = erosion_map_bytes(map, maps.columns);
    if (bytes == 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "erosion_read: unknown map %d", map);
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    if (capacity_bytes < bytes) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %lld bytes of the map", (long long)capacity_bytes, (long long)bytes);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VTMC_HIP(ctx, hipMemcpy(dst, maps.map[map], (size_t)bytes, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_erosion_device_results(vtmc_ctx *ctx, const float **d_height_before, const float **d_height_after, const float **d_water,
                                    const float **d_sediment, const uint8_t **d_active)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->erosion.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "erosion_device_results before an erosion");
    const ErosionMaps maps = erosion_maps(ctx->erosion);
    if (d_height_before) *d_height_before = (const float *)maps.map[VTMC_EROSION_HEIGHT_BEFORE];
    if (d_height_after) *d_height_after = (const float *)maps.map[VTMC_EROSION_HEIGHT_AFTER];
    if (d_water) *d_water = (const float *)maps.map[VTMC_EROSION_WATER];
    if (d_sediment) *d_sediment = (const float *)maps.map[VTMC_EROSION_SEDIMENT];
    if (d_active) *d_active = (const uint8_t *)maps.map[VTMC_EROSION_ACTIVE];
    return VTMC_OK;
}

// Not in the header (diagnostics, tools/erosion_bench.py).
// The step's variant for later erosions: 0 neighbour loads through the caches (the library's choice), 1 staged in LDS.
int32_t vtmc_debug_erosion_lds(vtmc_ctx *ctx, int32_t on)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    ctx->erosion.lds = on != 0;
    return VTMC_OK;
}

// Device time of the last erosion: the height pass, all its steps, the finish and write-back.
int32_t vtmc_debug_erosion_ms(vtmc_ctx *ctx, float ms[3])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->erosion_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_erosion_ms before an erosion");
    if (int rc = ctx->erosion_clock.sync_last(ctx)) return rc;
    for (int k = 0; k < 3; ++k)
        if (int rc = ctx->erosion_clock.elapsed(ctx, k, k + 1, &ms[k])) return rc;
    return VTMC_OK;
}

// Device time of `steps` more steps on the state of the last erosion, with fixed parameters, in the given variant (erosion_launch_step:
// 0 direct, 1 LDS, 2 empty launches).  The maps do not describe the grid afterwards: the snapshot is dropped, the state stays.
int32_t vtmc_debug_erosion_step_ms(vtmc_ctx *ctx, int32_t variant, int32_t steps, float *ms)
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    VtmcErosion &er = ctx->erosion;
    if (variant < 0 || variant > 2 || steps < 1 || steps > VTMC_EROSION_MAX_ITERATIONS) return fail(ctx, VTMC_ERR_INVALID_ARG, "debug_erosion_step_ms: variant or steps out of range");
    if (!er.has_state) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_erosion_step_ms before an erosion");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    er.valid = false;
    const ErosionLayout l = erosion_layout(er.info.nx, er.info.nz);
    const ErosionPlanes p = erosion_planes(er.state.p, l);
    const float params[8] = {0.02f, 0.05f, 1.0f, 0.3f, 0.3f, 0.25f, 0.5f, 0.1f};
    const ErosionStep e = erosion_step(params);
    VTMC_HIP(ctx, ctx->erosion_clock.begin());
    VTMC_HIP(ctx, ctx->erosion_clock.mark(0, ctx->stream));
    for (int32_t i = 0; i < steps; ++i) VTMC_HIP(ctx, erosion_launch_step(variant, p, er.info.nx, er.info.nz, i & 1, e, ctx->stream));
    VTMC_HIP(ctx, ctx->erosion_clock.mark(3, ctx->stream));
    if (int rc = ctx->erosion_clock.sync_last(ctx)) return rc;
    return ctx->erosion_clock.elapsed(ctx, 0, 3, ms);
}

}  // extern "C"
