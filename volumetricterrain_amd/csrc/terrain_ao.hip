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
// Records go through LDS in 16-byte pieces (record_tile.h), kAoChunk at a time; a block's first record is not 16-byte aligned in general,
// so the load starts at the aligned piece below it.  The bytes of a chunk are assembled in LDS at the byte phase they have in the output
// and leave as whole dwords; only the first and the last dword of a chunk, shared with the neighbouring blocks, leave byte by byte.
#include "terrain_ao.h"
#include "material_filter.h"
#include "record_tile.h"
#include "vtmc_ctx.h"
#include <cmath>
#include <type_traits>

namespace vtmc {

constexpr int kAoSoupChunk = 128;     // triangles (384 vertices) per pass of a workgroup: 9.7 KB of records, so tile + records stay under 53 KB and
                                      // three workgroups share a CU's 160 KB at the largest radius
constexpr int kAoIndexedChunk = 256;  // vertices per pass
constexpr int kAoDirectMax = 12;      // vertices up to which a block's workgroup reads global memory directly

struct AoArgs {
    const float *grid;  // the terrain's samples, x fastest
    int n[3];           // samples per axis
    const BlockDesc *active;
    BlockMap map;       // material_filter.h
    int reach, extent;  // R and 10 + 2R
    FastDiv d_extent;
    int steps;
    float strength;
    float hd[3][VTMC_AO_MAX_STEPS];  // terrain_ao.h
    float fall[VTMC_AO_MAX_STEPS];
    uint32_t direct_max;
    uint32_t *stats;  // [0] workgroups that staged a tile, [1] workgroups on the direct route
    uint8_t *out;
};

// where the workgroup's samples lie: the tile (origin o in grid samples, E per axis) and the grid
struct AoField {
    const float *tile;
    const float *__restrict__ grid;
    int o[3];
    int E;
    int n[3];
};

struct AoAxis {
    uint32_t off;  // the lower sample's offset along this axis, multiplied out
    float f;
};

// the rule's per-axis step of fetch(): the clamped coordinate cut into the sample below it and the weight
template <bool TILE>
__device__ __forceinline__ AoAxis ao_axis(const AoField &F, int k, float q)
{
    const int n = F.n[k];
    const float top = (float)(n - 1);
    const float t = q < 0.0f ? 0.0f : (q > top ? top : q);
    int i0 = (int)floorf(t);
    if (i0 > n - 2) i0 = n - 2;
    if (i0 < 0) i0 = 0;  // a NaN coordinate only (no result of the library holds one): stay inside the grid
    AoAxis a;
    a.f = t - (float)i0;
    if (TILE) a.off = (uint32_t)(i0 - F.o[k]) * (k == 0 ? 1u : (k == 1 ? (uint32_t)F.E : (uint32_t)(F.E * F.E)));
    else a.off = (uint32_t)i0 * (k == 0 ? 1u : (k == 1 ? (uint32_t)F.n[0] : (uint32_t)F.n[0] * (uint32_t)F.n[1]));
    return a;
}

template <bool TILE>
__device__ __forceinline__ float ao_fetch(const AoField &F, AoAxis X, AoAxis Y, AoAxis Z)
{
    const uint32_t sy = TILE ? (uint32_t)F.E : (uint32_t)F.n[0];
    const uint32_t sz = TILE ? (uint32_t)(F.E * F.E) : (uint32_t)F.n[0] * (uint32_t)F.n[1];
    const float *p = (TILE ? F.tile : F.grid) + (size_t)(X.off + Y.off + Z.off);
    const float v000 = p[0], v100 = p[1], v010 = p[sy], v110 = p[sy + 1];
    const float v001 = p[sz], v101 = p[sz + 1], v011 = p[sz + sy], v111 = p[sz + sy + 1];
    const float a00 = v000 + (v100 - v000) * X.f, a10 = v010 + (v110 - v010) * X.f;
    const float a01 = v001 + (v101 - v001) * X.f, a11 = v011 + (v111 - v011) * X.f;
    const float b0 = a00 + (a10 - a00) * Y.f, b1 = a01 + (a11 - a01) * Y.f;
    return b0 + (b1 - b0) * Z.f;
}

template <int M, class Fn>
__device__ __forceinline__ void ao_for_directions(Fn &&fn)
{
    if constexpr (M < 27) {
        if constexpr (M != 13) fn(std::integral_constant<int, M>{});
        ao_for_directions<M + 1>(fn);
    }
}

// The byte of a vertex at grid coordinates g with record normal nrm.  The directions are compile-time constants; a component of d that
// is zero contributes +-0 to a sum of the rule, which changes no value the rule goes on to use (c only where c > 0, q only through the
// clamp), so those terms are left out; (+-len) * h[s] is +-hd[s] exactly.
template <bool TILE>
__device__ __forceinline__ uint32_t ao_vertex(const AoArgs &a, const AoField &F, float gx, float gy, float gz, float n0, float n1, float n2)
{
    const float l = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    if (!(l > 0.0f) || !(l < INFINITY)) return 255u;
    const float N0 = n0 / l, N1 = n1 / l, N2 = n2 / l;
    // the axes a direction leaves alone fetch at the vertex's own coordinate
    const AoAxis X0 = ao_axis<TILE>(F, 0, gx), Y0 = ao_axis<TILE>(F, 1, gy), Z0 = ao_axis<TILE>(F, 2, gz);
    float num = 0.0f, den = 0.0f;
    const int S = a.steps;
    ao_for_directions<0>([&](auto code) {
        constexpr int M = decltype(code)::value;
        constexpr int I = M % 3 - 1, J = (M / 3) % 3 - 1, K = M / 9 - 1;
        constexpr int NZ = (I != 0) + (J != 0) + (K != 0);
        constexpr float LEN = NZ == 1 ? 1.0f : (NZ == 2 ? 0.70710678f : 0.57735027f);
        float c = 0.0f;
        if (I) c = N0 * ((float)I * LEN);
        if (J) c = I ? c + N1 * ((float)J * LEN) : N1 * ((float)J * LEN);
        if (K) c = (I || J) ? c + N2 * ((float)K * LEN) : N2 * ((float)K * LEN);
        if (c > 0.0f) {
            float o = 0.0f;
            for (int s = 0; s < S; ++s) {
                const float hd = a.hd[NZ - 1][s];
                const AoAxis X = I ? ao_axis<TILE>(F, 0, I > 0 ? gx + hd : gx - hd) : X0;
                const AoAxis Y = J ? ao_axis<TILE>(F, 1, J > 0 ? gy + hd : gy - hd) : Y0;
                const AoAxis Z = K ? ao_axis<TILE>(F, 2, K > 0 ? gz + hd : gz - hd) : Z0;
                float r = ao_fetch<TILE>(F, X, Y, Z);
                r = r > 0.0f ? (r < 1.0f ? r : 1.0f) : 0.0f;
                r = r * a.fall[s];
                if (r > o) o = r;
            }
            num = num + c * o;
            den = den + c;
        }
    });
    float v = 1.0f - a.strength * (num / den);
    v = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (uint32_t)rintf(v * 255.0f);
}

// One workgroup per non-empty block.  RD = dwords per record: 19 (soup, three vertices: corner c has its position at dwords 3c.. and its
// normal at 9 + 3c..) or 6 (indexed: position, normal).
template <bool INDEXED>
__global__ __launch_bounds__(256) void ao_kernel(const uint32_t *__restrict__ recs, AoArgs a)
{
    constexpr uint32_t RD = INDEXED ? 6u : 19u;
    constexpr uint32_t CHUNK = INDEXED ? (uint32_t)kAoIndexedChunk : (uint32_t)kAoSoupChunk;
    constexpr uint32_t CHUNK_VERTS = INDEXED ? CHUNK : 3u * CHUNK;
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ __attribute__((aligned(16))) uint32_t rec[CHUNK * RD + 4];
    __shared__ uint32_t outw[CHUNK_VERTS / 4 + 2];
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
    for (int k = 0; k < 3; ++k) F.n[k] = a.n[k], F.o[k] = 8 * b[k] - a.reach;
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
    const float bx = (float)(8 * b[0]), by = (float)(8 * b[1]), bz = (float)(8 * b[2]);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(outw);
    for (uint32_t r0 = 0; r0 < count; r0 += CHUNK) {
        const uint32_t nr = count - r0 < CHUNK ? count - r0 : CHUNK;
        const size_t d0 = ((size_t)first + r0) * RD;
        const uint32_t head = (uint32_t)(d0 & 3u);  // dwords between the 16-byte piece the chunk starts in and its first record
        if (r0) __syncthreads();                    // the pass before has read rec and outw
        load_record_tile(rec, recs + (d0 - head), nr * RD + head);
        __syncthreads();  // also behind the tile
        const uint32_t nv = nr * vpr;
        const size_t v0 = ((size_t)first + r0) * vpr;  // the chunk's first vertex = its first byte of the output
        const uint32_t phase = (uint32_t)(v0 & 3u);
        for (uint32_t v = threadIdx.x; v < nv; v += 256u) {
            const uint32_t *r;
            uint32_t c;
            if (INDEXED) {
                r = rec + head + 6u * v, c = 0u;
            } else {
                const uint32_t t = v / 3u;
                r = rec + head + 19u * t, c = v - 3u * t;
            }
            const float p0 = __uint_as_float(r[3 * c]), p1 = __uint_as_float(r[3 * c + 1]), p2 = __uint_as_float(r[3 * c + 2]);
            const uint32_t *nr3 = r + (INDEXED ? 3u : 9u + 3u * c);
            const float n0 = __uint_as_float(nr3[0]), n1 = __uint_as_float(nr3[1]), n2 = __uint_as_float(nr3[2]);
            const float gx = bx + p0, gy = by + p1, gz = bz + p2;
            // the tile holds every fetch of a vertex inside its block's cells, p in [0, 8]; any other record reads the grid itself
            const bool inside = p0 >= 0.0f && p0 <= 8.0f && p1 >= 0.0f && p1 <= 8.0f && p2 >= 0.0f && p2 <= 8.0f;
            uint32_t val;
            if (!direct && inside) val = ao_vertex<true>(a, F, gx, gy, gz, n0, n1, n2);
            else val = ao_vertex<false>(a, F, gx, gy, gz, n0, n1, n2);
            bytes[phase + v] = (uint8_t)val;
        }
        __syncthreads();
        // dword w of outw is dword w of the output counted from the aligned byte below v0
        uint8_t *dst = a.out + (v0 - phase);
        const uint32_t end = phase + nv;
        for (uint32_t w = threadIdx.x; 4u * w < end; w += 256u) {
            if (4u * w >= phase && 4u * w + 4u <= end) {
                reinterpret_cast<uint32_t *>(dst)[w] = outw[w];
            } else {
                const uint32_t lo = 4u * w < phase ? phase : 4u * w, hi = 4u * w + 4u < end ? 4u * w + 4u : end;
                for (uint32_t i = lo; i < hi; ++i) dst[i] = bytes[i];
            }
        }
    }
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
        a.steps = params->steps;
        a.strength = params->strength;
        for (int s = 0; s < VTMC_AO_MAX_STEPS; ++s) {
            a.fall[s] = tb.fall[s];
            for (int c = 0; c < 3; ++c) a.hd[c][s] = tb.hd[c][s];
        }
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
