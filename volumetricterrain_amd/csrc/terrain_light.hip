// terrain_light.hip -- voxel lighting: floods the two channels "sky" and "torch" through the open samples of a box of the resident grid
// (vtmc_terrain_light and the readers of its result, include/vtmc_light.h).  Not in the reference.  The rule LIGHT is in the header;
// everything here is integers and 32-bit copies but the probe's nearest-sample formula.  Hand-written for gfx950 / CDNA4.  The host half
// -- argument checks, the seeds, the rule on a plain array -- is terrain_light.h.
//
// A sample is two bytes, sky low and torch high, and both channels move together through every kernel.  Everything is queued on the
// context's stream; the host reads back the changed words of a batch of rounds, nothing else.
//   1. light_seed_kernel     the ONE read of the grid.  A wave holds 64 columns along x of one z and walks them down from the top of the
//                            box: a sample's openness is one ballot, which is also the row's word of the OPEN MASK (a 64-bit word per
//                            row of up to 64 samples along x; the relaxation never reads the 4-byte grid again); each lane carries its
//                            column's "all open so far" bit, which is the skylit test, exact; the sample takes its sky emission.
//   2. light_torch_kernel    a lane per source: lit or dark by the mask, and the torch emission of the sample.  The host has put the
//                            largest level of a sample on the first source of that sample (terrain_light.h), so no two lanes write one
//                            sample and the scatter needs no atomic.
//   3. the relaxation, in rounds that ping-pong between two volumes: a round reads only what the round before wrote, so the result of
//      every round, and with it the round count, does not depend on scheduling.  Two variants (vtmc_debug_light_variant):
//        light_tile_kernel   a workgroup owns a tile of 64 x 8 x 8 samples (tile_label.h's shape).  It loads the tile with a halo of one
//                            sample (66 x 10 x 10 two-byte samples, 13.2 KB) and the tile's 64 mask words into LDS, sweeps both channels
//                            there in place until a workgroup-wide vote sees no change -- a sample is written by its own lane only, a
//                            neighbour read mid-sweep holds an older or a newer value of a sequence that only rises towards the one
//                            fixed point, so the sweep order cannot change where it ends --, and writes its samples back.  A tile runs in
//                            a round only when it or one of its six face neighbours changed in the round before (a byte per tile and
//                            round parity); a tile that did not run has equal contents in both volumes, so skipping it is exact.
//        light_plain_kernel  the plain one-hop Jacobi round, a lane per sample.
//      A round that changed a sample sets the round's word; the first round whose word stays 0 ends the loop and both volumes are equal.
//      The host queues `batch` rounds between two read-backs: rounds past the settled one are launches of workgroups that return at once.
//   4. light_count_kernel    the samples with sky > 0 and with torch > 0: ballots, a sum per workgroup in LDS, one atomic pair per
//                            workgroup.
// light_probe_kernel (a lane per position) and the two vertex kernels (a lane per vertex over tiles of records brought in by
// record_tile.h, as the material pass does) are gathers of 2-byte samples.
//
// EVERY LOOP IS BOUNDED: a tile's sweeps by kLightMaxSweeps (a tile cut short there has changed, so it runs again in the next round and
// nothing is lost), the rounds by VTMC_LIGHT_MAX_ROUNDS; beyond that the call answers VTMC_ERR_DEVICE ("light did not settle").
#include "terrain_edit.h"
#include "terrain_light.h"
#include "tile_label.h"
#include "material_filter.h"
#include <cstring>
#include <vector>

namespace vtmc {

typedef unsigned long long LightMask;

constexpr int kLightHaloX = kTileX + 2, kLightHaloY = kTileY + 2, kLightHaloZ = kTileZ + 2;
constexpr int kLightHaloSamples = kLightHaloX * kLightHaloY * kLightHaloZ;
constexpr int kLightMaxSweeps = 512;
// ctl: word r (1..VTMC_LIGHT_MAX_ROUNDS) is set when round r changed a sample; the two 64-bit counts lie behind them
constexpr int kLightCtlWords = VTMC_LIGHT_MAX_ROUNDS + 4, kLightCountWord = kLightCtlWords;   // 16-byte aligned: 260 words, then 4
constexpr size_t kLightCtlBytes = (kLightCtlWords + 4) * sizeof(int);
constexpr int kLightCountRun = 16;   // samples per lane of the count pass

__device__ __forceinline__ size_t light_index(const TerrainBox &b, int ix, int iy, int iz) { return (size_t)ix + (size_t)b.dx * ((size_t)iy + (size_t)b.dy * (size_t)iz); }
// the mask word of the row (iy, iz) of x segment xs; nxs: segments per row
__device__ __forceinline__ size_t light_mask_index(const TerrainBox &b, int nxs, int xs, int iy, int iz) { return (size_t)xs + (size_t)nxs * ((size_t)iy + (size_t)b.dy * (size_t)iz); }

// 64 x 4 threads: 64 columns along x of 4 z planes; grid = (x segments, z quads)
__global__ __launch_bounds__(256) void light_seed_kernel(const float *__restrict__ grid, uint16_t *__restrict__ volume, LightMask *__restrict__ mask, TerrainShape sh,
                                                         TerrainBox b, int sky_level)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iz = blockIdx.y * 4 + threadIdx.y;
    if (iz >= b.dz) return;   // the whole wave
    const bool column = ix < b.dx;
    const int nxs = gridDim.x;
    bool lit = true;
    for (int iy = b.dy - 1; iy >= 0; --iy) {
        bool open = false;
        if (column) open = !(grid[grid_index(sh, b.lx + ix, b.ly + iy, b.lz + iz)] > 0.0f);
        const LightMask row = __ballot(open);
        if (threadIdx.x == 0) mask[light_mask_index(b, nxs, blockIdx.x, iy, iz)] = row;
        lit = lit && open;
        if (column) volume[light_index(b, ix, iy, iz)] = (uint16_t)(lit ? sky_level : 0);
    }
}

__global__ __launch_bounds__(256) void light_torch_kernel(const LightSeed *__restrict__ seeds, int n, const LightMask *__restrict__ mask, uint16_t *__restrict__ volume,
                                                          uint8_t *__restrict__ lit_out, TerrainBox b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const LightSeed s = seeds[i];
    bool lit = false;
    if (s.box_index >= 0) {
        const int row = s.box_index / b.dx, ix = s.box_index - row * b.dx;   // row = iy + dy * iz
        lit = mask[(size_t)(ix >> 6) + (size_t)((b.dx + 63) / 64) * (size_t)row] >> (ix & 63) & 1ull;
        if (lit && s.emission > 0) reinterpret_cast<uint8_t *>(volume)[2 * (size_t)s.box_index + 1] = (uint8_t)s.emission;
    }
    lit_out[i] = lit ? 1 : 0;
}

// what a sample holds after one step: per channel its own value or what its brightest neighbour hands on
__device__ __forceinline__ uint32_t light_step(uint32_t own, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f, uint32_t sky_falloff,
                                               uint32_t torch_falloff)
{
    const uint32_t sky = max(max(max(a & 0xffu, b & 0xffu), max(c & 0xffu, d & 0xffu)), max(e & 0xffu, f & 0xffu));
    const uint32_t torch = max(max(max(a >> 8, b >> 8), max(c >> 8, d >> 8)), max(e >> 8, f >> 8));
    const uint32_t s = max(own & 0xffu, sky > sky_falloff ? sky - sky_falloff : 0u);
    const uint32_t t = max(own >> 8, torch > torch_falloff ? torch - torch_falloff : 0u);
    return s | t << 8;
}

// One round of the tiled variant.  64 x 4 threads; thread (tx, tq) owns the 16 samples (tx, r & 7, r >> 3), r = tq + 4 k, of the tile, as
// in tile_label.h.  flags: nt bytes of round parity 0, then nt of parity 1.
__global__ __launch_bounds__(256) void light_tile_kernel(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, const LightMask *__restrict__ mask,
                                                         uint8_t *__restrict__ flags, int *__restrict__ ctl, TerrainBox b, int round, uint32_t sky_falloff,
                                                         uint32_t torch_falloff)
{
    __shared__ uint16_t T[kLightHaloSamples];
    __shared__ LightMask M[kTileY * kTileZ];
    const int ntx = gridDim.x, nty = gridDim.y, ntz = gridDim.z;
    const size_t nt = (size_t)ntx * nty * ntz, tile = blockIdx.x + (size_t)ntx * (blockIdx.y + (size_t)nty * blockIdx.z);
    const uint8_t *before = flags + (size_t)((round - 1) & 1) * nt;
    uint8_t *now = flags + (size_t)(round & 1) * nt;
    const int tx = threadIdx.x, tq = threadIdx.y, tid = tx + 64 * tq;
    bool run = round == 1 || before[tile];
    if (!run) {
        run = (blockIdx.x > 0 && before[tile - 1]) || ((int)blockIdx.x + 1 < ntx && before[tile + 1]) || (blockIdx.y > 0 && before[tile - ntx]) ||
              ((int)blockIdx.y + 1 < nty && before[tile + ntx]) || (blockIdx.z > 0 && before[tile - (size_t)ntx * nty]) ||
              ((int)blockIdx.z + 1 < ntz && before[tile + (size_t)ntx * nty]);
    }
    if (!run) {   // the whole workgroup: nothing this tile reads has changed, and its samples are equal in both volumes
        if (tid == 0) now[tile] = 0;
        return;
    }
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY, z0 = blockIdx.z * kTileZ;
    for (int i = tid; i < kLightHaloSamples; i += 256) {
        const int hx = i % kLightHaloX, hy = i / kLightHaloX % kLightHaloY, hz = i / (kLightHaloX * kLightHaloY);
        const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
        uint16_t v = 0;   // outside the box: no light enters through its faces
        if (x >= 0 && x < b.dx && y >= 0 && y < b.dy && z >= 0 && z < b.dz) v = src[light_index(b, x, y, z)];
        T[i] = v;
    }
    if (tid < kTileY * kTileZ) {
        const int y = y0 + (tid & 7), z = z0 + (tid >> 3);
        M[tid] = y < b.dy && z < b.dz ? mask[light_mask_index(b, ntx, blockIdx.x, y, z)] : 0ull;   // a mask bit past dx is 0
    }
    __syncthreads();
    unsigned open = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) open |= (unsigned)(M[tq + 4 * k] >> tx & 1ull) << k;
    bool any = false;
    for (int sweep = 0; sweep < kLightMaxSweeps; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (!(open >> k & 1)) continue;
            const int r = tq + 4 * k;
            const int c = tx + 1 + kLightHaloX * ((r & 7) + 1 + kLightHaloY * ((r >> 3) + 1));
            const uint32_t own = T[c];
            const uint32_t v = light_step(own, T[c - 1], T[c + 1], T[c - kLightHaloX], T[c + kLightHaloX], T[c - kLightHaloX * kLightHaloY], T[c + kLightHaloX * kLightHaloY],
                                          sky_falloff, torch_falloff);
            if (v != own) {
                T[c] = (uint16_t)v;
                changed = true;
            }
        }
        if (!__syncthreads_or(changed)) break;   // the barrier between two sweeps, and the vote
        any = true;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3;
        if (x0 + tx < b.dx && y0 + ly < b.dy && z0 + lz < b.dz) dst[light_index(b, x0 + tx, y0 + ly, z0 + lz)] = T[tx + 1 + kLightHaloX * (ly + 1 + kLightHaloY * (lz + 1))];
    }
    if (tid == 0) {
        now[tile] = any ? 1 : 0;
        if (any) ctl[round] = 1;
    }
}

// One round of the plain variant, on the row walk: every sample of the box is written, so the two volumes need no bookkeeping.
__global__ __launch_bounds__(256) void light_plain_kernel(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, const LightMask *__restrict__ mask,
                                                          int *__restrict__ ctl, TerrainBox b, int round, uint32_t sky_falloff, uint32_t torch_falloff)
{
    const RowThread t;
    if (!t.inside(b)) return;
    const size_t i = light_index(b, t.ix, t.iy, t.iz), py = (size_t)b.dx, pz = (size_t)b.dx * b.dy;
    const uint32_t own = src[i];
    uint32_t v = own;
    if (mask[light_mask_index(b, gridDim.x, blockIdx.x, t.iy, t.iz)] >> threadIdx.x & 1ull) {
        const uint32_t xm = t.ix > 0 ? src[i - 1] : 0u, xp = t.ix + 1 < b.dx ? src[i + 1] : 0u;
        const uint32_t ym = t.iy > 0 ? src[i - py] : 0u, yp = t.iy + 1 < b.dy ? src[i + py] : 0u;
        const uint32_t zm = t.iz > 0 ? src[i - pz] : 0u, zp = t.iz + 1 < b.dz ? src[i + pz] : 0u;
        v = light_step(own, xm, xp, ym, yp, zm, zp, sky_falloff, torch_falloff);
    }
    dst[i] = (uint16_t)v;
    if (v != own) ctl[round] = 1;
}

// counts[0]: samples with sky > 0, counts[1]: with torch > 0.  A lane reads kLightCountRun samples 256 apart; a wave's ballots are summed
// in a register, the four waves' sums in LDS, and one lane adds the workgroup's two totals.
__global__ __launch_bounds__(256) void light_count_kernel(const uint16_t *__restrict__ volume, size_t n, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned sums[2];
    if (threadIdx.x < 2) sums[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * (256 * kLightCountRun) + threadIdx.x;
    unsigned sky = 0, torch = 0;
#pragma unroll 4
    for (int k = 0; k < kLightCountRun; ++k) {
        const size_t i = base + (size_t)k * 256;
        const uint32_t v = i < n ? volume[i] : 0u;
        sky += __popcll(__ballot((v & 0xffu) != 0u));
        torch += __popcll(__ballot((v >> 8) != 0u));
    }
    if ((threadIdx.x & 63) == 0) {
        if (sky) atomicAdd(&sums[0], sky);
        if (torch) atomicAdd(&sums[1], torch);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sums[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)sums[threadIdx.x]);
}

// One lane per position: the nearest sample by the source rule and its two bytes.
__global__ __launch_bounds__(256) void light_probe_kernel(const float *__restrict__ positions, int n, const uint16_t *__restrict__ volume, uint8_t *__restrict__ sky_out,
                                                          uint8_t *__restrict__ torch_out, TerrainShape sh, TerrainBox b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {positions[3 * (size_t)i], positions[3 * (size_t)i + 1], positions[3 * (size_t)i + 2]};
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
    const int ix = c[0] - b.lx, iy = c[1] - b.ly, iz = c[2] - b.lz;
    uint32_t v = 0u;
    if (in && ix >= 0 && ix < b.dx && iy >= 0 && iy < b.dy && iz >= 0 && iz < b.dz) v = volume[light_index(b, ix, iy, iz)];
    sky_out[i] = (uint8_t)(v & 0xffu);
    torch_out[i] = (uint8_t)(v >> 8);
}

struct LightVertexArgs {
    const uint16_t *volume;
    TerrainBox b;   // the light box
    int n[3];       // the grid's samples per axis
    BlockMap map;
};

// the rule's per-axis step of the occlusion's fetch: the cell origin of a grid coordinate
__device__ __forceinline__ int light_cell(float g, int n)
{
    const float top = (float)(n - 1);
    const float t = g < 0.0f ? 0.0f : (g > top ? top : g);
    if (t != t) return 0;   // a NaN coordinate (no result of the library holds one), as terrain_light.h has it
    int i0 = (int)floorf(t);
    if (i0 > n - 2) i0 = n - 2;
    return i0;
}

// the two bytes of a vertex at block-local position p of block blk (an index into the dirty list)
__device__ __forceinline__ uint16_t light_vertex_of(const LightVertexArgs &a, uint32_t blk, float p0, float p1, float p2)
{
    int bx, by, bz;
    material_block(a.map, blk, bx, by, bz);
    const int x0 = light_cell((float)(8 * bx) + p0, a.n[0]) - a.b.lx, y0 = light_cell((float)(8 * by) + p1, a.n[1]) - a.b.ly, z0 = light_cell((float)(8 * bz) + p2, a.n[2]) - a.b.lz;
    uint32_t sky = 0u, torch = 0u;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int x = x0 + (corner & 1), y = y0 + (corner >> 1 & 1), z = z0 + (corner >> 2);
        if (x < 0 || x >= a.b.dx || y < 0 || y >= a.b.dy || z < 0 || z >= a.b.dz) continue;
        const uint32_t v = a.volume[light_index(a.b, x, y, z)];
        sky = max(sky, v & 0xffu), torch = max(torch, v >> 8);
    }
    return (uint16_t)(sky | torch << 8);
}

// soup: one workgroup per tile of kMatTile triangles of 19 dwords, a lane per vertex; out[3t + v]
__global__ __launch_bounds__(256) void light_soup_kernel(const uint32_t *__restrict__ tris, uint32_t n_tris, uint16_t *__restrict__ out, LightVertexArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 19];
    const uint32_t t0 = blockIdx.x * (uint32_t)kMatTile;
    const uint32_t nt = n_tris - t0 < (uint32_t)kMatTile ? n_tris - t0 : (uint32_t)kMatTile;
    load_record_tile(rec, tris + (size_t)t0 * 19, nt * 19);   // tile base: 256 * 76 bytes per tile, 16-byte aligned
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < 3 * nt; v += 256) {
        const uint32_t t = v / 3, c = v - 3 * t;
        const uint32_t *r = rec + 19 * t;
        out[(size_t)t0 * 3 + v] = light_vertex_of(a, r[18], __uint_as_float(r[3 * c]), __uint_as_float(r[3 * c + 1]), __uint_as_float(r[3 * c + 2]));
    }
}

// indexed: one workgroup per tile of kMatTile vertices of 6 dwords; the block of a vertex from the per-block vertex offsets, as the
// material pass finds it
__global__ __launch_bounds__(256) void light_indexed_kernel(const uint32_t *__restrict__ verts, uint32_t n_verts, const uint32_t *__restrict__ voffsets,
                                                            uint16_t *__restrict__ out, LightVertexArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 6];
    __shared__ uint32_t range[2];
    const uint32_t v0 = blockIdx.x * (uint32_t)kMatTile;
    const uint32_t nv = n_verts - v0 < (uint32_t)kMatTile ? n_verts - v0 : (uint32_t)kMatTile;
    load_record_tile(rec, verts + (size_t)v0 * 6, nv * 6);   // tile base: 256 * 24 bytes per tile, 16-byte aligned
    if (threadIdx.x < 2) range[threadIdx.x] = material_block_of(voffsets, 0u, a.map.n_blocks - 1, threadIdx.x ? v0 + nv - 1 : v0);
    __syncthreads();
    if (threadIdx.x < nv) {
        const uint32_t v = v0 + threadIdx.x;
        const uint32_t blk = material_block_of(voffsets, range[0], range[1], v);
        const uint32_t *r = rec + 6 * threadIdx.x;
        out[v] = light_vertex_of(a, blk, __uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]));
    }
}

static TerrainBox light_box(const VtmcLight &r) { return TerrainBox{r.lo[0], r.lo[1], r.lo[2], r.d[0], r.d[1], r.d[2]}; }

static int light_gate(const vtmc_ctx *ctx, const char *who)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->light.valid) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_NO_RESULT, "%s before terrain_light", who);
    return VTMC_OK;
}

static bool light_vertices_current(const vtmc_ctx *ctx) { return ctx->light.valid && ctx->light.vertices_serial == ctx->light.serial; }

// The rounds of the relaxation on a seeded volume[0], queued on s in batches; *rounds: the round whose word stayed 0.
static int light_relax(vtmc_ctx *ctx, const TerrainBox &b, const vtmc_light_params &p, hipStream_t s, int *rounds)
{
    VtmcLight &r = ctx->light;
    uint16_t *vol[2] = {(uint16_t *)r.volume[0].p, (uint16_t *)r.volume[1].p};
    const LightMask *mask = (const LightMask *)r.mask.p;
    int *ctl = (int *)r.ctl.p;
    const int batch = std::max(1, std::min(r.batch, VTMC_LIGHT_MAX_ROUNDS));
    int h_ctl[kLightCtlWords];
    for (int first = 1; first <= VTMC_LIGHT_MAX_ROUNDS; first += batch) {
        const int last = std::min(first + batch - 1, VTMC_LIGHT_MAX_ROUNDS);
        for (int round = first; round <= last; ++round) {   // round 1 reads volume[0]; an odd round writes volume[1]
            const uint16_t *src = vol[(round - 1) & 1];
            uint16_t *dst = vol[round & 1];
            if (r.plain) VTMC_HIP(ctx, launch_rows(light_plain_kernel, b, s, src, dst, mask, ctl, b, round, (uint32_t)p.sky_falloff, (uint32_t)p.torch_falloff));
            else VTMC_HIP(ctx, launch(light_tile_kernel, tile_grid(b), dim3(64, 4, 1), 0, s, src, dst, mask, (uint8_t *)r.tiles.p, ctl, b, round, (uint32_t)p.sky_falloff,
                                      (uint32_t)p.torch_falloff));
        }
        VTMC_HIP(ctx, hipMemcpyAsync(h_ctl + first, ctl + first, sizeof(int) * (size_t)(last - first + 1), hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        for (int round = first; round <= last; ++round)
            if (!h_ctl[round]) {
                *rounds = round;
                return VTMC_OK;
            }
    }
    return fail(ctx, VTMC_ERR_DEVICE, "terrain_light: light did not settle in %d rounds", VTMC_LIGHT_MAX_ROUNDS);
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_light(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_light_params *params, const vtmc_light_source *sources,
                           int32_t n_sources, uint8_t *source_lit)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_light before terrain_init");
    if (const char *what = light_args_fault(lower, upper, params, sources, n_sources)) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_light: %s", what);
    const TerrainShape &sh = ctx->tshape;
    const TerrainBox b = bounds_box(sh, lower, upper);
    VtmcLight &r = ctx->light;
    if (box_empty(b)) {   // a success with dims (0, 0, 0): every source is dark
        for (int32_t i = 0; source_lit && i < n_sources; ++i) source_lit[i] = 0;
        r.valid = true, r.n_sky = r.n_torch = 0, r.rounds = 0, ++r.serial;
        for (int k = 0; k < 3; ++k) r.d[k] = 0;
        r.lo[0] = b.lx, r.lo[1] = b.ly, r.lo[2] = b.lz;
        return VTMC_OK;
    }
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t box_lo[3] = {b.lx, b.ly, b.lz}, box_d[3] = {b.dx, b.dy, b.dz};
    const size_t n = light_samples(box_d), nt = light_tiles(box_d);
    const std::vector<LightSeed> seeds = light_seeds(sources, n_sources, sh.origin, sh.scale, box_lo, box_d);
    // the buffers hold the previous result: grown and written only after the stream has drained, and from here on it is gone
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    r.valid = false;
    if (int rc = ensure(ctx, r.volume[0], 2 * n)) return rc;
    if (int rc = ensure(ctx, r.volume[1], 2 * n)) return rc;
    if (int rc = ensure(ctx, r.mask, sizeof(LightMask) * light_mask_words(box_d))) return rc;
    if (int rc = ensure(ctx, r.tiles, 2 * nt)) return rc;
    if (int rc = ensure(ctx, r.seeds, sizeof(LightSeed) * VTMC_LIGHT_MAX_SOURCES)) return rc;
    if (int rc = ensure(ctx, r.lit, VTMC_LIGHT_MAX_SOURCES)) return rc;
    if (int rc = ensure(ctx, r.ctl, kLightCtlBytes)) return rc;
    hipStream_t s = ctx->stream;
    uint16_t *volume = (uint16_t *)r.volume[0].p;
    LightMask *mask = (LightMask *)r.mask.p;
    int *ctl = (int *)r.ctl.p;
    VTMC_HIP(ctx, ctx->light_clock.begin());
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kLightCtlBytes, s));
    VTMC_HIP(ctx, ctx->light_clock.mark(0, s));
    VTMC_HIP(ctx, launch(light_seed_kernel, dim3((unsigned)((b.dx + 63) / 64), (unsigned)((b.dz + 3) / 4)), dim3(64, 4, 1), 0, s, (const float *)ctx->terrain.p, volume,
                         mask, sh, b, (int)params->sky_level));
    if (n_sources > 0) {
        VTMC_HIP(ctx, hipMemcpyAsync(r.seeds.p, seeds.data(), sizeof(LightSeed) * seeds.size(), hipMemcpyHostToDevice, s));
        VTMC_HIP(ctx, launch(light_torch_kernel, lanes256(n_sources), dim3(256), 0, s, (const LightSeed *)r.seeds.p, (int)n_sources, (const LightMask *)mask, volume,
                             (uint8_t *)r.lit.p, b));
    }
    VTMC_HIP(ctx, ctx->light_clock.mark(1, s));
    int rounds = 0;
    if (int rc = light_relax(ctx, b, *params, s, &rounds)) return rc;
    VTMC_HIP(ctx, ctx->light_clock.mark(2, s));
    unsigned long long *counts = (unsigned long long *)(ctl + kLightCountWord);
    VTMC_HIP(ctx, launch(light_count_kernel, dim3((unsigned)((n + 256 * kLightCountRun - 1) / (256 * kLightCountRun))), dim3(256), 0, s, (const uint16_t *)volume, n, counts));
    VTMC_HIP(ctx, ctx->light_clock.mark(3, s));
    unsigned long long h_counts[2];
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    VTMC_HIP(ctx, hipMemcpy(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost));
    if (source_lit && n_sources) VTMC_HIP(ctx, hipMemcpy(source_lit, r.lit.p, (size_t)n_sources, hipMemcpyDeviceToHost));
    r.n_sky = (int64_t)h_counts[0], r.n_torch = (int64_t)h_counts[1], r.rounds = rounds;
    for (int k = 0; k < 3; ++k) r.lo[k] = box_lo[k], r.d[k] = box_d[k];
    ctx->light_clock.arm();
    ++r.serial;
    r.valid = true;
    return VTMC_OK;
}

int32_t vtmc_light_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int64_t *n_sky, int64_t *n_torch, int32_t *rounds)
{
    if (int rc = light_gate(ctx, "light_info")) return rc;
    const VtmcLight &r = ctx->light;
    for (int k = 0; k < 3; ++k) {
        if (box_lo) box_lo[k] = r.lo[k];
        if (box_dims) box_dims[k] = r.d[k];
    }
    if (n_sky) *n_sky = r.n_sky;
    if (n_torch) *n_torch = r.n_torch;
    if (rounds) *rounds = r.rounds;
    return VTMC_OK;
}

int32_t vtmc_light_read(vtmc_ctx *ctx, vtmc_light_sample *dst, int64_t capacity_samples)
{
    if (int rc = light_gate(ctx, "light_read")) return rc;
    const VtmcLight &r = ctx->light;
    const size_t n = light_samples(r.d);
    if (capacity_samples < 0 || (uint64_t)capacity_samples < n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %zu samples", (long long)capacity_samples, n);
    if (n == 0) return VTMC_OK;
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "light_read: dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipMemcpy(dst, r.volume[0].p, 2 * n, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_light_device_results(vtmc_ctx *ctx, const vtmc_light_sample **d_volume, int32_t box_dims[3])
{
    if (int rc = light_gate(ctx, "light_device_results")) return rc;
    const VtmcLight &r = ctx->light;
    if (d_volume) *d_volume = light_samples(r.d) ? (const vtmc_light_sample *)r.volume[0].p : nullptr;
    for (int k = 0; box_dims && k < 3; ++k) box_dims[k] = r.d[k];
    return VTMC_OK;
}

int32_t vtmc_light_probe(vtmc_ctx *ctx, const float *positions, int32_t n, uint8_t *sky_out, uint8_t *torch_out)
{
    if (int rc = light_gate(ctx, "light_probe")) return rc;
    if (n < 0 || (n > 0 && !positions)) return fail(ctx, VTMC_ERR_INVALID_ARG, "light_probe: positions is null or n < 0");
    if (n == 0) return VTMC_OK;
    VtmcLight &r = ctx->light;
    if (light_samples(r.d) == 0) {   // an empty box: nothing is lit
        if (sky_out) memset(sky_out, 0, (size_t)n);
        if (torch_out) memset(torch_out, 0, (size_t)n);
        return VTMC_OK;
    }
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = 12 * (size_t)n, out_bytes = ((size_t)n + 15) & ~(size_t)15;
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier probe may still be reading the stage
    if (int rc = ensure(ctx, r.probe, in_bytes + 2 * out_bytes)) return rc;
    float *d_pos = (float *)r.probe.p;
    uint8_t *d_sky = (uint8_t *)r.probe.p + in_bytes, *d_torch = d_sky + out_bytes;
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipMemcpyAsync(d_pos, positions, in_bytes, hipMemcpyHostToDevice, s));
    VTMC_HIP(ctx, launch(light_probe_kernel, lanes256(n), dim3(256), 0, s, (const float *)d_pos, (int)n, (const uint16_t *)r.volume[0].p, d_sky, d_torch, ctx->tshape,
                         light_box(r)));
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    if (sky_out) VTMC_HIP(ctx, hipMemcpy(sky_out, d_sky, (size_t)n, hipMemcpyDeviceToHost));
    if (torch_out) VTMC_HIP(ctx, hipMemcpy(torch_out, d_torch, (size_t)n, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_light_vertices(vtmc_ctx *ctx, int64_t *n_vertices)
{
    if (int rc = light_gate(ctx, "light_vertices")) return rc;
    if (int rc = attr_gate(ctx, "light_vertices")) return rc;
    VtmcLight &r = ctx->light;
    const VtmcResult &res = ctx->result;
    const int64_t n = res.vertices();
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        if (int rc = ensure(ctx, r.vertices.values, 2 * (size_t)n)) return rc;
        uint16_t *out = (uint16_t *)r.vertices.values.p;
        if (light_samples(r.d) == 0) {   // an empty box: no corner of any cell lies in it
            VTMC_HIP(ctx, hipMemsetAsync(out, 0, 2 * (size_t)n, ctx->stream));
        } else {
            LightVertexArgs a{};
            a.volume = (const uint16_t *)r.volume[0].p;
            a.b = light_box(r);
            a.n[0] = ctx->tshape.dim_x, a.n[1] = ctx->tshape.dim_y, a.n[2] = ctx->tshape.dim_z;
            a.map = block_map(res.space, res.blocks);
            if (res.indexed) {
                const uint32_t V = (uint32_t)res.verts;
                VTMC_HIP(ctx, launch(light_indexed_kernel, dim3((V + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->verts.p, V,
                                     (const uint32_t *)ctx->voffsets.p, out, a));
            } else {
                const uint32_t T = (uint32_t)res.tris;
                VTMC_HIP(ctx, launch(light_soup_kernel, dim3((T + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->tris.p, T, out, a));
            }
        }
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    r.vertices.n = n;
    r.vertices.epoch = res.epoch;
    r.vertices_serial = r.serial;
    if (n_vertices) *n_vertices = n;
    return VTMC_OK;
}

static const char kLightStale[] = "no vertex light of the current result and the current light (call vtmc_light_vertices)";

int32_t vtmc_light_read_vertices(vtmc_ctx *ctx, vtmc_light_sample *dst, int64_t capacity_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!light_vertices_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "light_read_vertices: %s", kLightStale);
    return attr_read(ctx, ctx->light.vertices, kLightStale, 2, (uint8_t *)dst, capacity_vertices);
}

int32_t vtmc_light_vertices_device_results(vtmc_ctx *ctx, const vtmc_light_sample **d_values, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!light_vertices_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "light_vertices_device_results: %s", kLightStale);
    return attr_device_results(ctx, ctx->light.vertices, kLightStale, (const uint8_t **)d_values, n_vertices);
}

// Not part of the ABI (tests, tools/light_bench.py).  plain: the relaxation of later light calls, 0 the tiled rounds, 1 the plain one-hop
// rounds, -1 leaves it; batch: the rounds queued between two read-backs, 1..VTMC_LIGHT_MAX_ROUNDS, anything else leaves it.
int32_t vtmc_debug_light_variant(vtmc_ctx *ctx, int32_t plain, int32_t batch)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (plain == 0 || plain == 1) ctx->light.plain = plain == 1;
    if (batch >= 1 && batch <= VTMC_LIGHT_MAX_ROUNDS) ctx->light.batch = batch;
    return VTMC_OK;
}

// device time of the last light call's three phases: the seeds, the relaxation (with its read-backs), the count (not in the header)
int32_t vtmc_debug_light_ms(vtmc_ctx *ctx, float ms[3])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->light_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "no light call has run its kernels");
    if (int rc = ctx->light_clock.sync_last(ctx)) return rc;
    for (int i = 0; i < 3; ++i)
        if (int rc = ctx->light_clock.elapsed(ctx, i, i + 1, ms + i)) return rc;
    return VTMC_OK;
}

}  // extern "C"
