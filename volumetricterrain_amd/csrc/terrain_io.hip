// terrain_io.hip -- the resident terrain as a sparse brick file (vtmc_terrain_save / _load) and the inverse of vtmc_terrain_read_samples
// (vtmc_terrain_write_samples).  Hand-written gfx950 / CDNA4; layout = volumetricterrain_amd/terrainfile.py.  New in the build: the
// reference keeps its grid in memory only ("Checkpoint / resume: none").
//
// BRICKS.  The (W+2, E+2, H+2) sample grid is cut into disjoint 8x8x8-sample bricks, nb = W/8 + 1 per axis (the last one holds 2 sample
// planes), brick index bx + nbx*(by + nby*bz).  A brick is
//   1 VOID  every own sample s <= -1, and no sample of the up-to-27 bricks around it (clipped at the grid) has s > 0;
//   2 FULL  every own sample s >= 1, and every sample of those bricks has s > 0;
//   0 RAW   anything else (any brick holding a NaN: a NaN fails both own tests).
// RAW bricks are stored as 32-bit copies; a VOID / FULL brick is one byte, and load redraws it from the counter hash the edit kernels
// draw voidDensity / fullDensity from (terrain_hash.h) under ONE new event number e = saved events + 1:
//   VOID sample -> terrain_uniform(seed, e, grid index, 0) - 2,   FULL sample -> terrain_uniform(seed, e, grid index, 1) + 1.
//
// WHY THE RULE IS SAFE.  The extract path reads a sample only as a corner of an active cell (one whose 8 corners differ in `s > 0`) or as
// the forward neighbour of such a corner (the normal's forward difference, SampleNormal.compute:27-30).  An active cell has a corner with
// s > 0 and one without, and all its corners lie within 1 sample of each other, so a sample that is read lies within 2 samples (per axis)
// of a sample with s > 0 AND of one without.  Bricks are 8 samples wide, so both of these lie in the 27-brick neighbourhood of the read
// sample's brick: that brick is neither VOID (a neighbourhood sample has s > 0) nor FULL (one has not).  The neighbourhood test is a
// conservative whole-brick dilation of that distance.  A redrawn sample keeps its `s > 0` class ([-2,-1) or [1,2)), so no cell changes
// its case either: elided samples never reach a triangle, a ray hit or a sphere query.  What IS lossy by contract: the 23 random
// mantissa bits of saturated samples far from the surface (a later smooth brush that reaches them blends other random numbers).
//
// DEVICE SIDE.  brick_flags_kernel streams the grid once (the hot kernel: 4.3 GB at 1024^3) and leaves four predicates per brick;
// brick_kinds_kernel combines 27 flag bytes into the kind; the scan of classify_kernels.hip gives every RAW brick its slot;
// brick_pack_kernel / brick_unpack_kernel move slices of RAW bricks between the grid and a fixed, double-buffered, pinned stage, so only
// the kind table and the RAW bricks cross PCIe and the host never holds more than two slices.  Everything rides the context's ordinary
// stream ("Streams").
#include "vtmc_ctx.h"
#include "terrain_hash.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <sys/stat.h>
#include <vector>

using namespace vtmc;

namespace {

constexpr uint32_t kMagic = 0x544D5456u;   // "VTMT", little endian
constexpr uint32_t kVersion = 1;
constexpr int kBrickSamples = 512;
constexpr size_t kBrickBytes = 2048;
constexpr uint32_t kSliceBricks = 8192;    // one half of the stage: 16 MiB on the device and 16 MiB pinned
constexpr size_t kSliceBytes = kSliceBricks * kBrickBytes;
enum : uint8_t { kRaw = 0, kVoid = 1, kFull = 2 };
enum : uint32_t { kAllLe = 1, kAllGe = 2, kAnyPos = 4, kAllPos = 8 };   // a brick's flag byte: all s <= -1, all s >= 1, any s > 0, all s > 0

struct __attribute__((packed)) TerrainHeader {
    uint32_t magic, version, flags;
    int32_t cells[3];
    float scale, origin[3];
    uint64_t seed;
    uint32_t events, n_raw;
    uint8_t reserved[8];
};
static_assert(sizeof(TerrainHeader) == 64, "terrain header is 64 bytes (terrainfile.py HEADER)");

size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }
size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

struct BrickGrid {
    int dim_x, dim_y, dim_z;   // samples
    int nbx, nby, nbz;         // bricks
};
BrickGrid brick_grid(int w, int e, int h) { return BrickGrid{w + 2, e + 2, h + 2, w / 8 + 1, e / 8 + 1, h / 8 + 1}; }
size_t n_bricks_of(const BrickGrid &g) { return (size_t)g.nbx * g.nby * g.nbz; }

// ---- brick flags: the streaming pass ------------------------------------------------------------------------------------------------
// One wave per (128-sample x segment, by, bz): lane l reads the two samples x = 128*seg + 2l, +1 of each of the brick row's (up to) 64
// rows as one 8-byte load -- a row starts on an even sample (dim_x is even), so the load is aligned although rows are not 16-byte
// aligned -- and a wave-instruction reads 512 contiguous bytes covering 16 bricks.  A lane folds its rows into four predicates; four
// adjacent lanes hold one brick, so a wave64 ballot per predicate gives every brick its nibble.  Lanes past the row's end stay neutral
// (all-of true, any-of false).  Every sample is read exactly once; 16 loads per lane are issued before the first is consumed.
struct LanePredicates {
    bool all_le = true, all_ge = true, any_pos = false, all_pos = true;
    __device__ __forceinline__ void add(float s)
    {
        all_le &= s <= -1.0f;
        all_ge &= s >= 1.0f;
        any_pos |= s > 0.0f;
        all_pos &= s > 0.0f;
    }
};

__global__ __launch_bounds__(256) void brick_flags_kernel(const float *__restrict__ grid, BrickGrid g, int nseg, unsigned n_tasks,
                                                          uint8_t *__restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const unsigned task = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (task >= n_tasks) return;   // uniform over the wave
    const int seg = (int)(task % (unsigned)nseg);
    const unsigned r = task / (unsigned)nseg;
    const int by = (int)(r % (unsigned)g.nby), bz = (int)(r / (unsigned)g.nby);
    const int x0 = seg * 128 + 2 * lane;
    const bool live = x0 < g.dim_x;   // dim_x is even: x0 + 1 is inside with x0
    const int ny = g.dim_y - 8 * by < 8 ? g.dim_y - 8 * by : 8, nz = g.dim_z - 8 * bz < 8 ? g.dim_z - 8 * bz : 8;
    const size_t row = (size_t)g.dim_x, plane = row * (size_t)g.dim_y;
    const float *p = grid + (size_t)x0 + row * (size_t)(8 * by) + plane * (size_t)(8 * bz);
    LanePredicates q;
    if (live) {
        if (ny == 8 && nz == 8) {
#pragma unroll 1
            for (int z = 0; z < 8; z += 2) {
                float2 v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = *reinterpret_cast<const float2 *>(p + row * (size_t)(k & 7) + plane * (size_t)(z + (k >> 3)));
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    q.add(v[k].x);
                    q.add(v[k].y);
                }
            }
        } else {   // the last brick row along y or z: 2 rows or 2 planes
            for (int z = 0; z < nz; ++z)
                for (int y = 0; y < ny; ++y) {
                    const float2 v = *reinterpret_cast<const float2 *>(p + row * (size_t)y + plane * (size_t)z);
                    q.add(v.x);
                    q.add(v.y);
                }
        }
    }
    const unsigned long long m_le = __builtin_amdgcn_ballot_w64(q.all_le), m_ge = __builtin_amdgcn_ballot_w64(q.all_ge);
    const unsigned long long m_any = __builtin_amdgcn_ballot_w64(q.any_pos), m_pos = __builtin_amdgcn_ballot_w64(q.all_pos);
    const int bx = seg * 16 + (lane >> 2);
    if ((lane & 3) == 0 && bx < g.nbx) {
        const uint32_t f = (((m_le >> lane) & 15ull) == 15ull ? kAllLe : 0u) | (((m_ge >> lane) & 15ull) == 15ull ? kAllGe : 0u) |
                           (((m_any >> lane) & 15ull) != 0ull ? kAnyPos : 0u) | (((m_pos >> lane) & 15ull) == 15ull ? kAllPos : 0u);
        flags[(size_t)bx + (size_t)g.nbx * ((size_t)by + (size_t)g.nby * (size_t)bz)] = (uint8_t)f;
    }
}

// ---- brick kinds: one thread per brick, 27 flag bytes (L2-resident: the table is at most 2.1 MB) -> kind byte and RAW count word ------
__global__ __launch_bounds__(256) void brick_kinds_kernel(const uint8_t *__restrict__ flags, BrickGrid g, unsigned n, int exact,
                                                          uint8_t *__restrict__ kinds, uint32_t *__restrict__ counts)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n) return;
    uint32_t kind = kRaw;
    if (!exact) {
        const int bx = (int)(b % (unsigned)g.nbx), by = (int)(b / (unsigned)g.nbx % (unsigned)g.nby), bz = (int)(b / ((unsigned)g.nbx * (unsigned)g.nby));
        uint32_t any = 0u, all = ~0u;   // OR / AND of the neighbourhood's flag bytes
        for (int z = bz > 0 ? bz - 1 : 0; z <= (bz + 1 < g.nbz ? bz + 1 : bz); ++z)
            for (int y = by > 0 ? by - 1 : 0; y <= (by + 1 < g.nby ? by + 1 : by); ++y)
                for (int x = bx > 0 ? bx - 1 : 0; x <= (bx + 1 < g.nbx ? bx + 1 : bx); ++x) {
                    const uint32_t f = flags[(size_t)x + (size_t)g.nbx * ((size_t)y + (size_t)g.nby * (size_t)z)];
                    any |= f;
                    all &= f;
                }
        const uint32_t own = flags[b];
        if ((own & kAllLe) && !(any & kAnyPos)) kind = kVoid;
        else if ((own & kAllGe) && (all & kAllPos)) kind = kFull;
    }
    kinds[b] = (uint8_t)kind;
    counts[b] = kind == kRaw ? 1u : 0u;
}

// load: the RAW count words of a kind table that came from a file
__global__ __launch_bounds__(256) void brick_counts_kernel(const uint8_t *__restrict__ kinds, unsigned n, uint32_t *__restrict__ counts)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b < n) counts[b] = kinds[b] == kRaw ? 1u : 0u;
}

// raw_list[slot] = brick index, from the scan's exclusive offsets
__global__ __launch_bounds__(256) void brick_list_kernel(const uint8_t *__restrict__ kinds, const uint32_t *__restrict__ slots, unsigned n,
                                                         uint32_t *__restrict__ raw_list)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b < n && kinds[b] == kRaw) raw_list[slots[b]] = b;
}

// ---- pack / unpack: one workgroup per RAW brick of the slice, sample (i, j, k) at i + 8j + 64k, 32-bit copies ----------------------------
// where sample i of brick b lies in the grid; false: outside (the last brick of an axis holds 2 planes)
__device__ __forceinline__ bool brick_sample(const BrickGrid &g, uint32_t b, int i, size_t &at)
{
    const int bx = (int)(b % (unsigned)g.nbx), by = (int)(b / (unsigned)g.nbx % (unsigned)g.nby), bz = (int)(b / ((unsigned)g.nbx * (unsigned)g.nby));
    const int x = 8 * bx + (i & 7), y = 8 * by + ((i >> 3) & 7), z = 8 * bz + (i >> 6);
    at = (size_t)x + (size_t)g.dim_x * ((size_t)y + (size_t)g.dim_y * (size_t)z);
    return x < g.dim_x && y < g.dim_y && z < g.dim_z;
}

__global__ __launch_bounds__(256) void brick_pack_kernel(const uint32_t *__restrict__ grid, BrickGrid g, const uint32_t *__restrict__ raw_list,
                                                         uint32_t *__restrict__ stage)
{
    const uint32_t b = raw_list[blockIdx.x];
#pragma unroll
    for (int i = threadIdx.x; i < kBrickSamples; i += 256) {
        size_t at;
        const bool in = brick_sample(g, b, i, at);
        stage[(size_t)blockIdx.x * kBrickSamples + i] = in ? grid[at] : 0u;   // +0.0f outside the grid
    }
}

__global__ __launch_bounds__(256) void brick_unpack_kernel(uint32_t *__restrict__ grid, BrickGrid g, const uint32_t *__restrict__ raw_list,
                                                           const uint32_t *__restrict__ stage)
{
    const uint32_t b = raw_list[blockIdx.x];
#pragma unroll
    for (int i = threadIdx.x; i < kBrickSamples; i += 256) {
        size_t at;
        if (brick_sample(g, b, i, at)) grid[at] = stage[(size_t)blockIdx.x * kBrickSamples + i];
    }
}

// ---- redraw: every sample of a VOID / FULL brick from the hash; 64 x 4 threads over (x, z), 16 samples along y each, as terrain.hip's box walk
constexpr int kRedrawRun = 16;
__global__ __launch_bounds__(256) void brick_redraw_kernel(float *__restrict__ grid, BrickGrid g, const uint8_t *__restrict__ kinds, uint64_t seed,
                                                           uint32_t event)
{
    const int x = blockIdx.x * 64 + threadIdx.x, z = blockIdx.y * 4 + threadIdx.y, y0 = blockIdx.z * kRedrawRun;
    if (x >= g.dim_x || z >= g.dim_z) return;
    const int y1 = y0 + kRedrawRun < g.dim_y ? y0 + kRedrawRun : g.dim_y;
    for (int y = y0; y < y1; ++y) {
        const uint32_t kind = kinds[(size_t)(x >> 3) + (size_t)g.nbx * ((size_t)(y >> 3) + (size_t)g.nby * (size_t)(z >> 3))];
        if (kind == kRaw) continue;
        const uint64_t sample = (uint64_t)x + (uint64_t)g.dim_x * ((uint64_t)y + (uint64_t)g.dim_y * (uint64_t)z);
        grid[sample] = kind == kVoid ? terrain_uniform(seed, event, sample, 0u) - 2.0f : terrain_uniform(seed, event, sample, 1u) + 1.0f;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the brick scratch of a context, carved out of one grow-only buffer
struct BrickScratch {
    uint8_t *flags = nullptr, *kinds = nullptr;
    uint32_t *counts = nullptr, *slots = nullptr, *raw_list = nullptr, *totals = nullptr;
    unsigned long long *ctrl = nullptr;
    size_t ctrl_bytes = 0;
};

int brick_scratch(vtmc_ctx *ctx, size_t n, BrickScratch &s)
{
    const size_t table = pad256(pad16(n)), words = pad256(4 * (n + 1));
    s.ctrl_bytes = pad256(8 * scan_ctrl_words((int)n));
    if (int rc = ensure(ctx, ctx->tio_bricks, 2 * table + 3 * words + s.ctrl_bytes + 256)) return rc;
    char *p = (char *)ctx->tio_bricks.p;
    s.flags = (uint8_t *)p, p += table;
    s.kinds = (uint8_t *)p, p += table;
    s.counts = (uint32_t *)p, p += words;
    s.slots = (uint32_t *)p, p += words;
    s.raw_list = (uint32_t *)p, p += words;
    s.ctrl = (unsigned long long *)p, p += s.ctrl_bytes;
    s.totals = (uint32_t *)p;   // 64 words
    return VTMC_OK;
}

int stage_buffers(vtmc_ctx *ctx)
{
    if (int rc = ensure(ctx, ctx->tio_stage, 2 * kSliceBytes)) return rc;
    if (!ctx->h_tio.p) VTMC_HIP(ctx, pin(ctx->h_tio, 2 * kSliceBytes));
    return VTMC_OK;
}

// counts (one word per brick, 1 = RAW) -> slots (exclusive scan, slots[n] = n_raw) -> raw_list, queued on the context's stream
int queue_raw_list(vtmc_ctx *ctx, const BrickScratch &s, size_t n)
{
    hipStream_t st = ctx->stream;
    VTMC_HIP(ctx, hipMemsetAsync(s.ctrl, 0, s.ctrl_bytes + 256, st));   // the scan's ticket, error word and tile status; the totals behind them
    const BlockSpace none{};   // the scan reads it only for the active list, which is not asked for
    VTMC_HIP(ctx, launch_scan_fused(none, s.counts, (int)n, s.slots, nullptr, s.ctrl, s.totals, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, st));
    VTMC_HIP(ctx, launch(brick_list_kernel, lanes256((int64_t)n), dim3(256), 0, st, s.kinds, s.slots, (unsigned)n, s.raw_list));
    return VTMC_OK;
}

struct Events {   // the two "this half of the pinned stage is free / filled" events of a save or load
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t create()
    {
        for (hipEvent_t &e : ev)
            if (hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
        return hipSuccess;
    }
    ~Events()
    {
        for (hipEvent_t e : ev)
            if (e) quiet(hipEventDestroy(e));
    }
};
struct File {
    FILE *f = nullptr;
    ~File()
    {
        if (f) fclose(f);
    }
};

int save_file(vtmc_ctx *ctx, FILE *f, const char *path, uint32_t flags, int64_t *bytes_written)
{
    hipStream_t st = ctx->stream;
    const TerrainShape &sh = ctx->tshape;
    const BrickGrid g = brick_grid(sh.dim_x - 2, sh.dim_y - 2, sh.dim_z - 2);
    const size_t n = n_bricks_of(g);
    BrickScratch s;
    if (int rc = brick_scratch(ctx, n, s)) return rc;
    if (int rc = stage_buffers(ctx)) return rc;
    Events events;
    VTMC_HIP(ctx, events.create());
    const bool exact = (flags & VTMC_TERRAIN_SAVE_EXACT) != 0u;
    const int nseg = (g.dim_x + 127) / 128;
    const unsigned n_tasks = (unsigned)nseg * (unsigned)g.nby * (unsigned)g.nbz;
    VTMC_HIP(ctx, hipMemsetAsync(s.kinds, 0, pad16(n), st));   // the table's padding bytes are zero in the file
    if (!exact) VTMC_HIP(ctx, launch(brick_flags_kernel, dim3((n_tasks + 3) / 4), dim3(256), 0, st, (const float *)ctx->terrain.p, g, nseg, n_tasks, s.flags));
    VTMC_HIP(ctx, launch(brick_kinds_kernel, lanes256((int64_t)n), dim3(256), 0, st, s.flags, g, (unsigned)n, exact ? 1 : 0, s.kinds, s.counts));
    if (int rc = queue_raw_list(ctx, s, n)) return rc;
    std::vector<uint8_t> kinds;
    try {   // nothing is thrown through the C boundary
        kinds.resize(pad16(n));
    } catch (const std::exception &) {
        return fail(ctx, VTMC_ERR_DEVICE, "out of host memory for a kind table of %zu bytes", pad16(n));
    }
    uint32_t n_raw = 0, scan_failed = 0;
    VTMC_HIP(ctx, hipMemcpyAsync(kinds.data(), s.kinds, kinds.size(), hipMemcpyDeviceToHost, st));
    VTMC_HIP(ctx, hipMemcpyAsync(&n_raw, s.slots + n, sizeof n_raw, hipMemcpyDeviceToHost, st));
    VTMC_HIP(ctx, hipMemcpyAsync(&scan_failed, s.totals + 8, sizeof scan_failed, hipMemcpyDeviceToHost, st));
    VTMC_HIP(ctx, hipStreamSynchronize(st));
    if (scan_failed || n_raw > n) return fail(ctx, VTMC_ERR_DEVICE, "terrain_save: the brick scan did not complete");

    TerrainHeader h{};
    h.magic = kMagic;
    h.version = kVersion;
    h.flags = flags;
    h.cells[0] = sh.dim_x - 2, h.cells[1] = sh.dim_y - 2, h.cells[2] = sh.dim_z - 2;
    h.scale = sh.scale;
    memcpy(h.origin, sh.origin, sizeof h.origin);
    h.seed = sh.seed;
    h.events = ctx->terrain_events;
    h.n_raw = n_raw;
    bool wrote = fwrite(&h, 1, sizeof h, f) == sizeof h && fwrite(kinds.data(), 1, kinds.size(), f) == kinds.size();
    // slice i is packed and copied into half i & 1 of the stages while the host writes slice i - 1 out of the other half
    const uint32_t n_slices = (n_raw + kSliceBricks - 1) / kSliceBricks;
    auto slice_bricks = [&](uint32_t i) { return i + 1 < n_slices ? kSliceBricks : n_raw - i * kSliceBricks; };
    for (uint32_t i = 0; i <= n_slices && wrote; ++i) {
        if (i < n_slices) {
            const size_t half = (i & 1) * kSliceBytes, bytes = (size_t)slice_bricks(i) * kBrickBytes;
            uint32_t *d_stage = (uint32_t *)((char *)ctx->tio_stage.p + half);
            VTMC_HIP(ctx, launch(brick_pack_kernel, dim3(slice_bricks(i)), dim3(256), 0, st, (const uint32_t *)ctx->terrain.p, g, s.raw_list + (size_t)i * kSliceBricks,
                                 d_stage));
            VTMC_HIP(ctx, hipMemcpyAsync(ctx->h_tio.p + half, d_stage, bytes, hipMemcpyDeviceToHost, st));
            VTMC_HIP(ctx, hipEventRecord(events.ev[i & 1], st));
        }
        if (i > 0) {
            const size_t half = ((i - 1) & 1) * kSliceBytes, bytes = (size_t)slice_bricks(i - 1) * kBrickBytes;
            VTMC_HIP(ctx, hipEventSynchronize(events.ev[(i - 1) & 1]));
            wrote = fwrite(ctx->h_tio.p + half, 1, bytes, f) == bytes;
        }
    }
    VTMC_HIP(ctx, hipStreamSynchronize(st));   // also on a short write: nothing queued may outlive the call
    if (!wrote) return fail(ctx, VTMC_ERR_INVALID_ARG, "short write to %s: %s", path, strerror(errno));
    if (bytes_written) *bytes_written = (int64_t)(sizeof h + kinds.size() + kBrickBytes * (size_t)n_raw);
    return VTMC_OK;
}

// The file is untrusted input: everything is checked against the format's limits and the size of the file BEFORE anything is allocated,
// uploaded or launched.  Leaves the header and the kind table (padded) behind, the file positioned at the first RAW brick.
int read_checked(vtmc_ctx *ctx, FILE *f, const char *path, TerrainHeader &h, std::vector<uint8_t> &kinds)
{
    bool ok = fread(&h, 1, sizeof h, f) == sizeof h && h.magic == kMagic && h.version == kVersion;
    for (int k = 0; ok && k < 3; ++k) ok = h.cells[k] > 0 && h.cells[k] <= 1024 && h.cells[k] % 8 == 0;
    ok = ok && std::isfinite(h.scale) && h.scale > 0.0f;
    for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(h.origin[k]);
    size_t n = 0;
    if (ok) {
        n = n_bricks_of(brick_grid(h.cells[0], h.cells[1], h.cells[2]));
        struct stat sb;
        ok = (size_t)h.n_raw <= n && fstat(fileno(f), &sb) == 0 &&
             (unsigned long long)sb.st_size == (unsigned long long)(sizeof h + pad16(n)) + (unsigned long long)kBrickBytes * h.n_raw;
    }
    if (ok) {
        try {
            kinds.resize(pad16(n));
        } catch (const std::exception &) {
            return fail(ctx, VTMC_ERR_DEVICE, "out of host memory for a kind table of %zu bytes", pad16(n));
        }
        ok = fread(kinds.data(), 1, kinds.size(), f) == kinds.size();
        size_t n_raw = 0;
        for (size_t b = 0; ok && b < n; ++b) {
            ok = kinds[b] <= kFull;
            n_raw += kinds[b] == kRaw;
        }
        ok = ok && n_raw == (size_t)h.n_raw;
    }
    if (!ok)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "%s is not a complete version-1 terrain file (bad magic or version, dims, scale or origin beyond the format's "
                                               "limits, an unknown brick kind, or a size or RAW count that does not match its header)", path);
    return VTMC_OK;
}

int load_file(vtmc_ctx *ctx, FILE *f, const char *path, const TerrainHeader &h, const std::vector<uint8_t> &kinds)
{
    hipStream_t st = ctx->stream;
    const BrickGrid g = brick_grid(h.cells[0], h.cells[1], h.cells[2]);
    const size_t n = n_bricks_of(g), n_samples = (size_t)g.dim_x * g.dim_y * g.dim_z;
    const uint32_t event = h.events + 1u;
    if (int rc = ensure(ctx, ctx->terrain, sizeof(float) * n_samples)) return rc;
    BrickScratch s;
    if (int rc = brick_scratch(ctx, n, s)) return rc;
    if (int rc = stage_buffers(ctx)) return rc;
    Events events;
    VTMC_HIP(ctx, events.create());
    VTMC_HIP(ctx, hipMemcpyAsync(s.kinds, kinds.data(), kinds.size(), hipMemcpyHostToDevice, st));
    VTMC_HIP(ctx, launch(brick_counts_kernel, lanes256((int64_t)n), dim3(256), 0, st, s.kinds, (unsigned)n, s.counts));
    if (int rc = queue_raw_list(ctx, s, n)) return rc;
    VTMC_HIP(ctx, launch(brick_redraw_kernel, dim3((unsigned)((g.dim_x + 63) / 64), (unsigned)((g.dim_z + 3) / 4), (unsigned)((g.dim_y + kRedrawRun - 1) / kRedrawRun)),
                         dim3(64, 4, 1), 0, st, (float *)ctx->terrain.p, g, s.kinds, h.seed, event));
    // slice i is read from the file into half i & 1 of the pinned stage while slice i - 1 is copied and scattered out of the other half
    const uint32_t n_slices = (h.n_raw + kSliceBricks - 1) / kSliceBricks;
    bool got = true;
    for (uint32_t i = 0; i < n_slices && got; ++i) {
        const uint32_t nb = i + 1 < n_slices ? kSliceBricks : h.n_raw - i * kSliceBricks;
        const size_t half = (i & 1) * kSliceBytes, bytes = (size_t)nb * kBrickBytes;
        if (i >= 2) VTMC_HIP(ctx, hipEventSynchronize(events.ev[i & 1]));   // the copy of slice i - 2 has left this half
        got = fread(ctx->h_tio.p + half, 1, bytes, f) == bytes;
        if (!got) break;
        uint32_t *d_stage = (uint32_t *)((char *)ctx->tio_stage.p + half);
        VTMC_HIP(ctx, hipMemcpyAsync(d_stage, ctx->h_tio.p + half, bytes, hipMemcpyHostToDevice, st));
        VTMC_HIP(ctx, hipEventRecord(events.ev[i & 1], st));
        VTMC_HIP(ctx, launch(brick_unpack_kernel, dim3(nb), dim3(256), 0, st, (uint32_t *)ctx->terrain.p, g, s.raw_list + (size_t)i * kSliceBricks, d_stage));
    }
    VTMC_HIP(ctx, hipStreamSynchronize(st));
    uint32_t scan_failed = 0;
    VTMC_HIP(ctx, hipMemcpy(&scan_failed, s.totals + 8, sizeof scan_failed, hipMemcpyDeviceToHost));
    if (!got) return fail(ctx, VTMC_ERR_INVALID_ARG, "read of %s failed after its header was accepted: %s; the context holds no terrain now", path, strerror(errno));
    if (scan_failed) return fail(ctx, VTMC_ERR_DEVICE, "terrain_load: the brick scan did not complete; the context holds no terrain now");
    TerrainShape sh{};
    sh.dim_x = g.dim_x, sh.dim_y = g.dim_y, sh.dim_z = g.dim_z;
    sh.scale = h.scale;
    memcpy(sh.origin, h.origin, sizeof sh.origin);
    sh.seed = h.seed;
    ctx->tshape = sh;
    ctx->terrain_events = event;
    ctx->has_terrain = true;
    return VTMC_OK;
}

}  // namespace

extern "C" {

int32_t vtmc_terrain_save(vtmc_ctx *ctx, const char *path, uint32_t flags, int64_t *bytes_written)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!path) return fail(ctx, VTMC_ERR_INVALID_ARG, "path is null");
    if (flags & ~VTMC_TERRAIN_SAVE_EXACT) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown terrain_save flags 0x%x", flags);
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_save before terrain_init");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // as vtmc_terrain_read_samples
    File file;
    file.f = fopen(path, "wb");
    if (!file.f) return fail(ctx, VTMC_ERR_INVALID_ARG, "cannot open %s for writing: %s", path, strerror(errno));
    const int rc = save_file(ctx, file.f, path, flags, bytes_written);
    const int cl = fclose(file.f);
    file.f = nullptr;
    if (rc == VTMC_OK && cl != 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "short write to %s: %s", path, strerror(errno));
    return rc;
}

int32_t vtmc_terrain_load(vtmc_ctx *ctx, const char *path, uint32_t flags, int32_t *n_dirty_blocks, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!path) return fail(ctx, VTMC_ERR_INVALID_ARG, "path is null");
    if (flags & ~VTMC_TERRAIN_LOAD_NO_EXTRACT) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown terrain_load flags 0x%x", flags);
    File file;
    file.f = fopen(path, "rb");
    if (!file.f) return fail(ctx, VTMC_ERR_INVALID_ARG, "cannot open %s: %s", path, strerror(errno));
    TerrainHeader h{};
    std::vector<uint8_t> kinds;
    if (int rc = read_checked(ctx, file.f, path, h, kinds)) return rc;
    // accepted: from here on the resident terrain is replaced
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->has_terrain = false;
    ctx->result.valid = false;
    history_clear(ctx);
    material_drop(ctx);
    nav_drop(ctx);
    water_drop(ctx);
    erosion_drop(ctx);
    light_drop(ctx);
    ctx->dirty.clear();
    ctx->dirty_is_all = false;
    if (int rc = load_file(ctx, file.f, path, h, kinds)) return rc;
    if (n_dirty_blocks) *n_dirty_blocks = 0;
    if (tri_count) *tri_count = 0;
    if (flags & VTMC_TERRAIN_LOAD_NO_EXTRACT) return VTMC_OK;
    return terrain_extract_all(ctx, n_dirty_blocks, tri_count);
}

int32_t vtmc_terrain_write_samples(vtmc_ctx *ctx, const float *src, int64_t stride_x, int64_t stride_y, int64_t stride_z)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_write_samples before terrain_init");
    if (!src) return fail(ctx, VTMC_ERR_INVALID_ARG, "src is null");
    if (stride_x <= 0 || stride_y <= 0 || stride_z <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const TerrainShape &sh = ctx->tshape;
    const size_t n = (size_t)sh.dim_x * sh.dim_y * sh.dim_z;
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // nothing queued may still read the samples about to be replaced
    history_clear(ctx);   // no image of the journal describes this grid
    if (stride_x == 1 && stride_y == sh.dim_x && stride_z == (int64_t)sh.dim_x * sh.dim_y) {
        VTMC_HIP(ctx, hipMemcpy(ctx->terrain.p, src, n * sizeof(float), hipMemcpyHostToDevice));
        return VTMC_OK;
    }
    std::vector<uint32_t> tmp;   // 32-bit copies: NaN payloads and -0 survive
    try {
        tmp.resize(n);
    } catch (const std::exception &) {
        return fail(ctx, VTMC_ERR_DEVICE, "out of host memory for %zu samples", n);
    }
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
    size_t i = 0;
    for (int z = 0; z < sh.dim_z; ++z)
        for (int y = 0; y < sh.dim_y; ++y)
            for (int x = 0; x < sh.dim_x; ++x) tmp[i++] = s32[x * stride_x + y * stride_y + z * stride_z];
    VTMC_HIP(ctx, hipMemcpy(ctx->terrain.p, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return VTMC_OK;
}

}  // extern "C"
