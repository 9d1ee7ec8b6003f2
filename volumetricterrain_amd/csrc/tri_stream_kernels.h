// tri_stream_kernels.h -- the stream over the triangles of the result the context holds, which the passes that emit records per triangle share
// (terrain_scatter.hip: instances, a mask bit per surviving candidate; terrain_lodskirt.hip: skirt records, a mask bit per face, two records a
// bit).  Tiles of kTriTile = 256 triangles (tri_stream.h), one lane per triangle, and no atomic decides where a record goes: the order is a
// function of the result alone.
//   1. the pass's count kernel writes one MASK byte per triangle and the tile's record total.
//   2. the two-level scan of the tile totals (scan_kernels.h over a ScanLayout); the grand total goes to the host, which checks it against
//      the pass's limit and grows the record buffer (tri_scan_total).
//   3. the pass's emit kernel, the same tiling: a workgroup scan of the masks' popcounts gives every lane its slot; a tile without a set bit
//      reads no record; only triangles with a set bit are loaded, only set bits are recomputed.  A lane's records are consecutive slots
//      and consecutive lanes continue each other, so a tile's records are one contiguous run of the output.
//   4. tri_block_offsets_kernel, a thread per block of the result: the tile offset of the block's first triangle plus the popcounts of
//      the mask bytes of the tile before it, read as dwords, times the records a set bit stands for.
// The count and the emit kernels are the passes' own and call the pieces here (view, tile bounds, bracket, soup stage, loader) in their
// order.  Soup records come into LDS as consecutive 16-byte pieces (record_tile.h), never at a 76-byte lane stride; a lane then reads its
// record at a stride of 19 dwords, which is odd, so the LDS banks do not collide.  In indexed mode a lane finds its block in the triangle
// offsets (two lanes bracket the tile's blocks first), reads its index triple and gathers its three vtmc_vertex through the block's
// vertex offset; the vertices of a block are shared by about six triangles and come from L2.
// Traffic that must reach HBM, soup: 76 T' (count: the tiles it reads; the scatter all of them, the skirts those near a flagged node) +
// T (masks out) + T (masks in) + 76 T'' (emit: the tiles with a set bit) + the N records emitted (32 N instances, 76 N skirt records).
//
// Bounds.  Both passes rest on this one argument.  It holds for T > 0 triangles, B > 0 blocks; the host launches nothing otherwise.
//   toffsets     B + 1 words (the result's per-block triangle offsets); material_block_of reads indices in [0, B - 1] (the bracket's two
//                lanes) or [range[0], range[1]], both of which came out of it; the offsets kernel's thread b <= B reads toffsets[b] and
//                writes block_offsets[b], B + 1 words too.
//   records      soup: the tile's nt * 19 dwords from t0 * 19, t0 + nt <= T, of a buffer of T records; LDS holds 256 * 19 dwords and a
//                lane reads record threadIdx.x < nt of it.  A soup record's `block` is the library's own and below B; the loader clamps it
//                to B - 1, which keeps a foreign record inside whatever a pass indexes with it.
//   indexed      a triangle's three indices at 3 t + c, t < T, of 3 T words.  A vertex is read at voffsets[b] + index: the index is
//                block-local and below the block's vertex count by the emit kernel's construction, so the sum is below voffsets[b + 1] <=
//                V; the loader clamps the sum to V - 1 all the same (b <= B - 1 indexes the B + 1 vertex offsets), so no value of an index
//                reads outside the V vertices.  tri_view refuses an indexed result of T > 0 triangles with V = 0.
//   masks        whole tiles: tiles * 256 bytes; every lane of every workgroup writes (count) or reads (emit) its own byte; the offsets
//                kernel reads the dwords before byte r < 256 of tile t / 256 < tiles.
//   scan         ScanLayout(tiles): the count writes tile_totals[blockIdx.x], the emit and the offsets kernel read tile_offsets[tile] and
//                group_offsets[tile / 1024], tile < tiles.
//   out          `capacity` = the scan's grand total of records; an emit kernel stores a record only at a slot below it.  That holds for
//                the masks of this call (the slots are the scan of the same masks) and keeps every store inside the buffer whatever the
//                masks say.  (Device code and host glue are forced inline or static: a translation unit has its own offsets kernel.)
#ifndef VTMC_TRI_STREAM_KERNELS_H
#define VTMC_TRI_STREAM_KERNELS_H
#include "material_filter.h"
#include "record_tile.h"
#include "scan_kernels.h"
#include "tri_stream.h"
#include "vtmc_ctx.h"

namespace vtmc {

// the result as the stream reads it
struct TriView {
    const uint32_t *recs;      // soup: T records of 19 dwords (vtmc_triangle); indexed: V records of 6 dwords (vtmc_vertex)
    const int32_t *indices;    // indexed: 3 T block-local indices
    const uint32_t *toffsets;  // the n_blocks + 1 per-block triangle offsets
    const uint32_t *voffsets;  // indexed: the n_blocks + 1 per-block vertex offsets
    uint32_t n_tris, n_blocks, n_verts;
};

// a triangle as the stream hands it over: positions and record normals as their bits, and the block
struct TriWords {
    uint32_t p[3][3], n[3][3];
    uint32_t block;
};

// the tile of this workgroup: its first triangle and how many it holds (the last tile is ragged)
__device__ __forceinline__ void tri_tile_bounds(const TriView &v, uint32_t &t0, uint32_t &nt)
{
    t0 = blockIdx.x * (uint32_t)kTriTile;
    nt = v.n_tris - t0 < (uint32_t)kTriTile ? v.n_tris - t0 : (uint32_t)kTriTile;
}

// the blocks of the tile's first and last triangle into range[0..1], for the whole workgroup
__device__ __forceinline__ void tri_tile_bracket(const TriView &v, uint32_t *range, uint32_t t0, uint32_t nt)
{
    if (threadIdx.x < 2) range[threadIdx.x] = material_block_of(v.toffsets, 0u, v.n_blocks - 1u, threadIdx.x ? t0 + nt - 1u : t0);
    __syncthreads();
}

// the tile's soup records into LDS, for the whole workgroup
__device__ __forceinline__ void tri_tile_stage(const TriView &v, uint32_t *rec, uint32_t t0, uint32_t nt)
{
    load_record_tile(rec, v.recs + (size_t)t0 * 19, nt * 19);   // tile base: 256 * 76 bytes per tile, 16-byte aligned
    __syncthreads();
}

// the block of triangle t of the tile, once it is bracketed (indexed) or staged (soup)
template <bool INDEXED>
__device__ __forceinline__ uint32_t tri_block_of(const TriView &v, const uint32_t *rec, const uint32_t *range, uint32_t t)
{
    if (INDEXED) return material_block_of(v.toffsets, range[0], range[1], t);
    return min(rec[19u * (t % (uint32_t)kTriTile) + 18u], v.n_blocks - 1u);
}

// Triangle t of that tile, which lies in block b = tri_block_of(t).  (Two steps, so that a pass can start what it reads per block
// before the gather, as the scatter does with its list entry: behind the gather that load delays the hashing, profiles/r28/tri_stream.)
template <bool INDEXED>
__device__ __forceinline__ void tri_load(const TriView &v, const uint32_t *rec, uint32_t t, uint32_t b, TriWords &tri)
{
    tri.block = b;
    if (INDEXED) {
        const uint32_t vb = v.voffsets[b];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // a vtmc_vertex is 24 bytes at a multiple of 24: three 8-byte loads
            const uint32_t i = min(vb + (uint32_t)v.indices[3 * (size_t)t + c], v.n_verts - 1u);
            const uint2 *r = reinterpret_cast<const uint2 *>(v.recs + 6 * (size_t)i);
            const uint2 r0 = r[0], r1 = r[1], r2 = r[2];
            tri.p[c][0] = r0.x, tri.p[c][1] = r0.y, tri.p[c][2] = r1.x;
            tri.n[c][0] = r1.y, tri.n[c][1] = r2.x, tri.n[c][2] = r2.y;
        }
    } else {
        const uint32_t *r = rec + 19u * (t % (uint32_t)kTriTile);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) tri.p[c][k] = r[3 * c + k], tri.n[c][k] = r[9 + 3 * c + k];
    }
}

// out[b], b = 0..n_blocks: the records of triangles before the block's first one, `weight` of them per set mask bit
static __global__ __launch_bounds__(256) void tri_block_offsets_kernel(const uint32_t *__restrict__ toffsets, uint32_t n_blocks, uint32_t n_tris,
                                                                       const uint32_t *__restrict__ mask_words, const uint32_t *__restrict__ tile_offsets,
                                                                       const uint32_t *__restrict__ group_offsets, const unsigned long long *__restrict__ total,
                                                                       uint32_t weight, int32_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > n_blocks) return;
    const uint32_t t = toffsets[b];
    if (t >= n_tris) {
        out[b] = (int32_t)*total;
        return;
    }
    const uint32_t tile = t / (uint32_t)kTriTile, r = t % (uint32_t)kTriTile;
    const uint32_t *w = mask_words + (size_t)tile * (kTriTile / 4);
    const uint32_t base = group_offsets[tile / (uint32_t)kScanThreads] + tile_offsets[tile];
    uint32_t sum = 0u;
    for (uint32_t j = 0; j < r / 4u; ++j) sum += (uint32_t)__popc(w[j]);
    if (r & 3u) sum += (uint32_t)__popc(w[r / 4u] & ((1u << (8u * (r & 3u))) - 1u));
    out[b] = (int32_t)(base + weight * sum);
}

// -- the host's side -----------------------------------------------------------------------------------------------------------------------

// the view of the context's current result, which holds triangles, for the pass `who`
static int tri_view(vtmc_ctx *ctx, const char *who, TriView *v)
{
    const VtmcResult &res = ctx->result;
    if (res.indexed && res.verts <= 0) return fail(ctx, VTMC_ERR_DEVICE, "%s: an indexed result of %lld triangles without vertices", who, (long long)res.tris);
    v->recs = (const uint32_t *)(res.indexed ? ctx->verts.p : ctx->tris.p);
    v->indices = (const int32_t *)ctx->indices.p;
    v->toffsets = (const uint32_t *)ctx->offsets.p;
    v->voffsets = (const uint32_t *)ctx->voffsets.p;
    v->n_tris = (uint32_t)res.tris, v->n_blocks = (uint32_t)res.blocks, v->n_verts = (uint32_t)res.verts;
    return VTMC_OK;
}

// grows the masks and the scan's buffer of a pass over n_tris > 0 triangles; *scan is then the layout inside that buffer
static int tri_stream_scratch(vtmc_ctx *ctx, VtmcTriStream &st, int64_t n_tris, ScanLayout *scan)
{
    const uint32_t tiles = tri_tiles(n_tris);
    if (int rc = ensure(ctx, st.masks, tri_mask_bytes(n_tris))) return rc;
    if (int rc = ensure(ctx, st.scan, ScanLayout(tiles).bytes())) return rc;
    *scan = ScanLayout(tiles, st.scan.p);
    return VTMC_OK;
}

// behind the count kernel: mark 1 of the pass's clock, the scan, mark 2, and the grand total, waited for
static int tri_scan_total(vtmc_ctx *ctx, const ScanLayout &scan, StageClock<6> &clock, unsigned long long *total)
{
    VTMC_HIP(ctx, clock.mark(1, ctx->stream));
    VTMC_HIP(ctx, launch_scan(scan, ctx->stream));
    VTMC_HIP(ctx, clock.mark(2, ctx->stream));
    VTMC_HIP(ctx, hipMemcpyAsync(total, scan.total(), sizeof(*total), hipMemcpyDeviceToHost, ctx->stream));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VTMC_OK;
}

// Behind the emit kernel: mark 4, the per-block offsets of the pass's records into st.block_offsets (v.n_blocks + 1 entries) from the masks
// and the scanned layout, mark 5, and the clock armed
static int tri_launch_offsets(vtmc_ctx *ctx, const TriView &v, const VtmcTriStream &st, const ScanLayout &scan, uint32_t weight, StageClock<6> &clock)
{
    VTMC_HIP(ctx, clock.mark(4, ctx->stream));
    VTMC_HIP(ctx, launch(tri_block_offsets_kernel, lanes256((int64_t)v.n_blocks + 1), dim3(256), 0, ctx->stream, v.toffsets, v.n_blocks, v.n_tris, (const uint32_t *)st.masks.p,
                         scan.tile_offsets(), scan.group_offsets(), scan.total(), weight, (int32_t *)st.block_offsets.p));
    VTMC_HIP(ctx, clock.mark(5, ctx->stream));
    clock.arm();
    return VTMC_OK;
}

// The records and, where asked for, the block offsets of a pass that holds the current result's (the caller has checked that) to the
// host.  A capacity below the count is answered with `short_code`; `what` names the records in that text.
static int tri_stream_read(vtmc_ctx *ctx, const VtmcTriStream &st, size_t record_bytes, const char *what, int short_code, void *dst, int64_t capacity,
                           int32_t *block_offsets)
{
    if (capacity < st.n) return fail(ctx, short_code, "capacity %lld < %lld %s", (long long)capacity, (long long)st.n, what);
    if (st.n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (st.n > 0) VTMC_HIP(ctx, hipMemcpy(dst, st.records.p, record_bytes * (size_t)st.n, hipMemcpyDeviceToHost));
    if (block_offsets) VTMC_HIP(ctx, hipMemcpy(block_offsets, st.block_offsets.p, sizeof(int32_t) * ((size_t)st.blocks + 1), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

// ... and as they lie in device memory
template <class Record>
void tri_stream_device_results(const VtmcTriStream &st, const Record **d_records, const int32_t **d_block_offsets, int64_t *n)
{
    if (d_records) *d_records = (const Record *)st.records.p;
    if (d_block_offsets) *d_block_offsets = (const int32_t *)st.block_offsets.p;
    if (n) *n = st.n;
}

// device time of the last run of the pass that launched kernels: ms[0..3] = the count kernel, the scan, the emit kernel, the block offsets
static int tri_stream_ms(vtmc_ctx *ctx, const StageClock<6> &clock, const char *unarmed, float ms[4])
{
    if (!clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "%s", unarmed);
    if (int rc = clock.sync_last(ctx)) return rc;
    static const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
    for (int i = 0; i < 4; ++i)
        if (int rc = clock.elapsed(ctx, pairs[i][0], pairs[i][1], &ms[i])) return rc;
    return VTMC_OK;
}

}  // namespace vtmc
#endif
