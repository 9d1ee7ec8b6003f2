// terrain_lodskirt.hip -- skirt triangles over the seams of a level-of-detail extract (vtmc_lod_skirts, vtmc_lodskirt_*): for every
// triangle of the result with exactly two positions on a FLAGGED face of its node, a quad in the face's plane hung from that edge towards
// the solid side.  The rule, operation by operation, is LODSKIRT of include/vtmc_lodskirt.h; the kernels follow it bit for bit (library
// built with -ffp-contract=off; FP32 division and square root are the correctly rounded ones).  The host half -- argument checks, the face
// masks of the node list, the count bound, the sizes -- is terrain_lodskirt.h.  The pass reads the records of the result and never the grid.
//
// The pass is the scatter's scheme (terrain_scatter.hip): a stream over the records in tiles of kLodSkirtTile = 256 triangles, one lane
// per triangle, and no atomic decides where a record goes -- the order is a function of the result alone.
//   1. lodskirt_count_kernel  two lanes find the nodes of the tile's first and last triangle in the triangle offsets; the workgroup ORs the
//      mask bytes of the nodes between them and LEAVES when none is flagged (nodes are contiguous in the result, so away from the seams
//      whole runs of tiles leave here, before any record is read).  Otherwise every lane tests its triangle against the flagged faces of
//      its node and writes one FACE MASK byte (bit f: face f yields a quad) and the tile's record total, 2 per set bit.
//   2. the two-level scan of the tile totals (scan_kernels.h over a ScanLayout); the grand total goes to the host, for the 2^31 - 1 check
//      and the growth of the record buffer.
//   3. lodskirt_emit_kernel   the same tiling; a workgroup scan of 2 * popcount(mask) gives every lane its slot; a tile without a set bit
//      reads no record; only set bits are recomputed.  DIRECT: a lane writes its records dword by dword at its slot (its quads are
//      consecutive slots, consecutive lanes continue each other: the tile's records are one contiguous run of the output).  STAGED: the
//      records are put together in LDS, kLodSkirtStage at a time, shifted by the run's misalignment, and leave as 16-byte pieces.  The
//      library uses DIRECT: tools/lodskirt_bench.py measured its emit kernel no slower at split 1 and a fifth faster at split 2
//      (LODSEAMS.md, profiles/r27/lodskirt/); STAGED stays built for the tool, behind vtmc_debug_lodskirt_store.
//   4. lodskirt_offsets_kernel  a thread per node: the tile offset of the node's first triangle plus twice the popcounts of the mask bytes
//      of the tile before it, read as dwords.
// Soup records come into LDS as consecutive 16-byte pieces (record_tile.h); a lane then reads its record at a stride of 19 dwords, which is
// odd, so the LDS banks do not collide.  In indexed mode a lane finds its node in the triangle offsets, between the two the tile brackets,
// reads its index triple and gathers its three vtmc_vertex through the node's vertex offset.
// Traffic that must reach HBM, soup: 76 T' (count: the tiles near a flagged node) + T (masks out) + T (masks in) + 76 T'' (emit: the tiles
// with a quad) + 76 N.
//
// Bounds.  Every argument below holds for T > 0 triangles, B > 0 nodes; the host launches nothing otherwise.
//   toffsets     B + 1 words (the result's per-block triangle offsets); material_block_of reads indices in [0, B - 1] (the count's two
//                lanes) or [range[0], range[1]], both of which came out of it; the offsets kernel reads toffsets[b], b <= B.
//   node_masks   B bytes; read at b in [range[0], range[1]] <= B - 1, or at the lane's node, clamped to B - 1 (a soup record's `block`
//                is the library's own and below B; the clamp keeps a foreign record inside the array).
//   records      soup: the tile's nt * 19 dwords from t0 * 19, t0 + nt <= T, of a buffer of T records; LDS holds 256 * 19 dwords and a
//                lane reads record threadIdx.x < nt of it.
//   indexed      a triangle's three indices at 3 t + c, t < T, of 3 T words.  A vertex is read at voffsets[b] + index: the index is
//                block-local and below the block's vertex count by the emit kernel's construction, so the sum is below voffsets[b + 1] <=
//                V; the kernels clamp the sum to V - 1 all the same (b <= B - 1 indexes the B + 1 vertex offsets), so no value of an index
//                reads outside the V vertices.
//   masks        whole tiles: tiles * 256 bytes; every lane of every workgroup writes (count) or reads (emit) its own byte; the offsets
//                kernel reads the dwords before byte r < 256 of tile t / 256 < tiles.
//   scan         ScanLayout(tiles): the count writes tile_totals[blockIdx.x], the emit and the offsets kernel read tile_offsets[tile] and
//                group_offsets[tile / 1024], tile < tiles.
//   out          `capacity` = the scan's grand total of records; a quad is stored only when slot + 2 <= capacity.  That holds for the
//                masks of this call (the slots are the scan of the same masks) and keeps every store inside the buffer whatever the
//                masks say.  STAGED stores dwords [19 base, 19 (base + n)) of the run, base + n <= capacity checked the same way; its LDS
//                stage holds 3 + 19 kLodSkirtStage dwords and record j of a chunk lies at shift + 19 j, shift <= 3, j < kLodSkirtStage.
//   node_offsets B + 1 words, thread b <= B.
#include "terrain_lodskirt.h"
#include "material_filter.h"
#include "record_tile.h"
#include "scan_kernels.h"
#include "vtmc_ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace vtmc {

constexpr int kLodSkirtStage = 256;   // records the STAGED emit puts together in LDS at a time

struct SkirtArgs {
    const uint32_t *recs;        // soup: T records of 19 dwords (vtmc_triangle); indexed: V records of 6 dwords (vtmc_vertex)
    const int32_t *indices;      // indexed: 3 T block-local indices
    const uint32_t *toffsets;    // the n_nodes + 1 per-node triangle offsets
    const uint32_t *voffsets;    // indexed: the n_nodes + 1 per-node vertex offsets
    const uint8_t *node_masks;   // the n_nodes face masks
    uint32_t n_tris, n_nodes, n_verts;
    float depth;
};

// a triangle as the rule reads it: positions and record normals as their bits, and the node
struct SkirtTri {
    uint32_t p[3][3], n[3][3];
    uint32_t node;
};

template <bool INDEXED>
__device__ __forceinline__ void skirt_load(const SkirtArgs &a, const uint32_t *rec, const uint32_t *range, uint32_t t, SkirtTri &tri)
{
    if (INDEXED) {
        const uint32_t b = material_block_of(a.toffsets, range[0], range[1], t);
        tri.node = b;
        const uint32_t vb = a.voffsets[b];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // a vtmc_vertex is 24 bytes at a multiple of 24: three 8-byte loads
            const uint32_t v = min(vb + (uint32_t)a.indices[3 * (size_t)t + c], a.n_verts - 1u);
            const uint2 *r = reinterpret_cast<const uint2 *>(a.recs + 6 * (size_t)v);
            const uint2 r0 = r[0], r1 = r[1], r2 = r[2];
            tri.p[c][0] = r0.x, tri.p[c][1] = r0.y, tri.p[c][2] = r1.x;
            tri.n[c][0] = r1.y, tri.n[c][1] = r2.x, tri.n[c][2] = r2.y;
        }
    } else {
        const uint32_t *r = rec + 19u * (t % (uint32_t)kLodSkirtTile);
        tri.node = min(r[18], a.n_nodes - 1u);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) tri.p[c][k] = r[3 * c + k], tri.n[c][k] = r[9 + 3 * c + k];
    }
}

// the faces of the node's mask on which exactly two of the triangle's positions lie
__device__ __forceinline__ uint32_t skirt_faces(const SkirtTri &t, uint32_t node_mask)
{
    uint32_t m = 0u;
#pragma unroll
    for (int f = 0; f < kLodSkirtFaces; ++f) {
        const uint32_t want = (f & 1) ? 0x41000000u : 0u;   // 8.0f, 0.0f
        const int on = (t.p[0][f >> 1] == want) + (t.p[1][f >> 1] == want) + (t.p[2][f >> 1] == want);
        if (((node_mask >> f) & 1u) && on == 2) m |= 1u << f;
    }
    return m;
}

// Displacement of the rule: q = p' of the vertex (p, n) for a face of axis AXIS
template <int AXIS>
__device__ __forceinline__ void skirt_displace(const uint32_t p[3], const uint32_t n[3], float depth, uint32_t q[3])
{
    constexpr int U = AXIS == 0 ? 1 : 0, V = AXIS == 2 ? 1 : 2;
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
    const float du = -__uint_as_float(n[U]), dv = -__uint_as_float(n[V]);
    const float uu = du * du, vv = dv * dv;
    const float l2 = uu + vv;
    if (!(l2 > 0.0f) || l2 == INFINITY) return;
    const float l = sqrtf(l2);
    const float su = depth * du, sv = depth * dv;
    q[U] = __float_as_uint(__uint_as_float(p[U]) + su / l);
    q[V] = __float_as_uint(__uint_as_float(p[V]) + sv / l);
}

// one record (x, y, z) with their normals at dst[0..18]
__device__ __forceinline__ void skirt_record(uint32_t *dst, const uint32_t x[3], const uint32_t y[3], const uint32_t z[3], const uint32_t nx[3],
                                             const uint32_t ny[3], const uint32_t nz[3], uint32_t node)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dst[k] = x[k], dst[3 + k] = y[k], dst[6 + k] = z[k];
        dst[9 + k] = nx[k], dst[12 + k] = ny[k], dst[15 + k] = nz[k];
    }
    dst[18] = node;
}

// The quad of face F of the triangle: c is the position off the plane, a and b follow it in cyclic order.  WHICH: 0 the record (b, a, a'),
// 1 the record (b, a', b'), 2 both at dst and dst + 19.
template <int F>
__device__ __forceinline__ void skirt_quad(const SkirtTri &t, float depth, int which, uint32_t *dst)
{
    constexpr int AXIS = F >> 1;
    constexpr uint32_t want = (F & 1) ? 0x41000000u : 0u;
    // exactly one position c is off the plane; a = c + 1 and b = c + 2 are picked with masks, value by value, so the triangle stays in
    // registers (a select between array elements would become a select between their addresses)
    const uint32_t m0 = t.p[0][AXIS] != want ? ~0u : 0u, m1 = ~m0 & (t.p[1][AXIS] != want ? ~0u : 0u), m2 = ~(m0 | m1);
    uint32_t pa[3], na[3], pb[3], nb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pa[k] = (t.p[1][k] & m0) | (t.p[2][k] & m1) | (t.p[0][k] & m2), na[k] = (t.n[1][k] & m0) | (t.n[2][k] & m1) | (t.n[0][k] & m2);
        pb[k] = (t.p[2][k] & m0) | (t.p[0][k] & m1) | (t.p[1][k] & m2), nb[k] = (t.n[2][k] & m0) | (t.n[0][k] & m1) | (t.n[1][k] & m2);
    }
    uint32_t qa[3], qb[3];
    skirt_displace<AXIS>(pa, na, depth, qa);
    skirt_displace<AXIS>(pb, nb, depth, qb);
    if (which != 1) skirt_record(dst, pb, pa, qa, nb, na, na, t.node);
    if (which != 0) skirt_record(which == 2 ? dst + 19 : dst, pb, qa, qb, nb, na, nb, t.node);
}

// Face F of a lane's mask in the DIRECT emit: both records at the lane's slot, which moves on
template <int F>
__device__ __forceinline__ void skirt_store_direct(const SkirtTri &t, float depth, uint32_t mask, uint32_t &slot, uint32_t capacity, uint32_t *__restrict__ out)
{
    if (!(mask & (1u << F))) return;
    if (slot + 2u <= capacity && slot + 2u > slot) skirt_quad<F>(t, depth, 2, out + 19 * (size_t)slot);
    slot += 2u;
}

// Face F of a lane's mask in the STAGED emit: those of its two records j, j + 1 of the tile that fall into the chunk [c0, c0 + n)
template <int F>
__device__ __forceinline__ void skirt_store_staged(const SkirtTri &t, float depth, uint32_t mask, uint32_t &j, uint32_t c0, uint32_t n, uint32_t *stage)
{
    if (!(mask & (1u << F))) return;
    if (j >= c0 && j < c0 + n) skirt_quad<F>(t, depth, 0, stage + 19u * (j - c0));
    if (j + 1u >= c0 && j + 1u < c0 + n) skirt_quad<F>(t, depth, 1, stage + 19u * (j + 1u - c0));
    j += 2u;
}

// the nodes of the tile's first and last triangle, for the whole workgroup
__device__ __forceinline__ void skirt_bracket(const SkirtArgs &a, uint32_t *range, uint32_t t0, uint32_t nt)
{
    if (threadIdx.x < 2) range[threadIdx.x] = material_block_of(a.toffsets, 0u, a.n_nodes - 1u, threadIdx.x ? t0 + nt - 1u : t0);
    __syncthreads();
}

template <bool INDEXED>
__global__ __launch_bounds__(256) void lodskirt_count_kernel(SkirtArgs a, uint8_t *__restrict__ masks, uint32_t *__restrict__ tile_totals)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kLodSkirtTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    const uint32_t t0 = blockIdx.x * (uint32_t)kLodSkirtTile;
    const uint32_t nt = a.n_tris - t0 < (uint32_t)kLodSkirtTile ? a.n_tris - t0 : (uint32_t)kLodSkirtTile;
    skirt_bracket(a, range, t0, nt);
    int any = 0;
    for (uint32_t b = range[0] + threadIdx.x; b <= range[1]; b += 256u) any |= a.node_masks[b];
    if (!__syncthreads_or(any)) {   // no node of the tile has a flagged face: no record is read (uniform across the workgroup)
        masks[(size_t)t0 + threadIdx.x] = 0;
        if (threadIdx.x == 0) tile_totals[blockIdx.x] = 0u;
        return;
    }
    if (!INDEXED) {
        load_record_tile(rec, a.recs + (size_t)t0 * 19, nt * 19);   // tile base: 256 * 76 bytes per tile, 16-byte aligned
        __syncthreads();
    }
    uint32_t mask = 0u;
    if (threadIdx.x < nt) {
        SkirtTri tri;
        skirt_load<INDEXED>(a, rec, range, t0 + threadIdx.x, tri);
        mask = skirt_faces(tri, a.node_masks[tri.node]);
    }
    masks[(size_t)t0 + threadIdx.x] = (uint8_t)mask;   // the buffer holds whole tiles: the ragged tile's tail is written as zeros
    uint32_t total;
    block_scan<4>(2u * (uint32_t)__popc(mask), wave_sums, total);
    if (threadIdx.x == 0) tile_totals[blockIdx.x] = total;
}

template <bool INDEXED, bool STAGED>
__global__ __launch_bounds__(256) void lodskirt_emit_kernel(SkirtArgs a, const uint8_t *__restrict__ masks, const uint32_t *__restrict__ tile_offsets,
                                                            const uint32_t *__restrict__ group_offsets, uint32_t capacity, uint32_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kLodSkirtTile * 19];
    __shared__ __attribute__((aligned(16))) uint32_t stage[STAGED ? 4 + kLodSkirtStage * 19 : 4];
    __shared__ uint32_t range[2], wave_sums[4];
    const uint32_t t0 = blockIdx.x * (uint32_t)kLodSkirtTile;
    const uint32_t nt = a.n_tris - t0 < (uint32_t)kLodSkirtTile ? a.n_tris - t0 : (uint32_t)kLodSkirtTile;
    uint32_t mask = masks[(size_t)t0 + threadIdx.x];
    uint32_t total;
    const uint32_t before = block_scan<4>(2u * (uint32_t)__popc(mask), wave_sums, total);
    if (total == 0u) return;   // a tile without a quad reads no record (uniform across the workgroup)
    if (INDEXED) {
        skirt_bracket(a, range, t0, nt);
    } else {
        load_record_tile(rec, a.recs + (size_t)t0 * 19, nt * 19);
        __syncthreads();
    }
    if (threadIdx.x >= nt) mask = 0u;   // the tail of the ragged tile holds zeros anyway
    SkirtTri tri;
    if (mask) skirt_load<INDEXED>(a, rec, range, t0 + threadIdx.x, tri);
    const uint32_t base = group_offsets[blockIdx.x / (uint32_t)kScanThreads] + tile_offsets[blockIdx.x];   // the tile's first record
    if (!STAGED) {
        uint32_t slot = base + before;
        if (mask) {   // faces in ascending order
            skirt_store_direct<0>(tri, a.depth, mask, slot, capacity, out);
            skirt_store_direct<1>(tri, a.depth, mask, slot, capacity, out);
            skirt_store_direct<2>(tri, a.depth, mask, slot, capacity, out);
            skirt_store_direct<3>(tri, a.depth, mask, slot, capacity, out);
            skirt_store_direct<4>(tri, a.depth, mask, slot, capacity, out);
            skirt_store_direct<5>(tri, a.depth, mask, slot, capacity, out);
        }
        return;
    }
    // STAGED: the tile's records [base, base + total) in chunks; a chunk's dwords lie in LDS as they lie in memory, shifted so that a
    // 16-byte piece of the output is a 16-byte piece of the stage
    for (uint32_t c0 = 0u; c0 < total; c0 += (uint32_t)kLodSkirtStage) {   // uniform across the workgroup
        const uint32_t n = total - c0 < (uint32_t)kLodSkirtStage ? total - c0 : (uint32_t)kLodSkirtStage;
        const uint32_t first = base + c0;
        if (first + n > capacity || first + n < first) return;   // never for the masks of this call
        const size_t d0 = 19 * (size_t)first;   // the chunk's first dword of the output
        const uint32_t shift = (uint32_t)(d0 & 3u);
        uint32_t j = before;   // record j of the tile
        if (mask) {   // faces in ascending order
            skirt_store_staged<0>(tri, a.depth, mask, j, c0, n, stage + shift);
            skirt_store_staged<1>(tri, a.depth, mask, j, c0, n, stage + shift);
            skirt_store_staged<2>(tri, a.depth, mask, j, c0, n, stage + shift);
            skirt_store_staged<3>(tri, a.depth, mask, j, c0, n, stage + shift);
            skirt_store_staged<4>(tri, a.depth, mask, j, c0, n, stage + shift);
            skirt_store_staged<5>(tri, a.depth, mask, j, c0, n, stage + shift);
        }
        __syncthreads();
        const uint32_t nd = 19u * n;   // dwords [shift, shift + nd) of the stage go to out[d0 - shift + ...]
        uint32_t *dst = out + (d0 - shift);
        for (uint32_t q = threadIdx.x; 4u * q < shift + nd; q += 256u) {
            if (4u * q >= shift && 4u * q + 4u <= shift + nd) {
                *reinterpret_cast<uint4 *>(dst + 4u * q) = *reinterpret_cast<const uint4 *>(stage + 4u * q);
            } else {
                for (uint32_t d = 4u * q < shift ? shift : 4u * q; d < 4u * q + 4u && d < shift + nd; ++d) dst[d] = stage[d];
            }
        }
        __syncthreads();
    }
}

// out[b], b = 0..n_nodes: the records of triangles before the node's first one
__global__ __launch_bounds__(256) void lodskirt_offsets_kernel(const uint32_t *__restrict__ toffsets, uint32_t n_nodes, uint32_t n_tris,
                                                               const uint32_t *__restrict__ mask_words, const uint32_t *__restrict__ tile_offsets,
                                                               const uint32_t *__restrict__ group_offsets, const unsigned long long *__restrict__ total,
                                                               int32_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > n_nodes) return;
    const uint32_t t = toffsets[b];
    if (t >= n_tris) {
        out[b] = (int32_t)*total;
        return;
    }
    const uint32_t tile = t / (uint32_t)kLodSkirtTile, r = t % (uint32_t)kLodSkirtTile;
    const uint32_t *w = mask_words + (size_t)tile * (kLodSkirtTile / 4);
    uint32_t sum = 0u;
    for (uint32_t j = 0; j < r / 4u; ++j) sum += (uint32_t)__popc(w[j]);
    if (r & 3u) sum += (uint32_t)__popc(w[r / 4u] & ((1u << (8u * (r & 3u))) - 1u));
    out[b] = (int32_t)(group_offsets[tile / (uint32_t)kScanThreads] + tile_offsets[tile] + 2u * sum);
}

// a plain read of n 16-byte pieces, for vtmc_debug_lodskirt_read_ms: every workgroup leaves the XOR of what it read
__global__ __launch_bounds__(256) void lodskirt_read_kernel(const uint4 *__restrict__ src, size_t n, uint32_t *__restrict__ sink)
{
    uint32_t x = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const uint4 v = src[i];
        x ^= v.x ^ v.y ^ v.z ^ v.w;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d, 64);
    if ((threadIdx.x & 63u) == 0u) sink[blockIdx.x * 4u + (threadIdx.x >> 6)] = x;
}

static bool lod_result(const vtmc_ctx *ctx) { return ctx->result.valid && ctx->result.source == ResultSource::TerrainLod; }
static bool lodskirt_current(const vtmc_ctx *ctx) { return lod_result(ctx) && ctx->lodskirt.epoch == ctx->result.epoch; }

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_lod_skirts(vtmc_ctx *ctx, const vtmc_lodskirt_params *params, int64_t *n_triangles)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!params) return fail(ctx, VTMC_ERR_INVALID_ARG, "lod_skirts: params is null");
    if (!lod_result(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lod_skirts: the context's current result is not a level-of-detail extract's");
    if (const char *fault = lodskirt_params_fault(*params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "lod_skirts: %s", fault);
    const VtmcResult &res = ctx->result;
    VtmcLodSkirt &sk = ctx->lodskirt;
    const int64_t T = res.tris;
    const size_t B = ctx->lod_nodes.size();
    if ((size_t)res.blocks != B) return fail(ctx, VTMC_ERR_DEVICE, "lod_skirts: the result holds %d blocks for %zu nodes", res.blocks, B);
    const int32_t cells[3] = {ctx->tshape.dim_x - 2, ctx->tshape.dim_y - 2, ctx->tshape.dim_z - 2};
    std::vector<uint8_t> face_masks;
    const int32_t flagged = lodskirt_face_masks(ctx->lod_nodes.data(), B, cells, params->flags, face_masks);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    // the scratch of the pass first: the previous skirts (records, offsets, masks of the nodes) stand until the total is known to fit
    StageClock<6> &clock = ctx->lodskirt_clock;
    VTMC_HIP(ctx, clock.begin());   // disarmed: a result without triangles leaves it so
    unsigned long long total = 0;
    const bool launches = T > 0 && B > 0;
    const uint32_t tiles = lodskirt_tiles(T);
    ScanLayout scan(tiles);
    SkirtArgs a{};
    if (launches) {
        if (int rc = ensure(ctx, sk.masks, lodskirt_mask_bytes(T))) return rc;
        if (int rc = ensure(ctx, sk.tiles, scan.bytes())) return rc;
        if (int rc = ensure(ctx, sk.node_masks, B)) return rc;
        scan = ScanLayout(tiles, sk.tiles.p);
        a.recs = (const uint32_t *)(res.indexed ? ctx->verts.p : ctx->tris.p);
        a.indices = (const int32_t *)ctx->indices.p;
        a.toffsets = (const uint32_t *)ctx->offsets.p;
        a.voffsets = (const uint32_t *)ctx->voffsets.p;
        a.node_masks = (const uint8_t *)sk.node_masks.p;
        a.n_tris = (uint32_t)T, a.n_nodes = (uint32_t)B, a.n_verts = (uint32_t)res.verts;
        a.depth = params->depth;
        if (res.indexed && res.verts <= 0) return fail(ctx, VTMC_ERR_DEVICE, "lod_skirts: an indexed result of %lld triangles without vertices", (long long)T);
        VTMC_HIP(ctx, hipMemcpy(sk.node_masks.p, face_masks.data(), B, hipMemcpyHostToDevice));   // blocking: face_masks is this call's own
        VTMC_HIP(ctx, clock.mark(0, ctx->stream));
        VTMC_HIP(ctx, launch(res.indexed ? lodskirt_count_kernel<true> : lodskirt_count_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a, (uint8_t *)sk.masks.p,
                             scan.tile_totals()));
        VTMC_HIP(ctx, clock.mark(1, ctx->stream));
        VTMC_HIP(ctx, launch_scan(scan, ctx->stream));
        VTMC_HIP(ctx, clock.mark(2, ctx->stream));
        VTMC_HIP(ctx, hipMemcpyAsync(&total, scan.total(), sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (!lodskirt_total_fits(total)) return fail(ctx, VTMC_ERR_TOO_LARGE, "lod_skirts: %llu skirt triangles exceed 2^31 - 1", total);
    }
    // From here on the buffers no longer hold the previous skirts.  What is refused above (INVALID_ARG, NO_RESULT, TOO_LARGE) keeps them; a
    // device error below (a buffer that cannot grow, a launch that fails) leaves the context without skirts, as the scatter does.
    sk.epoch = 0;
    if (int rc = ensure(ctx, sk.node_offsets, sizeof(int32_t) * (B + 1))) return rc;
    if (total > 0)
        if (int rc = ensure(ctx, sk.tris, sizeof(vtmc_triangle) * (size_t)total)) return rc;
    if (!launches) {
        VTMC_HIP(ctx, hipMemsetAsync(sk.node_offsets.p, 0, sizeof(int32_t) * (B + 1), ctx->stream));
    } else {
        VTMC_HIP(ctx, clock.mark(3, ctx->stream));
        if (total > 0) {
            void (*emit)(SkirtArgs, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t *) =
                res.indexed ? (sk.staged ? lodskirt_emit_kernel<true, true> : lodskirt_emit_kernel<true, false>)
                            : (sk.staged ? lodskirt_emit_kernel<false, true> : lodskirt_emit_kernel<false, false>);
            VTMC_HIP(ctx, launch(emit, dim3(tiles), dim3(256), 0, ctx->stream, a, (const uint8_t *)sk.masks.p, scan.tile_offsets(), scan.group_offsets(), (uint32_t)total,
                                 (uint32_t *)sk.tris.p));
        }
        VTMC_HIP(ctx, clock.mark(4, ctx->stream));
        VTMC_HIP(ctx, launch(lodskirt_offsets_kernel, lanes256((int64_t)B + 1), dim3(256), 0, ctx->stream, a.toffsets, (uint32_t)B, (uint32_t)T, (const uint32_t *)sk.masks.p,
                             scan.tile_offsets(), scan.group_offsets(), scan.total(), (int32_t *)sk.node_offsets.p));
        VTMC_HIP(ctx, clock.mark(5, ctx->stream));
        clock.arm();
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sk.face_masks.swap(face_masks);
    sk.n = (int64_t)total;
    sk.nodes = (int32_t)B;
    sk.flagged = flagged;
    sk.epoch = res.epoch;
    if (n_triangles) *n_triangles = sk.n;
    return VTMC_OK;
}

int32_t vtmc_lodskirt_info(vtmc_ctx *ctx, int32_t *n_nodes, int32_t *n_flagged_nodes, int64_t *n_triangles)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_info: no skirts of the current result (call vtmc_lod_skirts)");
    if (n_nodes) *n_nodes = ctx->lodskirt.nodes;
    if (n_flagged_nodes) *n_flagged_nodes = ctx->lodskirt.flagged;
    if (n_triangles) *n_triangles = ctx->lodskirt.n;
    return VTMC_OK;
}

int32_t vtmc_lodskirt_masks(vtmc_ctx *ctx, uint8_t *dst, int32_t capacity_nodes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_masks: no skirts of the current result (call vtmc_lod_skirts)");
    const VtmcLodSkirt &sk = ctx->lodskirt;
    if (capacity_nodes < sk.nodes) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d nodes", capacity_nodes, sk.nodes);
    if (sk.nodes > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    if (sk.nodes > 0) memcpy(dst, sk.face_masks.data(), (size_t)sk.nodes);
    return VTMC_OK;
}

int32_t vtmc_lodskirt_read(vtmc_ctx *ctx, vtmc_triangle *dst, int64_t capacity, int32_t *node_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_read: no skirts of the current result (call vtmc_lod_skirts)");
    const VtmcLodSkirt &sk = ctx->lodskirt;
    if (capacity < sk.n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %lld skirt triangles", (long long)capacity, (long long)sk.n);
    if (sk.n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (sk.n > 0) VTMC_HIP(ctx, hipMemcpy(dst, sk.tris.p, sizeof(vtmc_triangle) * (size_t)sk.n, hipMemcpyDeviceToHost));
    if (node_offsets) VTMC_HIP(ctx, hipMemcpy(node_offsets, sk.node_offsets.p, sizeof(int32_t) * ((size_t)sk.nodes + 1), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_lodskirt_device_results(vtmc_ctx *ctx, const vtmc_triangle **d_triangles, const int32_t **d_node_offsets, int64_t *n_triangles)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_device_results: no skirts of the current result (call vtmc_lod_skirts)");
    if (d_triangles) *d_triangles = (const vtmc_triangle *)ctx->lodskirt.tris.p;
    if (d_node_offsets) *d_node_offsets = (const int32_t *)ctx->lodskirt.node_offsets.p;
    if (n_triangles) *n_triangles = ctx->lodskirt.n;
    return VTMC_OK;
}

// Not part of the ABI (tests, tools/lodskirt_bench.py): which store variant the emit kernel of later calls uses, 0 DIRECT, 1 STAGED.
int32_t vtmc_debug_lodskirt_store(vtmc_ctx *ctx, int32_t staged)
{
    if (!ctx || (staged != 0 && staged != 1)) return VTMC_ERR_INVALID_ARG;
    ctx->lodskirt.staged = staged != 0;
    return VTMC_OK;
}

// Not part of the ABI (tools/lodskirt_bench.py): device time of the last vtmc_lod_skirts that launched kernels, ms[0..3] = the count
// kernel, the scan, the emit kernel, the node offsets.
int32_t vtmc_debug_lodskirt_ms(vtmc_ctx *ctx, float ms[4])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->lodskirt_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_lodskirt_ms before skirts that launched kernels");
    if (int rc = ctx->lodskirt_clock.sync_last(ctx)) return rc;
    static const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
    for (int i = 0; i < 4; ++i)
        if (int rc = ctx->lodskirt_clock.elapsed(ctx, pairs[i][0], pairs[i][1], &ms[i])) return rc;
    return VTMC_OK;
}

// Not part of the ABI (tools/lodskirt_bench.py): the median device time of `reps` plain reads of the records of the result the context
// holds (soup: the triangles; indexed: the vertices), 16 bytes a lane, after one read that is not timed.
int32_t vtmc_debug_lodskirt_read_ms(vtmc_ctx *ctx, int32_t reps, float *ms)
{
    if (!ctx || !ms || reps < 1 || reps > 64) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_lodskirt_read_ms without a result");
    const VtmcResult &res = ctx->result;
    const size_t pieces = (res.indexed ? sizeof(vtmc_vertex) * (size_t)res.verts : sizeof(vtmc_triangle) * (size_t)res.tris) / 16;
    if (pieces == 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "debug_lodskirt_read_ms: an empty result");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    const unsigned groups = (unsigned)std::min<size_t>((pieces + 255) / 256, (size_t)ctx->n_cus * 8);
    if (int rc = ensure(ctx, ctx->lodskirt.sink, sizeof(uint32_t) * 4 * (size_t)groups)) return rc;
    StageClock<6> &clock = ctx->lodskirt_clock;
    VTMC_HIP(ctx, clock.begin());   // borrowed, and left disarmed: its events no longer hold the pass's times
    float t[64];
    for (int i = -1; i < reps; ++i) {
        VTMC_HIP(ctx, clock.mark(0, s));
        VTMC_HIP(ctx, launch(lodskirt_read_kernel, dim3(groups), dim3(256), 0, s, (const uint4 *)(res.indexed ? ctx->verts.p : ctx->tris.p), pieces, (uint32_t *)ctx->lodskirt.sink.p));
        VTMC_HIP(ctx, clock.mark(1, s));
        VTMC_HIP(ctx, hipEventSynchronize(clock.event(1)));
        if (i >= 0)
            if (int rc = clock.elapsed(ctx, 0, 1, &t[i])) return rc;
    }
    std::sort(t, t + reps);
    *ms = t[reps / 2];
    return VTMC_OK;
}

}  // extern "C"
