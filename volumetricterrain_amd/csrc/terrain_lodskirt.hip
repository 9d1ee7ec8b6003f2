// terrain_lodskirt.hip -- skirt triangles over the seams of a level-of-detail extract (vtmc_lod_skirts, vtmc_lodskirt_*): for every
// triangle of the result with exactly two positions on a FLAGGED face of its node, a quad in the face's plane hung from that edge towards
// the solid side.  The rule, operation by operation, is LODSKIRT of include/vtmc_lodskirt.h; the kernels follow it bit for bit (library
// built with -ffp-contract=off; FP32 division and square root are the correctly rounded ones).  The host half -- argument checks, the face
// masks of the node list, the count bound -- is terrain_lodskirt.h.  The pass reads the records of the result and never the grid.
//
// The pass is the stream over the result's triangles of tri_stream_kernels.h: the scheme, its traffic and the bounds of every access are
// written down there, and the view of the result, the tiles, the loader, the offsets kernel and the host glue come from there.  The
// skirts' own, two records per set bit:
//   lodskirt_count_kernel  brackets the nodes of its tile first; the workgroup ORs the mask bytes of the nodes between them and LEAVES
//      when none is flagged (nodes are contiguous in the result, so away from the seams whole runs of tiles leave here, before any record
//      is read).  Otherwise every lane tests its triangle against the flagged faces of its node and writes one FACE MASK byte (bit f:
//      face f yields a quad).  The host checks the grand total against 2^31 - 1.
//   lodskirt_emit_kernel   DIRECT: a lane writes its records dword by dword at its slot.  STAGED: the records are put together in
//      LDS, kLodSkirtStage at a time, shifted by the run's misalignment, and leave as 16-byte pieces.  The library uses DIRECT:
//      tools/lodskirt_bench.py measured its emit kernel no slower at split 1 and a fifth faster at split 2 (LODSEAMS.md,
//      profiles/r27/lodskirt/); STAGED stays built for the tool, behind vtmc_debug_lodskirt_store.
//
// Bounds, beside those of the stream:
//   node_masks   B bytes; read at b in [range[0], range[1]] <= B - 1, or at the lane's node, which the loader keeps at or below B - 1.
//   out          a quad is stored only when slot + 2 <= capacity.  STAGED stores dwords [19 base, 19 (base + n)) of the run, base + n <=
//                capacity checked the same way; its LDS stage holds 3 + 19 kLodSkirtStage dwords and record j of a chunk lies at
//                shift + 19 j, shift <= 3, j < kLodSkirtStage.
#include "terrain_lodskirt.h"
#include "tri_stream_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace vtmc {

constexpr int kLodSkirtStage = 256;   // records the STAGED emit puts together in LDS at a time

struct SkirtArgs {
    TriView v;                   // its blocks are the nodes
    const uint8_t *node_masks;   // the n_blocks face masks
    float depth;
};

// the faces of the node's mask on which exactly two of the triangle's positions lie (a triangle's `block` is its node)
__device__ __forceinline__ uint32_t skirt_faces(const TriWords &t, uint32_t node_mask)
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
__device__ __forceinline__ void skirt_quad(const TriWords &t, float depth, int which, uint32_t *dst)
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
    if (which != 1) skirt_record(dst, pb, pa, qa, nb, na, na, t.block);
    if (which != 0) skirt_record(which == 2 ? dst + 19 : dst, pb, qa, qb, nb, na, nb, t.block);
}

// Face F of a lane's mask in the DIRECT emit: both records at the lane's slot, which moves on
template <int F>
__device__ __forceinline__ void skirt_store_direct(const TriWords &t, float depth, uint32_t mask, uint32_t &slot, uint32_t capacity, uint32_t *__restrict__ out)
{
    if (!(mask & (1u << F))) return;
    if (slot + 2u <= capacity && slot + 2u > slot) skirt_quad<F>(t, depth, 2, out + 19 * (size_t)slot);
    slot += 2u;
}

// Face F of a lane's mask in the STAGED emit: those of its two records j, j + 1 of the tile that fall into the chunk [c0, c0 + n)
template <int F>
__device__ __forceinline__ void skirt_store_staged(const TriWords &t, float depth, uint32_t mask, uint32_t &j, uint32_t c0, uint32_t n, uint32_t *stage)
{
    if (!(mask & (1u << F))) return;
    if (j >= c0 && j < c0 + n) skirt_quad<F>(t, depth, 0, stage + 19u * (j - c0));
    if (j + 1u >= c0 && j + 1u < c0 + n) skirt_quad<F>(t, depth, 1, stage + 19u * (j + 1u - c0));
    j += 2u;
}

template <bool INDEXED>
__global__ __launch_bounds__(256) void lodskirt_count_kernel(SkirtArgs a, uint8_t *__restrict__ masks, uint32_t *__restrict__ tile_totals)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kTriTile * 19];
    __shared__ uint32_t range[2], wave_sums[4];
    uint32_t t0, nt;
    tri_tile_bounds(a.v, t0, nt);
    tri_tile_bracket(a.v, range, t0, nt);
    int any = 0;
    for (uint32_t b = range[0] + threadIdx.x; b <= range[1]; b += 256u) any |= a.node_masks[b];
    if (!__syncthreads_or(any)) {   // no node of the tile has a flagged face: no record is read (uniform across the workgroup)
        masks[(size_t)t0 + threadIdx.x] = 0;
        if (threadIdx.x == 0) tile_totals[blockIdx.x] = 0u;
        return;
    }
    if (!INDEXED) tri_tile_stage(a.v, rec, t0, nt);
    uint32_t mask = 0u;
    if (threadIdx.x < nt) {
        TriWords tri;
        tri_load<INDEXED>(a.v, rec, t0 + threadIdx.x, tri_block_of<INDEXED>(a.v, rec, range, t0 + threadIdx.x), tri);
        mask = skirt_faces(tri, a.node_masks[tri.block]);
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
    __shared__ __attribute__((aligned(16))) uint32_t rec[INDEXED ? 4 : kTriTile * 19];
    __shared__ __attribute__((aligned(16))) uint32_t stage[STAGED ? 4 + kLodSkirtStage * 19 : 4];
    __shared__ uint32_t range[2], wave_sums[4];
    uint32_t t0, nt;
    tri_tile_bounds(a.v, t0, nt);
    uint32_t mask = masks[(size_t)t0 + threadIdx.x];
    uint32_t total;
    const uint32_t before = block_scan<4>(2u * (uint32_t)__popc(mask), wave_sums, total);
    if (total == 0u) return;   // a tile without a quad reads no record (uniform across the workgroup)
    if (INDEXED) tri_tile_bracket(a.v, range, t0, nt);
    else tri_tile_stage(a.v, rec, t0, nt);
    if (threadIdx.x >= nt) mask = 0u;   // the tail of the ragged tile holds zeros anyway
    TriWords tri;
    if (mask) tri_load<INDEXED>(a.v, rec, t0 + threadIdx.x, tri_block_of<INDEXED>(a.v, rec, range, t0 + threadIdx.x), tri);
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
static bool lodskirt_current(const vtmc_ctx *ctx) { return lod_result(ctx) && ctx->lodskirt.pass.epoch == ctx->result.epoch; }

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
    VtmcTriStream &st = sk.pass;
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
    const uint32_t tiles = tri_tiles(T);
    ScanLayout scan(tiles);
    SkirtArgs a{};
    if (launches) {
        if (int rc = tri_stream_scratch(ctx, st, T, &scan)) return rc;
        if (int rc = ensure(ctx, sk.node_masks, B)) return rc;
        if (int rc = tri_view(ctx, "lod_skirts", &a.v)) return rc;
        a.node_masks = (const uint8_t *)sk.node_masks.p;
        a.depth = params->depth;
        VTMC_HIP(ctx, hipMemcpy(sk.node_masks.p, face_masks.data(), B, hipMemcpyHostToDevice));   // blocking: face_masks is this call's own
        VTMC_HIP(ctx, clock.mark(0, ctx->stream));
        VTMC_HIP(ctx, launch(res.indexed ? lodskirt_count_kernel<true> : lodskirt_count_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, a, (uint8_t *)st.masks.p,
                             scan.tile_totals()));
        if (int rc = tri_scan_total(ctx, scan, clock, &total)) return rc;
        if (!lodskirt_total_fits(total)) return fail(ctx, VTMC_ERR_TOO_LARGE, "lod_skirts: %llu skirt triangles exceed 2^31 - 1", total);
    }
    // From here on the buffers no longer hold the previous skirts.  What is refused above (INVALID_ARG, NO_RESULT, TOO_LARGE) keeps them; a
    // device error below (a buffer that cannot grow, a launch that fails) leaves the context without skirts, as the scatter does.
    st.epoch = 0;
    lodattr_drop_skirts(ctx);   // include/vtmc_lodattr.h: the values of the previous skirts' corners go with them
    if (int rc = ensure(ctx, st.block_offsets, sizeof(int32_t) * (B + 1))) return rc;
    if (total > 0)
        if (int rc = ensure(ctx, st.records, sizeof(vtmc_triangle) * (size_t)total)) return rc;
    if (!launches) {
        VTMC_HIP(ctx, hipMemsetAsync(st.block_offsets.p, 0, sizeof(int32_t) * (B + 1), ctx->stream));
    } else {
        VTMC_HIP(ctx, clock.mark(3, ctx->stream));
        if (total > 0) {
            void (*emit)(SkirtArgs, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t *) =
                res.indexed ? (sk.staged ? lodskirt_emit_kernel<true, true> : lodskirt_emit_kernel<true, false>)
                            : (sk.staged ? lodskirt_emit_kernel<false, true> : lodskirt_emit_kernel<false, false>);
            VTMC_HIP(ctx, launch(emit, dim3(tiles), dim3(256), 0, ctx->stream, a, (const uint8_t *)st.masks.p, scan.tile_offsets(), scan.group_offsets(), (uint32_t)total,
                                 (uint32_t *)st.records.p));
        }
        if (int rc = tri_launch_offsets(ctx, a.v, st, scan, 2u, clock)) return rc;
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sk.face_masks.swap(face_masks);
    sk.flagged = flagged;
    st.n = (int64_t)total;
    st.blocks = (int)B;
    st.epoch = res.epoch;
    if (n_triangles) *n_triangles = st.n;
    return VTMC_OK;
}

int32_t vtmc_lodskirt_info(vtmc_ctx *ctx, int32_t *n_nodes, int32_t *n_flagged_nodes, int64_t *n_triangles)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_info: no skirts of the current result (call vtmc_lod_skirts)");
    if (n_nodes) *n_nodes = ctx->lodskirt.pass.blocks;
    if (n_flagged_nodes) *n_flagged_nodes = ctx->lodskirt.flagged;
    if (n_triangles) *n_triangles = ctx->lodskirt.pass.n;
    return VTMC_OK;
}

int32_t vtmc_lodskirt_masks(vtmc_ctx *ctx, uint8_t *dst, int32_t capacity_nodes)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_masks: no skirts of the current result (call vtmc_lod_skirts)");
    const int nodes = ctx->lodskirt.pass.blocks;
    if (capacity_nodes < nodes) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d nodes", capacity_nodes, nodes);
    if (nodes > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    if (nodes > 0) memcpy(dst, ctx->lodskirt.face_masks.data(), (size_t)nodes);
    return VTMC_OK;
}

int32_t vtmc_lodskirt_read(vtmc_ctx *ctx, vtmc_triangle *dst, int64_t capacity, int32_t *node_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_read: no skirts of the current result (call vtmc_lod_skirts)");
    return tri_stream_read(ctx, ctx->lodskirt.pass, sizeof(vtmc_triangle), "skirt triangles", VTMC_ERR_CAPACITY, dst, capacity, node_offsets);
}

int32_t vtmc_lodskirt_device_results(vtmc_ctx *ctx, const vtmc_triangle **d_triangles, const int32_t **d_node_offsets, int64_t *n_triangles)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!lodskirt_current(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "lodskirt_device_results: no skirts of the current result (call vtmc_lod_skirts)");
    tri_stream_device_results(ctx->lodskirt.pass, d_triangles, d_node_offsets, n_triangles);
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
    return tri_stream_ms(ctx, ctx->lodskirt_clock, "debug_lodskirt_ms before skirts that launched kernels", ms);
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
