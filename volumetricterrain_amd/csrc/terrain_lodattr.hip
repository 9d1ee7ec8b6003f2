// terrain_lodattr.hip -- per-vertex material weights and ambient occlusion of a level-of-detail extract and of its skirts
// (vtmc_lod_material_vertices, vtmc_lod_ao_vertices, vtmc_lodattr_*).  The rule, operation by operation, is LODATTR of
// include/vtmc_lodattr.h; the kernels follow it bit for bit (library built with -ffp-contract=off).  The host half -- the selector checks,
// a node's lattice and its two index clamps, the coordinate formulas, the map from a skirt corner to its source -- is terrain_lodattr.h,
// and the kernels call those same functions.  The layer owns its buffers (ctx->lodattr) and writes nothing else the context holds.
//
// Occlusion, the mesh.  The pass of terrain_ao.hip with a node in place of a block: one workgroup of 256 per non-empty node (the
// BlockDesc the scan left names the node; (o, L) comes from the node list on the device), which stages the node's neighbourhood of its
// own SAMPLE LATTICE in LDS -- (10 + 2R)^3 floats, R = ceil(Rg) <= 6, lattice samples o/s - R .. o/s + 9 + R per axis -- and then runs the
// march of ao_march.h on the tile exactly as the block pass does: a tile holds lattice samples whatever stride they were gathered at.
// The staging loop applies both clamps of the rule, the lattice index into [0, n_L - 1] and then the grid index min(i * s, dim - 1).  Its
// loads walk x at stride s: at s = 1 a row of the tile is one or two lines, at s >= 32 every sample is a 128-byte line of its own, the
// same property of the subsample the gather kernel of terrain_lod.hip has; what LDS saves is the 26 x steps x 8 re-reads of those lines
// per vertex.  A node of at most kAoDirectMax vertices takes the direct route instead (kAoStrided: each axis carries the offsets of both
// neighbours, because the upper one of lattice sample i0 is min((i0 + 1) * s, dim - 1)).  Record loader, chunks and the dword-assembled
// byte output are ao_chunks of ao_march.h.
// Materials, the mesh.  The tile-of-records pass of material_filter.h with MaterialOfNodes in place of the BlockMap.
// Skirts.  A lane per quad reads record 2q of the skirts, evaluates its corners 0 (b) and 1 (a) with the record's node, and writes the
// six corners of records 2q and 2q + 1: (b, a, a), (b, a, b).  For the materials that is a pass of its own over all quads.  For the
// occlusion the node's workgroup takes its node's quads behind its own vertices, with the tile it has staged (a node's skirt records are
// contiguous: node_offsets; a node without triangles has no skirts): a pass of their own, a lane per quad on the direct route, has too few
// lanes to hide the latency of its fetches and cost 0.11 ms of device time where the nodes' kernel grows by 0.01 to 0.05 ms
// (tools/lodattr_bench.py; LODSHADING.md, "What it costs").  That pass stays built behind vtmc_debug_lodattr_skirts_in_node so that the
// tool can repeat the comparison.
//
// Bounds.  nodes: read at the BlockDesc's / the record's block, kept at or below n_nodes - 1.  grid: every index is
// lodattr_fine_index(i, s, dim) <= dim - 1 of an i >= 0.  tile: E^3 floats of dynamic LDS; a fetch stays inside by the argument of
// terrain_ao.hip, in lattice coordinates.  mesh values: ao_chunks writes bytes [first * vpr, (first + count) * vpr) of a buffer of
// n rounded up to 4 bytes; the material kernels write out[v], v < n.  skirt values: quad q < n_records / 2 writes corners 6q .. 6q + 5
// of 3 * n_records.
#include "terrain_lodattr.h"
#include "ao_march.h"
#include "material_filter.h"
#include "terrain_material.h"
#include "vtmc_ctx.h"

namespace vtmc {

struct LodAoArgs {
    const float *grid;  // the terrain's samples, x fastest
    int dim[3];         // samples per axis
    const BlockDesc *active;
    const vtmc_lod_node *nodes;
    uint32_t n_nodes;
    int reach, extent;  // R and 10 + 2R
    FastDiv d_extent;
    AoMarch march;
    uint32_t direct_max;
    uint32_t *stats;    // [0] workgroups that staged a tile, [1] workgroups on the direct route
    uint8_t *out;
    // the skirts: null where there are none, and in the nodes' kernel when the skirts are given a pass of their own
    const uint32_t *skirts;
    const int32_t *node_offsets;
    uint32_t n_quads;
    uint8_t *skirt_out;
};

// the lattice of node nd over the grid, and the tile origin of a workgroup that stages one
__device__ __forceinline__ AoField lod_ao_field(const LodAoArgs &a, const vtmc_lod_node &nd, const float *tile)
{
    const int s = 1 << nd.level;
    AoField F;
    F.tile = tile;
    F.grid = a.grid;
    F.E = a.extent;
    F.stride = s;
    for (int k = 0; k < 3; ++k) {
        F.dim[k] = a.dim[k];
        F.n[k] = lodattr_lattice_samples(a.dim[k], s);
        F.o[k] = nd.origin[k] / s - a.reach;
    }
    return F;
}

// The six bytes of quad q: corners 0 (b) and 1 (a) of skirt record 2q, evaluated through ROUTE (kAoTile: where the corner lies in the
// node's cells, as every corner of the library's own skirts does)
template <int ROUTE>
__device__ __forceinline__ void lod_ao_quad(const LodAoArgs &a, const AoField &F, const vtmc_lod_node &nd, uint32_t q)
{
    const uint32_t *r = a.skirts + 38 * (size_t)q;
    const int s = F.stride;
    uint32_t val[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float p0 = __uint_as_float(r[3 * c]), p1 = __uint_as_float(r[3 * c + 1]), p2 = __uint_as_float(r[3 * c + 2]);
        const float n0 = __uint_as_float(r[9 + 3 * c]), n1 = __uint_as_float(r[10 + 3 * c]), n2 = __uint_as_float(r[11 + 3 * c]);
        const float gx = lodattr_ao_coord(nd.origin[0], s, p0), gy = lodattr_ao_coord(nd.origin[1], s, p1), gz = lodattr_ao_coord(nd.origin[2], s, p2);
        const bool inside = p0 >= 0.0f && p0 <= 8.0f && p1 >= 0.0f && p1 <= 8.0f && p2 >= 0.0f && p2 <= 8.0f;
        if (ROUTE == kAoTile && inside) val[c] = ao_vertex<kAoTile>(a.march, F, gx, gy, gz, n0, n1, n2);
        else val[c] = ao_vertex<kAoStrided>(a.march, F, gx, gy, gz, n0, n1, n2);
    }
    uint16_t *dst = reinterpret_cast<uint16_t *>(a.skirt_out + 6 * (size_t)q);   // 6 q is even and the buffer is the allocator's
#pragma unroll
    for (int w = 0; w < 3; ++w) dst[w] = (uint16_t)(val[lodattr_skirt_source(2 * w)] | val[lodattr_skirt_source(2 * w + 1)] << 8);
}

// One workgroup per non-empty node.
template <bool INDEXED>
__global__ __launch_bounds__(256) void lod_ao_kernel(const uint32_t *__restrict__ recs, LodAoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ __attribute__((aligned(16))) uint32_t rec[AoChunkLds<INDEXED>::REC_WORDS];
    __shared__ uint32_t outw[AoChunkLds<INDEXED>::OUT_WORDS];
    const BlockDesc d = a.active[blockIdx.x];
    const uint32_t first = INDEXED ? d.vert_base : d.tri_base;
    const uint32_t count = INDEXED ? d.vert_cnt : (d.cnt_mask & kCountMask);
    if (count == 0u) return;
    const uint32_t vpr = INDEXED ? 1u : 3u;
    const uint32_t node = d.b < a.n_nodes ? d.b : a.n_nodes - 1;   // never taken for a result of the library
    const vtmc_lod_node nd = a.nodes[node];
    const AoField F = lod_ao_field(a, nd, tile);
    const bool direct = count * vpr <= a.direct_max;
    if (threadIdx.x == 0) atomicAdd(a.stats + (direct ? 1 : 0), 1u);
    if (!direct) {
        // the box of lattice samples, row by row along x: the lattice index clamped to the lattice, then the grid index of that sample
        const uint32_t E = (uint32_t)a.extent, E3 = E * E * E;
        for (uint32_t i = threadIdx.x; i < E3; i += 256u) {
            const uint32_t row = a.d_extent.quot(i), x = i - row * E;
            const uint32_t z = a.d_extent.quot(row), y = row - z * E;
            const int gx = lodattr_fine_index(lodattr_clamp_lattice(F.o[0] + (int)x, F.n[0]), F.stride, F.dim[0]);
            const int gy = lodattr_fine_index(lodattr_clamp_lattice(F.o[1] + (int)y, F.n[1]), F.stride, F.dim[1]);
            const int gz = lodattr_fine_index(lodattr_clamp_lattice(F.o[2] + (int)z, F.n[2]), F.stride, F.dim[2]);
            tile[i] = F.grid[(size_t)gx + (size_t)F.dim[0] * ((size_t)gy + (size_t)F.dim[1] * (size_t)gz)];
        }
    }
    const float base[3] = {lodattr_ao_coord(nd.origin[0], F.stride, 0.0f), lodattr_ao_coord(nd.origin[1], F.stride, 0.0f), lodattr_ao_coord(nd.origin[2], F.stride, 0.0f)};
    ao_chunks<INDEXED, kAoStrided>(recs, first, count, direct, base, a.march, F, a.out, rec, outw);
    if (!a.skirt_out) return;
    // the node's own quads, with the tile where there is one (nothing has overwritten it)
    const uint32_t q0 = (uint32_t)a.node_offsets[node] / 2u, q1 = (uint32_t)a.node_offsets[node + 1] / 2u;
    for (uint32_t q = q0 + threadIdx.x; q < q1 && q < a.n_quads; q += 256u) {
        if (direct) lod_ao_quad<kAoStrided>(a, F, nd, q);
        else lod_ao_quad<kAoTile>(a, F, nd, q);
    }
}

// the skirts in a pass of their own (vtmc_debug_lodattr_skirts_in_node(0)): a lane per quad, every fetch from the grid
__global__ __launch_bounds__(256) void lod_ao_skirt_kernel(LodAoArgs a)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.n_quads) return;
    const uint32_t b = a.skirts[38 * (size_t)q + 18];
    const vtmc_lod_node nd = a.nodes[b < a.n_nodes ? b : a.n_nodes - 1];
    lod_ao_quad<kAoStrided>(a, lod_ao_field(a, nd, nullptr), nd, q);
}

// where the local positions of a level-of-detail result lie (material_filter.h): node b's (o, s) in place of the BlockMap's 8 b
struct MaterialOfNodes {
    const vtmc_lod_node *nodes;
    __device__ __forceinline__ uint2 operator()(const MaterialVertexArgs &a, uint32_t b, float p0, float p1, float p2) const
    {
        const vtmc_lod_node nd = nodes[b < a.map.n_blocks ? b : a.map.n_blocks - 1];
        const int s = 1 << nd.level;
        return material_pack(material_taps_at(a, lodattr_material_coord(nd.origin[0], p0, s), lodattr_material_coord(nd.origin[1], p1, s),
                                              lodattr_material_coord(nd.origin[2], p2, s)));
    }
};

__global__ __launch_bounds__(256) void lod_material_soup_kernel(const uint32_t *__restrict__ tris, uint32_t n_tris, uint2 *__restrict__ out, MaterialVertexArgs a,
                                                                MaterialOfNodes where)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 19];
    material_soup_tile(tris, n_tris, out, a, where, rec);
}

__global__ __launch_bounds__(256) void lod_material_indexed_kernel(const uint32_t *__restrict__ verts, uint32_t n_verts, const uint32_t *__restrict__ voffsets,
                                                                   uint2 *__restrict__ out, MaterialVertexArgs a, MaterialOfNodes where)
{
    __shared__ __attribute__((aligned(16))) uint32_t rec[kMatTile * 6];
    __shared__ uint32_t range[2];
    material_indexed_tile(verts, n_verts, voffsets, out, a, where, rec, range);
}

// a lane per quad: the weights of corners 0 (b) and 1 (a) of skirt record 2q to the six corners of records 2q and 2q + 1
__global__ __launch_bounds__(256) void lod_material_skirt_kernel(const uint32_t *__restrict__ skirts, uint32_t n_quads, uint2 *__restrict__ out, MaterialVertexArgs a,
                                                                 MaterialOfNodes where)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_quads) return;
    const uint32_t *r = skirts + 38 * (size_t)q;
    uint2 w[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) w[c] = where(a, r[18], __uint_as_float(r[3 * c]), __uint_as_float(r[3 * c + 1]), __uint_as_float(r[3 * c + 2]));
#pragma unroll
    for (int c = 0; c < 6; ++c) out[6 * (size_t)q + c] = w[lodattr_skirt_source(c)];
}

static bool lod_result(const vtmc_ctx *ctx) { return ctx->result.valid && ctx->result.source == ResultSource::TerrainLod; }

// The call's view of the result: refuses what is not a level-of-detail extract's; *n_skirt_records = -1 when the result has no skirts
static int lodattr_gate(vtmc_ctx *ctx, const char *who, int64_t *n_skirt_records)
{
    if (!lod_result(ctx)) return fail(ctx, VTMC_ERR_NO_RESULT, "%s: the context's current result is not a level-of-detail extract's", who);
    if ((size_t)ctx->result.blocks != ctx->lod_nodes.size())
        return fail(ctx, VTMC_ERR_DEVICE, "%s: the result holds %d blocks for %zu nodes", who, ctx->result.blocks, ctx->lod_nodes.size());
    const VtmcTriStream &sk = ctx->lodskirt.pass;
    *n_skirt_records = sk.epoch == ctx->result.epoch ? sk.n : -1;
    return VTMC_OK;
}

// what a compute call leaves behind: the mesh target current, the skirt target current when the result had skirts
static void lodattr_publish(vtmc_ctx *ctx, int attribute, int64_t n, int64_t n_skirt_records, int64_t *n_vertices, int64_t *n_skirt_vertices)
{
    VertexAttr *v = ctx->lodattr.values[attribute];
    v[VTMC_LODATTR_MESH].n = n, v[VTMC_LODATTR_MESH].epoch = ctx->result.epoch;
    v[VTMC_LODATTR_SKIRTS].n = n_skirt_records < 0 ? 0 : 3 * n_skirt_records;
    v[VTMC_LODATTR_SKIRTS].epoch = n_skirt_records < 0 ? 0 : ctx->result.epoch;
    if (n_vertices) *n_vertices = n;
    if (n_skirt_vertices) *n_skirt_vertices = v[VTMC_LODATTR_SKIRTS].n;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_lod_material_vertices(vtmc_ctx *ctx, int64_t *n_vertices, int64_t *n_skirt_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    int64_t ns = -1;
    if (int rc = lodattr_gate(ctx, "lod_material_vertices", &ns)) return rc;
    if (!ctx->mat_c) return fail(ctx, VTMC_ERR_NO_RESULT, "lod_material_vertices before material_init");
    const VtmcResult &res = ctx->result;
    const int64_t n = res.vertices();
    VertexAttr *v = ctx->lodattr.values[VTMC_LODATTR_MATERIAL];
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    MaterialVertexArgs a{};
    const int cells[3] = {ctx->tshape.dim_x - 2, ctx->tshape.dim_y - 2, ctx->tshape.dim_z - 2};
    a.layer = (const uint2 *)ctx->material.p;
    a.C = ctx->mat_c;
    material_vertex_scale(cells, a.C, a.s);
    a.map = BlockMap{};
    a.map.n_blocks = (uint32_t)res.blocks;
    const MaterialOfNodes where{(const vtmc_lod_node *)ctx->lod_nodes_dev.p};
    if (n > 0) {
        if (int rc = ensure(ctx, v[VTMC_LODATTR_MESH].values, (size_t)n * VTMC_MATERIAL_CHANNELS)) return rc;
        uint2 *out = (uint2 *)v[VTMC_LODATTR_MESH].values.p;
        if (res.indexed) {
            const uint32_t V = (uint32_t)res.verts;
            VTMC_HIP(ctx, launch(lod_material_indexed_kernel, dim3((V + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->verts.p, V,
                                 (const uint32_t *)ctx->voffsets.p, out, a, where));
        } else {
            const uint32_t T = (uint32_t)res.tris;
            VTMC_HIP(ctx, launch(lod_material_soup_kernel, dim3((T + kMatTile - 1) / kMatTile), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->tris.p, T, out, a, where));
        }
    }
    if (ns > 0) {
        if (int rc = ensure(ctx, v[VTMC_LODATTR_SKIRTS].values, (size_t)(3 * ns) * VTMC_MATERIAL_CHANNELS)) return rc;
        VTMC_HIP(ctx, launch(lod_material_skirt_kernel, lanes256(ns / 2), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->lodskirt.pass.records.p, (uint32_t)(ns / 2),
                             (uint2 *)v[VTMC_LODATTR_SKIRTS].values.p, a, where));
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lodattr_publish(ctx, VTMC_LODATTR_MATERIAL, n, ns, n_vertices, n_skirt_vertices);
    return VTMC_OK;
}

int32_t vtmc_lod_ao_vertices(vtmc_ctx *ctx, const vtmc_ao_params *params, int64_t *n_vertices, int64_t *n_skirt_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!params) return fail(ctx, VTMC_ERR_INVALID_ARG, "lod_ao_vertices: params is null");
    int64_t ns = -1;
    if (int rc = lodattr_gate(ctx, "lod_ao_vertices", &ns)) return rc;
    if (const char *fault = ao_params_fault(*params, ctx->tshape.scale)) return fail(ctx, VTMC_ERR_INVALID_ARG, "lod_ao_vertices: %s", fault);
    const VtmcResult &res = ctx->result;
    const int64_t n = res.vertices();
    VtmcLodAttr &la = ctx->lodattr;
    VertexAttr *v = la.values[VTMC_LODATTR_AO];
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure(ctx, la.stats, 2 * sizeof(uint32_t))) return rc;
    VTMC_HIP(ctx, hipMemsetAsync(la.stats.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    VTMC_HIP(ctx, ctx->lodattr_clock.begin());   // disarmed: a result without vertices leaves it so
    if (n > 0 && res.active > 0) {
        if (int rc = ensure(ctx, v[VTMC_LODATTR_MESH].values, ((size_t)n + 3) & ~(size_t)3)) return rc;
        if (ns > 0)
            if (int rc = ensure(ctx, v[VTMC_LODATTR_SKIRTS].values, ((size_t)(3 * ns) + 3) & ~(size_t)3)) return rc;
        const AoTables tb = ao_tables(*params, ctx->tshape.scale);
        LodAoArgs a{};
        a.grid = (const float *)ctx->terrain.p;
        a.dim[0] = ctx->tshape.dim_x, a.dim[1] = ctx->tshape.dim_y, a.dim[2] = ctx->tshape.dim_z;
        a.active = (const BlockDesc *)ctx->active.p;
        a.nodes = (const vtmc_lod_node *)ctx->lod_nodes_dev.p;
        a.n_nodes = (uint32_t)res.blocks;
        a.reach = tb.reach, a.extent = tb.extent;
        a.d_extent = FastDiv((unsigned)tb.extent);
        a.march = ao_march(*params, tb);
        a.direct_max = (uint32_t)(la.direct_max >= 0 ? la.direct_max : kAoDirectMax);
        a.stats = (uint32_t *)la.stats.p;
        a.out = (uint8_t *)v[VTMC_LODATTR_MESH].values.p;
        LodAoArgs sk = a;   // the skirts' view; the nodes' kernel gets it only when it takes the quads itself
        if (ns > 0) {
            sk.skirts = (const uint32_t *)ctx->lodskirt.pass.records.p;
            sk.node_offsets = (const int32_t *)ctx->lodskirt.pass.block_offsets.p;
            sk.n_quads = (uint32_t)(ns / 2);
            sk.skirt_out = (uint8_t *)v[VTMC_LODATTR_SKIRTS].values.p;
        }
        const bool in_node = ns > 0 && la.skirts_in_node;
        const size_t lds = ao_tile_bytes(tb.extent);
        VTMC_HIP(ctx, ctx->lodattr_clock.mark(0, ctx->stream));
        if (res.indexed) VTMC_HIP(ctx, launch(lod_ao_kernel<true>, dim3(res.active), dim3(256), lds, ctx->stream, (const uint32_t *)ctx->verts.p, in_node ? sk : a));
        else VTMC_HIP(ctx, launch(lod_ao_kernel<false>, dim3(res.active), dim3(256), lds, ctx->stream, (const uint32_t *)ctx->tris.p, in_node ? sk : a));
        VTMC_HIP(ctx, ctx->lodattr_clock.mark(1, ctx->stream));
        if (ns > 0 && !in_node) VTMC_HIP(ctx, launch(lod_ao_skirt_kernel, lanes256(ns / 2), dim3(256), 0, ctx->stream, sk));
        VTMC_HIP(ctx, ctx->lodattr_clock.mark(2, ctx->stream));
        ctx->lodattr_clock.arm();
    }
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lodattr_publish(ctx, VTMC_LODATTR_AO, n, ns, n_vertices, n_skirt_vertices);
    return VTMC_OK;
}

int32_t vtmc_lodattr_info(vtmc_ctx *ctx, int32_t attribute, int64_t *n_vertices, int64_t *n_skirt_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (const char *fault = lodattr_selector_fault(attribute, VTMC_LODATTR_MESH)) return fail(ctx, VTMC_ERR_INVALID_ARG, "lodattr_info: %s %d", fault, attribute);
    const VertexAttr *v = ctx->lodattr.values[attribute];
    if (!lod_result(ctx) || v[VTMC_LODATTR_MESH].epoch != ctx->result.epoch)
        return fail(ctx, VTMC_ERR_NO_RESULT, "lodattr_info: no values of the current result (call vtmc_lod_material_vertices / vtmc_lod_ao_vertices)");
    if (n_vertices) *n_vertices = v[VTMC_LODATTR_MESH].n;
    if (n_skirt_vertices) *n_skirt_vertices = v[VTMC_LODATTR_SKIRTS].epoch == ctx->result.epoch ? v[VTMC_LODATTR_SKIRTS].n : 0;
    return VTMC_OK;
}

int32_t vtmc_lodattr_read(vtmc_ctx *ctx, int32_t attribute, int32_t target, uint8_t *dst, int64_t capacity_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (const char *fault = lodattr_selector_fault(attribute, target)) return fail(ctx, VTMC_ERR_INVALID_ARG, "lodattr_read: %s (%d, %d)", fault, attribute, target);
    return attr_read(ctx, ctx->lodattr.values[attribute][target], "lodattr_read: no values of this target for the current result and its skirts",
                     lodattr_bytes_per_vertex(attribute), dst, capacity_vertices);
}

int32_t vtmc_lodattr_device_results(vtmc_ctx *ctx, int32_t attribute, int32_t target, const uint8_t **d_values, int64_t *n_vertices)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (const char *fault = lodattr_selector_fault(attribute, target))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "lodattr_device_results: %s (%d, %d)", fault, attribute, target);
    return attr_device_results(ctx, ctx->lodattr.values[attribute][target], "lodattr_device_results: no values of this target for the current result and its skirts",
                               d_values, n_vertices);
}

// Not part of the ABI (tests, tools/lodattr_bench.py): counts[0] = workgroups of the last vtmc_lod_ao_vertices that staged a tile,
// counts[1] = those that took the direct route; direct_max >= 0 sets the vertex count up to which a node goes direct, -1 restores the
// default, -2 leaves it.
int32_t vtmc_debug_lodattr_routes(vtmc_ctx *ctx, uint32_t counts[2], int32_t direct_max)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (direct_max >= -1) ctx->lodattr.direct_max = direct_max;
    if (counts) {
        counts[0] = counts[1] = 0u;
        if (ctx->lodattr.stats.p) {
            VTMC_HIP(ctx, hipSetDevice(ctx->device));
            VTMC_HIP(ctx, hipMemcpy(counts, ctx->lodattr.stats.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    }
    return VTMC_OK;
}

// Not part of the ABI (tests, tools/lodattr_bench.py): whether later vtmc_lod_ao_vertices calls hand a node's skirt quads to the node's
// own workgroup (1, the library's choice) or to a pass of their own (0).
int32_t vtmc_debug_lodattr_skirts_in_node(vtmc_ctx *ctx, int32_t on)
{
    if (!ctx || (on != 0 && on != 1)) return VTMC_ERR_INVALID_ARG;
    ctx->lodattr.skirts_in_node = on != 0;
    return VTMC_OK;
}

// Not part of the ABI (tools/lodattr_bench.py): device time of the last vtmc_lod_ao_vertices that launched kernels, ms[0] the nodes'
// kernel, ms[1] the skirts' own pass (0 without one).
int32_t vtmc_debug_lodattr_ms(vtmc_ctx *ctx, float ms[2])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->lodattr_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_lodattr_ms before an occlusion call that launched kernels");
    if (int rc = ctx->lodattr_clock.sync_last(ctx)) return rc;
    if (int rc = ctx->lodattr_clock.elapsed(ctx, 0, 1, &ms[0])) return rc;
    return ctx->lodattr_clock.elapsed(ctx, 1, 2, &ms[1]);
}

}  // extern "C"
