// material_filter.h -- the material layer's trilinear filter, shared by the passes that read the layer at points of the surface (the vertex
// weights, terrain_material.hip, and the material filter of the scatter, terrain_scatter.hip: one piece of code, so both follow the rule
// of include/vtmc.h, vtmc_material_vertices, operation by operation), and the block mapping of a result: BlockMap, which block_map() fills
// from the result's BlockSpace for every pass that turns a block index into (bx, by, bz) (those two and terrain_ao.hip), and the search
// of a block in the per-block offsets (material_block_of: terrain_material.hip and tri_stream_kernels.h), and the vertex pass over a tile of
// records (material_soup_tile, material_indexed_tile: terrain_material.hip on a terrain extract, terrain_lodattr.hip on a level-of-detail
// result).  Device code but for block_map().
#ifndef VTMC_MATERIAL_FILTER_H
#define VTMC_MATERIAL_FILTER_H
#include "vtmc_internal.h"
#include "record_tile.h"
#include <cmath>

namespace vtmc {

// how the blocks of a result map to (bx, by, bz)
struct BlockMap {
    const int *list;  // device (bx, by, bz) triples of the dirty list, or null: every block, b = bx + nbx * (by + nby * bz)
    uint32_t n_blocks;
    int nbx, nby;
    FastDiv d_nbx, d_nby;
};

// the mapping of a result of `blocks` blocks over `sp`
inline BlockMap block_map(const BlockSpace &sp, int blocks) { return BlockMap{sp.list, (uint32_t)blocks, sp.nbx, sp.nby, sp.d_nbx, sp.d_nby}; }

struct MaterialVertexArgs {
    const uint2 *layer;  // C^3 texels, x fastest
    int C;
    float s[3];       // texels per cell, per axis
    BlockMap map;
};

// (bx, by, bz) of block b, an index into the dirty list
__device__ __forceinline__ void material_block(const BlockMap &a, uint32_t b, int &bx, int &by, int &bz)
{
    if (b >= a.n_blocks) b = a.n_blocks - 1;  // never taken for a result of the library; keeps a foreign record inside the list
    if (a.list) {
        bx = a.list[3 * (size_t)b], by = a.list[3 * (size_t)b + 1], bz = a.list[3 * (size_t)b + 2];
    } else {
        const unsigned q = a.d_nbx.quot(b);
        bx = (int)(b - q * (unsigned)a.nbx);
        bz = (int)a.d_nby.quot(q);
        by = (int)(q - (unsigned)bz * (unsigned)a.nby);
    }
}

// the largest b in [lo, hi] with off[b] <= v (off[lo] <= v holds): the block whose range of the offsets holds v, empty blocks skipped
__device__ __forceinline__ uint32_t material_block_of(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t v)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tx = g * s - 0.5 cut into the texel below it, wrapped as a Repeat texture, the one after it, and the weight
__device__ __forceinline__ void material_axis(float g, float s, int C, int &i0, int &i1, float &f)
{
    float t = g * s;
    t = t - 0.5f;
    i0 = (int)floorf(t);
    f = t - (float)i0;
    // ((i0 % C) + C) % C; a vertex of the terrain gives i0 in -1..C-1, which needs no division
    if (i0 == -1) i0 = C - 1;
    else if ((unsigned)i0 >= (unsigned)C) i0 = ((i0 % C) + C) % C;
    i1 = i0 + 1 == C ? 0 : i0 + 1;
}

__device__ __forceinline__ float material_channel(uint2 w, int k) { return (float)(((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xffu); }

// a + (b - a) * f per channel k of two texels
__device__ __forceinline__ float material_lerp(uint2 a, uint2 b, int k, float f)
{
    const float x = material_channel(a, k), y = material_channel(b, k);
    return x + (y - x) * f;
}

// the eight texels around a point and its three weights
struct MaterialTaps {
    uint2 m000, m100, m010, m110, m001, m101, m011, m111;
    float fx, fy, fz;
};

// the taps of the fine grid coordinate g
__device__ __forceinline__ MaterialTaps material_taps_at(const MaterialVertexArgs &a, float gx, float gy, float gz)
{
    int i0, i1, j0, j1, k0, k1;
    MaterialTaps t;
    material_axis(gx, a.s[0], a.C, i0, i1, t.fx);
    material_axis(gy, a.s[1], a.C, j0, j1, t.fy);
    material_axis(gz, a.s[2], a.C, k0, k1, t.fz);
    const int C = a.C;
    const int r00 = C * (j0 + C * k0), r10 = C * (j1 + C * k0), r01 = C * (j0 + C * k1), r11 = C * (j1 + C * k1);
    const uint2 *__restrict__ m = a.layer;
    t.m000 = m[r00 + i0], t.m100 = m[r00 + i1], t.m010 = m[r10 + i0], t.m110 = m[r10 + i1];
    t.m001 = m[r01 + i0], t.m101 = m[r01 + i1], t.m011 = m[r11 + i0], t.m111 = m[r11 + i1];
    return t;
}

// the taps of block-local position p of block (bx, by, bz)
__device__ __forceinline__ MaterialTaps material_taps(const MaterialVertexArgs &a, int bx, int by, int bz, float p0, float p1, float p2)
{
    return material_taps_at(a, (float)(8 * bx) + p0, (float)(8 * by) + p1, (float)(8 * bz) + p2);
}

// the byte of channel k: along x, then y, then z, rounded ties to even
__device__ __forceinline__ uint32_t material_filter_channel(const MaterialTaps &t, int k)
{
    const float a00 = material_lerp(t.m000, t.m100, k, t.fx), a10 = material_lerp(t.m010, t.m110, k, t.fx);
    const float a01 = material_lerp(t.m001, t.m101, k, t.fx), a11 = material_lerp(t.m011, t.m111, k, t.fx);
    const float b0 = a00 + (a10 - a00) * t.fy, b1 = a01 + (a11 - a01) * t.fy;
    const float q = b0 + (b1 - b0) * t.fz;
    return (uint32_t)rintf(q) & 0xffu;
}

// the 8 weights of the taps
__device__ __forceinline__ uint2 material_pack(const MaterialTaps &t)
{
    uint32_t out[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k >> 2] |= material_filter_channel(t, k) << (8 * (k & 3));
    return make_uint2(out[0], out[1]);
}

// the 8 weights of a vertex at block-local position p of block b (an index into the dirty list)
__device__ __forceinline__ uint2 material_weights(const MaterialVertexArgs &a, uint32_t b, float p0, float p1, float p2)
{
    int bx, by, bz;
    material_block(a.map, b, bx, by, bz);
    return material_pack(material_taps(a, bx, by, bz, p0, p1, p2));
}

// Where the local positions of a result's records lie, for the vertex pass below: a functor gives the weights of local position p of block
// (or node) b.  MaterialOfBlocks is a terrain extract's, through the BlockMap; terrain_lodattr.hip has the one of a level-of-detail result.
struct MaterialOfBlocks {
    __device__ __forceinline__ uint2 operator()(const MaterialVertexArgs &a, uint32_t b, float p0, float p1, float p2) const { return material_weights(a, b, p0, p1, p2); }
};

// The vertex pass over a result's records, one workgroup of 256 threads per tile of kMatTile records (triangles or vertices): the scheme
// is written down in terrain_material.hip.
constexpr int kMatTile = 256;

// soup: tris = T records of 19 dwords (vtmc_triangle); out[3t + v] = the weights of corner v of triangle t.  rec: kMatTile * 19 dwords of LDS
template <class Where>
__device__ __forceinline__ void material_soup_tile(const uint32_t *__restrict__ tris, uint32_t n_tris, uint2 *__restrict__ out, const MaterialVertexArgs &a,
                                                   const Where &where, uint32_t *rec)
{
    const uint32_t t0 = blockIdx.x * (uint32_t)kMatTile;
    const uint32_t nt = n_tris - t0 < (uint32_t)kMatTile ? n_tris - t0 : (uint32_t)kMatTile;
    load_record_tile(rec, tris + (size_t)t0 * 19, nt * 19);  // tile base: 256 * 76 bytes per tile, 16-byte aligned
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < 3 * nt; v += 256) {
        const uint32_t t = v / 3, c = v - 3 * t;
        const uint32_t *r = rec + 19 * t;
        const uint2 w = where(a, r[18], __uint_as_float(r[3 * c]), __uint_as_float(r[3 * c + 1]), __uint_as_float(r[3 * c + 2]));
        out[(size_t)t0 * 3 + v] = w;
    }
}

// indexed: verts = V records of 6 dwords (vtmc_vertex), voffsets = the n_blocks + 1 per-block vertex offsets; out[v] = the weights of
// vertex v.  Two lanes find the blocks of the tile's first and last vertex; every lane then searches only between them.  rec: kMatTile * 6
// dwords of LDS, range: 2
template <class Where>
__device__ __forceinline__ void material_indexed_tile(const uint32_t *__restrict__ verts, uint32_t n_verts, const uint32_t *__restrict__ voffsets,
                                                      uint2 *__restrict__ out, const MaterialVertexArgs &a, const Where &where, uint32_t *rec, uint32_t *range)
{
    const uint32_t v0 = blockIdx.x * (uint32_t)kMatTile;
    const uint32_t nv = n_verts - v0 < (uint32_t)kMatTile ? n_verts - v0 : (uint32_t)kMatTile;
    load_record_tile(rec, verts + (size_t)v0 * 6, nv * 6);  // tile base: 256 * 24 bytes per tile, 16-byte aligned
    if (threadIdx.x < 2) range[threadIdx.x] = material_block_of(voffsets, 0u, a.map.n_blocks - 1, threadIdx.x ? v0 + nv - 1 : v0);
    __syncthreads();
    if (threadIdx.x < nv) {
        const uint32_t v = v0 + threadIdx.x;
        const uint32_t b = material_block_of(voffsets, range[0], range[1], v);
        const uint32_t *r = rec + 6 * threadIdx.x;
        out[v] = where(a, b, __uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]));
    }
}

}  // namespace vtmc
#endif
