// ao_march.h -- the occlusion march of include/vtmc.h's rule (vtmc_ao_vertices) as device code, shared by the two passes that run it:
// terrain_ao.hip on the blocks of a terrain extract and terrain_lodattr.hip on the nodes of a level-of-detail extract.  One piece of
// code, so both follow the rule operation by operation: fetch()'s per-axis step (ao_axis), the trilinear sample (ao_fetch), the unrolled
// 26 directions and a vertex's byte (ao_vertex), and the pass of a workgroup over the records of its block or node (ao_chunks: the record
// loader of record_tile.h, the chunking, the dword-assembled byte output).  What differs between the two passes is where a sample lies,
// the ROUTE of a fetch:
//   kAoGrid     a lattice that IS the grid: sample i of an axis lies at offset i * stride of that axis.
//   kAoTile     the workgroup's LDS tile of E^3 samples whose first one is lattice sample F.o: the same for both passes, since the tile
//               holds lattice samples whatever they were gathered from.
//   kAoStrided  the sample lattice of a level-of-detail node of stride s, read from the grid itself: lattice sample i lies at grid index
//               min(i * s, dim - 1), so the upper neighbour of i0 is min((i0 + 1) * s, dim - 1) -- not i0 * s + s, and not the lower
//               offset plus one: each axis carries both offsets.
// Device code only.
#ifndef VTMC_AO_MARCH_H
#define VTMC_AO_MARCH_H
#include "terrain_ao.h"
#include "terrain_lodattr.h"   // lodattr_fine_index: kAoStrided's index clamp
#include "record_tile.h"
#include <cmath>
#include <type_traits>

namespace vtmc {

constexpr int kAoSoupChunk = 128;     // triangles (384 vertices) per pass of a workgroup: 9.7 KB of records, so tile + records stay under 53 KB and
                                      // three workgroups share a CU's 160 KB at the largest radius
constexpr int kAoIndexedChunk = 256;  // vertices per pass
constexpr int kAoDirectMax = 12;      // vertices up to which a block's workgroup reads global memory directly

constexpr int kAoGrid = 0, kAoTile = 1, kAoStrided = 2;

// the per-call tables of terrain_ao.h as a kernel argument
struct AoMarch {
    int steps;
    float strength;
    float hd[3][VTMC_AO_MAX_STEPS];
    float fall[VTMC_AO_MAX_STEPS];
};

inline AoMarch ao_march(const vtmc_ao_params &p, const AoTables &tb)
{
    AoMarch m{};
    m.steps = p.steps;
    m.strength = p.strength;
    for (int s = 0; s < VTMC_AO_MAX_STEPS; ++s) {
        m.fall[s] = tb.fall[s];
        for (int c = 0; c < 3; ++c) m.hd[c][s] = tb.hd[c][s];
    }
    return m;
}

// where the workgroup's samples lie: the tile (origin o in lattice samples, E per axis), and the lattice of n samples per axis over the
// grid; kAoStrided alone reads stride and dim (the grid's samples per axis), and kAoGrid has n == dim
struct AoField {
    const float *tile;
    const float *__restrict__ grid;
    int o[3];
    int E;
    int n[3];
    int stride;
    int dim[3];
};

struct AoAxis {
    uint32_t off;  // the lower sample's offset along this axis, multiplied out
    uint32_t up;   // kAoStrided: the upper sample's
    float f;
};

// the rule's per-axis step of fetch(): the clamped coordinate cut into the sample below it and the weight
template <int ROUTE>
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
    a.up = 0u;
    if (ROUTE == kAoTile) {
        a.off = (uint32_t)(i0 - F.o[k]) * (k == 0 ? 1u : (k == 1 ? (uint32_t)F.E : (uint32_t)(F.E * F.E)));
    } else if (ROUTE == kAoGrid) {
        a.off = (uint32_t)i0 * (k == 0 ? 1u : (k == 1 ? (uint32_t)F.n[0] : (uint32_t)F.n[0] * (uint32_t)F.n[1]));
    } else {
        const uint32_t pitch = k == 0 ? 1u : (k == 1 ? (uint32_t)F.dim[0] : (uint32_t)F.dim[0] * (uint32_t)F.dim[1]);
        a.off = (uint32_t)lodattr_fine_index(i0, F.stride, F.dim[k]) * pitch;
        a.up = (uint32_t)lodattr_fine_index(i0 + 1, F.stride, F.dim[k]) * pitch;
    }
    return a;
}

template <int ROUTE>
__device__ __forceinline__ float ao_fetch(const AoField &F, AoAxis X, AoAxis Y, AoAxis Z)
{
    float v000, v100, v010, v110, v001, v101, v011, v111;
    if (ROUTE == kAoStrided) {
        const float *p = F.grid;
        const size_t y0 = Y.off, y1 = Y.up, z0 = Z.off, z1 = Z.up;
        v000 = p[X.off + y0 + z0], v100 = p[X.up + y0 + z0], v010 = p[X.off + y1 + z0], v110 = p[X.up + y1 + z0];
        v001 = p[X.off + y0 + z1], v101 = p[X.up + y0 + z1], v011 = p[X.off + y1 + z1], v111 = p[X.up + y1 + z1];
    } else {
        const uint32_t sy = ROUTE == kAoTile ? (uint32_t)F.E : (uint32_t)F.n[0];
        const uint32_t sz = ROUTE == kAoTile ? (uint32_t)(F.E * F.E) : (uint32_t)F.n[0] * (uint32_t)F.n[1];
        const float *p = (ROUTE == kAoTile ? F.tile : F.grid) + (size_t)(X.off + Y.off + Z.off);
        v000 = p[0], v100 = p[1], v010 = p[sy], v110 = p[sy + 1];
        v001 = p[sz], v101 = p[sz + 1], v011 = p[sz + sy], v111 = p[sz + sy + 1];
    }
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

// The byte of a vertex at lattice coordinates g with record normal nrm.  The directions are compile-time constants; a component of d that
// is zero contributes +-0 to a sum of the rule, which changes no value the rule goes on to use (c only where c > 0, q only through the
// clamp), so those terms are left out; (+-len) * h[s] is +-hd[s] exactly.
template <int ROUTE>
__device__ __forceinline__ uint32_t ao_vertex(const AoMarch &a, const AoField &F, float gx, float gy, float gz, float n0, float n1, float n2)
{
    const float l = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    if (!(l > 0.0f) || !(l < INFINITY)) return 255u;
    const float N0 = n0 / l, N1 = n1 / l, N2 = n2 / l;
    // the axes a direction leaves alone fetch at the vertex's own coordinate
    const AoAxis X0 = ao_axis<ROUTE>(F, 0, gx), Y0 = ao_axis<ROUTE>(F, 1, gy), Z0 = ao_axis<ROUTE>(F, 2, gz);
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
                const AoAxis X = I ? ao_axis<ROUTE>(F, 0, I > 0 ? gx + hd : gx - hd) : X0;
                const AoAxis Y = J ? ao_axis<ROUTE>(F, 1, J > 0 ? gy + hd : gy - hd) : Y0;
                const AoAxis Z = K ? ao_axis<ROUTE>(F, 2, K > 0 ? gz + hd : gz - hd) : Z0;
                float r = ao_fetch<ROUTE>(F, X, Y, Z);
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

// the LDS a workgroup of ao_chunks needs beside its tile
template <bool INDEXED>
struct AoChunkLds {
    static constexpr uint32_t RD = INDEXED ? 6u : 19u;   // dwords per record
    static constexpr uint32_t CHUNK = INDEXED ? (uint32_t)kAoIndexedChunk : (uint32_t)kAoSoupChunk;
    static constexpr uint32_t CHUNK_VERTS = INDEXED ? CHUNK : 3u * CHUNK;
    static constexpr uint32_t REC_WORDS = CHUNK * RD + 4, OUT_WORDS = CHUNK_VERTS / 4 + 2;
};

// The pass of a workgroup of 256 over the `count` records from `first` of its block or node: the bytes of their vertices to `out`.
// RD = dwords per record: 19 (soup, three vertices: corner c has its position at dwords 3c.. and its normal at 9 + 3c..) or 6 (indexed:
// position, normal).  base: the lattice coordinate of the block's or node's local origin; `direct`: no tile was staged, every vertex
// reads the grid through FAR.  Records go through LDS in 16-byte pieces, a chunk at a time; a first record is not 16-byte aligned in
// general, so the load starts at the aligned piece below it.  The bytes of a chunk are assembled in LDS at the byte phase they have in
// the output and leave as whole dwords; only the first and the last dword of a chunk, shared with the neighbours, leave byte by byte.
// The caller's __syncthreads() behind the tile is the one behind the first chunk's records.
template <bool INDEXED, int FAR>
__device__ __forceinline__ void ao_chunks(const uint32_t *__restrict__ recs, uint32_t first, uint32_t count, bool direct, const float base[3], const AoMarch &a,
                                          const AoField &F, uint8_t *__restrict__ out, uint32_t *rec, uint32_t *outw)
{
    constexpr uint32_t RD = AoChunkLds<INDEXED>::RD, CHUNK = AoChunkLds<INDEXED>::CHUNK;
    const uint32_t vpr = INDEXED ? 1u : 3u;
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
            const float gx = base[0] + p0, gy = base[1] + p1, gz = base[2] + p2;
            // the tile holds every fetch of a vertex inside its block's cells, p in [0, 8]; any other record reads the grid itself
            const bool inside = p0 >= 0.0f && p0 <= 8.0f && p1 >= 0.0f && p1 <= 8.0f && p2 >= 0.0f && p2 <= 8.0f;
            uint32_t val;
            if (!direct && inside) val = ao_vertex<kAoTile>(a, F, gx, gy, gz, n0, n1, n2);
            else val = ao_vertex<FAR>(a, F, gx, gy, gz, n0, n1, n2);
            bytes[phase + v] = (uint8_t)val;
        }
        __syncthreads();
        // dword w of outw is dword w of the output counted from the aligned byte below v0
        uint8_t *dst = out + (v0 - phase);
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
#endif
