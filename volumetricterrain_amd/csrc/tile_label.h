// tile_label.h -- the tile-local connected-component labelling of a box of samples that terrain_fragments.hip (the solid samples) and
// terrain_water.hip (the open, dry samples under a level) share: the bodies of its three kernels, with the predicate a template
// parameter.  A file that uses them wraps each in a kernel of its own; everything is forced inline.  (terrain_fragments.hip keeps its
// own copy of phase 1: through the template its kernel compiles to different code, DESIGN.md.)  Labels are box-linear int32 indices (1026^3 < 2^31); box-linear order is grid-index order, so "root =
// smallest index" is the sample of smallest grid index.  Three phases, a kernel boundary between every phase and the next one's reads:
//   1. label_local    tiles of 64 x 8 x 8 samples (long in x, the stride-1 axis: a wave reads 256 contiguous bytes), union-find in LDS
//                     over the runs along x (a run is one ballot); leaves every sample of the predicate pointing at the smallest index of
//                     its piece of the tile, -1 in the others.  The one evaluation of the predicate.
//   2. label_merge    the samples on a tile's low faces join their neighbour across the face: union by smaller index on the global
//                     parent array.
//   3. the flatten    every sample to its root: each file's own kernel, fused with what it counts there.
// VISIBILITY and the BOUNDS OF EVERY LOOP: terrain_fragments.hip and union_find.h.  Device code only.
#ifndef VTMC_TILE_LABEL_H
#define VTMC_TILE_LABEL_H
#include "vtmc_ctx.h"
#include "union_find.h"

namespace vtmc {

constexpr int kTileX = 64, kTileY = 8, kTileZ = 8, kTileSamples = kTileX * kTileY * kTileZ;

// box-linear index of sample (ix, iy, iz) of the box; below 2^31 for every box of a grid
__device__ __forceinline__ int frag_index(const TerrainBox &b, int ix, int iy, int iz) { return ix + b.dx * (iy + b.dy * iz); }

static dim3 tile_grid(const TerrainBox &b) { return dim3((unsigned)((b.dx + kTileX - 1) / kTileX), (unsigned)((b.dy + kTileY - 1) / kTileY), (unsigned)((b.dz + kTileZ - 1) / kTileZ)); }

// Phase 1.  64 x 4 threads; thread (tx, tq) owns the 16 samples (tx, r & 7, r >> 3), r = tq + 4 k, of the tile, so a wave holds one row
// of 64 samples along x at a time.  A row's mask is one ballot: every sample starts out pointing at the first sample of its run
// along x (no union along x at all), and two neighbouring rows need one union per stretch in which both hold, made by the
// stretch's first lane -- within a stretch both rows are one run each.  pred(ix, iy, iz): is this sample of the box in the graph;
// store(j, label): the label of box sample j, -1 outside the graph.
template <class Pred, class Store>
__device__ __forceinline__ void label_local(int *__restrict__ flag, const TerrainBox &b, Pred pred, Store store)
{
    __shared__ int L[kTileSamples];
    __shared__ unsigned long long M[kTileY * kTileZ];   // the mask of row r
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int tx = threadIdx.x, tq = threadIdx.y;
    const int ix = blockIdx.x * kTileX + tx, y0 = blockIdx.y * kTileY, z0 = blockIdx.z * kTileZ;
    unsigned solid = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        bool s = false;
        if (ix < b.dx && y0 + ly < b.dy && z0 + lz < b.dz) s = pred(ix, y0 + ly, z0 + lz);
        const unsigned long long mask = __ballot(s);
        if (tx == 0) M[r] = mask;
        const unsigned long long air_below = ~mask & ((1ull << tx) - 1ull);   // the lanes below tx that are not in the graph
        L[li] = s ? kTileX * r + (air_below ? 64 - __clzll((long long)air_below) : 0) : -1;
        solid |= (unsigned)s << k;
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        if (!(solid >> k & 1)) continue;
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        const unsigned long long here = M[r];
        if (ly > 0) {
            const unsigned long long both = here & M[r - 1];
            if ((both >> tx & 1) && !(tx > 0 && (both >> (tx - 1) & 1))) uf_union<kScope, false>(L, li, li - kTileX, kTileSamples, flag);
        }
        if (lz > 0) {
            const unsigned long long both = here & M[r - kTileY];
            if ((both >> tx & 1) && !(tx > 0 && (both >> (tx - 1) & 1))) uf_union<kScope, false>(L, li, li - kTileX * kTileY, kTileSamples, flag);
        }
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        if (!(ix < b.dx && y0 + ly < b.dy && z0 + lz < b.dz)) continue;
        int label = -1;
        if (solid >> k & 1) {
            const int root = uf_find<kScope>(L, li, kTileSamples, flag);
            // a failed find leaves the sample its own root: the flag is set, nothing reads the labels
            const int rl = root < 0 ? li : root;
            label = frag_index(b, blockIdx.x * kTileX + (rl & (kTileX - 1)), y0 + (rl / kTileX & (kTileY - 1)), z0 + rl / (kTileX * kTileY));
        }
        store(frag_index(b, ix, y0 + ly, z0 + lz), label);
    }
}

// The walk of the kernels below: 64 x 4 threads, one sample per thread, a wave is 64 samples along x of one row; grid = (x segments,
// y quads, z planes).
struct RowThread {
    int ix, iy, iz;
    __device__ __forceinline__ RowThread() : ix(blockIdx.x * 64 + threadIdx.x), iy(blockIdx.y * 4 + threadIdx.y), iz(blockIdx.z) {}
    __device__ __forceinline__ bool inside(const TerrainBox &b) const { return ix < b.dx && iy < b.dy; }
};

static dim3 row_grid(const TerrainBox &b) { return dim3((unsigned)((b.dx + 63) / 64), (unsigned)((b.dy + 3) / 4), (unsigned)b.dz); }

template <class... Params, class... Args>
static hipError_t launch_rows(void (*kernel)(Params...), const TerrainBox &b, hipStream_t stream, Args... args)
{
    return launch(kernel, row_grid(b), dim3(64, 4, 1), 0, stream, args...);
}

// Phase 2, on the row walk.  Only rows on a low face of their tile load anything.  A wave is the 64 samples of one tile's row, and within
// a tile neighbours along x are joined already, so across a y or z face one union per stretch in which both rows are in the graph is enough
// (its first lane makes it); across an x face the row's first lane joins its neighbour.  fx, fy, fz are the same for every lane of a wave.
__device__ __forceinline__ void label_merge(int *__restrict__ P, int *__restrict__ flag, const TerrainBox &b, int n)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const RowThread t;
    const int lane = threadIdx.x;
    const bool row = t.iy < b.dy;
    const bool fx = row && blockIdx.x > 0, fy = row && t.iy % kTileY == 0 && t.iy > 0, fz = row && t.iz % kTileZ == 0 && t.iz > 0;
    if (!(fx || fy || fz)) return;
    const bool in = t.ix < b.dx;
    const int j = in ? frag_index(b, t.ix, t.iy, t.iz) : 0;
    const bool solid = in && (fy || fz || lane == 0) && uf_load<kScope>(P, j) >= 0;
    if (fy) {
        const bool both = solid && uf_load<kScope>(P, j - b.dx) >= 0;
        const unsigned long long m = __ballot(both);
        if (both && !(lane > 0 && (m >> (lane - 1) & 1))) uf_union<kScope, true>(P, j, j - b.dx, n, flag);
    }
    if (fz) {
        const bool both = solid && uf_load<kScope>(P, j - b.dx * b.dy) >= 0;
        const unsigned long long m = __ballot(both);
        if (both && !(lane > 0 && (m >> (lane - 1) & 1))) uf_union<kScope, true>(P, j, j - b.dx * b.dy, n, flag);
    }
    if (fx && lane == 0 && solid && uf_load<kScope>(P, j - 1) >= 0) uf_union<kScope, true>(P, j, j - 1, n, flag);
}

// Lanes of a wave that hold the same key >= 0 next to each other form a run; its first lane learns the run's length, the others 0.
__device__ __forceinline__ int run_length(int key)
{
    const int lane = __lane_id();
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (!head || key < 0) return 0;
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    return above ? __ffsll(above) : 64 - lane;
}

}  // namespace vtmc
#endif
