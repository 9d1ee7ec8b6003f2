// scan_kernels.h -- the two-level exclusive scan of up to 2^23 uint32 totals that the counting passes share (tri_stream_kernels.h: the
// records of a tile of triangles, for the scatter and the skirts; terrain_nav.hip and terrain_naverode.hip: the spans of a column).
// scan_tiles_kernel gives every tile its prefix inside its group of kScanThreads tiles and every group its total; scan_groups_kernel,
// one workgroup, scans the group totals and leaves the grand total in 64 bits.  A tile's offset is the sum of the two prefixes.  (One
// workgroup over all the tile totals took 0.19 ms of the scatter pass's 0.88 at 1024^3: profiles/r19/scatter.)  The kernels are static:
// every translation unit that includes this launches its own copy.  The buffer they work in is a ScanLayout (scan_layout.h, which the
// host halves read too); launch_scan queues the pair over one.
#ifndef VTMC_SCAN_KERNELS_H
#define VTMC_SCAN_KERNELS_H
#include "scan_layout.h"
#include "vtmc_ctx.h"

namespace vtmc {

// exclusive prefix of v over the 64 * WAVES threads of the workgroup, wave by wave and then across the waves; total = the sum
template <int WAVES>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63u) wave_sums[w] = x;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)WAVES; ++j) {
        const uint32_t s = wave_sums[j];
        if (j < w) base += s;
        total += s;
    }
    return base + x - v;
}

// A workgroup per group of 1024 tiles, a thread per tile: the tile's prefix inside its group, and the group's total (at most 1024 * 256 * 8)
static __global__ __launch_bounds__(kScanThreads) void scan_tiles_kernel(const uint32_t *__restrict__ tile_totals, uint32_t n_tiles,
                                                                                 uint32_t *__restrict__ tile_offsets, uint32_t *__restrict__ group_totals)
{
    __shared__ uint32_t wave_sums[kScanThreads / 64];
    const uint32_t tile = blockIdx.x * (uint32_t)kScanThreads + threadIdx.x;
    const uint32_t v = tile < n_tiles ? tile_totals[tile] : 0u;
    uint32_t total;
    const uint32_t before = block_scan<kScanThreads / 64>(v, wave_sums, total);
    if (tile < n_tiles) tile_offsets[tile] = before;
    if (threadIdx.x == 0) group_totals[blockIdx.x] = total;
}

// One workgroup.  Thread i owns a contiguous run of the groups (8 at the most): it sums the run, the sums are scanned across the
// workgroup, and the run is walked again to write the prefixes.  The total is kept in 64 bits (T * 8 can pass 2^32).
static __global__ __launch_bounds__(kScanThreads) void scan_groups_kernel(const uint32_t *__restrict__ group_totals, uint32_t n_groups,
                                                                                  uint32_t *__restrict__ group_offsets, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long part[kScanThreads];
    const uint32_t run = (n_groups + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * run < n_groups ? threadIdx.x * run : n_groups;
    const uint32_t hi = lo + run < n_groups ? lo + run : n_groups;
    unsigned long long s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += group_totals[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)kScanThreads; d <<= 1) {
        const unsigned long long y = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += y;
        __syncthreads();
    }
    unsigned long long at = part[threadIdx.x] - s;
    for (uint32_t i = lo; i < hi; ++i) {
        group_offsets[i] = (uint32_t)at;   // the host goes on only when the total fits an int32
        at += group_totals[i];
    }
    if (threadIdx.x == kScanThreads - 1) *total = part[threadIdx.x];
}

// Both levels over a layout whose tile totals are written (at least one tile), asynchronous on `stream`; the status of the launches
static hipError_t launch_scan(const ScanLayout &l, hipStream_t stream)
{
    const uint32_t groups = (uint32_t)l.groups();
    if (hipError_t e = launch(scan_tiles_kernel, dim3(groups), dim3(kScanThreads), 0, stream, l.tile_totals(), (uint32_t)l.n_tiles, l.tile_offsets(), l.group_totals()))
        return e;
    return launch(scan_groups_kernel, dim3(1), dim3(kScanThreads), 0, stream, l.group_totals(), groups, l.group_offsets(), l.total());
}

}  // namespace vtmc
#endif
