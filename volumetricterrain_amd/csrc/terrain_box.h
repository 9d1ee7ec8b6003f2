// terrain_box.h -- the box walk and the clamp draws every edit kernel of the resident terrain shares: a thread's place in a modifier's
// sample box, the grid and image indices, Mathf.Clamp against the drawn void / full values, the CSG write rule, and launch_box: the launch
// (vtmc_ctx.h) in the shape of a box kernel.
#ifndef VTMC_TERRAIN_BOX_H
#define VTMC_TERRAIN_BOX_H
#include "vtmc_ctx.h"
#include "terrain_hash.h"

namespace vtmc {

// Mathf.Clamp(v, voidDensity, fullDensity) with void = draw k, full = draw k+1.  void lies in [-2,-1)
// and full in [1,2), so a value in [-1,1] is never clamped and neither draw is evaluated for it; the
// result is the same as drawing both (each draw is a pure function of its counter).
__device__ __forceinline__ float clamp_drawn(float v, uint64_t seed, uint32_t event, uint64_t sample, uint32_t k)
{
    if (v < -1.0f) {
        const float lo = terrain_uniform(seed, event, sample, k) - 2.0f;
        if (v < lo) v = lo;
    } else if (v > 1.0f) {
        const float hi = terrain_uniform(seed, event, sample, k + 1u) + 1.0f;
        if (v > hi) v = hi;
    }
    return v;
}

// what a sample s becomes under the clamped density md: Mathf.Max(S, md) (add) or Clamp(Min(S, -md), void, full) (erode)
__device__ __forceinline__ float csg_combine(const TerrainShape &sh, uint32_t event, uint64_t sample, int add_or_erode, float md, float s)
{
    if (add_or_erode) return s > md ? s : md;
    const float minus_md = -md;
    return clamp_drawn(s < minus_md ? s : minus_md, sh.seed, event, sample, 2u);
}

constexpr int kYRun = 16;  // samples along y per thread

// ---- the box walk every edit kernel shares --------------------------------------------------------------------------------------
// launch shape: 64 x 4 threads = 64 samples along x (the stride-1 axis) of 4 z-planes; a thread walks kYRun samples along y;
// grid = (x segments, z quads, y runs)
// A thread's place in a box (a TerrainBox, or a TerrainModifierArgs for its six ints).  The box is asked, not stored: a kernel reads
// dy only behind its bounds test, as the kernels did when each wrote this out.
struct BoxThread {
    int ix, iz, iy0;  // this thread's column of the box and the first sample of its run along y
    __device__ __forceinline__ BoxThread() : ix(blockIdx.x * 64 + threadIdx.x), iz(blockIdx.y * 4 + threadIdx.y), iy0(blockIdx.z * kYRun) {}
    template <class Box>
    __device__ __forceinline__ bool inside(const Box &b) const { return ix < b.dx && iz < b.dz; }
    template <class Box>
    __device__ __forceinline__ int iy1(const Box &b) const { return iy0 + kYRun < b.dy ? iy0 + kYRun : b.dy; }  // the run is [iy0, iy1)
};
// sample (x, y, z) of the grid, x fastest; 64 bits: the hash counts samples with it
__device__ __forceinline__ uint64_t grid_index(const TerrainShape &sh, int x, int y, int z)
{
    return (uint64_t)x + (uint64_t)sh.dim_x * ((uint64_t)y + (uint64_t)sh.dim_y * (uint64_t)z);
}
// sample (ix, iy, iz) of a box in its journal image or stage, x fastest, so a wave stores 256 contiguous bytes; a box reaches 4.3 GB
template <class Box>
__device__ __forceinline__ uint64_t box_index(const Box &b, int ix, int iy, int iz)
{
    return (uint64_t)ix + (uint64_t)b.dx * ((uint64_t)iy + (uint64_t)b.dy * (uint64_t)iz);
}

static bool box_empty(const TerrainBox &b) { return b.dx <= 0 || b.dy <= 0 || b.dz <= 0; }

static dim3 box_grid(const TerrainBox &b) { return dim3((unsigned)((b.dx + 63) / 64), (unsigned)((b.dz + 3) / 4), (unsigned)((b.dy + kYRun - 1) / kYRun)); }
static bool box_launchable(const TerrainBox &b) { return (b.dz + 3) / 4 <= 65535 && (b.dy + kYRun - 1) / kYRun <= 65535; }  // grid y, z: 16 bits

// the one launch of a box kernel, on a non-empty box
template <class... Params, class... Args>
static hipError_t launch_box(void (*kernel)(Params...), const TerrainBox &b, hipStream_t stream, Args... args)
{
    return box_launchable(b) ? launch(kernel, box_grid(b), dim3(64, 4, 1), 0, stream, args...) : hipErrorInvalidValue;
}

}  // namespace vtmc
#endif
