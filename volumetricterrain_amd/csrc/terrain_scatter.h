// terrain_scatter.h -- the host half of the surface scatter (terrain_scatter.hip): the argument checks, dc, and the hash of the rule, which
// host and device share; the tile count and the mask bytes are tri_stream.h's.  Outside the library's own build it takes no HIP header and
// holds no device-only code, so a stand-alone program compiles it for the CPU (tools/scatter_host_check.cpp runs it under the host
// sanitizers).  The arithmetic of scatter_density_cells is part of the rule of include/vtmc.h: FP32, one IEEE operation per step
// (-ffp-contract=off).
#ifndef VTMC_TERRAIN_SCATTER_H
#define VTMC_TERRAIN_SCATTER_H
#include "../../include/vtmc.h"
#include "tri_stream.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__   // the library's build: the hash below is also the kernels'
#include <hip/hip_runtime.h>
#define VTMC_SCATTER_HD __host__ __device__ __forceinline__
#else
#define VTMC_SCATTER_HD inline
#endif

namespace vtmc {

// dc = density * (voxel_scale * voxel_scale): instances per cell^2, the factor the kernel multiplies a triangle's area (in cells) with
inline float scatter_density_cells(float density, float voxel_scale)
{
    const float s2 = voxel_scale * voxel_scale;
    return density * s2;
}

// What is wrong with the parameters on a terrain of the given voxel scale, or null: the texts of vtmc_last_error
inline const char *scatter_params_fault(const vtmc_scatter_params &p, float voxel_scale)
{
    if (!std::isfinite(p.density) || !(p.density > 0.0f)) return "density not finite or <= 0";
    if (!(scatter_density_cells(p.density, voxel_scale) <= VTMC_SCATTER_MAX_DENSITY_CELLS)) return "density * voxel_scale^2 above VTMC_SCATTER_MAX_DENSITY_CELLS";
    if (p.min_up != p.min_up || p.max_up != p.max_up || !(p.min_up <= p.max_up)) return "min_up / max_up NaN or min_up > max_up";
    if (p.min_y != p.min_y || p.max_y != p.max_y || !(p.min_y <= p.max_y)) return "min_y / max_y NaN or min_y > max_y";
    if (p.material_channel < -1 || p.material_channel >= VTMC_MATERIAL_CHANNELS) return "material_channel outside -1..7";
    if (p.max_instances <= 0) return "max_instances <= 0";
    if (p.flags != 0u) return "flags must be 0";
    return nullptr;
}

// -- the hash of the rule ------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kScatterGolden = 0x9E3779B97F4A7C15ull;

VTMC_SCATTER_HD uint64_t scatter_fin(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

VTMC_SCATTER_HD uint64_t scatter_step(uint64_t k, uint64_t w) { return scatter_fin((k ^ w) + kScatterGolden); }

VTMC_SCATTER_HD uint64_t scatter_seed_key(uint32_t seed) { return scatter_fin((uint64_t)seed + kScatterGolden); }

// word(k, i, d): draw d of candidate i of the triangle with key k
VTMC_SCATTER_HD uint64_t scatter_word(uint64_t k, uint32_t i, uint32_t d) { return scatter_step(k, ((uint64_t)i << 8) | (uint64_t)d); }

// U(k, i, d): 24 bits * 2^-24, exact, in [0, 1)
VTMC_SCATTER_HD float scatter_uniform(uint64_t k, uint32_t i, uint32_t d)
{
    return (float)(uint32_t)(scatter_word(k, i, d) >> 40) * 5.9604644775390625e-08f;
}

}  // namespace vtmc
#endif
