// terrain_hash.h -- the counter hash behind voidDensity / fullDensity (terrain.hip's header comment): a pure function of (seed, event,
// sample index, draw index), shared by the edit kernels (terrain_box.h) and the redraw of elided bricks on load (terrain_io.hip).  The CPU
// oracle (oracle/terrain_ref.c) and volumetricterrain_amd/terrainfile.py restate it.
#ifndef VTMC_TERRAIN_HASH_H
#define VTMC_TERRAIN_HASH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vtmc {

__host__ __device__ __forceinline__ float terrain_uniform(uint64_t seed, uint32_t event, uint64_t sample, uint32_t draw)
{
    uint64_t z = (seed ^ ((uint64_t)event << 40) ^ (sample << 2) ^ (uint64_t)draw) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * 5.9604644775390625e-08f;  // 24 bits * 2^-24: exact, in [0,1)
}

}  // namespace vtmc
#endif
