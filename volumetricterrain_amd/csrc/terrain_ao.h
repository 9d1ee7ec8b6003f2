// terrain_ao.h -- the host half of the per-vertex ambient occlusion (terrain_ao.hip): the argument checks, Rg, the per-call h[] / fall[]
// tables, the 26 directions and the extent of the LDS tile.  Plain C++ with no device code and no HIP header, so a stand-alone program
// compiles it for the CPU (tools/ao_host_check.cpp runs it under the host sanitizers).  The arithmetic of ao_tables is part of the rule of
// include/vtmc.h: FP32, one IEEE operation per step (-ffp-contract=off).
#ifndef VTMC_TERRAIN_AO_H
#define VTMC_TERRAIN_AO_H
#include "../../include/vtmc.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vtmc {

constexpr int kAoDirections = 26;
constexpr int kAoBlockSamples = 10;   // a block's vertices lie at g = 8b .. 8b + 8; the cell above the last one ends at sample 8b + 9

// What is wrong with the parameters on a terrain of the given voxel scale, or null: the texts of vtmc_last_error
inline const char *ao_params_fault(const vtmc_ao_params &p, float voxel_scale)
{
    if (!std::isfinite(p.radius) || !(p.radius > 0.0f)) return "radius not finite or <= 0";
    if (!(p.radius / voxel_scale <= (float)VTMC_AO_MAX_RADIUS_CELLS)) return "radius / voxel_scale above VTMC_AO_MAX_RADIUS_CELLS";
    if (!std::isfinite(p.strength) || !(p.strength >= 0.0f && p.strength <= 1.0f)) return "strength not finite or outside [0, 1]";
    if (p.steps < 1 || p.steps > VTMC_AO_MAX_STEPS) return "steps outside 1..VTMC_AO_MAX_STEPS";
    if (p.flags != 0u) return "flags must be 0";
    return nullptr;
}

// len of a direction by the number of its non-zero components (1, 2, 3); the literals are part of the rule
inline float ao_direction_length(int nonzero) { return nonzero == 1 ? 1.0f : (nonzero == 2 ? 0.70710678f : 0.57735027f); }

// d_m = ((float)i * len, (float)j * len, (float)k * len), m counting up with (i+1) + 3*(j+1) + 9*(k+1), the centre left out
inline void ao_directions(float d[kAoDirections][3])
{
    int m = 0;
    for (int code = 0; code < 27; ++code) {
        const int i = code % 3 - 1, j = (code / 3) % 3 - 1, k = code / 9 - 1;
        const int nonzero = (i != 0) + (j != 0) + (k != 0);
        if (!nonzero) continue;
        const float len = ao_direction_length(nonzero);
        d[m][0] = (float)i * len, d[m][1] = (float)j * len, d[m][2] = (float)k * len;
        ++m;
    }
}

// The per-call tables.  h and fall are the rule's, entry s - 1 for step s; hd[c - 1][s - 1] = len_c * h[s] is |d.x * h[s]| of a direction
// with c non-zero components (the product the kernel adds to or subtracts from a coordinate: (+-len) * h = +-(len * h) exactly).
struct AoTables {
    float rg;        // radius / voxel_scale
    int reach;       // ceil(rg): whole samples a march can leave the block's own 10^3 samples by
    int extent;      // samples per axis of the LDS tile: 10 + 2 * reach (22 at the largest radius)
    float h[VTMC_AO_MAX_STEPS], fall[VTMC_AO_MAX_STEPS];
    float hd[3][VTMC_AO_MAX_STEPS];
};

// p has passed ao_params_fault
inline AoTables ao_tables(const vtmc_ao_params &p, float voxel_scale)
{
    AoTables t{};
    const int S = p.steps;
    t.rg = p.radius / voxel_scale;
    t.reach = (int)std::ceil(t.rg);
    t.extent = kAoBlockSamples + 2 * t.reach;
    for (int s = 1; s <= S; ++s) {
        const float frac = (float)s / (float)S;
        t.h[s - 1] = t.rg * frac;
        const float back = (float)(s - 1) / (float)S;
        t.fall[s - 1] = 1.0f - back;
        for (int c = 1; c <= 3; ++c) t.hd[c - 1][s - 1] = ao_direction_length(c) * t.h[s - 1];
    }
    return t;
}

inline size_t ao_tile_bytes(int extent) { return sizeof(float) * (size_t)extent * extent * extent; }

}  // namespace vtmc
#endif
