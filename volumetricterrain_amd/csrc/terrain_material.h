// terrain_material.h -- the host half of the material layer (terrain_material.hip): the argument checks, the per-axis factors of the rule
// and the texel box a paint call walks.  Plain C++ with no device code and no HIP header, so a stand-alone program compiles it for the
// CPU (tools/material_host_check.cpp runs it under the host sanitizers).  The arithmetic of material_texel_size and material_vertex_scale
// is part of the rule of include/vtmc.h: FP32, one IEEE operation per step (-ffp-contract=off).
#ifndef VTMC_TERRAIN_MATERIAL_H
#define VTMC_TERRAIN_MATERIAL_H
#include "../../include/vtmc.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vtmc {

constexpr int kMaterialMinFineness = 1, kMaterialMaxFineness = 8;  // VoxelTerrain.cs:191

// texels per axis of a layer of the given fineness, 0 when the fineness is out of range
inline int material_size(int32_t fineness) { return fineness < kMaterialMinFineness || fineness > kMaterialMaxFineness ? 0 : 16 * fineness; }

// index of the first NaN of the n floats, -1 when there is none
inline long long material_first_nan(const float *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (v[i] != v[i]) return (long long)i;
    return -1;
}

// Copies the n floats to dst and reports the first NaN as material_first_nan does (the copy into the pinned stage and the check in one pass).
inline long long material_copy_checked(float *dst, const float *src, size_t n)
{
    long long bad = -1;
    for (size_t i = 0; i < n; ++i) {
        const float f = src[i];
        if (f != f && bad < 0) bad = (long long)i;
        dst[i] = f;
    }
    return bad;
}

// What is wrong with stroke i, or null: the texts of vtmc_last_error
inline const char *material_stroke_fault(const vtmc_material_stroke &s)
{
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(s.center[k])) return "centre not finite";
    if (!std::isfinite(s.radius) || !(s.radius > 0.0f)) return "radius not finite or <= 0";
    if (!std::isfinite(s.strength) || !(s.strength >= 0.0f && s.strength <= 1.0f)) return "strength not finite or outside [0, 1]";
    if (s.channel < 0 || s.channel >= VTMC_MATERIAL_CHANNELS) return "channel outside 0..7";
    return nullptr;
}

// The index of the first faulty stroke and its fault, or -1.  n is in 0..VTMC_MATERIAL_MAX_STROKES and strokes non-null when n > 0.
inline int32_t material_check_strokes(const vtmc_material_stroke *strokes, int32_t n, const char **fault)
{
    for (int32_t i = 0; i < n; ++i)
        if (const char *f = material_stroke_fault(strokes[i])) {
            *fault = f;
            return i;
        }
    return -1;
}

// ts = ((float)cells * scale) / (float)C per axis: the world size of a texel (paint)
inline void material_texel_size(const int cells[3], float scale, int C, float ts[3])
{
    for (int k = 0; k < 3; ++k) {
        const float world = (float)cells[k] * scale;
        ts[k] = world / (float)C;
    }
}

// s = (float)C / (float)cells per axis: texels per cell (vertex weights)
inline void material_vertex_scale(const int cells[3], int C, float s[3])
{
    for (int k = 0; k < 3; ++k) s[k] = (float)C / (float)cells[k];
}

// The texels a paint call walks: lo[k] .. lo[k] + n[k] - 1 per axis, n[k] = 0 on some axis when no stroke can reach a texel.
struct MaterialBox {
    int lo[3], n[3];
};

// A box that holds every texel some stroke gives w != 0.  A texel centre with w != 0 lies less than r from c; the box is that range of
// texel indices per axis, evaluated in double and grown by one texel for the roundings of the FP32 rule, then clamped to 0..C-1 (a
// stroke does not wrap).  Where a texel is too small beside the coordinates' magnitude for that margin to cover the FP32 roundings
// (ts below 2^-20 of the largest coordinate in play), the whole cube is walked: the rule is pointwise, the box is only a saving.
inline MaterialBox material_paint_box(const vtmc_material_stroke *strokes, int32_t n, const float ts[3], const float origin[3], int C)
{
    MaterialBox b;
    for (int k = 0; k < 3; ++k) {
        double lo = (double)C, hi = -1.0, reach = std::fabs((double)origin[k]) + (double)ts[k] * C;
        for (int32_t i = 0; i < n; ++i) {
            const double c = (double)strokes[i].center[k], r = (double)strokes[i].radius;
            reach = std::max(reach, std::fabs(c) + r);
            // texel i's centre lies at (i + 0.5) * ts + origin
            lo = std::min(lo, std::floor((c - r - (double)origin[k]) / (double)ts[k] - 0.5) - 1.0);
            hi = std::max(hi, std::ceil((c + r - (double)origin[k]) / (double)ts[k] - 0.5) + 1.0);
        }
        if (!((double)ts[k] > reach * (1.0 / 1048576.0)) || !(lo == lo) || !(hi == hi)) lo = 0.0, hi = (double)C - 1.0;
        lo = std::max(lo, 0.0);
        hi = std::min(hi, (double)C - 1.0);
        b.lo[k] = (int)lo;
        b.n[k] = n > 0 && hi >= lo ? (int)hi - (int)lo + 1 : 0;
    }
    return b;
}

}  // namespace vtmc
#endif
