// terrain_water.h -- the host half of the flood (terrain_water.hip): the argument checks, the distinct levels in the order they are
// processed, the level -> plane search, the nearest sample of a position and the dims of the volumes.  Plain C++ with no device code and no
// HIP header, so a stand-alone program compiles it for the CPU (tools/water_host_check.cpp runs it under the host sanitizers).  The FP32
// steps are the rule's (include/vtmc_water.h, WATER), one IEEE operation each.
#ifndef VTMC_TERRAIN_WATER_H
#define VTMC_TERRAIN_WATER_H
#include "../../include/vtmc_water.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vtmc {

inline uint32_t water_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// What is wrong with the arguments of vtmc_terrain_flood by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *flood_args_fault(const float *lower, const float *upper, const vtmc_water_source *sources, int32_t n_sources, uint32_t flags)
{
    if (!lower || !upper) return "lower or upper is null";
    for (int k = 0; k < 3; ++k)
        if (std::isnan(lower[k]) || std::isnan(upper[k])) return "a bound is NaN";
    if (flags != 0) return "flags must be 0";
    if (n_sources < 0 || n_sources > VTMC_WATER_MAX_SOURCES) return "n_sources outside 0..VTMC_WATER_MAX_SOURCES";
    if (n_sources > 0 && !sources) return "sources is null";
    uint32_t seen[VTMC_WATER_MAX_LEVELS];
    int n_seen = 0;
    for (int32_t i = 0; i < n_sources; ++i) {
        const vtmc_water_source &s = sources[i];
        if (!std::isfinite(s.position[0]) || !std::isfinite(s.position[1]) || !std::isfinite(s.position[2])) return "a source's position is not finite";
        if (!std::isfinite(s.level)) return "a source's level is not finite";
        const uint32_t u = water_bits(s.level);
        if (std::find(seen, seen + n_seen, u) != seen + n_seen) continue;
        if (n_seen == VTMC_WATER_MAX_LEVELS) return "more than VTMC_WATER_MAX_LEVELS distinct levels";
        seen[n_seen++] = u;
    }
    return nullptr;
}

// The distinct level bit patterns of checked sources in the order the flood processes them: descending value, +0 before -0.
inline std::vector<float> water_levels(const vtmc_water_source *sources, int32_t n_sources)
{
    std::vector<float> levels;
    for (int32_t i = 0; i < n_sources; ++i) {
        const uint32_t u = water_bits(sources[i].level);
        if (std::none_of(levels.begin(), levels.end(), [u](float l) { return water_bits(l) == u; })) levels.push_back(sources[i].level);
    }
    std::sort(levels.begin(), levels.end(), [](float a, float b) { return a > b || (a == b && water_bits(a) < water_bits(b)); });
    return levels;
}

// the height of grid plane j: the terrain's own position formula
inline float water_plane_height(int32_t j, float scale, float origin_y) { return (float)j * scale + origin_y; }

// The highest plane j of 0..dim_y-1 that is under `level` (y_j <= level), or -1.  y_j does not decrease with j (scale > 0; rounding is
// monotonic), so the planes under a level are a prefix and a bisection finds its end.
inline int32_t water_plane(float level, float scale, float origin_y, int32_t dim_y)
{
    int32_t lo = -1, hi = dim_y;   // plane lo is under (or -1), plane hi is not (or dim_y)
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (water_plane_height(mid, scale, origin_y) <= level) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the nearest sample of a world coordinate along one axis: g = (p - origin) / scale; i = (int)floorf(g + 0.5f), saturating; NaN gives
// INT32_MIN, which is outside every box
inline int32_t water_nearest(float p, float origin, float scale)
{
    float g = p - origin;
    g = g / scale;
    g = std::floor(g + 0.5f);
    if (!(g > -2147483648.0f)) return INT32_MIN;
    if (g >= 2147483648.0f) return INT32_MAX;
    return (int32_t)g;
}

// samples per axis of the volumes of a box of d samples: 8 * ceil(max(d - 2, 1) / 8) + 2, whole 8-cell blocks for the extract
inline int32_t water_volume_dim(int32_t d) { return 8 * ((std::max(d - 2, 1) + 7) / 8) + 2; }

// One source as the device takes it: the box-linear index of its sample (-1: outside the box, dry), the index of that sample in the
// volumes, and its place in the caller's array.  16 bytes.
struct WaterSeed {
    int32_t box_index, volume_index, source, reserved;
};
static_assert(sizeof(WaterSeed) == 16, "copied to the device as it lies");
static_assert(sizeof(vtmc_water_body) == 64 && sizeof(vtmc_water_source) == 16, "include/vtmc_water.h");

// The seeds of the sources of one level (bit pattern), in the caller's order.  box_lo / box_d: the flood's box; vd: the volume dims.
inline void water_level_seeds(const vtmc_water_source *sources, int32_t n_sources, float level, const float origin[3], float scale,
                              const int32_t box_lo[3], const int32_t box_d[3], const int32_t vd[3], std::vector<WaterSeed> &out)
{
    for (int32_t i = 0; i < n_sources; ++i) {
        if (water_bits(sources[i].level) != water_bits(level)) continue;
        int64_t c[3];
        bool in = true;
        for (int k = 0; k < 3; ++k) {
            c[k] = (int64_t)water_nearest(sources[i].position[k], origin[k], scale) - box_lo[k];
            in = in && c[k] >= 0 && c[k] < box_d[k];
        }
        WaterSeed s{-1, -1, i, 0};
        if (in) {
            s.box_index = (int32_t)(c[0] + box_d[0] * (c[1] + box_d[1] * c[2]));
            s.volume_index = (int32_t)(c[0] + vd[0] * (c[1] + vd[1] * c[2]));
        }
        out.push_back(s);
    }
}

}  // namespace vtmc
#endif
