// terrain_light.h -- the host half of the voxel lighting (terrain_light.hip): the argument checks, the sample of a source and the seeds the
// device takes (one per source, the largest level of a sample on its first source), one relaxation step on a plain array, the vertex rule
// and the sizes.  Plain C++ with no device code and no HIP header, so a stand-alone program compiles it for the CPU
// (tools/light_host_check.cpp runs it under the host sanitizers).  The rule is include/vtmc_light.h's, LIGHT: integers but for the
// nearest-sample formula, which is terrain_water.h's.
#ifndef VTMC_TERRAIN_LIGHT_H
#define VTMC_TERRAIN_LIGHT_H
#include "../../include/vtmc_light.h"
#include "terrain_water.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vtmc {

static_assert(sizeof(vtmc_light_source) == 16 && sizeof(vtmc_light_params) == 16 && sizeof(vtmc_light_sample) == 2, "include/vtmc_light.h");

// What is wrong with the arguments of vtmc_terrain_light by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *light_args_fault(const float *lower, const float *upper, const vtmc_light_params *params, const vtmc_light_source *sources, int32_t n_sources)
{
    if (!lower || !upper) return "lower or upper is null";
    if (!params) return "params is null";
    for (int k = 0; k < 3; ++k)
        if (std::isnan(lower[k]) || std::isnan(upper[k])) return "a bound is NaN";
    if (params->flags != 0) return "flags must be 0";
    if (params->sky_level < 0 || params->sky_level > VTMC_LIGHT_MAX_LEVEL) return "sky_level outside 0..255";
    if (params->sky_falloff < 1 || params->sky_falloff > 255) return "sky_falloff outside 1..255";
    if (params->torch_falloff < 1 || params->torch_falloff > 255) return "torch_falloff outside 1..255";
    if (n_sources < 0 || n_sources > VTMC_LIGHT_MAX_SOURCES) return "n_sources outside 0..VTMC_LIGHT_MAX_SOURCES";
    if (n_sources > 0 && !sources) return "sources is null";
    for (int32_t i = 0; i < n_sources; ++i) {
        const vtmc_light_source &s = sources[i];
        if (!std::isfinite(s.position[0]) || !std::isfinite(s.position[1]) || !std::isfinite(s.position[2])) return "a source's position is not finite";
        if (s.level < 1 || s.level > VTMC_LIGHT_MAX_LEVEL) return "a source's level is outside 1..255";
    }
    return nullptr;
}

// One source as the device takes it: the box-linear index of its sample (-1: outside the box, dark), and the torch emission it writes
// there when the sample is open: the largest level of the sources on that sample on the first of them, 0 on the others, so no two lanes
// write one sample.  8 bytes, in the caller's order.
struct LightSeed {
    int32_t box_index, emission;
};
static_assert(sizeof(LightSeed) == 8, "copied to the device as it lies");

inline std::vector<LightSeed> light_seeds(const vtmc_light_source *sources, int32_t n_sources, const float origin[3], float scale, const int32_t box_lo[3],
                                          const int32_t box_d[3])
{
    std::vector<LightSeed> seeds((size_t)n_sources);
    std::vector<int32_t> order;
    for (int32_t i = 0; i < n_sources; ++i) {
        int64_t c[3];
        bool in = true;
        for (int k = 0; k < 3; ++k) {
            c[k] = (int64_t)water_nearest(sources[i].position[k], origin[k], scale) - box_lo[k];
            in = in && c[k] >= 0 && c[k] < box_d[k];
        }
        seeds[(size_t)i] = LightSeed{in ? (int32_t)(c[0] + box_d[0] * (c[1] + (int64_t)box_d[1] * c[2])) : -1, 0};
        if (in) order.push_back(i);
    }
    // the sources of one sample next to each other, the first of them in front
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return seeds[(size_t)a].box_index != seeds[(size_t)b].box_index ? seeds[(size_t)a].box_index < seeds[(size_t)b].box_index : a < b;
    });
    for (size_t i = 0; i < order.size();) {
        size_t j = i;
        int32_t top = 0;
        for (; j < order.size() && seeds[(size_t)order[j]].box_index == seeds[(size_t)order[i]].box_index; ++j) top = std::max(top, sources[order[j]].level);
        seeds[(size_t)order[i]].emission = top;
        i = j;
    }
    return seeds;
}

inline int light_channel(uint16_t v, int channel) { return channel ? v >> 8 : v & 0xff; }   // a sample as it lies in memory: sky low, torch high
inline uint16_t light_pack(int sky, int torch) { return (uint16_t)(sky | torch << 8); }

// one channel of a sample after one step: what it held, or what its brightest neighbour hands on
inline int light_step_channel(int own, int brightest_neighbour, int falloff) { return std::max(own, brightest_neighbour - falloff); }

// One relaxation step of the rule on a plain array of d[0] x d[1] x d[2] samples, x fastest: `next` from `prev`; open[i] != 0: sample i is
// open.  Returns whether any sample changed.  Repeated from the emissions until it returns false it leaves the rule's field.
inline bool light_relax_step(const uint16_t *prev, uint16_t *next, const uint8_t *open, const int32_t d[3], int sky_falloff, int torch_falloff)
{
    bool changed = false;
    const int64_t pitch[3] = {1, d[0], (int64_t)d[0] * d[1]};
    for (int32_t z = 0; z < d[2]; ++z)
        for (int32_t y = 0; y < d[1]; ++y)
            for (int32_t x = 0; x < d[0]; ++x) {
                const int64_t i = x + pitch[1] * y + pitch[2] * z;
                if (!open[i]) {
                    next[i] = 0;
                    continue;
                }
                const int32_t c[3] = {x, y, z};
                int sky = 0, torch = 0;
                for (int k = 0; k < 3; ++k) {
                    if (c[k] > 0) sky = std::max(sky, light_channel(prev[i - pitch[k]], 0)), torch = std::max(torch, light_channel(prev[i - pitch[k]], 1));
                    if (c[k] + 1 < d[k]) sky = std::max(sky, light_channel(prev[i + pitch[k]], 0)), torch = std::max(torch, light_channel(prev[i + pitch[k]], 1));
                }
                next[i] = light_pack(light_step_channel(light_channel(prev[i], 0), sky, sky_falloff), light_step_channel(light_channel(prev[i], 1), torch, torch_falloff));
                changed = changed || next[i] != prev[i];
            }
    return changed;
}

// the cell origin of a grid coordinate along an axis of n samples, as the occlusion rule's fetch finds it (include/vtmc.h)
inline int32_t light_cell_origin(float g, int32_t n)
{
    const float top = (float)(n - 1);
    const float t = g < 0.0f ? 0.0f : (g > top ? top : g);
    if (t != t) return 0;   // a NaN coordinate (no result of the library holds one): what the device's conversion makes of it
    int32_t i0 = (int32_t)std::floor(t);
    if (i0 > n - 2) i0 = n - 2;
    return i0;
}

// The two bytes of a vertex at grid coordinate g of a grid of n samples per axis, from the volume of the box lo, d: per channel the
// largest of the cell's corners inside the box, (0, 0) with none.
inline uint16_t light_vertex(const uint16_t *volume, const int32_t lo[3], const int32_t d[3], const int32_t n[3], const float g[3])
{
    int32_t c0[3];
    for (int k = 0; k < 3; ++k) c0[k] = light_cell_origin(g[k], n[k]) - lo[k];
    int sky = 0, torch = 0;
    for (int corner = 0; corner < 8; ++corner) {
        const int32_t x = c0[0] + (corner & 1), y = c0[1] + (corner >> 1 & 1), z = c0[2] + (corner >> 2);
        if (x < 0 || x >= d[0] || y < 0 || y >= d[1] || z < 0 || z >= d[2]) continue;
        const uint16_t v = volume[x + (int64_t)d[0] * (y + (int64_t)d[1] * z)];
        sky = std::max(sky, light_channel(v, 0)), torch = std::max(torch, light_channel(v, 1));
    }
    return light_pack(sky, torch);
}

inline size_t light_samples(const int32_t d[3]) { return (size_t)d[0] * (size_t)d[1] * (size_t)d[2]; }
// words of 64 bits of the open mask: one per row of up to 64 samples along x
inline size_t light_mask_words(const int32_t d[3]) { return (size_t)((d[0] + 63) / 64) * (size_t)d[1] * (size_t)d[2]; }
inline size_t light_tiles(const int32_t d[3]) { return (size_t)((d[0] + 63) / 64) * (size_t)((d[1] + 7) / 8) * (size_t)((d[2] + 7) / 8); }

}  // namespace vtmc
#endif
