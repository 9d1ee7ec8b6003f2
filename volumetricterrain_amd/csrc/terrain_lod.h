// terrain_lod.h -- the host half of the level-of-detail extract (terrain_lod.hip): the argument checks, the selection descent and the node
// list.  Plain C++ with no device code and no HIP header, so a stand-alone program compiles it for the CPU (tools/lod_host_check.cpp runs it
// under the host sanitizers).  The arithmetic of lod_select is part of the rule of include/vtmc.h: double, one IEEE operation per step
// (-ffp-contract=off).
#ifndef VTMC_TERRAIN_LOD_H
#define VTMC_TERRAIN_LOD_H
#include "../../include/vtmc.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vtmc {

// What is wrong with the parameters by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *lod_params_fault(const vtmc_lod_params &p)
{
    if (!std::isfinite(p.viewer[0]) || !std::isfinite(p.viewer[1]) || !std::isfinite(p.viewer[2])) return "viewer not finite";
    if (!std::isfinite(p.split) || !(p.split >= 1.0f)) return "split not finite or < 1";
    if (p.max_level < 0 || p.max_level > VTMC_LOD_MAX_LEVEL) return "max_level outside 0..VTMC_LOD_MAX_LEVEL";
    if (p.max_nodes <= 0) return "max_nodes <= 0";
    return nullptr;
}

// cells per axis of a node of the level
inline int32_t lod_node_cells(int32_t level) { return VTMC_BLOCK_SIZE << level; }

// VTMC_ERR_DIMS: the roots must tile the terrain (cells = W, E, H; max_level has passed lod_params_fault)
inline bool lod_dims_fit(const int32_t cells[3], int32_t max_level)
{
    const int32_t n = lod_node_cells(max_level);
    return cells[0] > 0 && cells[1] > 0 && cells[2] > 0 && cells[0] % n == 0 && cells[1] % n == 0 && cells[2] % n == 0;
}

// d of the rule: the Chebyshev distance from c to the box [o, o + n], 0 inside
inline double lod_distance(const double c[3], const int32_t o[3], int32_t n)
{
    double d = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double below = (double)o[k] - c[k], above = c[k] - ((double)o[k] + (double)n);
        if (below > d) d = below;
        if (above > d) d = above;
    }
    return d;
}

struct LodSelection {
    double c[3];
    double split;
    size_t max_nodes;
    std::vector<vtmc_lod_node> *out;
};

// one node of the descent; false: the list would pass max_nodes
inline bool lod_descend(const LodSelection &s, const int32_t o[3], int32_t level)
{
    const int32_t n = lod_node_cells(level);
    if (level > 0 && lod_distance(s.c, o, n) < s.split * (double)n) {
        const int32_t h = n / 2;
        for (int k = 0; k < 8; ++k) {
            const int32_t child[3] = {o[0] + h * (k & 1), o[1] + h * ((k >> 1) & 1), o[2] + h * ((k >> 2) & 1)};
            if (!lod_descend(s, child, level - 1)) return false;
        }
        return true;
    }
    if (s.out->size() >= s.max_nodes) return false;
    s.out->push_back(vtmc_lod_node{{o[0], o[1], o[2]}, level});
    return true;
}

// The node list of include/vtmc.h's rule into `out` (cleared first).  p has passed lod_params_fault and lod_dims_fit; voxel_scale > 0.
// false: more than p.max_nodes nodes (out is then incomplete).
inline bool lod_select(const int32_t cells[3], const float terrain_origin[3], float voxel_scale, const vtmc_lod_params &p,
                       std::vector<vtmc_lod_node> &out)
{
    out.clear();
    LodSelection s{};
    for (int k = 0; k < 3; ++k) s.c[k] = ((double)p.viewer[k] - (double)terrain_origin[k]) / (double)voxel_scale;
    s.split = (double)p.split;
    s.max_nodes = (size_t)p.max_nodes;
    s.out = &out;
    const int32_t n = lod_node_cells(p.max_level);
    for (int32_t rz = 0; rz < cells[2] / n; ++rz)
        for (int32_t ry = 0; ry < cells[1] / n; ++ry)
            for (int32_t rx = 0; rx < cells[0] / n; ++rx) {
                const int32_t o[3] = {rx * n, ry * n, rz * n};
                if (!lod_descend(s, o, p.max_level)) return false;
            }
    return true;
}

}  // namespace vtmc
#endif
