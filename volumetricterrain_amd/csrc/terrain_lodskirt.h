// terrain_lodskirt.h -- the host half of the level-of-detail skirts (terrain_lodskirt.hip): the argument checks, the face masks of the node
// list (a hash of (origin, level)) and the count bound; the sizes of the pass's buffers are tri_stream.h's.  Plain C++ with no device code
// and no HIP header, so a stand-alone program compiles it for the CPU (tools/lodskirt_host_check.cpp runs it under the host sanitizers).
// The rule is LODSKIRT of include/vtmc_lodskirt.h.
#ifndef VTMC_TERRAIN_LODSKIRT_H
#define VTMC_TERRAIN_LODSKIRT_H
#include "../../include/vtmc_lodskirt.h"
#include "tri_stream.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vtmc {

constexpr int kLodSkirtFaces = 6;
constexpr int kLodSkirtPerTriangle = 12;    // records a triangle can yield at the most: a quad of two records on each of six faces

static_assert(sizeof(vtmc_lodskirt_params) == 8 && sizeof(vtmc_triangle) == 76 && sizeof(vtmc_lod_node) == 16, "include/vtmc_lodskirt.h");

// What is wrong with the parameters by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *lodskirt_params_fault(const vtmc_lodskirt_params &p)
{
    if (!std::isfinite(p.depth) || !(p.depth > 0.0f)) return "depth not finite or <= 0";
    if (!(p.depth <= (float)VTMC_LODSKIRT_MAX_DEPTH)) return "depth above VTMC_LODSKIRT_MAX_DEPTH";
    if (p.flags & ~VTMC_LODSKIRT_ALL_FACES) return "unknown flag bits";
    return nullptr;
}

// The count bound: no result of T triangles yields more records than this, and a tile's total (at most 256 * 12 = 3072) and a scan group's
// (1024 tiles: 3 145 728) stay far inside the 32 bits the scan keeps them in; the grand total is summed in 64 bits and compared with
// 2^31 - 1 before anything is placed.
inline int64_t lodskirt_max_records(int64_t n_tris) { return n_tris * kLodSkirtPerTriangle; }
inline bool lodskirt_total_fits(unsigned long long total) { return total <= 0x7fffffffull; }

// the key of a node: three origins and a level, mixed into 64 bits (the splitmix64 finaliser)
inline uint64_t lodskirt_hash(int32_t ox, int32_t oy, int32_t oz, int32_t level)
{
    uint64_t z = ((uint64_t)(uint32_t)ox * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(uint32_t)oy * 0xC2B2AE3D27D4EB4Full) ^ ((uint64_t)(uint32_t)oz * 0x165667B19E3779F9ull) ^
                 ((uint64_t)(uint32_t)level << 56);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The set of (origin, level) of a node list: open addressing over a power-of-two table at most half full, the entries indices into the list.
struct LodSkirtNodeSet {
    const vtmc_lod_node *nodes;
    std::vector<int32_t> slots;   // -1: empty
    size_t mask;
    LodSkirtNodeSet(const vtmc_lod_node *list, size_t n) : nodes(list)
    {
        size_t cap = 16;
        while (cap < 2 * n) cap *= 2;
        slots.assign(cap, -1);
        mask = cap - 1;
        for (size_t i = 0; i < n; ++i) {
            size_t at = (size_t)lodskirt_hash(list[i].origin[0], list[i].origin[1], list[i].origin[2], list[i].level) & mask;
            while (slots[at] >= 0) at = (at + 1) & mask;
            slots[at] = (int32_t)i;
        }
    }
    bool holds(const int32_t o[3], int32_t level) const
    {
        for (size_t at = (size_t)lodskirt_hash(o[0], o[1], o[2], level) & mask; slots[at] >= 0; at = (at + 1) & mask) {
            const vtmc_lod_node &nd = nodes[slots[at]];
            if (nd.origin[0] == o[0] && nd.origin[1] == o[1] && nd.origin[2] == o[2] && nd.level == level) return true;
        }
        return false;
    }
};

// The mask byte of every node of the list by the rule's Flagged (out is resized to n); cells = (W, E, H).  Returns the number of nodes
// with a flagged face.  The list is the library's own (lod_select): levels 0..VTMC_LOD_MAX_LEVEL, origins inside the terrain; the
// arithmetic is 64-bit all the same, so a foreign list cannot overflow it.
inline int32_t lodskirt_face_masks(const vtmc_lod_node *nodes, size_t n, const int32_t cells[3], uint32_t flags, std::vector<uint8_t> &out)
{
    out.assign(n, 0);
    const LodSkirtNodeSet set(nodes, n);
    int32_t flagged = 0;
    for (size_t i = 0; i < n; ++i) {
        const vtmc_lod_node &nd = nodes[i];
        if (nd.level < 0 || nd.level > VTMC_LOD_MAX_LEVEL) continue;
        const int64_t size = (int64_t)VTMC_BLOCK_SIZE << nd.level;
        uint8_t m = 0;
        for (int f = 0; f < kLodSkirtFaces; ++f) {
            const int axis = f >> 1;
            const int64_t o = (int64_t)nd.origin[axis] + ((f & 1) ? size : -size);
            if (o < 0 || o + size > (int64_t)cells[axis]) continue;   // the terrain's boundary
            int32_t beyond[3] = {nd.origin[0], nd.origin[1], nd.origin[2]};
            beyond[axis] = (int32_t)o;
            if ((flags & VTMC_LODSKIRT_ALL_FACES) || !set.holds(beyond, nd.level)) m |= (uint8_t)(1u << f);
        }
        out[i] = m;
        flagged += m != 0;
    }
    return flagged;
}

}  // namespace vtmc
#endif
