// terrain_lodattr.h -- the host half of the per-vertex materials and occlusion of a level-of-detail result (terrain_lodattr.hip): the
// argument checks, a node's sample lattice (n_L and the two index clamps), the coordinates a vertex's attribute is evaluated at, and the
// map from a skirt corner to the mesh vertex it came from.  Plain C++ with no HIP header, so a stand-alone program compiles it for the
// CPU (tools/lodattr_host_check.cpp runs it under the host sanitizers); the kernels call the same functions, so what the program checks
// is what the device computes.  The rule is LODATTR of include/vtmc_lodattr.h: FP32, one IEEE operation per step (-ffp-contract=off).
#ifndef VTMC_TERRAIN_LODATTR_H
#define VTMC_TERRAIN_LODATTR_H
#include "../../include/vtmc_lodattr.h"
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define VTMC_LODATTR_FN __host__ __device__ inline
#else
#define VTMC_LODATTR_FN inline
#endif

namespace vtmc {

constexpr int kLodAttrAttributes = 2, kLodAttrTargets = 2;

static_assert(sizeof(vtmc_lod_node) == 16 && sizeof(vtmc_triangle) == 76 && VTMC_MATERIAL_CHANNELS == 8, "include/vtmc_lodattr.h");

// What is wrong with a reader's selectors, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *lodattr_selector_fault(int32_t attribute, int32_t target)
{
    if (attribute != VTMC_LODATTR_MATERIAL && attribute != VTMC_LODATTR_AO) return "unknown attribute";
    if (target != VTMC_LODATTR_MESH && target != VTMC_LODATTR_SKIRTS) return "unknown target";
    return nullptr;
}

// bytes per vertex of an attribute that has passed lodattr_selector_fault
inline size_t lodattr_bytes_per_vertex(int32_t attribute) { return attribute == VTMC_LODATTR_MATERIAL ? (size_t)VTMC_MATERIAL_CHANNELS : 1u; }

// n_L: samples per axis of the lattice of stride s = 2^L over an axis of dim = cells + 2 samples; s divides cells
VTMC_LODATTR_FN int32_t lodattr_lattice_samples(int32_t dim, int32_t s) { return (dim - 2) / s + 2; }

// the first clamp: a lattice index into [0, n_L - 1] (fetch's clamp-to-edge, as the staging loop applies it)
VTMC_LODATTR_FN int32_t lodattr_clamp_lattice(int32_t i, int32_t n_l) { return i < 0 ? 0 : (i > n_l - 1 ? n_l - 1 : i); }

// the second clamp: the grid index of lattice sample i >= 0.  The last lattice sample, i = n_L - 1, maps to the replicated plane dim - 1,
// as tile index 9 does in the extract's rule.  64-bit product: i * s passes 2^31 for no lattice the library makes, and for none at all here.
VTMC_LODATTR_FN int32_t lodattr_fine_index(int32_t i, int32_t s, int32_t dim)
{
    const int64_t fine = (int64_t)i * (int64_t)s;
    return fine > (int64_t)dim - 1 ? dim - 1 : (int32_t)fine;
}

// Materials: the fine grid coordinate of node-local p on one axis of node (o, s).  The product is exact (p in [0, 8] times a power of two),
// only the sum rounds; at s = 1 this is vtmc_material_vertices' (float)(8 * b) + p.
VTMC_LODATTR_FN float lodattr_material_coord(int32_t o, float p, int32_t s)
{
    const float scaled = p * (float)s;
    return (float)o + scaled;
}

// Occlusion: the coordinate of node-local p in the node's own lattice; o is a multiple of 8 s
VTMC_LODATTR_FN float lodattr_ao_coord(int32_t o, int32_t s, float p) { return (float)(o / s) + p; }

// Skirts: records come in pairs per quad, 2 q = (b, a, a') and 2 q + 1 = (b, a', b').  Corner c = 0..5 of the pair takes the attribute of
// corner lodattr_skirt_source(c) of record 2 q: 0 is b, 1 is a.  A displaced corner is never evaluated at its own position.
VTMC_LODATTR_FN int32_t lodattr_skirt_source(int32_t c) { return c == 1 || c == 2 || c == 4 ? 1 : 0; }

}  // namespace vtmc
#endif
