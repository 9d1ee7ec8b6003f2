// lodattr_host_check.cpp -- a stand-alone run of the host half of the level-of-detail materials and occlusion (csrc/terrain_lodattr.h:
// the selector checks, n_L, the two index clamps, the coordinate formulas and the quad-to-source map -- the same functions the kernels
// call), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/lodattr_host_check.cpp -o lodattr_host_check && ./lodattr_host_check
// Exits 0 when every answer is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_lodattr.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace vtmc;

static int failures = 0;
#define EXPECT(c) \
    do { \
        if (!(c)) { \
            std::printf("line %d: %s\n", __LINE__, #c); \
            ++failures; \
        } \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main()
{
    static_assert(VTMC_LODATTR_MATERIAL == 0 && VTMC_LODATTR_AO == 1 && VTMC_LODATTR_MESH == 0 && VTMC_LODATTR_SKIRTS == 1, "include/vtmc_lodattr.h");

    // the selectors
    for (int32_t a : {0, 1})
        for (int32_t t : {0, 1}) EXPECT(lodattr_selector_fault(a, t) == nullptr);
    for (int32_t bad : {-1, 2, 3, 1 << 30, -(1 << 30)}) {
        EXPECT(lodattr_selector_fault(bad, 0) != nullptr && lodattr_selector_fault(bad, 1) != nullptr);
        EXPECT(lodattr_selector_fault(0, bad) != nullptr && lodattr_selector_fault(1, bad) != nullptr);
    }
    EXPECT(std::strcmp(lodattr_selector_fault(2, 0), "unknown attribute") == 0 && std::strcmp(lodattr_selector_fault(1, 2), "unknown target") == 0);
    EXPECT(lodattr_bytes_per_vertex(VTMC_LODATTR_MATERIAL) == 8 && lodattr_bytes_per_vertex(VTMC_LODATTR_AO) == 1);

    // n_L: the test scene's 64 x 32 x 32 cells at levels 0, 1, 2 and a 1024-cell axis at every level
    EXPECT(lodattr_lattice_samples(66, 1) == 66 && lodattr_lattice_samples(34, 1) == 34);   // level 0: the grid itself
    EXPECT(lodattr_lattice_samples(66, 2) == 34 && lodattr_lattice_samples(34, 2) == 18);
    EXPECT(lodattr_lattice_samples(66, 4) == 18 && lodattr_lattice_samples(34, 4) == 10);
    for (int level = 0; level <= VTMC_LOD_MAX_LEVEL; ++level) EXPECT(lodattr_lattice_samples(1026, 1 << level) == (1024 >> level) + 2);

    // the second clamp: sample i of the lattice is grid sample i * s up to the last cell corner, and the last one is the replicated plane
    for (int level = 0; level <= VTMC_LOD_MAX_LEVEL; ++level) {
        const int32_t s = 1 << level, dim = 1026, n = lodattr_lattice_samples(dim, s);
        for (int32_t i = 0; i <= n - 2; ++i) EXPECT(lodattr_fine_index(i, s, dim) == i * s);
        EXPECT(lodattr_fine_index(n - 2, s, dim) == dim - 2);
        EXPECT(lodattr_fine_index(n - 1, s, dim) == dim - 1);                                  // not (n - 1) * s = dim - 2 + s
        EXPECT(level == 0 || lodattr_fine_index(n - 2, s, dim) + s != lodattr_fine_index(n - 1, s, dim));   // the upper neighbour is not offset + s
    }
    EXPECT(lodattr_fine_index(17, 4, 66) == 65 && lodattr_fine_index(16, 4, 66) == 64 && lodattr_fine_index(9, 4, 34) == 33);
    EXPECT(lodattr_fine_index(0x7fffffff, 128, 1026) == 1025);                                // no overflow on the way to the clamp

    // the first clamp: a tile wider than the lattice on both sides (level 2 of the test scene at the largest radius: 22 samples over 10)
    {
        const int32_t n = 10, o = 0 - 6;
        for (int32_t x = 0; x < 22; ++x) {
            const int32_t l = lodattr_clamp_lattice(o + x, n);
            EXPECT(l >= 0 && l <= n - 1 && l == (o + x < 0 ? 0 : (o + x > 9 ? 9 : o + x)));
            const int32_t fine = lodattr_fine_index(l, 4, 34);
            EXPECT(fine >= 0 && fine <= 33 && (l == 9 ? fine == 33 : fine == 4 * l));
        }
        EXPECT(lodattr_clamp_lattice(-1, 1) == 0 && lodattr_clamp_lattice(5, 1) == 0);
    }

    // the coordinates.  Materials: (float)o + p * (float)s, the product exact; at s = 1 the block rule's (float)(8 b) + p, bit for bit
    for (float p : {0.0f, 8.0f, 0.3f, 7.9999995f, 1e-30f, 4.4999995f}) {
        for (int32_t b : {0, 1, 7, 127}) EXPECT(bits(lodattr_material_coord(8 * b, p, 1)) == bits((float)(8 * b) + p));
        for (int level = 0; level <= VTMC_LOD_MAX_LEVEL; ++level) {
            const int32_t s = 1 << level, o = 3 * 8 * s;
            const float scaled = p * (float)s;
            EXPECT(scaled / (float)s == p);                                                   // exact: a power of two
            EXPECT(bits(lodattr_material_coord(o, p, s)) == bits((float)o + scaled));
            EXPECT(bits(lodattr_ao_coord(o, s, p)) == bits(24.0f + p));                        // occlusion: (float)(o / s) + p
        }
    }
    EXPECT(lodattr_material_coord(32, 0.5f, 4) == 34.0f && lodattr_ao_coord(32, 4, 0.5f) == 8.5f);
    EXPECT(bits(lodattr_ao_coord(0, 4, 0.0f)) == 0u);                                         // +0, the base of a node at the origin

    // the source map: (b, a, a) and (b, a, b)
    {
        const int32_t want[6] = {0, 1, 1, 0, 1, 0};
        for (int32_t c = 0; c < 6; ++c) EXPECT(lodattr_skirt_source(c) == want[c]);
    }
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("lodattr_host_check: ok\n");
    return failures ? 1 : 0;
}
