// light_host_check.cpp -- a stand-alone run of the host half of the voxel lighting (csrc/terrain_light.h: the argument checks, the seeds,
// one relaxation step on a plain array, the vertex rule and the sizes), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/light_host_check.cpp -o light_host_check && ./light_host_check
// It checks known answers on small arrays -- the corridor of the rule's tests, a wall, two torches, the seeds of sources that share a
// sample -- and exits 0 when every one is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_light.h"
#include <cstdio>
#include <limits>

using namespace vtmc;

static int failures = 0;
#define EXPECT(c) \
    do { \
        if (!(c)) { \
            std::printf("line %d: %s\n", __LINE__, #c); \
            ++failures; \
        } \
    } while (0)

static vtmc_light_source source(float x, float y, float z, int32_t level)
{
    vtmc_light_source s;
    s.position[0] = x, s.position[1] = y, s.position[2] = z, s.level = level;
    return s;
}

// the step repeated from the emissions until nothing changes; returns the rounds, the last, unchanged one included
static int settle(std::vector<uint16_t> &v, const std::vector<uint8_t> &open, const int32_t d[3], int sky_falloff, int torch_falloff)
{
    std::vector<uint16_t> next(v.size());
    for (int round = 1; round <= VTMC_LIGHT_MAX_ROUNDS; ++round) {
        const bool changed = light_relax_step(v.data(), next.data(), open.data(), d, sky_falloff, torch_falloff);
        v.swap(next);
        if (!changed) return round;
    }
    return -1;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(VTMC_LIGHT_MAX_SOURCES == 4096 && VTMC_LIGHT_MAX_ROUNDS == 256 && VTMC_LIGHT_MAX_LEVEL == 255, "include/vtmc_light.h");

    // the argument checks: every fault of include/vtmc_light.h
    const float lo[3] = {-inf, 0.0f, -1e30f}, up[3] = {inf, 5.0f, 1e30f};
    const vtmc_light_params good_p = {255, 1, 255, 0u};
    std::vector<vtmc_light_source> good = {source(1, 2, 3, 1), source(-1e30f, 0, 3e38f, 255), source(0, 0, 0, 17)};
    EXPECT(light_args_fault(lo, up, &good_p, good.data(), 3) == nullptr);
    EXPECT(light_args_fault(lo, up, &good_p, nullptr, 0) == nullptr && light_args_fault(lo, up, &good_p, good.data(), 0) == nullptr);
    EXPECT(light_args_fault(nullptr, up, &good_p, good.data(), 3) != nullptr && light_args_fault(lo, nullptr, &good_p, good.data(), 3) != nullptr);
    EXPECT(light_args_fault(lo, up, nullptr, good.data(), 3) != nullptr);
    EXPECT(light_args_fault(lo, up, &good_p, nullptr, 1) != nullptr && light_args_fault(lo, up, &good_p, good.data(), -1) != nullptr);
    {
        std::vector<vtmc_light_source> many((size_t)VTMC_LIGHT_MAX_SOURCES + 1, source(0, 0, 0, 1));
        EXPECT(light_args_fault(lo, up, &good_p, many.data(), VTMC_LIGHT_MAX_SOURCES) == nullptr);
        EXPECT(light_args_fault(lo, up, &good_p, many.data(), VTMC_LIGHT_MAX_SOURCES + 1) != nullptr);
    }
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {0.0f, 0.0f, 0.0f};
        bad[k] = nan;
        EXPECT(light_args_fault(bad, up, &good_p, good.data(), 3) != nullptr && light_args_fault(lo, bad, &good_p, good.data(), 3) != nullptr);
        for (float v : {nan, inf, -inf}) {
            std::vector<vtmc_light_source> s = good;
            s[1].position[k] = v;
            EXPECT(light_args_fault(lo, up, &good_p, s.data(), 3) != nullptr);
            EXPECT(light_args_fault(lo, up, &good_p, s.data(), 1) == nullptr);   // only the sources of the call are looked at
        }
    }
    for (int32_t level : {0, -1, 256, INT32_MIN, INT32_MAX}) {
        std::vector<vtmc_light_source> s = good;
        s[2].level = level;
        EXPECT(light_args_fault(lo, up, &good_p, s.data(), 3) != nullptr);
    }
    for (int32_t v : {-1, 256, INT32_MIN, INT32_MAX}) {
        vtmc_light_params p = good_p;
        p.sky_level = v;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) != nullptr);
    }
    for (int32_t v : {0, -1, 256, INT32_MIN, INT32_MAX}) {
        vtmc_light_params p = good_p;
        p.sky_falloff = v;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) != nullptr);
        p = good_p, p.torch_falloff = v;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) != nullptr);
    }
    {
        vtmc_light_params p = good_p;
        p.sky_level = 0;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) == nullptr);
        p.flags = 1u;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) != nullptr);
        p.flags = 0x80000000u;
        EXPECT(light_args_fault(lo, up, &p, good.data(), 3) != nullptr);
    }

    // the seeds: scale 0.5, origin (-3, 1, 2), box first (2, 1, 0), dims (5, 4, 3).  Sample (4, 2, 1) lies at (-1, 2, 2.5).
    {
        const float origin[3] = {-3.0f, 1.0f, 2.0f};
        const int32_t first[3] = {2, 1, 0}, d[3] = {5, 4, 3};
        const std::vector<vtmc_light_source> s = {source(-1.0f, 2.0f, 2.5f, 9),     // box sample (2, 1, 1)
                                                  source(-0.9f, 2.1f, 2.4f, 200),   // the same sample, a little off it
                                                  source(-1.0f, 2.0f, 2.5f, 30),    // and once more
                                                  source(-2.5f, 2.0f, 2.5f, 77),    // grid x = 1: outside
                                                  source(0.25f, 3.0f, 3.0f, 5),     // grid (6.5, 4, 2): the half rounds up to 7, outside
                                                  source(0.0f, 3.0f, 3.0f, 5),      // grid (6, 4, 2): the last sample of the box
                                                  source(1e30f, 2.0f, 2.5f, 1)};    // saturates
        const std::vector<LightSeed> seeds = light_seeds(s.data(), (int32_t)s.size(), origin, 0.5f, first, d);
        const int32_t at = 2 + 5 * (1 + 4 * 1), corner = 4 + 5 * (3 + 4 * 2);
        EXPECT(seeds.size() == 7);
        EXPECT(seeds[0].box_index == at && seeds[0].emission == 200);   // the largest level, on the first source of the sample
        EXPECT(seeds[1].box_index == at && seeds[1].emission == 0 && seeds[2].box_index == at && seeds[2].emission == 0);
        EXPECT(seeds[3].box_index == -1 && seeds[4].box_index == -1 && seeds[6].box_index == -1);
        EXPECT(seeds[5].box_index == corner && seeds[5].emission == 5);
        EXPECT(light_seeds(nullptr, 0, origin, 0.5f, first, d).empty());
    }

    // the corridor: 8 x 1 x 1 open samples, a torch of level 10 at x = 1, falloff 3: 7 10 7 4 1 0 0 0, settled after 3 rounds and seen in the 4th
    {
        const int32_t d[3] = {8, 1, 1};
        std::vector<uint8_t> open(8, 1);
        std::vector<uint16_t> v(8, 0);
        v[1] = light_pack(0, 10);
        EXPECT(settle(v, open, d, 1, 3) == 4);
        const int want[8] = {7, 10, 7, 4, 1, 0, 0, 0};
        for (int i = 0; i < 8; ++i) EXPECT(light_channel(v[(size_t)i], 1) == want[i] && light_channel(v[(size_t)i], 0) == 0);
        // a wall at x = 3: nothing passes, and the wall holds 0
        std::fill(v.begin(), v.end(), (uint16_t)0);
        v[1] = light_pack(0, 10), open[3] = 0;
        EXPECT(settle(v, open, d, 1, 3) == 2);
        const int walled[8] = {7, 10, 7, 0, 0, 0, 0, 0};
        for (int i = 0; i < 8; ++i) EXPECT(light_channel(v[(size_t)i], 1) == walled[i]);
    }

    // two torches meet at their maximum, the two channels do not mix, and level 255 with falloff 1 takes 254 hops and 255 rounds
    {
        const int32_t d[3] = {9, 1, 1};
        std::vector<uint8_t> open(9, 1);
        std::vector<uint16_t> v(9, 0);
        v[0] = light_pack(20, 10), v[8] = light_pack(0, 12);
        EXPECT(settle(v, open, d, 5, 2) > 0);
        const int torch[9] = {10, 8, 6, 4, 4, 6, 8, 10, 12}, sky[9] = {20, 15, 10, 5, 0, 0, 0, 0, 0};
        for (int i = 0; i < 9; ++i) EXPECT(light_channel(v[(size_t)i], 1) == torch[i] && light_channel(v[(size_t)i], 0) == sky[i]);
        const int32_t line[3] = {300, 1, 1};
        std::vector<uint8_t> all(300, 1);
        std::vector<uint16_t> w(300, 0);
        w[0] = light_pack(255, 0);
        EXPECT(settle(w, all, line, 1, 1) == 255);
        EXPECT(light_channel(w[254], 0) == 1 && light_channel(w[255], 0) == 0);
        w.assign(300, 0), w[0] = light_pack(255, 0);
        EXPECT(settle(w, all, line, 255, 1) == 1 && light_channel(w[1], 0) == 0);
    }

    // a 3-D box: a 5 x 4 x 3 room, light turns a corner round a pillar; the step against the hop distance by hand
    {
        const int32_t d[3] = {3, 3, 1};
        std::vector<uint8_t> open = {1, 1, 1, 1, 0, 1, 1, 1, 1};   // a ring round a pillar
        std::vector<uint16_t> v(9, 0);
        v[0] = light_pack(0, 9);
        EXPECT(settle(v, open, d, 1, 2) > 0);
        const int want[9] = {9, 7, 5, 7, 0, 3, 5, 3, 1};
        for (int i = 0; i < 9; ++i) EXPECT(light_channel(v[(size_t)i], 1) == want[i]);
    }

    // the vertex rule: the cell origin as the occlusion's fetch finds it, and the largest corner inside the box
    {
        EXPECT(light_cell_origin(-0.5f, 10) == 0 && light_cell_origin(0.0f, 10) == 0 && light_cell_origin(3.999f, 10) == 3 && light_cell_origin(4.0f, 10) == 4);
        EXPECT(light_cell_origin(9.0f, 10) == 8 && light_cell_origin(1e30f, 10) == 8 && light_cell_origin(8.5f, 10) == 8 && light_cell_origin(nan, 10) == 0);
        const int32_t n[3] = {10, 10, 10}, first[3] = {2, 2, 2}, d[3] = {2, 2, 2};
        std::vector<uint16_t> volume(8, 0);
        volume[0] = light_pack(3, 0), volume[7] = light_pack(1, 9), volume[1] = light_pack(5, 2);
        const float inside[3] = {2.5f, 2.25f, 2.75f}, edge[3] = {1.5f, 1.5f, 1.5f}, far[3] = {5.0f, 5.0f, 5.0f}, just[3] = {4.0f, 4.0f, 4.0f}, last[3] = {3.5f, 3.0f, 3.0f};
        EXPECT(light_vertex(volume.data(), first, d, n, inside) == light_pack(5, 9));   // all eight corners
        EXPECT(light_vertex(volume.data(), first, d, n, edge) == light_pack(3, 0));     // one corner, (2, 2, 2)
        EXPECT(light_vertex(volume.data(), first, d, n, far) == 0 && light_vertex(volume.data(), first, d, n, just) == 0);
        EXPECT(light_vertex(volume.data(), first, d, n, last) == light_pack(1, 9));     // the cell (3, 3, 3): one corner inside
    }

    // sizes
    {
        const int32_t a[3] = {1, 1, 1}, b[3] = {64, 8, 8}, c[3] = {65, 9, 9}, e[3] = {1026, 1026, 1026};
        EXPECT(light_samples(a) == 1 && light_mask_words(a) == 1 && light_tiles(a) == 1);
        EXPECT(light_samples(b) == 4096 && light_mask_words(b) == 64 && light_tiles(b) == 1);
        EXPECT(light_samples(c) == 5265 && light_mask_words(c) == 162 && light_tiles(c) == 8);
        EXPECT(light_samples(e) == 1080045576u && light_mask_words(e) == 17u * 1026u * 1026u && light_tiles(e) == 17u * 129u * 129u);
    }

    if (failures) {
        std::printf("light_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("light_host_check: ok\n");
    return 0;
}
