// water_host_check.cpp -- a stand-alone run of the host half of the flood (csrc/terrain_water.h: the argument checks, the levels in the
// order they are processed, the level -> plane search, the nearest sample and the dims of the volumes), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/water_host_check.cpp -o water_host_check && ./water_host_check
// It checks known answers, and the plane search against a scan over every plane for awkward scales and origins, and exits 0 when every one
// is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_water.h"
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

static vtmc_water_source source(float x, float y, float z, float level)
{
    vtmc_water_source s;
    s.position[0] = x, s.position[1] = y, s.position[2] = z, s.level = level;
    return s;
}

// the rule itself: the highest plane with y_j <= level, by looking at every plane
static int32_t plane_by_scan(float level, float scale, float origin_y, int32_t dim_y)
{
    int32_t best = -1;
    for (int32_t j = 0; j < dim_y; ++j)
        if (water_plane_height(j, scale, origin_y) <= level) best = j;
    return best;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vtmc_water_source) == 16 && sizeof(vtmc_water_body) == 64 && VTMC_WATER_MAX_SOURCES == 4096 && VTMC_WATER_MAX_LEVELS == 8, "include/vtmc_water.h");

    // the argument checks: every fault of include/vtmc_water.h
    const float lo[3] = {-inf, 0.0f, -1e30f}, up[3] = {inf, 5.0f, 1e30f};
    std::vector<vtmc_water_source> good = {source(1, 2, 3, 4), source(-1e30f, 0, 3e38f, -0.0f), source(0, 0, 0, 0.0f)};
    EXPECT(flood_args_fault(lo, up, good.data(), 3, 0) == nullptr);
    EXPECT(flood_args_fault(lo, up, nullptr, 0, 0) == nullptr && flood_args_fault(lo, up, good.data(), 0, 0) == nullptr);
    EXPECT(flood_args_fault(nullptr, up, good.data(), 3, 0) != nullptr && flood_args_fault(lo, nullptr, good.data(), 3, 0) != nullptr);
    EXPECT(flood_args_fault(lo, up, nullptr, 1, 0) != nullptr && flood_args_fault(lo, up, good.data(), -1, 0) != nullptr);
    EXPECT(flood_args_fault(lo, up, good.data(), 3, 1) != nullptr && flood_args_fault(lo, up, good.data(), 3, 0x80000000u) != nullptr);
    for (int k = 0; k < 3; ++k) {
        float bad[3] = {0.0f, 0.0f, 0.0f};
        bad[k] = nan;
        EXPECT(flood_args_fault(bad, up, good.data(), 3, 0) != nullptr && flood_args_fault(lo, bad, good.data(), 3, 0) != nullptr);
        for (float v : {nan, inf, -inf}) {
            std::vector<vtmc_water_source> s = good;
            s[1].position[k] = v;
            EXPECT(flood_args_fault(lo, up, s.data(), 3, 0) != nullptr);
            EXPECT(flood_args_fault(lo, up, s.data(), 1, 0) == nullptr);   // only the sources of the call are looked at
        }
    }
    for (float v : {nan, inf, -inf}) {
        std::vector<vtmc_water_source> s = good;
        s[2].level = v;
        EXPECT(flood_args_fault(lo, up, s.data(), 3, 0) != nullptr);
    }
    std::vector<vtmc_water_source> many((size_t)VTMC_WATER_MAX_SOURCES + 1, source(0, 0, 0, 1.0f));
    EXPECT(flood_args_fault(lo, up, many.data(), VTMC_WATER_MAX_SOURCES, 0) == nullptr && flood_args_fault(lo, up, many.data(), VTMC_WATER_MAX_SOURCES + 1, 0) != nullptr);
    for (int i = 0; i < VTMC_WATER_MAX_SOURCES; ++i) many[(size_t)i].level = (float)(i % 8);
    EXPECT(flood_args_fault(lo, up, many.data(), VTMC_WATER_MAX_SOURCES, 0) == nullptr);
    many[4000].level = 8.0f;   // a ninth level
    EXPECT(flood_args_fault(lo, up, many.data(), VTMC_WATER_MAX_SOURCES, 0) != nullptr && flood_args_fault(lo, up, many.data(), 4000, 0) == nullptr);
    many[4000].level = -0.0f;  // levels are told apart by their bits: -0 is a ninth beside +0
    EXPECT(flood_args_fault(lo, up, many.data(), VTMC_WATER_MAX_SOURCES, 0) != nullptr);

    // the levels: descending, +0 before -0, each bit pattern once
    const std::vector<vtmc_water_source> mixed = {source(0, 0, 0, 1.0f), source(0, 0, 0, -0.0f), source(0, 0, 0, 7.0f), source(0, 0, 0, 0.0f), source(0, 0, 0, 1.0f),
                                                  source(0, 0, 0, -3.5f)};
    const std::vector<float> levels = water_levels(mixed.data(), (int32_t)mixed.size());
    EXPECT(levels.size() == 5 && levels[0] == 7.0f && levels[1] == 1.0f && water_bits(levels[2]) == 0u && water_bits(levels[3]) == 0x80000000u && levels[4] == -3.5f);
    EXPECT(water_levels(nullptr, 0).empty());

    // the level -> plane search against the scan, over awkward scales and origins: levels on, just under and just over every plane
    const float scales[] = {0.5f, 1.0f, 0.1f, 0.3f, 1.0f / 3.0f, 7.77f, 1e-3f, 1e-20f, 3e37f, 1.17549435e-38f, 1e6f};
    const float origins[] = {0.0f, 1.0f, -3.0f, 0.1f, -1e-3f, 1e7f, -1e7f, 16777216.0f, 3e38f, -3e38f, 1e-30f};
    const int32_t dims[] = {1, 2, 3, 26, 1026};
    long checked = 0;
    for (float scale : scales)
        for (float origin : origins)
            for (int32_t dim : dims) {
                for (int32_t j = 0; j < dim; j += dim > 64 ? 41 : 1) {
                    const float y = water_plane_height(j, scale, origin);
                    for (float level : {y, std::nextafter(y, -inf), std::nextafter(y, inf), y - 0.5f * scale, y + 0.5f * scale}) {
                        if (!std::isfinite(level)) continue;
                        const int32_t got = water_plane(level, scale, origin, dim), want = plane_by_scan(level, scale, origin, dim);
                        if (got != want) {
                            std::printf("plane: scale %g origin %g dim %d level %.9g: %d, the scan says %d\n", scale, origin, dim, level, got, want);
                            ++failures;
                        }
                        ++checked;
                    }
                }
                EXPECT(water_plane(-3.4e38f, scale, origin, dim) == plane_by_scan(-3.4e38f, scale, origin, dim));
                EXPECT(water_plane(3.4e38f, scale, origin, dim) == plane_by_scan(3.4e38f, scale, origin, dim));
            }
    EXPECT(checked > 10000);
    EXPECT(water_plane(1.0f, 0.5f, 1.0f, 26) == 0 && water_plane(0.99f, 0.5f, 1.0f, 26) == -1 && water_plane(1.24f, 0.5f, 1.0f, 26) == 0 && water_plane(99.0f, 0.5f, 1.0f, 26) == 25);
    EXPECT(water_plane(1.0f, 0.5f, nan, 26) == -1);   // a NaN origin: no plane is under anything

    // the dims of the volumes: whole 8-cell blocks, never fewer than the box's samples
    const int32_t d_in[] = {1, 2, 3, 10, 11, 18, 19, 20, 26, 30, 42, 80, 138, 1025, 1026}, d_out[] = {10, 10, 10, 10, 18, 18, 26, 26, 26, 34, 42, 82, 138, 1026, 1026};
    for (size_t i = 0; i < sizeof d_in / sizeof *d_in; ++i) EXPECT(water_volume_dim(d_in[i]) == d_out[i]);
    for (int32_t d = 1; d <= 1026; ++d) EXPECT(water_volume_dim(d) >= d && water_volume_dim(d) < d + 10 && (water_volume_dim(d) - 2) % 8 == 0 && water_volume_dim(d) >= 10);

    // the nearest sample: halves round up, the conversion saturates, NaN is outside everything
    EXPECT(water_nearest(-3.0f, -3.0f, 0.5f) == 0 && water_nearest(-2.75f, -3.0f, 0.5f) == 1 && water_nearest(-2.76f, -3.0f, 0.5f) == 0 && water_nearest(-3.26f, -3.0f, 0.5f) == -1);
    EXPECT(water_nearest(-3.25f, -3.0f, 0.5f) == 0 && water_nearest(65.9f, -3.0f, 0.5f) == 138);
    EXPECT(water_nearest(1e30f, -3.0f, 0.5f) == INT32_MAX && water_nearest(-1e30f, -3.0f, 0.5f) == INT32_MIN && water_nearest(nan, -3.0f, 0.5f) == INT32_MIN);
    EXPECT(water_nearest(3e38f, -3e38f, 1e-30f) == INT32_MAX && water_nearest(2147483520.0f, 0.0f, 1.0f) == 2147483520 && water_nearest(2147483648.0f, 0.0f, 1.0f) == INT32_MAX);
    EXPECT(water_nearest(-2147483648.0f, 0.0f, 1.0f) == INT32_MIN);

    // the seeds of a level: the caller's order, the box-linear and the volume index, -1 outside the box
    const float origin[3] = {-3.0f, 1.0f, 2.0f};
    const int32_t box_lo[3] = {30, 2, 2}, box_d[3] = {80, 20, 30}, vd[3] = {82, 26, 34};
    const std::vector<vtmc_water_source> src = {source(-3.0f + 0.5f * 30, 1.0f + 0.5f * 2, 2.0f + 0.5f * 2, 5.0f), source(-3.0f + 0.5f * 109, 1.0f + 0.5f * 21, 2.0f + 0.5f * 31, 5.0f),
                                                source(0, 0, 0, 4.0f), source(-3.0f + 0.5f * 29, 2.0f, 3.0f, 5.0f), source(-3.0f + 0.5f * 110, 2.0f, 3.0f, 5.0f), source(1e30f, 2.0f, 3.0f, 5.0f)};
    std::vector<WaterSeed> seeds;
    water_level_seeds(src.data(), (int32_t)src.size(), 5.0f, origin, 0.5f, box_lo, box_d, vd, seeds);
    EXPECT(seeds.size() == 5 && seeds[0].source == 0 && seeds[1].source == 1 && seeds[2].source == 3 && seeds[4].source == 5);
    EXPECT(seeds[0].box_index == 0 && seeds[0].volume_index == 0);
    EXPECT(seeds[1].box_index == 79 + 80 * (19 + 20 * 29) && seeds[1].volume_index == 79 + 82 * (19 + 26 * 29));
    EXPECT(seeds[2].box_index == -1 && seeds[3].box_index == -1 && seeds[4].box_index == -1 && seeds[4].volume_index == -1);
    water_level_seeds(src.data(), (int32_t)src.size(), 4.0f, origin, 0.5f, box_lo, box_d, vd, seeds);
    EXPECT(seeds.size() == 6 && seeds[5].source == 2 && seeds[5].box_index == -1);

    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("water_host_check: ok\n");
    return failures ? 1 : 0;
}
