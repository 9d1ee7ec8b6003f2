// material_host_check.cpp -- a stand-alone run of the host half of the material layer (csrc/terrain_material.h: the argument checks, the
// stroke records, the sx / ts factors and the texel box of a paint call), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/material_host_check.cpp -o material_host_check && ./material_host_check
// Exits 0 when every answer is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_material.h"
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace vtmc;

static int failures = 0;
#define EXPECT(c) \
    do { \
        if (!(c)) { \
            std::printf("line %d: %s\n", __LINE__, #c); \
            ++failures; \
        } \
    } while (0)

static vtmc_material_stroke stroke(float x, float y, float z, float r, float s, int32_t ch)
{
    vtmc_material_stroke k;
    k.center[0] = x, k.center[1] = y, k.center[2] = z;
    k.radius = r, k.strength = s, k.channel = ch;
    return k;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vtmc_material_stroke) == 24, "the record the kernel reads");

    EXPECT(material_size(0) == 0 && material_size(9) == 0 && material_size(-3) == 0);
    EXPECT(material_size(1) == 16 && material_size(8) == 128);

    // the checks: every fault of include/vtmc.h, and the index of the first faulty stroke
    EXPECT(material_stroke_fault(stroke(1, 2, 3, 4, 0.5f, 7)) == nullptr);
    EXPECT(material_stroke_fault(stroke(1, 2, 3, 4, 0.0f, 0)) == nullptr && material_stroke_fault(stroke(1, 2, 3, 4, 1.0f, 0)) == nullptr);
    const vtmc_material_stroke bad[] = {stroke(nan, 0, 0, 1, 1, 0), stroke(0, inf, 0, 1, 1, 0), stroke(0, 0, -inf, 1, 1, 0), stroke(0, 0, 0, nan, 1, 0),
                                        stroke(0, 0, 0, inf, 1, 0), stroke(0, 0, 0, 0, 1, 0), stroke(0, 0, 0, -1, 1, 0), stroke(0, 0, 0, 1, nan, 0),
                                        stroke(0, 0, 0, 1, inf, 0), stroke(0, 0, 0, 1, -0.25f, 0), stroke(0, 0, 0, 1, 1.25f, 0), stroke(0, 0, 0, 1, 1, -1),
                                        stroke(0, 0, 0, 1, 1, 8)};
    for (const vtmc_material_stroke &b : bad) {
        EXPECT(material_stroke_fault(b) != nullptr);
        std::vector<vtmc_material_stroke> q(VTMC_MATERIAL_MAX_STROKES, stroke(1, 2, 3, 4, 1, 5));
        const char *fault = nullptr;
        EXPECT(material_check_strokes(q.data(), (int32_t)q.size(), &fault) == -1 && fault == nullptr);
        q[4095] = b;
        q[17] = b;
        EXPECT(material_check_strokes(q.data(), (int32_t)q.size(), &fault) == 17 && fault != nullptr);
    }
    const char *fault = nullptr;
    EXPECT(material_check_strokes(nullptr, 0, &fault) == -1);

    // the factors: FP32, the operations of the header
    const int cells[3] = {64, 24, 48};
    float ts[3], sx[3];
    material_texel_size(cells, 0.5f, 16, ts);
    EXPECT(ts[0] == 2.0f && ts[1] == 0.75f && ts[2] == 1.5f);
    material_vertex_scale(cells, 16, sx);
    EXPECT(sx[0] == 0.25f && sx[1] == 16.0f / 24.0f && sx[2] == 16.0f / 48.0f);
    material_texel_size(cells, 0.3f, 48, ts);
    EXPECT(ts[1] == (24.0f * 0.3f) / 48.0f);

    // the image check and the checked copy
    std::vector<float> img(4 * 16 * 16 * 16, 0.25f), copy(img.size(), -1.0f);
    EXPECT(material_first_nan(img.data(), img.size()) == -1);
    EXPECT(material_copy_checked(copy.data(), img.data(), img.size()) == -1 && std::memcmp(copy.data(), img.data(), img.size() * sizeof(float)) == 0);
    img[img.size() - 1] = nan;
    img[777] = nan;
    EXPECT(material_first_nan(img.data(), img.size()) == 777 && material_copy_checked(copy.data(), img.data(), img.size()) == 777);
    img[5] = inf;   // an infinity is no NaN: it clamps
    EXPECT(material_first_nan(img.data(), 700) == -1);
    EXPECT(material_first_nan(img.data(), 0) == -1);

    // the paint box: holds every texel within r of a centre, never leaves 0..C-1, empty when nothing is reached
    const float origin[3] = {3.0f, -2.0f, 7.5f};
    material_texel_size(cells, 0.5f, 16, ts);
    {
        const vtmc_material_stroke s = stroke(12.0f, 4.0f, 18.0f, 3.0f, 1, 0);
        const MaterialBox b = material_paint_box(&s, 1, ts, origin, 16);
        for (int k = 0; k < 3; ++k) {
            EXPECT(b.lo[k] >= 0 && b.n[k] > 0 && b.lo[k] + b.n[k] <= 16);
            for (int i = 0; i < 16; ++i) {
                const double centre = (i + 0.5) * ts[k] + origin[k];
                if (std::fabs(centre - s.center[k]) < s.radius) EXPECT(i >= b.lo[k] && i < b.lo[k] + b.n[k]);
            }
        }
        EXPECT(b.n[0] < 16);   // a saving: not the whole axis
    }
    {
        const vtmc_material_stroke s[2] = {stroke(3.0f, -2.0f, 7.5f, 2.5f, 1, 0), stroke(35.0f, 10.0f, 31.5f, 3.0f, 1, 1)};   // both corners
        const MaterialBox b = material_paint_box(s, 2, ts, origin, 16);
        for (int k = 0; k < 3; ++k) EXPECT(b.lo[k] == 0 && b.n[k] == 16);
    }
    {
        const vtmc_material_stroke s = stroke(-40.0f, 50.0f, 90.0f, 3.0f, 1, 0);   // far outside
        const MaterialBox b = material_paint_box(&s, 1, ts, origin, 16);
        EXPECT(b.n[0] == 0 && b.n[1] == 0 && b.n[2] == 0);
    }
    {
        const vtmc_material_stroke s = stroke(1e30f, 0, 0, 3e38f, 1, 0);   // huge: the whole cube, no overflow of an index
        const MaterialBox b = material_paint_box(&s, 1, ts, origin, 16);
        for (int k = 0; k < 3; ++k) EXPECT(b.lo[k] == 0 && b.n[k] == 16);
    }
    {
        const float far_origin[3] = {1e7f, 1e7f, 1e7f};   // a texel far below the coordinates' precision: the whole cube
        const vtmc_material_stroke s = stroke(1e7f, 1e7f, 1e7f, 1.0f, 1, 0);
        const MaterialBox b = material_paint_box(&s, 1, ts, far_origin, 16);
        for (int k = 0; k < 3; ++k) EXPECT(b.lo[k] == 0 && b.n[k] == 16);
    }
    {
        const MaterialBox b = material_paint_box(nullptr, 0, ts, origin, 16);
        EXPECT(b.n[0] == 0 && b.n[1] == 0 && b.n[2] == 0);
    }
    std::printf(failures ? "%d checks failed\n" : "material_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
