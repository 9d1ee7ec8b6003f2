// navfield_host_check.cpp -- a stand-alone run of the host half of the flow fields (csrc/terrain_navfield.h: the edge cost, the argument
// checks of the entry points, the goal validation, the sizes and the round bound), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/navfield_host_check.cpp -o navfield_host_check && ./navfield_host_check
// It checks known answers and exits 0 when every one is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_navfield.h"
#include <cmath>
#include <cstdio>
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

static vtmc_navfield_params params(float climb_cost, float drop_cost, uint32_t max_cost, uint32_t flags)
{
    vtmc_navfield_params p;
    p.climb_cost = climb_cost, p.drop_cost = drop_cost, p.max_cost = max_cost, p.flags = flags;
    return p;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vtmc_navfield_params) == 16 && sizeof(vtmc_navfield_goal) == 8 && sizeof(vtmc_navfield_cell) == 8, "include/vtmc_navfield.h");
    static_assert(VTMC_NAVFIELD_UNIT == 1024 && VTMC_NAVFIELD_UNREACHED == 4294967295u && VTMC_NAVFIELD_MAX_GOALS == 1048576, "include/vtmc_navfield.h");

    // the edge cost against hand values: a level step; 0.5 up at 1 per unit; one ulp more truncates to the same; down takes the other rate
    const float ulp = std::ldexp(1.0f, -22);   // of a height in [2, 4)
    EXPECT(navfield_edge_cost(2.5f, 2.5f, 1024.0f, 1024.0f) == 1024u);
    EXPECT(navfield_edge_cost(2.5f, 3.0f, 1.0f, 9.0f) == 1024u + 512u);
    EXPECT(navfield_edge_cost(2.5f, 3.0f + ulp, 1.0f, 9.0f) == 1024u + 512u);
    EXPECT(navfield_edge_cost(2.5f, 3.0f - ulp, 1.0f, 9.0f) == 1024u + 511u);
    EXPECT(navfield_edge_cost(3.0f, 2.5f, 9.0f, 0.25f) == 1024u + 128u);
    EXPECT(navfield_edge_cost(3.0f, 2.5f, 9.0f, 0.0f) == 1024u && navfield_edge_cost(2.5f, 3.0f, 0.0f, 9.0f) == 1024u);
    // saturation: 2.5 up at 1024 per unit is 2.5 * 2^20; exactly 2^20 saturates to itself, the float under it does not
    EXPECT(navfield_edge_cost(2.5f, 5.0f, 1024.0f, 0.0f) == 1024u + 1048576u && navfield_edge_cost(5.0f, 2.5f, 1024.0f, 0.0f) == 1024u);
    EXPECT(navfield_edge_cost(2.5f, 3.5f, 1024.0f, 0.0f) == 1024u + 1048576u && navfield_edge_cost(2.5f, 3.5f, 1023.0f, 0.0f) == 1024u + 1023u * 1024u);
    EXPECT(navfield_edge_cost(0.0f, 1026.0f, 1024.0f, 0.0f) == 1024u + 1048576u && navfield_edge_cost(1026.0f, 0.0f, 0.0f, 1024.0f) == 1024u + 1048576u);
    EXPECT(navfield_edge_cost(1.0f, 1.0f + std::ldexp(1.0f, -23), 1.0f, 1.0f) == 1024u);   // 2^-13 of a unit: truncated away
    // the largest sum a relaxation forms stays inside 32 bits
    EXPECT((uint64_t)0x7fffffffu + (VTMC_NAVFIELD_UNIT + kNavFieldSaturated) < (uint64_t)VTMC_NAVFIELD_UNREACHED);

    // the parameter checks: every fault of include/vtmc_navfield.h
    const vtmc_navfield_params fine[] = {params(0.0f, 0.0f, 1u, 0u), params(1024.0f, 1024.0f, 0x7fffffffu, 0u), params(-0.0f, 0.5f, 4096u, 0u)};
    for (const vtmc_navfield_params &p : fine) EXPECT(navfield_params_fault(&p) == nullptr);
    EXPECT(navfield_params_fault(nullptr) != nullptr);
    const vtmc_navfield_params faults[] = {params(nan, 0.0f, 1u, 0u),       params(inf, 0.0f, 1u, 0u),       params(-inf, 0.0f, 1u, 0u),
                                           params(-1.0f, 0.0f, 1u, 0u),     params(1024.5f, 0.0f, 1u, 0u),   params(0.0f, nan, 1u, 0u),
                                           params(0.0f, inf, 1u, 0u),       params(0.0f, -0.5f, 1u, 0u),     params(0.0f, 1025.0f, 1u, 0u),
                                           params(1.0f, 1.0f, 0u, 0u),      params(1.0f, 1.0f, 0x80000000u, 0u), params(1.0f, 1.0f, 0xffffffffu, 0u),
                                           params(1.0f, 1.0f, 1u, 1u),      params(1.0f, 1.0f, 1u, 0x80000000u)};
    for (const vtmc_navfield_params &p : faults) EXPECT(navfield_params_fault(&p) != nullptr);

    // the goal validation: count, spans against n, costs against max_cost; the first bad record is named
    std::vector<vtmc_navfield_goal> goals = {{0, 0u}, {9, 5000u}, {9, 0u}, {4, 5000u}};
    int32_t at = 7;
    EXPECT(navfield_goals_fault(goals.data(), 4, 10, 5000u, &at) == nullptr && at == -1);
    EXPECT(navfield_goals_fault(goals.data(), 4, 10, 5000u, nullptr) == nullptr);
    EXPECT(navfield_goals_fault(nullptr, 4, 10, 5000u, &at) != nullptr && navfield_goals_fault(goals.data(), 0, 10, 5000u, &at) != nullptr);
    EXPECT(navfield_goals_fault(goals.data(), -1, 10, 5000u, &at) != nullptr && navfield_goals_fault(goals.data(), VTMC_NAVFIELD_MAX_GOALS + 1, 10, 5000u, &at) != nullptr);
    EXPECT(at == -1);   // refused by the count: no record was read
    EXPECT(navfield_goals_fault(goals.data(), 4, 9, 5000u, &at) != nullptr && at == 1);      // span 9 of 9 spans
    EXPECT(navfield_goals_fault(goals.data(), 4, 10, 4999u, &at) != nullptr && at == 1);     // cost above max_cost
    EXPECT(navfield_goals_fault(goals.data(), 1, 10, 4999u, &at) == nullptr && navfield_goals_fault(goals.data(), 4, 0, 5000u, &at) != nullptr && at == 0);
    goals[2].span = -1;
    EXPECT(navfield_goals_fault(goals.data(), 4, 10, 5000u, &at) != nullptr && at == 2 && navfield_goals_fault(goals.data(), 2, 10, 5000u, &at) == nullptr);
    goals[2].span = 2147483647;
    EXPECT(navfield_goals_fault(goals.data(), 4, 2147483647, 5000u, &at) != nullptr && at == 2);
    {
        std::vector<vtmc_navfield_goal> most((size_t)VTMC_NAVFIELD_MAX_GOALS, vtmc_navfield_goal{3, 1u});   // the most the call takes: every record is read
        EXPECT(navfield_goals_fault(most.data(), VTMC_NAVFIELD_MAX_GOALS, 4, 1u, &at) == nullptr);
        most.back().cost = 2u;
        EXPECT(navfield_goals_fault(most.data(), VTMC_NAVFIELD_MAX_GOALS, 4, 1u, &at) != nullptr && at == VTMC_NAVFIELD_MAX_GOALS - 1);
    }

    // locate: the count, the two distances, the pointers only when there is something to do
    const float pos[6] = {0, 0, 0, 1, 1, 1};
    int32_t out[4] = {0, 0, 0, 0};
    EXPECT(navfield_locate_fault(pos, 2, 0.0f, 0.0f, out) == nullptr && navfield_locate_fault(nullptr, 0, 1.0f, 2.0f, nullptr) == nullptr);
    EXPECT(navfield_locate_fault(pos, -1, 1.0f, 1.0f, out) != nullptr && navfield_locate_fault(nullptr, 2, 1.0f, 1.0f, out) != nullptr);
    EXPECT(navfield_locate_fault(pos, 2, 1.0f, 1.0f, nullptr) != nullptr && navfield_locate_fault(pos, 2, nan, 1.0f, out) != nullptr);
    EXPECT(navfield_locate_fault(pos, 2, 1.0f, inf, out) != nullptr && navfield_locate_fault(pos, 2, -0.5f, 1.0f, out) != nullptr);
    EXPECT(navfield_locate_fault(pos, 2, 1.0f, -1.0f, out) != nullptr && navfield_locate_fault(pos, 0, nan, 1.0f, out) != nullptr);

    // trace: -1 is a start (a locate miss); anything else outside the spans refuses the whole call
    const int32_t starts[4] = {0, -1, 9, 3};
    int32_t paths[16], lengths[4];
    EXPECT(navfield_trace_fault(starts, 4, 4, paths, lengths, 10, &at) == nullptr && at == -1);
    EXPECT(navfield_trace_fault(starts, 4, 4, paths, lengths, 9, &at) != nullptr && at == 2);
    EXPECT(navfield_trace_fault(starts, 2, 4, paths, lengths, 1, &at) == nullptr && navfield_trace_fault(nullptr, 0, 1, nullptr, nullptr, 10, &at) == nullptr);
    EXPECT(navfield_trace_fault(starts, -1, 4, paths, lengths, 10, &at) != nullptr && navfield_trace_fault(starts, 4, 0, paths, lengths, 10, &at) != nullptr);
    EXPECT(navfield_trace_fault(nullptr, 4, 4, paths, lengths, 10, &at) != nullptr && navfield_trace_fault(starts, 4, 4, nullptr, lengths, 10, &at) != nullptr);
    EXPECT(navfield_trace_fault(starts, 4, 4, paths, nullptr, 10, &at) != nullptr);
    const int32_t low[2] = {0, -2};
    EXPECT(navfield_trace_fault(low, 2, 4, paths, lengths, 10, &at) != nullptr && at == 1);

    // the sizes, in 64 bits; the runs; the round bound
    EXPECT(navfield_cell_bytes(0) == 0 && navfield_cell_bytes(3) == 24 && navfield_cell_bytes(2147483647) == 17179869176ull);
    EXPECT(navfield_work_bytes(3) == 72 && navfield_work_bytes(2147483647) == 51539607528ull);
    EXPECT(navfield_path_bytes(3, 4096) == 49152 && navfield_path_bytes(2147483647, 2147483647) == 18446744056529682436ull);
    EXPECT(navfield_runs(0) == 0 && navfield_runs(1) == 1 && navfield_runs(kNavFieldRun) == 1 && navfield_runs(kNavFieldRun + 1) == 2 && navfield_runs(2147483647) == 524288);
    EXPECT(navfield_max_rounds(1) == 2 && navfield_max_rounds(2147483647) == 2147483648ll);
    static_assert(kNavFieldRun == 4096 && kNavFieldBatch >= 1, "a run is 256 spans or more");

    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("navfield_host_check: ok\n");
    return failures ? 1 : 0;
}
