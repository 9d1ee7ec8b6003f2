// terrain_navfield.h -- the host half of the flow fields (terrain_navfield.hip): the edge cost, the argument checks of the six entry points,
// the goal validation, the buffer sizes and the round bound.  Plain C++ with no device code and no HIP header, so a stand-alone program
// compiles it for the CPU (tools/navfield_host_check.cpp runs it under the host sanitizers); the edge cost is the one function the
// kernels share with it.  Every size is 64-bit arithmetic.
#ifndef VTMC_TERRAIN_NAVFIELD_H
#define VTMC_TERRAIN_NAVFIELD_H
#include "../../include/vtmc_navfield.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTMC_NAVFIELD_HD __host__ __device__
#else
#define VTMC_NAVFIELD_HD
#endif

namespace vtmc {

constexpr int kNavFieldRun = 4096;      // consecutive spans a workgroup of the relaxation owns
constexpr int kNavFieldBatch = 4;       // rounds launched per read-back of the flag words
constexpr uint32_t kNavFieldSaturated = 1u << 20;   // the most a height difference adds to an edge

// NAVFIELD, Edge cost: the directed link from a span of height hs to one of height ht.  One IEEE operation per line (the library and the
// stand-alone check are built with -ffp-contract=off; there is no add to fuse anyway).  q is never NaN by the rule; a NaN would cost 1024.
VTMC_NAVFIELD_HD inline uint32_t navfield_edge_cost(float hs, float ht, float climb_cost, float drop_cost)
{
    const float d = ht - hs;
    const float w = d > 0.0f ? d * climb_cost : (-d) * drop_cost;
    const float q = w * 1024.0f;
    const uint32_t extra = q >= 1048576.0f ? kNavFieldSaturated : q > 0.0f ? (uint32_t)q : 0u;
    return (uint32_t)VTMC_NAVFIELD_UNIT + extra;
}

// What is wrong with the parameters of vtmc_navfield_build by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *navfield_params_fault(const vtmc_navfield_params *p)
{
    if (!p) return "params is null";
    if (!std::isfinite(p->climb_cost) || p->climb_cost < 0.0f || p->climb_cost > 1024.0f) return "climb_cost must be finite and in [0, 1024]";
    if (!std::isfinite(p->drop_cost) || p->drop_cost < 0.0f || p->drop_cost > 1024.0f) return "drop_cost must be finite and in [0, 1024]";
    if (p->max_cost < 1u || p->max_cost > 0x7fffffffu) return "max_cost outside 1..0x7fffffff";
    if (p->flags != 0u) return "flags != 0";
    return nullptr;
}

// ... and with its goals, against the n_spans of the nav result and the (valid) max_cost; *at is the first bad record
inline const char *navfield_goals_fault(const vtmc_navfield_goal *goals, int32_t n_goals, int32_t n_spans, uint32_t max_cost, int32_t *at)
{
    if (at) *at = -1;
    if (!goals) return "goals is null";
    if (n_goals < 1 || n_goals > VTMC_NAVFIELD_MAX_GOALS) return "n_goals outside 1..VTMC_NAVFIELD_MAX_GOALS";
    for (int32_t i = 0; i < n_goals; ++i) {
        const bool span_bad = goals[i].span < 0 || goals[i].span >= n_spans;
        if (span_bad || goals[i].cost > max_cost) {
            if (at) *at = i;
            return span_bad ? "a goal span outside 0..n-1" : "a goal cost above max_cost";
        }
    }
    return nullptr;
}

// vtmc_nav_locate's arguments
inline const char *navfield_locate_fault(const float *positions, int32_t n, float below, float above, const int32_t *spans_out)
{
    if (n < 0) return "n < 0";
    if (!std::isfinite(below) || below < 0.0f || !std::isfinite(above) || above < 0.0f) return "below and above must be finite and >= 0";
    if (n > 0 && (!positions || !spans_out)) return "null argument";
    return nullptr;
}

// vtmc_navfield_trace's arguments, the starts included: -1 (a locate miss) or a span of the field; *at is the first bad start
inline const char *navfield_trace_fault(const int32_t *starts, int32_t n_starts, int32_t max_len, const int32_t *paths, const int32_t *lengths,
                                        int32_t n_spans, int32_t *at)
{
    if (at) *at = -1;
    if (n_starts < 0) return "n_starts < 0";
    if (max_len < 1) return "max_len < 1";
    if (n_starts > 0 && (!starts || !paths || !lengths)) return "null argument";
    for (int32_t i = 0; i < n_starts; ++i)
        if (starts[i] < -1 || starts[i] >= n_spans) {
            if (at) *at = i;
            return "a start outside -1..n-1";
        }
    return nullptr;
}

// The bytes of a field over n spans: the cells; the work words (the four edge costs, 16 bytes, then the cost D and the cheapest goal cost,
// 4 bytes each); of a trace: the rows (the lengths follow them); the runs of the relaxation
inline size_t navfield_cell_bytes(int64_t n) { return (size_t)n * sizeof(vtmc_navfield_cell); }
inline size_t navfield_work_bytes(int64_t n) { return (size_t)n * 24u; }
inline size_t navfield_path_bytes(int64_t n_starts, int64_t max_len) { return (size_t)n_starts * (size_t)max_len * 4u; }
inline int64_t navfield_runs(int64_t n) { return (n + kNavFieldRun - 1) / kNavFieldRun; }
// The round bound: a round that changes anything settles at least one more span for good, so n rounds and the one that finds nothing
inline int64_t navfield_max_rounds(int64_t n) { return n + 1; }

}  // namespace vtmc
#endif
