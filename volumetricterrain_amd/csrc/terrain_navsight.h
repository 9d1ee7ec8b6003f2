// terrain_navsight.h -- the host half of the any-angle paths (terrain_navsight.hip): the argument checks of the two entry points, the
// column search, the WALK itself (the one function the kernels, the host and the stand-alone check share) and the sizes.  Plain C++ with
// no device code and no HIP header, so a stand-alone program compiles it for the CPU (tools/navsight_host_check.cpp runs it under the
// host sanitizers and compares the walk with a second formulation).  Every size is 64-bit arithmetic.
#ifndef VTMC_TERRAIN_NAVSIGHT_H
#define VTMC_TERRAIN_NAVSIGHT_H
#include "../../include/vtmc_navsight.h"
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTMC_NAVSIGHT_HD __host__ __device__
#else
#define VTMC_NAVSIGHT_HD
#endif

namespace vtmc {

constexpr int kNavSightColumnSteps = 32;   // halvings of the column search: more than any column count needs

// What is wrong with the arguments of vtmc_nav_sight, the pairs included: -1 or a span of the nav result; *at is the first bad pair
inline const char *navsight_sight_fault(const int32_t *from, const int32_t *to, int32_t n, const vtmc_navsight_hit *hits, int32_t n_spans, int32_t *at)
{
    if (at) *at = -1;
    if (n < 0) return "n < 0";
    if (n > 0 && (!from || !to || !hits)) return "null argument";
    for (int32_t i = 0; i < n; ++i)
        if (from[i] < -1 || from[i] >= n_spans || to[i] < -1 || to[i] >= n_spans) {
            if (at) *at = i;
            return "a span outside -1..n-1";
        }
    return nullptr;
}

// ... and of vtmc_navfield_trace_smooth by value, or null; the starts are vtmc_navfield_trace's to check (navfield_trace_fault)
inline const char *navsight_params_fault(const vtmc_navsight_params *p)
{
    if (!p) return "params is null";
    if (p->max_look < 1 || p->max_look > VTMC_NAVSIGHT_MAX_LOOK) return "max_look outside 1..VTMC_NAVSIGHT_MAX_LOOK";
    if (p->flags != 0u) return "flags != 0";
    if (p->reserved != 0u) return "reserved != 0";
    return nullptr;
}

// NAVSIGHT, Column: the c with offsets[c] <= s < offsets[c + 1] among `columns` > 0 columns, for 0 <= s < offsets[columns].  A bounded
// bisection: it reads offsets[1 .. columns - 1] only and ends after kNavSightColumnSteps halvings whatever the array holds.
template <class Offsets>
VTMC_NAVSIGHT_HD inline int32_t navsight_column(const Offsets &offsets, int32_t columns, int32_t s)
{
    int32_t lo = 0, hi = columns;   // offsets[lo] <= s < offsets[hi]
    for (int step = 0; step < kNavSightColumnSteps && hi - lo > 1; ++step) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Where a walk ended: the span, the links it followed and their cost by the rule (0 when the costs are not asked for)
struct NavSightWalk {
    int32_t last, steps;
    uint64_t w;
};

// NAVSIGHT, Walk: from span a (0 <= a < n) towards the column (ox, oz) columns away.  link(s, k) is link[k] of span s and cost(s, k) is
// c(s, k); both are called with 0 <= s < n only, and whatever link returns is checked against n before it is used.  The loop is bounded
// by nx + nz: every turn of it adds to i or to j.
template <class Link, class Cost>
VTMC_NAVSIGHT_HD inline NavSightWalk navsight_walk(int32_t a, int32_t ox, int32_t oz, int32_t n, const Link &link, const Cost &cost)
{
    const int32_t nx = ox < 0 ? -ox : ox, nz = oz < 0 ? -oz : oz;
    const int kx = ox > 0 ? 1 : 0, kz = oz > 0 ? 3 : 2;
    NavSightWalk r;
    r.last = a, r.steps = 0, r.w = 0;
    int32_t i = 0, j = 0;
    for (int32_t turn = 0; turn < nx + nz && (i < nx || j < nz); ++turn) {
        const int32_t ex = (2 * i + 1) * nz, ez = (2 * j + 1) * nx, s = r.last;
        if (ex != ez) {
            const int k = ex < ez ? kx : kz;
            const int32_t t = link(s, k);
            if (t < 0 || t >= n) break;
            r.w += cost(s, k);
            r.last = t, r.steps += 1;
            if (ex < ez) ++i;
            else ++j;
        } else {
            const int32_t p = link(s, kx), q = link(s, kz);
            if (p < 0 || p >= n || q < 0 || q >= n) break;
            const int32_t t1 = link(p, kz), t2 = link(q, kx);
            if (t1 < 0 || t1 >= n || t2 < 0 || t2 >= n || t1 != t2) break;
            const uint64_t by_x = (uint64_t)cost(s, kx) + cost(p, kz), by_z = (uint64_t)cost(s, kz) + cost(q, kx);
            r.w += by_x > by_z ? by_x : by_z;
            r.last = t1, r.steps += 2;
            ++i, ++j;
        }
    }
    return r;
}

// NAVSIGHT, Smoothed trace, the cost test of a candidate b from the anchor a: w(a -> b) + D(b) <= D(a) + max_extra_cost, in 64 bits
VTMC_NAVSIGHT_HD inline bool navsight_cost_ok(uint64_t w, uint32_t d_b, uint32_t d_a, uint32_t max_extra_cost)
{
    return max_extra_cost == VTMC_NAVSIGHT_ANY_COST || w + d_b <= (uint64_t)d_a + max_extra_cost;
}

// The offset of a chain entry from the start's column, two signed 16-bit halves in one word: a box has at most 1026 columns per axis
VTMC_NAVSIGHT_HD inline uint32_t navsight_pack(int32_t ox, int32_t oz) { return ((uint32_t)ox & 0xffffu) | ((uint32_t)oz << 16); }
VTMC_NAVSIGHT_HD inline int32_t navsight_ox(uint32_t packed) { return (int32_t)(int16_t)(packed & 0xffffu); }
VTMC_NAVSIGHT_HD inline int32_t navsight_oz(uint32_t packed) { return (int32_t)(int16_t)(packed >> 16); }

// The bytes of the answers: the hits of n pairs; the rows of a smoothed trace are navfield_path_bytes, the lengths follow them
inline size_t navsight_hit_bytes(int64_t n) { return (size_t)n * sizeof(vtmc_navsight_hit); }
// ... and of the packed links over n spans, which a smoothed trace makes for itself
inline size_t navsight_link_bytes(int64_t n) { return (size_t)n * 16u; }

}  // namespace vtmc
#endif
