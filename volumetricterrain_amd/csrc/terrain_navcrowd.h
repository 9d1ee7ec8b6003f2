// terrain_navcrowd.h -- the host half of the crowd (terrain_navcrowd.hip): the argument checks of the entry points, the CHOICE of one
// agent in one tick (the one function the kernel, the host and the stand-alone check share), the budget of a tick and the sizes.  Plain
// C++ with no device code and no HIP header, so a stand-alone program compiles it for the CPU (tools/navcrowd_host_check.cpp runs it under
// the host sanitizers and compares the choice with a second formulation).  Every size is 64-bit arithmetic.
#ifndef VTMC_TERRAIN_NAVCROWD_H
#define VTMC_TERRAIN_NAVCROWD_H
#include "../../include/vtmc_navcrowd.h"
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTMC_NAVCROWD_HD __host__ __device__
#else
#define VTMC_NAVCROWD_HD
#endif

namespace vtmc {

constexpr int32_t kNavCrowdNoClaim = 0x7fffffff;   // a claim word nobody has claimed: above every agent index

// What is wrong with the arguments of vtmc_navcrowd_spawn, the requests included; *at is the first bad agent
inline const char *navcrowd_spawn_fault(const int32_t *spans, const uint32_t *speeds, int32_t n_agents, int32_t n_spans, int32_t *at)
{
    if (at) *at = -1;
    if (n_agents < 1 || n_agents > VTMC_NAVCROWD_MAX_AGENTS) return "n_agents outside 1..VTMC_NAVCROWD_MAX_AGENTS";
    if (!spans || !speeds) return "null argument";
    for (int32_t i = 0; i < n_agents; ++i) {
        const bool span_bad = spans[i] < -1 || spans[i] >= n_spans;
        if (span_bad || speeds[i] < 1u || speeds[i] > (uint32_t)VTMC_NAVCROWD_MAX_SPEED) {
            if (at) *at = i;
            return span_bad ? "a span outside -1..n-1" : "a speed outside 1..VTMC_NAVCROWD_MAX_SPEED";
        }
    }
    return nullptr;
}

// ... and of vtmc_navcrowd_step by value, or null
inline const char *navcrowd_step_fault(const vtmc_navcrowd_params *p, int32_t n_ticks)
{
    if (!p) return "params is null";
    if (n_ticks < 0 || n_ticks > VTMC_NAVCROWD_MAX_TICKS) return "n_ticks outside 0..VTMC_NAVCROWD_MAX_TICKS";
    if (p->flags & ~(uint32_t)VTMC_NAVCROWD_LEAVE_ON_ARRIVAL) return "flags other than VTMC_NAVCROWD_LEAVE_ON_ARRIVAL";
    if (p->reserved[0] != 0u || p->reserved[1] != 0u) return "reserved != 0";
    return nullptr;
}

// NAVCROWD, Tick, step 4: what a walking agent holds after the tick's pay
VTMC_NAVCROWD_HD inline uint32_t navcrowd_budget(uint32_t budget, uint32_t speed)
{
    const uint64_t b = (uint64_t)budget + speed;
    return b > (uint64_t)VTMC_NAVCROWD_BUDGET_CAP ? (uint32_t)VTMC_NAVCROWD_BUDGET_CAP : (uint32_t)b;
}

// What an agent decided: the span it claims and what the step costs, or t == -1: it waits
struct NavCrowdChoice {
    int32_t t;
    uint32_t c;
    int32_t k;
};

// NAVCROWD, Tick, steps 5 to 7, of an agent on a span of cost d_s (reached, next != -1) with `budget` after the tick's pay.  link[k] and
// cost[k] are the span's own; d_t[k] is D(link[k]) and occupant[k] the occupancy word of link[k], both read only where 0 <= link[k] < n.
// At most four turns: every turn takes the cheapest candidate left, the smaller k on a tie, and removes it when its span is occupied.
VTMC_NAVCROWD_HD inline NavCrowdChoice navcrowd_choose(uint32_t d_s, const int32_t link[4], const uint32_t cost[4], const uint32_t d_t[4], const int32_t occupant[4],
                                                       int32_t n, uint32_t max_detour, uint32_t budget)
{
    constexpr uint64_t none = ~(uint64_t)0;
    uint64_t key[4];
    for (int k = 0; k < 4; ++k) {
        key[k] = none;
        if (link[k] < 0 || link[k] >= n || d_t[k] == VTMC_NAVFIELD_UNREACHED || d_t[k] >= d_s) continue;
        const uint64_t through = (uint64_t)d_t[k] + cost[k];
        if (max_detour != VTMC_NAVCROWD_ANY_DETOUR && through > (uint64_t)d_s + max_detour) continue;
        key[k] = through;
    }
    NavCrowdChoice wait;
    wait.t = -1, wait.c = 0u, wait.k = -1;
    for (int turn = 0; turn < 4; ++turn) {
        int best = -1;
        for (int k = 0; k < 4; ++k)
            if (key[k] != none && (best < 0 || key[k] < key[best])) best = k;
        if (best < 0) break;
        if (occupant[best] < 0) {   // empty at the start of the tick
            if (budget < cost[best]) break;
            NavCrowdChoice take;
            take.t = link[best], take.c = cost[best], take.k = best;
            return take;
        }
        key[best] = none;
    }
    return wait;
}

// The bytes of a crowd: the agent records, the {target, cost} word pair a tick leaves per agent between its two kernels, and per span the
// occupancy, the claim word and the four packed links
inline size_t navcrowd_agent_bytes(int64_t n_agents) { return (size_t)n_agents * sizeof(vtmc_navcrowd_agent); }
inline size_t navcrowd_pending_bytes(int64_t n_agents) { return (size_t)n_agents * 8u; }
inline size_t navcrowd_word_bytes(int64_t n_spans) { return (size_t)n_spans * 4u; }
inline size_t navcrowd_link_bytes(int64_t n_spans) { return (size_t)n_spans * 16u; }

}  // namespace vtmc
#endif
