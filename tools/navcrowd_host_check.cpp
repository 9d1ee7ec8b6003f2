// navcrowd_host_check.cpp -- a stand-alone run of the host half of the crowd (csrc/terrain_navcrowd.h: the argument checks, the budget of
// a tick, the choice of one agent that the claim kernel calls, the sizes), for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/navcrowd_host_check.cpp -o navcrowd_host_check && ./navcrowd_host_check
// It checks known answers, and the choice of every span of several random small graphs, under several occupancies, budgets and detours,
// against a second formulation written here: the candidates as a list, sorted by (D(t) + c, k), and then walked.  Exits 0 when every
// answer is the expected one.
#include "../volumetricterrain_amd/csrc/terrain_navcrowd.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
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

static vtmc_navcrowd_params params(uint32_t detour, uint32_t flags = 0u, uint32_t r0 = 0u, uint32_t r1 = 0u)
{
    vtmc_navcrowd_params p;
    p.max_detour = detour, p.flags = flags, p.reserved[0] = r0, p.reserved[1] = r1;
    return p;
}

static uint32_t lcg(uint32_t &state)
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

// A random small graph: n spans, four links each (some missing, some out of range, as a damaged record would hold them), a cost per link,
// a field value per span (some unreached) and an occupancy word per span
struct Graph {
    int n = 0;
    std::vector<int32_t> link, occupant;
    std::vector<uint32_t> cost, D;
};

static Graph make_graph(int n, uint32_t seed, unsigned missing, unsigned unreached, unsigned occupied, bool near)
{
    Graph g;
    g.n = n;
    uint32_t st = seed;
    for (int s = 0; s < n; ++s) {
        // near: costs and field values close together, so that sums tie and the detour bound decides
        g.D.push_back((lcg(st) & 255u) < unreached ? VTMC_NAVFIELD_UNREACHED : near ? 4096u + 512u * (lcg(st) & 7u) : lcg(st) & 0x7fffffu);
        g.occupant.push_back((lcg(st) & 255u) < occupied ? (int32_t)(lcg(st) & 0xffffu) : -1);
        for (int k = 0; k < 4; ++k) {
            const unsigned r = lcg(st) & 255u;
            g.link.push_back(r < missing ? -1 : r == 255u ? n + (int32_t)(lcg(st) & 3u) : r == 254u ? -2147483647 - 1 : (int32_t)(lcg(st) % (uint32_t)n));
            g.cost.push_back(near ? 1024u + 512u * (lcg(st) & 3u) : 1024u + (lcg(st) & 0xfffffu));
        }
    }
    return g;
}

// The second formulation, from the rule's text: steps 5, 6 and 7
static NavCrowdChoice slow_choose(const Graph &g, int s, uint32_t max_detour, uint32_t budget)
{
    std::vector<std::tuple<uint64_t, int, int32_t, uint32_t>> candidates;
    for (int k = 0; k < 4; ++k) {
        const int32_t t = g.link[(size_t)s * 4 + k];
        if (t < 0 || t >= g.n) continue;
        if (g.D[(size_t)t] == VTMC_NAVFIELD_UNREACHED || !(g.D[(size_t)t] < g.D[(size_t)s])) continue;
        const uint32_t c = g.cost[(size_t)s * 4 + k];
        if (max_detour != VTMC_NAVCROWD_ANY_DETOUR && (uint64_t)g.D[(size_t)t] + c > (uint64_t)g.D[(size_t)s] + max_detour) continue;
        candidates.emplace_back((uint64_t)g.D[(size_t)t] + c, k, t, c);
    }
    std::sort(candidates.begin(), candidates.end());
    NavCrowdChoice r;
    r.t = -1, r.c = 0u, r.k = -1;
    for (const auto &cand : candidates) {
        if (g.occupant[(size_t)std::get<2>(cand)] >= 0) continue;
        if (budget >= std::get<3>(cand)) r.t = std::get<2>(cand), r.c = std::get<3>(cand), r.k = std::get<1>(cand);
        break;   // the first empty one, whether the budget reaches or not
    }
    return r;
}

static NavCrowdChoice fast_choose(const Graph &g, int s, uint32_t max_detour, uint32_t budget)
{
    int32_t link[4], occupant[4];
    uint32_t cost[4], d_t[4];
    for (int k = 0; k < 4; ++k) {
        link[k] = g.link[(size_t)s * 4 + k], cost[k] = g.cost[(size_t)s * 4 + k];
        const bool has = link[k] >= 0 && link[k] < g.n;   // as the kernel gathers them
        d_t[k] = has ? g.D[(size_t)link[k]] : VTMC_NAVFIELD_UNREACHED;
        occupant[k] = has ? g.occupant[(size_t)link[k]] : 0;
    }
    return navcrowd_choose(g.D[(size_t)s], link, cost, d_t, occupant, g.n, max_detour, budget);
}

static void check_graph(const Graph &g, int *claims, int *waits, int *sidesteps, int *poor)
{
    const uint32_t detours[] = {0u, 512u, 2048u, 0xfffffffeu, VTMC_NAVCROWD_ANY_DETOUR};
    const uint32_t budgets[] = {0u, 1023u, 1024u, 1536u, 2560u, (uint32_t)VTMC_NAVCROWD_BUDGET_CAP};
    for (int s = 0; s < g.n; ++s) {
        if (g.D[(size_t)s] == VTMC_NAVFIELD_UNREACHED) continue;   // step 2: never asked
        for (uint32_t detour : detours)
            for (uint32_t budget : budgets) {
                const NavCrowdChoice fast = fast_choose(g, s, detour, budget), slow = slow_choose(g, s, detour, budget);
                EXPECT(fast.t == slow.t && fast.c == slow.c && fast.k == slow.k);
                if (fast.t < 0) {
                    ++*waits;
                    EXPECT(fast.k == -1 && fast.c == 0u);
                    *poor += slow_choose(g, s, detour, (uint32_t)VTMC_NAVCROWD_BUDGET_CAP).t >= 0;
                    continue;
                }
                ++*claims;
                EXPECT(fast.t < g.n && fast.k >= 0 && fast.k < 4 && g.link[(size_t)s * 4 + fast.k] == fast.t && g.cost[(size_t)s * 4 + fast.k] == fast.c);
                EXPECT(g.occupant[(size_t)fast.t] < 0 && g.D[(size_t)fast.t] < g.D[(size_t)s] && budget >= fast.c);
                // what it passed over was occupied, or no candidate at all
                Graph empty = g;
                std::fill(empty.occupant.begin(), empty.occupant.end(), -1);
                const NavCrowdChoice first = slow_choose(empty, s, detour, (uint32_t)VTMC_NAVCROWD_BUDGET_CAP);
                EXPECT(first.t >= 0);
                *sidesteps += first.k != fast.k;
                if (first.k != fast.k) EXPECT(g.occupant[(size_t)first.t] >= 0);
            }
    }
}

int main()
{
    static_assert(sizeof(vtmc_navcrowd_agent) == 16 && sizeof(vtmc_navcrowd_params) == 16, "include/vtmc_navcrowd.h");
    static_assert(VTMC_NAVCROWD_MAX_AGENTS == 1 << 24 && VTMC_NAVCROWD_MAX_TICKS == 4096 && VTMC_NAVCROWD_MAX_SPEED == 1 << 20 && VTMC_NAVCROWD_BUDGET_CAP == 1 << 21,
                  "include/vtmc_navcrowd.h");
    static_assert(VTMC_NAVCROWD_BUDGET_CAP > VTMC_NAVFIELD_UNIT + (1 << 20) && VTMC_NAVCROWD_ANY_DETOUR == 0xffffffffu, "the cap is above every edge cost");
    static_assert(kNavCrowdNoClaim >= VTMC_NAVCROWD_MAX_AGENTS, "no agent index reaches the empty claim word");

    // the step's checks: every fault of include/vtmc_navcrowd.h
    const vtmc_navcrowd_params fine[] = {params(0u), params(VTMC_NAVCROWD_ANY_DETOUR, VTMC_NAVCROWD_LEAVE_ON_ARRIVAL), params(2048u), params(0xfffffffeu, 1u)};
    for (const vtmc_navcrowd_params &p : fine) EXPECT(navcrowd_step_fault(&p, 0) == nullptr && navcrowd_step_fault(&p, 1) == nullptr && navcrowd_step_fault(&p, 4096) == nullptr);
    EXPECT(navcrowd_step_fault(nullptr, 1) != nullptr);
    EXPECT(navcrowd_step_fault(&fine[0], -1) != nullptr && navcrowd_step_fault(&fine[0], 4097) != nullptr && navcrowd_step_fault(&fine[0], 2147483647) != nullptr &&
           navcrowd_step_fault(&fine[0], -2147483647 - 1) != nullptr);
    const vtmc_navcrowd_params faults[] = {params(0u, 2u), params(0u, 3u), params(0u, 0x80000000u), params(0u, 0xffffffffu), params(0u, 0u, 1u), params(0u, 1u, 0u, 1u),
                                           params(0u, 0u, 0u, 0xffffffffu)};
    for (const vtmc_navcrowd_params &p : faults) EXPECT(navcrowd_step_fault(&p, 1) != nullptr);

    // the spawn's checks
    {
        const int32_t spans[4] = {0, -1, 4, 4};
        const uint32_t speeds[4] = {1u, 2u, 1u << 20, 7u};
        int32_t at = 7;
        EXPECT(navcrowd_spawn_fault(spans, speeds, 4, 5, &at) == nullptr && at == -1);
        EXPECT(navcrowd_spawn_fault(spans, speeds, 4, 5, nullptr) == nullptr);
        EXPECT(navcrowd_spawn_fault(spans, speeds, 0, 5, &at) != nullptr && navcrowd_spawn_fault(spans, speeds, -1, 5, &at) != nullptr);
        EXPECT(navcrowd_spawn_fault(spans, speeds, (1 << 24) + 1, 5, &at) != nullptr && at == -1);      // refused before any element is read
        EXPECT(navcrowd_spawn_fault(nullptr, speeds, 4, 5, &at) != nullptr && navcrowd_spawn_fault(spans, nullptr, 4, 5, &at) != nullptr);
        EXPECT(navcrowd_spawn_fault(spans, speeds, 4, 4, &at) != nullptr && at == 2);                   // spans[2] == n
        EXPECT(navcrowd_spawn_fault(spans, speeds, 2, 0, &at) != nullptr && at == 0);                   // no span at all: only -1 passes
        const int32_t low[4] = {0, -2, 4, 4}, none[2] = {-1, -1};
        EXPECT(navcrowd_spawn_fault(low, speeds, 4, 5, &at) != nullptr && at == 1);
        EXPECT(navcrowd_spawn_fault(none, speeds, 2, 0, &at) == nullptr);
        const uint32_t still[4] = {1u, 2u, 0u, 7u}, fast[4] = {1u, 2u, 3u, (1u << 20) + 1u};
        EXPECT(navcrowd_spawn_fault(spans, still, 4, 5, &at) != nullptr && at == 2);
        EXPECT(navcrowd_spawn_fault(spans, fast, 4, 5, &at) != nullptr && at == 3);
        EXPECT(navcrowd_spawn_fault(spans, fast, 3, 5, &at) == nullptr);
    }

    // the budget: the pay, and the cap in 64 bits
    EXPECT(navcrowd_budget(0u, 512u) == 512u && navcrowd_budget(512u, 512u) == 1024u && navcrowd_budget((1u << 21) - 1u, 1u) == 1u << 21);
    EXPECT(navcrowd_budget(1u << 21, 1u << 20) == 1u << 21 && navcrowd_budget(0xffffffffu, 0xffffffffu) == 1u << 21);

    // known answers: a span of cost 5000 with four links of cost 1024 to spans of cost 3976 (next), 3976, 4500 and 6000
    {
        Graph g;
        g.n = 5;
        g.D = {5000u, 3976u, 3976u, 4500u, 6000u};
        g.occupant = {9, -1, -1, -1, -1};
        g.link = {1, 2, 3, 4};
        g.cost = {1024u, 1024u, 1024u, 1024u};
        g.link.resize(20, -1), g.cost.resize(20, 0u);
        NavCrowdChoice c = fast_choose(g, 0, 0u, 1024u);
        EXPECT(c.t == 1 && c.c == 1024u && c.k == 0);                                      // the tie goes to the smaller k
        g.occupant[1] = 3;
        c = fast_choose(g, 0, 0u, 1024u);
        EXPECT(c.t == 2 && c.k == 1);                                                      // as cheap: within a detour of 0
        g.occupant[2] = 4;
        EXPECT(fast_choose(g, 0, 0u, 1024u).t == -1 && fast_choose(g, 0, 523u, 1024u).t == -1);   // 4500 + 1024 = 5000 + 524
        c = fast_choose(g, 0, 524u, 1024u);
        EXPECT(c.t == 3 && c.k == 2);
        EXPECT(fast_choose(g, 0, VTMC_NAVCROWD_ANY_DETOUR, 1023u).t == -1);                 // too poor: it waits
        g.occupant[3] = 5;
        EXPECT(fast_choose(g, 0, VTMC_NAVCROWD_ANY_DETOUR, 1u << 21).t == -1);             // 6000 is no lower: never a candidate
        g.occupant[1] = -1, g.cost[0] = 2000u;                                             // next is no longer the first link: D would be 5976
        g.D[0] = 5000u;
        c = fast_choose(g, 0, VTMC_NAVCROWD_ANY_DETOUR, 1999u);
        EXPECT(c.t == -1);                                                                 // spans 2 and 3 are occupied; 1 is empty and too dear: no later one is tried
        g.occupant[2] = -1;
        c = fast_choose(g, 0, VTMC_NAVCROWD_ANY_DETOUR, 1999u);
        EXPECT(c.t == 2 && c.c == 1024u);                                                  // 3976 + 1024 orders before 3976 + 2000
    }

    // random graphs: sparse and dense occupancy, far and near costs
    {
        int claims = 0, waits = 0, sidesteps = 0, poor = 0, spans = 0;
        for (uint32_t seed = 1; seed <= 12; ++seed) {
            const Graph g = make_graph(40 + 7 * (int)seed, seed, seed % 3u ? 40u : 100u, 24u, seed % 2u ? 60u : 150u, seed > 6u);
            spans += g.n;
            check_graph(g, &claims, &waits, &sidesteps, &poor);
        }
        EXPECT(spans > 900 && claims > 1000 && waits > 1000 && sidesteps > 100 && poor > 100);   // the graphs are not vacuous
        std::printf("%d spans: %d claims, %d waits (%d for want of budget), %d sidesteps\n", spans, claims, waits, poor, sidesteps);
    }

    // the sizes, in 64 bits
    EXPECT(navcrowd_agent_bytes(3) == 48 && navcrowd_agent_bytes(1 << 24) == 268435456ull && navcrowd_pending_bytes(1 << 24) == 134217728ull);
    EXPECT(navcrowd_word_bytes(0) == 0 && navcrowd_word_bytes(2147483647) == 8589934588ull && navcrowd_link_bytes(2147483647) == 34359738352ull);

    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("navcrowd_host_check: ok\n");
    return failures ? 1 : 0;
}
