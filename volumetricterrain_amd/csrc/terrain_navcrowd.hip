// terrain_navcrowd.hip -- a crowd stepped along the flow field (include/vtmc_navcrowd.h): agents on spans, one per span, that walk to the
// field's goals tick by tick and get in each other's way.  Not in the reference.  The rule is NAVCROWD in include/vtmc_navcrowd.h: integers
// only, so the kernels are compared for equality.  The host half -- the argument checks, the choice of one agent, the sizes -- is
// terrain_navcrowd.h; the claim kernel calls the same choice.  Works on the nav result and the field the context holds and never reads the
// grid.  Hand-written for gfx950 / CDNA4.
//
//   navcrowd_reset_kernel    a lane per span, at the spawn: the four links, packed into 16 bytes (the crowd is dropped with the nav result, so
//                            the copy cannot go stale), the occupancy word to -1 and the claim word to "nobody".
//   navcrowd_ask_kernel      a lane per agent, at the spawn: atomicMin of the agent index into the claim word of the span it asks for.
//   navcrowd_place_kernel    a lane per agent: the smallest index stands, writes the span's occupancy and resets the claim word; the record.
//   A TICK is two launches, a lane per agent in both:
//   navcrowd_claim_kernel    one 16-byte load of the record, the 8-byte cell of its span; for a walking agent the 16 bytes of links, the 16
//                            bytes of edge costs the field build left, the cells and the occupancy words of up to four targets; the choice
//                            (terrain_navcrowd.h); atomicMin of the agent index into the claim word of the chosen span.  It reads the
//                            occupancy and writes none of it, so every decision sees the start of the tick.  The new state and budget go
//                            back into the record (only the agent's own lane reads it), the {target, cost} pair into 8 bytes beside it.
//   navcrowd_resolve_kernel  the claimant whose index stands in the claim word moves: its record, the two occupancy words, and the claim
//                            word back to "nobody".  A loser reads the winner's index or, after the reset, "nobody": neither is its own.
//                            An agent that arrived under LEAVE_ON_ARRIVAL frees its span here.  Every span's words are written by exactly
//                            one lane -- the vacated span was occupied at the start of the tick, so nobody claimed it; the target span has
//                            one winner -- and no atomic decides a position but the claim's minimum.  The last tick of a call counts the
//                            moves, the occupying and the arrived agents, reduced per wave by ballot before one atomic each.
// All ticks of a call are queued back to back; the counters come back once, behind the last one.  Every random-access index is checked
// against n before it is used, whatever a record says.
//
// The agent record is an array of 16-byte structures: a lane's whole record is one load, and what the library hands out is what the kernels
// step.  Decided by tools/navcrowd_bench.py, this build against one that keeps four arrays of words (and refreshes the records behind a call),
// alternating, at 1024^3 cells, 1.36 M spans and 100 000 agents (profiles/r25/navcrowd): 11.6 and 11.9 us per tick against 11.9 and 11.9 us
// over 256 ticks, the same bytes.  Neither layout shows: at this size a tick is its two launches.
#include "surface_query.h"
#include "terrain_navfield.h"
#include "terrain_navcrowd.h"
#include <cstring>

namespace vtmc {

static_assert(sizeof(vtmc_navcrowd_agent) == 16 && sizeof(vtmc_navcrowd_params) == 16, "include/vtmc_navcrowd.h");
static_assert(VTMC_NAVCROWD_BUDGET_CAP > VTMC_NAVFIELD_UNIT + (1 << 20), "the cap is above every edge cost");
enum { kNavCrowdCtlMoved = 0, kNavCrowdCtlOccupying = 1, kNavCrowdCtlArrived = 2, kNavCrowdCtlPlaced = 3, kNavCrowdCtlWords = 4 };

__device__ __forceinline__ int32_t claim_load(const int32_t *word) { return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void claim_reset(int32_t *word) { __hip_atomic_store(word, kNavCrowdNoClaim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void count_wave(bool mine, int *counter)
{
    const unsigned long long m = __ballot(mine);
    if (m && __lane_id() == 0) atomicAdd(counter, __popcll(m));
}

__global__ __launch_bounds__(256) void navcrowd_reset_kernel(const vtmc_nav_span *__restrict__ spans, int4 *__restrict__ links, int32_t *__restrict__ occupancy,
                                                            int32_t *__restrict__ claims, int32_t n)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    links[s] = make_int4(spans[s].link[0], spans[s].link[1], spans[s].link[2], spans[s].link[3]);
    occupancy[s] = -1;
    claims[s] = kNavCrowdNoClaim;
}

__global__ __launch_bounds__(256) void navcrowd_ask_kernel(const int32_t *__restrict__ want, int32_t n_agents, int32_t *__restrict__ claims, int32_t n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_agents) return;
    const int32_t s = want[i];
    if (s >= 0 && s < n) atomicMin(&claims[s], i);
}

__global__ __launch_bounds__(256) void navcrowd_place_kernel(const int32_t *__restrict__ want, const uint32_t *__restrict__ speeds, int32_t n_agents,
                                                            vtmc_navcrowd_agent *__restrict__ agents, int32_t *__restrict__ occupancy, int32_t *claims, int32_t n,
                                                            int *__restrict__ counters)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool placed = false;
    if (i < n_agents) {
        const int32_t s = want[i];
        if (s >= 0 && s < n && claim_load(&claims[s]) == i) {
            placed = true;
            occupancy[s] = i;
            claim_reset(&claims[s]);
        }
        vtmc_navcrowd_agent a;
        a.span = placed ? s : -1, a.budget = 0u, a.speed = speeds[i], a.state = placed ? VTMC_NAVCROWD_WALKING : VTMC_NAVCROWD_UNPLACED;
        agents[i] = a;
    }
    count_wave(placed, counters + kNavCrowdCtlPlaced);
}

__device__ __forceinline__ int32_t link_of(const int4 &l, int k) { return k == 0 ? l.x : k == 1 ? l.y : k == 2 ? l.z : l.w; }
__device__ __forceinline__ uint32_t edge_of(const uint4 &c, int k) { return k == 0 ? c.x : k == 1 ? c.y : k == 2 ? c.z : c.w; }

// A tick, first half: the state, the pay, the choice and the claim of every agent
__global__ __launch_bounds__(256) void navcrowd_claim_kernel(uint4 *__restrict__ agents, int2 *__restrict__ pending, const int4 *__restrict__ links,
                                                            const uint4 *__restrict__ costs, const uint2 *__restrict__ cells, const int32_t *__restrict__ occupancy,
                                                            int32_t *__restrict__ claims, int32_t n, int32_t n_agents, uint32_t max_detour)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_agents) return;
    uint4 a = agents[i];   // {span, budget, speed, state}
    const int32_t s = (int32_t)a.x;
    if (a.w > (uint32_t)VTMC_NAVCROWD_STRANDED || s < 0 || s >= n) return;   // GONE, UNPLACED: nothing
    const uint2 cell = cells[s];                                             // {D, next}
    uint32_t state = VTMC_NAVCROWD_WALKING, budget = a.y;
    int2 pend = make_int2(-1, 0);
    if (cell.x == VTMC_NAVFIELD_UNREACHED) {
        state = VTMC_NAVCROWD_STRANDED;
    } else if ((int32_t)cell.y < 0) {
        state = VTMC_NAVCROWD_ARRIVED;
    } else {
        budget = navcrowd_budget(budget, a.z);
        const int4 l = links[s];
        const uint4 c = costs[s];
        int32_t link[4], occupant[4];
        uint32_t cost[4], d_t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            link[k] = link_of(l, k), cost[k] = edge_of(c, k);
            const bool has = link[k] >= 0 && link[k] < n;
            d_t[k] = has ? cells[link[k]].x : VTMC_NAVFIELD_UNREACHED;
            occupant[k] = has ? occupancy[link[k]] : 0;
        }
        const NavCrowdChoice choice = navcrowd_choose(cell.x, link, cost, d_t, occupant, n, max_detour, budget);
        if (choice.t >= 0) {
            atomicMin(&claims[choice.t], i);
            pend = make_int2(choice.t, (int)choice.c);
        }
    }
    if (state != a.w || budget != a.y) {
        a.y = budget, a.w = state;
        agents[i] = a;
    }
    pending[i] = pend;
}

// A tick, second half: the winners move; with `counters` (the last tick of a call) the moves, the occupying and the arrived agents
__global__ __launch_bounds__(256) void navcrowd_resolve_kernel(uint4 *__restrict__ agents, const int2 *__restrict__ pending, int32_t *__restrict__ occupancy,
                                                              int32_t *claims, int32_t n, int32_t n_agents, uint32_t flags, int *__restrict__ counters)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool moved = false, occupying = false, arrived = false;
    if (i < n_agents) {
        uint4 a = agents[i];
        const int32_t s = (int32_t)a.x;
        if (s >= 0 && s < n) {
            if (a.w == (uint32_t)VTMC_NAVCROWD_WALKING) {
                const int2 pend = pending[i];
                const int32_t t = pend.x;
                if (t >= 0 && t < n && claim_load(&claims[t]) == i) {
                    occupancy[s] = -1;
                    occupancy[t] = i;
                    claim_reset(&claims[t]);
                    a.x = (uint32_t)t, a.y -= (uint32_t)pend.y;
                    agents[i] = a;
                    moved = true;
                }
            } else if (a.w == (uint32_t)VTMC_NAVCROWD_ARRIVED && (flags & VTMC_NAVCROWD_LEAVE_ON_ARRIVAL)) {
                occupancy[s] = -1;
                a.w = VTMC_NAVCROWD_GONE;
                agents[i] = a;
            }
        }
        occupying = a.w <= (uint32_t)VTMC_NAVCROWD_STRANDED;
        arrived = a.w == (uint32_t)VTMC_NAVCROWD_ARRIVED || a.w == (uint32_t)VTMC_NAVCROWD_GONE;
    }
    if (counters) {   // uniform over the launch
        count_wave(moved, counters + kNavCrowdCtlMoved);
        count_wave(occupying, counters + kNavCrowdCtlOccupying);
        count_wave(arrived, counters + kNavCrowdCtlArrived);
    }
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_navcrowd_spawn(vtmc_ctx *ctx, const int32_t *spans, const uint32_t *speeds, int32_t n_agents, int32_t *n_placed)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navcrowd_spawn before terrain_nav_build");
    int32_t at = -1;
    if (const char *what = navcrowd_spawn_fault(spans, speeds, n_agents, nav.n, &at))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "navcrowd_spawn: %s (agent %d, %d spans)", what, at, nav.n);
    const int32_t n = nav.n;
    VtmcNavCrowd &nc = ctx->navcrowd;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nc.valid = false;   // from here on the buffers no longer hold the previous crowd
    if (int rc = ensure(ctx, nc.agents, navcrowd_agent_bytes(n_agents))) return rc;
    if (int rc = ensure(ctx, nc.pending, navcrowd_pending_bytes(n_agents))) return rc;
    if (int rc = ensure(ctx, nc.occupancy, navcrowd_word_bytes(n))) return rc;
    if (int rc = ensure(ctx, nc.claims, navcrowd_word_bytes(n))) return rc;
    if (int rc = ensure(ctx, nc.links, navcrowd_link_bytes(n))) return rc;
    if (int rc = ensure(ctx, nc.ctl, kNavCrowdCtlWords * sizeof(int))) return rc;
    const float *const src[3] = {(const float *)spans, (const float *)speeds, nullptr};
    const size_t bytes[3] = {(size_t)n_agents * 4u, (size_t)n_agents * 4u, 0};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, 0, &st)) return rc;
    int *ctl = (int *)nc.ctl.p;
    int32_t *occupancy = (int32_t *)nc.occupancy.p, *claims = (int32_t *)nc.claims.p;
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kNavCrowdCtlWords * sizeof(int), s));
    if (n > 0)
        VTMC_HIP(ctx, launch(navcrowd_reset_kernel, lanes256(n), dim3(256), 0, s, (const vtmc_nav_span *)nav.spans.p, (int4 *)nc.links.p, occupancy, claims, n));
    VTMC_HIP(ctx, launch(navcrowd_ask_kernel, lanes256(n_agents), dim3(256), 0, s, (const int32_t *)st.in[0], n_agents, claims, n));
    VTMC_HIP(ctx, launch(navcrowd_place_kernel, lanes256(n_agents), dim3(256), 0, s, (const int32_t *)st.in[0], (const uint32_t *)st.in[1], n_agents,
                         (vtmc_navcrowd_agent *)nc.agents.p, occupancy, claims, n, ctl));
    int placed = 0;
    VTMC_HIP(ctx, hipMemcpyAsync(&placed, ctl + kNavCrowdCtlPlaced, sizeof placed, hipMemcpyDeviceToHost, s));
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nc.n_agents = n_agents, nc.n_spans = n;
    nc.occupying = placed, nc.arrived = 0, nc.ticks = 0, nc.moved_last = 0;
    nc.valid = true;
    ctx->navcrowd_clock.armed = false;
    if (n_placed) *n_placed = placed;
    return VTMC_OK;
}

int32_t vtmc_navcrowd_step(vtmc_ctx *ctx, const vtmc_navcrowd_params *params, int32_t n_ticks)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    VtmcNavCrowd &nc = ctx->navcrowd;
    if (!nc.valid || !ctx->nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navcrowd_step before navcrowd_spawn");
    if (const char *what = navcrowd_step_fault(params, n_ticks)) return fail(ctx, VTMC_ERR_INVALID_ARG, "navcrowd_step: %s", what);
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid || nf.n != nc.n_spans) return fail(ctx, VTMC_ERR_NO_RESULT, "navcrowd_step before navfield_build");
    if (n_ticks == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    StageClock<2> &clock = ctx->navcrowd_clock;
    VTMC_HIP(ctx, clock.begin());
    const int32_t n = nc.n_spans, n_agents = nc.n_agents;
    uint4 *agents = (uint4 *)nc.agents.p;
    int2 *pending = (int2 *)nc.pending.p;
    int32_t *occupancy = (int32_t *)nc.occupancy.p, *claims = (int32_t *)nc.claims.p;
    const uint4 *costs = (const uint4 *)nf.work.p;   // the four edge costs of every span, as navfield_build left them
    int *ctl = (int *)nc.ctl.p;
    const dim3 grid = lanes256(n_agents);
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kNavCrowdCtlWords * sizeof(int), s));
    VTMC_HIP(ctx, clock.mark(0, s));
    for (int32_t tick = 0; tick < n_ticks; ++tick) {
        VTMC_HIP(ctx, launch(navcrowd_claim_kernel, grid, dim3(256), 0, s, agents, pending, (const int4 *)nc.links.p, costs, (const uint2 *)nf.cells.p,
                             (const int32_t *)occupancy, claims, n, n_agents, params->max_detour));
        VTMC_HIP(ctx, launch(navcrowd_resolve_kernel, grid, dim3(256), 0, s, agents, (const int2 *)pending, occupancy, claims, n, n_agents, params->flags,
                             tick == n_ticks - 1 ? ctl : (int *)nullptr));
    }
    VTMC_HIP(ctx, clock.mark(1, s));
    int h[kNavCrowdCtlWords] = {};
    VTMC_HIP(ctx, hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, s));
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nc.moved_last = h[kNavCrowdCtlMoved], nc.occupying = h[kNavCrowdCtlOccupying], nc.arrived = h[kNavCrowdCtlArrived];
    nc.ticks = nc.ticks > 0x7fffffff - n_ticks ? 0x7fffffff : nc.ticks + n_ticks;
    clock.arm();
    return VTMC_OK;
}

int32_t vtmc_navcrowd_read(vtmc_ctx *ctx, vtmc_navcrowd_agent *agents_dst, int32_t capacity, int32_t *occupancy_dst)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavCrowd &nc = ctx->navcrowd;
    if (!nc.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navcrowd_read before navcrowd_spawn");
    if (capacity < nc.n_agents) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d agents", capacity, nc.n_agents);
    if (!agents_dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "agents_dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipMemcpy(agents_dst, nc.agents.p, navcrowd_agent_bytes(nc.n_agents), hipMemcpyDeviceToHost));
    if (occupancy_dst && nc.n_spans > 0) VTMC_HIP(ctx, hipMemcpy(occupancy_dst, nc.occupancy.p, navcrowd_word_bytes(nc.n_spans), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_navcrowd_info(const vtmc_ctx *ctx, int32_t *n_agents, int32_t *n_occupying, int32_t *n_arrived, int32_t *ticks, int32_t *moved_last)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavCrowd &nc = ctx->navcrowd;
    if (!nc.valid) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_NO_RESULT, "navcrowd_info before navcrowd_spawn");
    if (n_agents) *n_agents = nc.n_agents;
    if (n_occupying) *n_occupying = nc.occupying;
    if (n_arrived) *n_arrived = nc.arrived;
    if (ticks) *ticks = nc.ticks;
    if (moved_last) *moved_last = nc.moved_last;
    return VTMC_OK;
}

int32_t vtmc_navcrowd_device_results(vtmc_ctx *ctx, const vtmc_navcrowd_agent **d_agents, const int32_t **d_occupancy, int32_t *n_agents)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavCrowd &nc = ctx->navcrowd;
    if (!nc.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navcrowd_device_results before navcrowd_spawn");
    if (d_agents) *d_agents = (const vtmc_navcrowd_agent *)nc.agents.p;
    if (d_occupancy) *d_occupancy = (const int32_t *)nc.occupancy.p;
    if (n_agents) *n_agents = nc.n_agents;
    return VTMC_OK;
}

// Not part of the ABI (tools/navcrowd_bench.py): device time of the ticks of the last vtmc_navcrowd_step that ran any, from the first
// claim kernel to the last resolve kernel.
int32_t vtmc_debug_navcrowd_ms(vtmc_ctx *ctx, float ms[1])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->navcrowd.valid || !ctx->navcrowd_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_navcrowd_ms before a navcrowd_step that ran a tick");
    if (int rc = ctx->navcrowd_clock.sync_last(ctx)) return rc;
    return ctx->navcrowd_clock.elapsed(ctx, 0, 1, &ms[0]);
}

}  // extern "C"
