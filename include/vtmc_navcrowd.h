/*
 * vtmc_navcrowd.h -- a crowd stepped along the flow field of libvtmc.so (not in the reference): agents that stand on spans, one per span,
 * and walk to the goals of the field tick by tick, on the device, getting in each other's way.  Same library, same context, same
 * conventions as vtmc_navfield.h, which this header includes; a host that moves its own agents never needs it.
 *
 * The field answers "where do I step next" for every span at once and is the same for everybody, wherever a path began: what a per-tick
 * stepper needs.  vtmc_navfield_trace follows it for one agent that ignores all others and copies every traced span to the host; here
 * the agents stay on the device, a tick is two kernel launches over them, and nothing but a status crosses to the host per call.  The
 * crowd works on the nav result and the flow field the context holds (vtmc_terrain_nav_build, vtmc_navfield_build) and never reads the
 * grid.
 *
 * NAVCROWD: the rule.  n spans; link[4] is NAVIGATION's link array; c(s, k), D and next are NAVFIELD's edge cost, cost and next.
 * Integers only; there is no tolerance in it.
 *   Agent      the record {span, budget, speed, state}, 16 bytes.  States: VTMC_NAVCROWD_WALKING 0, ARRIVED 1, STRANDED 2, GONE 3,
 *              UNPLACED 4.  WALKING, ARRIVED and STRANDED agents OCCUPY their span.  GONE and UNPLACED agents occupy nothing: UNPLACED has
 *              span == -1, GONE keeps the span it left from.
 *   Occupancy  one int32 per span: the index of the agent that occupies it, or -1.  No two agents ever occupy one span.
 *   Spawn      replaces the crowd.  Agent i asks for spans[i] in -1..n-1 with speeds[i] in 1..VTMC_NAVCROWD_MAX_SPEED (2^20) cost units
 *              per tick.  -1 gives UNPLACED.  Where several agents ask for one span the SMALLEST index is placed; the others become
 *              UNPLACED with span -1.  A placed agent starts WALKING.  Every agent starts with budget 0 and keeps its speed.
 *   Tick       synchronous: every decision reads the agents, the occupancy and the field as they stood at the start of the tick.  For
 *              agent i on span s, in this order:
 *                1. GONE and UNPLACED agents do nothing.
 *                2. D(s) unreached: the state becomes STRANDED; the budget is unchanged.
 *                3. next(s) == -1 (s reached): the state becomes ARRIVED -- with VTMC_NAVCROWD_LEAVE_ON_ARRIVAL it becomes GONE in this
 *                   tick, and its span is free from the next tick on.  The budget is unchanged.
 *                4. Otherwise the state is WALKING and budget = min(budget + speed, VTMC_NAVCROWD_BUDGET_CAP); the cap, 1 << 21, is
 *                   above every edge cost.
 *                5. CANDIDATES are the k in 0..3 with t = link[k] >= 0, D(t) reached, D(t) < D(s), and D(t) + c(s, k) <= D(s) +
 *                   max_detour, in 64 bits.  max_detour = VTMC_NAVCROWD_ANY_DETOUR removes that last test.
 *                6. They are ordered by (D(t) + c(s, k), k) ascending.  The first is always next(s).  Every move strictly lowers D, so
 *                   there is no livelock.
 *                7. The agent takes the FIRST candidate whose span was empty at the start of the tick.  If there is none, it waits.  If
 *                   budget < c(s, k) for that candidate it waits, and does not try a later one.  Otherwise it CLAIMS t.
 *                8. Every claimed span goes to the SMALLEST agent index among its claimants.  The winner moves: span = t, budget -= c,
 *                   and the occupancy of s and t is updated.  Losers stay.
 *              The state is recomputed every tick: after a new vtmc_navfield_build with other goals an ARRIVED or STRANDED agent walks
 *              again.
 *   Info       the agent count; the occupying agents; the arrived agents (ARRIVED plus GONE); the ticks since the spawn; the moves of the
 *              last tick (0: the crowd is settled, or jammed).
 * OUT OF SCOPE, deliberately: one agent per span -- a column is one voxel wide, and a wider agent keeps off walls through vtmc_nav_erode
 * (vtmc_naverode.h) only; a span vacated in a tick is free only from the next tick, so a queue moves at most every other tick; a waiting
 * agent saves budget up to the cap; an agent moves at most one span per tick; no steering inside a column; no adding agents to a live
 * crowd (spawn again); one box only.
 *
 * Life cycle.  The context holds one crowd.  It belongs to the nav result it was spawned on: vtmc_terrain_nav_build drops it (also a
 * build that fails after it invalidated the nav result), and so do vtmc_nav_erode, vtmc_terrain_init, vtmc_terrain_load and vtmc_destroy.
 * vtmc_navfield_build KEEPS it: that is the re-route.  An edit keeps it: the crowd walks a snapshot, as the spans are.  The buffers are
 * library-owned and grow-only.  No call of this layer changes anything else the context holds: not the grid, the history, the event
 * counter, the dirty list, the extract result, the materials, the occlusion, the scatter, the nav result, the flow field, the border
 * distance or the origin of an erosion.
 *
 * vtmc_navcrowd_spawn           the crowd of n_agents agents by Spawn; *n_placed (may be NULL) is the number of placed agents.  Needs a nav
 *                               result only.
 * vtmc_navcrowd_step            n_ticks ticks, all queued with no read-back and no flag between them; step(a) then step(b) equals
 *                               step(a + b).  n_ticks == 0 is a success that touches nothing.  Needs a field.
 * vtmc_navcrowd_read            copies the agents and, unless occupancy_dst is NULL, the occupancy (n spans); VTMC_ERR_CAPACITY when
 *                               capacity is below the agent count.
 * vtmc_navcrowd_info            by Info; each may be NULL.
 * vtmc_navcrowd_device_results  the device pointers of the agents and of the occupancy; each may be NULL.
 *   VTMC_ERR_NO_RESULT     spawn when the context holds no nav result; step when it holds no crowd or no field; read, info and device
 *                          results when it holds no crowd.
 *   VTMC_ERR_INVALID_ARG   (the previous crowd is kept) for a null pointer, n_agents outside 1..VTMC_NAVCROWD_MAX_AGENTS, a span outside
 *                          -1..n-1 or a speed outside 1..VTMC_NAVCROWD_MAX_SPEED (the whole call), n_ticks outside
 *                          0..VTMC_NAVCROWD_MAX_TICKS, flags other than VTMC_NAVCROWD_LEAVE_ON_ARRIVAL, reserved not 0.
 */
#ifndef VTMC_NAVCROWD_H
#define VTMC_NAVCROWD_H

#include "vtmc_navfield.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_NAVCROWD_MAX_AGENTS (1 << 24)
#define VTMC_NAVCROWD_MAX_TICKS 4096
#define VTMC_NAVCROWD_MAX_SPEED (1 << 20)
#define VTMC_NAVCROWD_BUDGET_CAP (1 << 21)
#define VTMC_NAVCROWD_ANY_DETOUR 0xffffffffu
#define VTMC_NAVCROWD_LEAVE_ON_ARRIVAL 1

#define VTMC_NAVCROWD_WALKING 0
#define VTMC_NAVCROWD_ARRIVED 1
#define VTMC_NAVCROWD_STRANDED 2
#define VTMC_NAVCROWD_GONE 3
#define VTMC_NAVCROWD_UNPLACED 4

typedef struct vtmc_navcrowd_agent {
    int32_t  span;         /* the span it stands on (GONE: the one it left from), or -1 (UNPLACED) */
    uint32_t budget;       /* cost units saved towards the next step, <= VTMC_NAVCROWD_BUDGET_CAP */
    uint32_t speed;        /* cost units per tick, 1..VTMC_NAVCROWD_MAX_SPEED */
    uint32_t state;        /* VTMC_NAVCROWD_WALKING .. VTMC_NAVCROWD_UNPLACED */
} vtmc_navcrowd_agent;     /* 16 bytes */

typedef struct vtmc_navcrowd_params {
    uint32_t max_detour;   /* what a step may cost above the cheapest one, or VTMC_NAVCROWD_ANY_DETOUR */
    uint32_t flags;        /* VTMC_NAVCROWD_LEAVE_ON_ARRIVAL or 0 */
    uint32_t reserved[2];  /* 0 */
} vtmc_navcrowd_params;    /* 16 bytes */

int32_t vtmc_navcrowd_spawn(vtmc_ctx *ctx, const int32_t *spans, const uint32_t *speeds, int32_t n_agents, int32_t *n_placed);
int32_t vtmc_navcrowd_step(vtmc_ctx *ctx, const vtmc_navcrowd_params *params, int32_t n_ticks);
int32_t vtmc_navcrowd_read(vtmc_ctx *ctx, vtmc_navcrowd_agent *agents_dst, int32_t capacity, int32_t *occupancy_dst /* n spans, may be NULL */);
int32_t vtmc_navcrowd_info(const vtmc_ctx *ctx, int32_t *n_agents, int32_t *n_occupying, int32_t *n_arrived, int32_t *ticks, int32_t *moved_last);
int32_t vtmc_navcrowd_device_results(vtmc_ctx *ctx, const vtmc_navcrowd_agent **d_agents, const int32_t **d_occupancy, int32_t *n_agents);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_NAVCROWD_H */
