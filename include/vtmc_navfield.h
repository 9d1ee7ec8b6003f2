/*
 * vtmc_navfield.h -- flow fields on the navigation layer of libvtmc.so (not in the reference): where on the spans a world position stands,
 * every span's cheapest cost to the nearest of a set of goals with the span to step to next, and the paths that follows give.  Same
 * library, same context, same conventions as vtmc_nav.h, which this header includes; a host that does its own path search never needs it.
 *
 * The question the navigation layer exists for: HOW DO I GET THERE?  The answer here is not a search per agent but one COST FIELD per goal
 * set, shared by any number of agents.  It works on the nav result the context holds (vtmc_terrain_nav_build) and never touches the grid.
 *
 * NAVFIELD: the rule.  n spans with heights h and link[4] as vtmc_terrain_nav_build left them.  All float arithmetic is FP32, one IEEE
 * operation per step in the order written, nothing fused; everything else is integers.  There is no tolerance in it.
 *   Edge cost  of the directed link s -> t = link[k] of s (t >= 0), with UNIT = VTMC_NAVFIELD_UNIT = 1024:
 *                d = h_t - h_s
 *                w = d > 0 ? d * climb_cost : (-d) * drop_cost
 *                q = w * 1024.0f
 *                extra = q >= 1048576.0f ? 1048576u : (uint32_t)q          (truncation)
 *                c(s, k) = 1024 + extra
 *              A span with a NaN height never links, so q is never NaN; climb_cost and drop_cost are finite and in [0, 1024]; every cost
 *              is at least 1024 and at most 1024 + 2^20.
 *   Goals      n_goals records {span, cost}.  Duplicates are allowed: the smaller cost wins.
 *   Cost       D(s) is the minimum, over every goal g and every directed walk s = s0 -> s1 -> ... -> sm = g.span along links (m = 0: the
 *              span is a goal), of g.cost + the sum of the walk's c.  Above max_cost, or without such a walk, D(s) =
 *              VTMC_NAVFIELD_UNREACHED.  max_cost is in 1..0x7fffffff, so D(t) + c never wraps in 32 bits.  Every c > 0, so D is unique,
 *              and every suffix of a cheapest walk is itself within max_cost: discarding candidates above max_cost during a relaxation
 *              gives the same field as discarding afterwards.  Links are directed; the walk follows link forwards, as an agent would.
 *   Next       -1 for an unreached span; -1 for a reached span that is a goal with g.cost == D(s) (arrived: a goal wins a tie against a
 *              link); otherwise link[k] for the SMALLEST k in 0..3 with link[k] >= 0, D(link[k]) reached and D(link[k]) + c(s, k) == D(s).
 *              Following next strictly lowers D, so it ends at a goal.
 *   Cell       {cost, next}, 8 bytes per span, indexed as the spans are.
 *   Locate     world position p to span.  Per axis g = (p - origin) / voxel_scale: one subtract, one divide, the terrain's own origin and
 *              scale.  ix = (int)floorf(gx + 0.5f) - box_lo.x, iz likewise.  If any coordinate of p is not finite, or ix / iz lies outside
 *              the nav box, the answer is -1.  Among the column's spans, e = gy - h; a span QUALIFIES iff -below <= e && e <= above (a NaN
 *              h fails).  The answer is the qualifying span with the smallest fabsf(e); on a tie the lower one wins; with none it is -1.
 *              below and above are in grid units, finite and >= 0.
 *   Trace      for start i: paths[i * max_len + 0] = start, then next, next ... until a span whose next is -1 or until max_len entries;
 *              lengths[i] is the number of entries written and the rest of the row is -1.  A start of -1 (a locate miss) or an unreached
 *              start gives length 0 and a row of -1.
 * OUT OF SCOPE, deliberately: no agent radius here (erode the spans first: vtmc_naverode.h); no any-angle smoothing (a path moves
 * from column to neighbour column; a layer of its own on top of this one pulls the traced paths straight on the device: vtmc_navsight.h,
 * line of sight and smoothed traces; PATHSMOOTHING.md); no agents that get in each other's way (a trace routes every start as if it were
 * alone; vtmc_navcrowd.h steps a crowd along the field on the device, one agent per span; CROWD.md); no field across the results of two boxes.
 *
 * Life cycle.  The field belongs to the nav result it was built on: vtmc_terrain_nav_build drops it (also a build that fails after it
 * invalidated the nav result), and so do vtmc_terrain_init, vtmc_terrain_load and vtmc_destroy.  An edit does not: the field is a snapshot,
 * as the spans are.  The buffers are library-owned and grow-only.  No call of this layer changes anything else the context holds: not the
 * grid, the history, the event counter, the dirty list, the extract result, the materials, the occlusion, the scatter or the nav result.
 *
 * vtmc_nav_locate              spans_out[i] for the n positions (x, y, z triples, world).  n == 0 is a success that touches nothing.
 * vtmc_navfield_build          builds the field of the goals; *n_reached (may be NULL) is the number of reached spans.
 * vtmc_navfield_read           copies the cells; VTMC_ERR_CAPACITY when capacity is below the span count.
 * vtmc_navfield_info           the span count, the reached count and the relaxation rounds of the field held; each may be NULL.
 * vtmc_navfield_device_results the device pointer of the cells; each may be NULL.
 * vtmc_navfield_trace          paths (n_starts * max_len int32) and lengths (n_starts int32) by the rule.  n_starts == 0 is a success
 *                              that touches nothing.
 *   VTMC_ERR_NO_RESULT     locate and build when the context holds no nav result; read, info, device results and trace when it holds no
 *                          field.
 *   VTMC_ERR_INVALID_ARG   (the previous field is kept) for a null pointer, n_goals outside 1..VTMC_NAVFIELD_MAX_GOALS, a goal span outside
 *                          0..n-1, a goal cost above max_cost, a climb or drop cost that is not finite or outside [0, 1024], max_cost
 *                          outside 1..0x7fffffff, flags != 0, below or above not finite or < 0, n < 0, n_starts < 0, max_len < 1, a start
 *                          outside -1..n-1 (the whole call).
 *   VTMC_ERR_DEVICE        ("relaxation did not converge") should the relaxation ever take more than n + 1 rounds; no field is left.
 */
#ifndef VTMC_NAVFIELD_H
#define VTMC_NAVFIELD_H

#include "vtmc_nav.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_NAVFIELD_UNIT 1024
#define VTMC_NAVFIELD_UNREACHED 0xffffffffu
#define VTMC_NAVFIELD_MAX_GOALS (1 << 20)

typedef struct vtmc_navfield_params {
    float    climb_cost;   /* per grid unit climbed, in units of a level step: finite, 0..1024 */
    float    drop_cost;    /* per grid unit dropped: finite, 0..1024 */
    uint32_t max_cost;     /* 1..0x7fffffff */
    uint32_t flags;        /* reserved, 0 */
} vtmc_navfield_params;    /* 16 bytes */

typedef struct vtmc_navfield_goal {
    int32_t  span;         /* 0..n-1 */
    uint32_t cost;         /* the cost of standing on it, <= max_cost */
} vtmc_navfield_goal;      /* 8 bytes */

typedef struct vtmc_navfield_cell {
    uint32_t cost;         /* D, or VTMC_NAVFIELD_UNREACHED */
    int32_t  next;         /* the span to step to, or -1 */
} vtmc_navfield_cell;      /* 8 bytes */

int32_t vtmc_nav_locate(vtmc_ctx *ctx, const float *positions /* n*3, world */, int32_t n, float below, float above, int32_t *spans_out);
int32_t vtmc_navfield_build(vtmc_ctx *ctx, const vtmc_navfield_goal *goals, int32_t n_goals, const vtmc_navfield_params *params, int32_t *n_reached);
int32_t vtmc_navfield_read(vtmc_ctx *ctx, vtmc_navfield_cell *dst, int32_t capacity);
int32_t vtmc_navfield_info(const vtmc_ctx *ctx, int32_t *n_spans, int32_t *n_reached, int32_t *rounds);
int32_t vtmc_navfield_device_results(vtmc_ctx *ctx, const vtmc_navfield_cell **d_cells, int32_t *n_spans);
int32_t vtmc_navfield_trace(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, int32_t *paths, int32_t *lengths);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_NAVFIELD_H */
