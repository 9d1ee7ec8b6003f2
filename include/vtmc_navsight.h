/*
 * vtmc_navsight.h -- any-angle paths on the navigation layer of libvtmc.so (not in the reference): whether one span can be walked to from
 * another in a straight line over the spans, and the traced paths of a flow field pulled straight wherever that is so.  Same library, same
 * context, same conventions as vtmc_navfield.h, which this header includes; a host that is content with the column-to-column paths of
 * vtmc_navfield_trace never needs it.
 *
 * A traced path moves from column to neighbour column along the four axis directions: a staircase.  The host's remedy was string-pulling
 * over the traced spans, after copying n_starts * max_len integers.  Here both happen on the device: the LINE-OF-SIGHT WALK over the spans
 * is the navigation analogue of vtmc_terrain_raycast and the query a host's steering asks every frame ("can I walk straight to that
 * span?"); the SMOOTHED TRACE keeps of every path only the waypoints between which the walk succeeds.  It works on the nav result (and,
 * for the smoothed trace, the flow field) the context holds and never touches the grid.  After vtmc_nav_erode (vtmc_naverode.h) a straight
 * walk between column centres stays the agent's radius away from every border: the walk only ever stands on spans the erosion kept.
 *
 * NAVSIGHT: the rule.  n spans with link[4] and column_offsets as the nav result holds them; k numbers the links as in NAVIGATION (0: -x,
 * 1: +x, 2: -z, 3: +z); c(s, k), D and next are NAVFIELD's edge cost, cost and next.  Integers only; there is no tolerance in it.
 *   Column     the column of span s is the c with column_offsets[c] <= s < column_offsets[c + 1]; cx = c % dx, cz = c / dx.
 *   Walk       from span a towards span b.  nx = |cx_b - cx_a|, nz = |cz_b - cz_a|; kx = 1 if cx_b > cx_a, else 0; kz = 3 if cz_b > cz_a,
 *              else 2.  Start with s = a, i = j = 0, steps = 0, w = 0.  While i < nx || j < nz, compare ex = (2i + 1) * nz with
 *              ez = (2j + 1) * nx: the order in which the segment between the two column centres crosses column boundaries (a box has
 *              at most 1026 columns per axis, so both fit 32 bits).
 *                ex < ez    t = link[kx] of s.  t < 0 ends the walk at s.  Otherwise w += c(s, kx), s = t, i += 1, steps += 1.
 *                ex > ez    the same with kz and j.
 *                ex == ez   the segment passes through a corner of four columns.  p = link[kx] of s, q = link[kz] of s, t1 = link[kz]
 *                           of p, t2 = link[kx] of q.  If any of the four is < 0, or t1 != t2, the walk ends at s.  Otherwise
 *                           w += max(c(s, kx) + c(p, kz), c(s, kz) + c(q, kx)), s = t1, i += 1, j += 1, steps += 2.
 *              A link value outside 0..n-1 ends the walk like -1.  The walk takes at most nx + nz steps.  w is needed only where a cost
 *              bound is asked for.
 *   Visible    (a, b): the walk ends with s == b.  Reaching b's column on another floor is not visibility.  Links are followed forwards,
 *              as an agent walks, so visibility is NOT symmetric (a one-way drop).  A linked neighbour is always visible, in one step.
 *   Sight      per pair the hit {last, steps}: the span the walk ended on and the steps it took; the pair is visible iff last == to.
 *              from == -1 or to == -1 gives {-1, 0}.
 *   Smoothed trace  of start s0 over the field held.  An invalid (-1) or unreached start gives length 0 and a row of -1, as in NAVFIELD's
 *              Trace.  Otherwise row[0] = s0 and the anchor is a = s0.  While the row has fewer than max_len entries and next(a) >= 0:
 *              the chain is next(a), next(next(a)), ...; it holds at most max_look entries and stops at a span whose next is -1.  The
 *              pick is the LAST chain entry b that passes both tests: Visible(a, b); and, when max_extra_cost is not
 *              VTMC_NAVSIGHT_ANY_COST, w(a -> b) + D(b) <= D(a) + max_extra_cost, in 64 bits.  chain[0] always passes both: it is a
 *              cheapest step.  Append b to the row and set a = b.  lengths[i] is the number of entries; the rest of the row is -1.
 *              A row ends on the span the plain trace ends on unless it was cut at max_len; it was cut when next of its last entry is
 *              not -1.  "Last", not "up to the first failure": visibility is not monotone along a chain.
 *              With max_extra_cost = 0 every straight stretch is itself a cheapest walk; with VTMC_NAVSIGHT_ANY_COST the smoothing is
 *              purely geometric and may cut over a hill the field went round.
 * OUT OF SCOPE, deliberately: waypoints are column centres; the only clearance is the erosion's radius (vtmc_naverode.h); the smoothing is
 * greedy and bounded by max_look, not the globally shortest any-angle path; no walk across the results of two boxes; an update after an
 * edit -- everything here is a snapshot, as the spans are.
 *
 * Life cycle.  The layer keeps nothing between calls: it reads the nav result, the cells and the edge costs the field build left.  No
 * call changes anything else the context holds: not the grid, the history, the event counter, the dirty list, the extract result, the
 * materials, the occlusion, the scatter, the nav result, the flow field, the border distance or the origin of an erosion.  Both wait for
 * work queued on the context's stream.
 *
 * vtmc_nav_sight              hits[i] of the n pairs (from[i], to[i]); needs a nav result only.  n == 0 is a success that touches nothing.
 * vtmc_navfield_trace_smooth  paths (n_starts * max_len int32) and lengths (n_starts int32) by the rule; needs a field.  n_starts == 0
 *                             is a success that touches nothing.
 *   VTMC_ERR_NO_RESULT     vtmc_nav_sight when the context holds no nav result; vtmc_navfield_trace_smooth when it holds no field.
 *   VTMC_ERR_INVALID_ARG   (nothing is written to the caller's arrays) for a null pointer, n < 0, n_starts < 0, a span outside -1..n-1
 *                          (the whole call), max_len < 1, max_look outside 1..VTMC_NAVSIGHT_MAX_LOOK, flags or reserved not 0.
 */
#ifndef VTMC_NAVSIGHT_H
#define VTMC_NAVSIGHT_H

#include "vtmc_navfield.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_NAVSIGHT_MAX_LOOK 256
#define VTMC_NAVSIGHT_ANY_COST 0xffffffffu

typedef struct vtmc_navsight_params {
    int32_t  max_look;         /* chain entries tested per anchor, 1..VTMC_NAVSIGHT_MAX_LOOK */
    uint32_t max_extra_cost;   /* what a straight stretch may cost above the field's own path, or VTMC_NAVSIGHT_ANY_COST */
    uint32_t flags;            /* reserved, 0 */
    uint32_t reserved;         /* 0 */
} vtmc_navsight_params;        /* 16 bytes */

typedef struct vtmc_navsight_hit {
    int32_t last;              /* the span the walk ended on; == to: visible.  -1 for a pair with a -1 */
    int32_t steps;             /* links followed */
} vtmc_navsight_hit;           /* 8 bytes */

int32_t vtmc_nav_sight(vtmc_ctx *ctx, const int32_t *from, const int32_t *to, int32_t n, vtmc_navsight_hit *hits);
int32_t vtmc_navfield_trace_smooth(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, const vtmc_navsight_params *params,
                                   int32_t *paths, int32_t *lengths);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_NAVSIGHT_H */
