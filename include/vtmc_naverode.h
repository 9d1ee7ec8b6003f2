/*
 * vtmc_naverode.h -- an agent radius on the navigation layer of libvtmc.so (not in the reference): every span's distance to the nearest
 * border of the walkable area, and the erosion of the nav result to the spans an agent of a given radius can occupy.  Same library, same
 * context, same conventions as vtmc_nav.h, which this header includes; a host whose agents are points never needs it.
 *
 * The navigation layer answers where a POINT can stand; the paths of vtmc_navfield.h are the paths of a point: they hug walls, cross a
 * bridge one column wide and follow the rim of a ledge.  This is the step between the spans and everything downstream that Recast takes
 * with rcErodeWalkableArea: a chamfer distance to the border over the span graph, and the removal of every span nearer than the radius.
 * It works on the nav result the context holds (vtmc_terrain_nav_build) and never touches the grid.
 *
 * NAVERODE: the rule.  n spans with link[4] as the nav result holds them; k numbers the links as in NAVIGATION (0: -x, 1: +x, 2: -z,
 * 3: +z).  Integers only; there is no tolerance in it.
 *   Border     span s is a border span iff some link[k] is -1.  With VTMC_NAVERODE_OPEN_BOX_FACES a missing link is not counted when the
 *              neighbour column of direction k lies outside the nav box, so a box cut out of a larger walkable area does not erode from
 *              its own faces.  A span with a NaN height never links, so it is always a border (with the flag: whenever one of its
 *              neighbour columns lies inside the box).
 *   Steps      from s there is a step of weight 2 to link[k](s) for each k whose link exists, and a step of weight 3 to
 *              link[k'](link[k](s)) for each k and each k' on the OTHER axis when both links exist: up to eight two-hop steps, x first
 *              and z first, so the rule does not change when x and z are exchanged.  Links are followed forwards only, as an agent walks.
 *   Distance   D(s) = min(2 * radius, the cheapest total weight of a chain of steps from s to a border span); D = 0 on a border span.
 *              The unit is half a column (VTMC_NAVERODE_UNIT = 2): Recast's 2-3 chamfer.  Every step weighs at least 2, so a span with
 *              D < 2 * radius has a cheapest chain of at most radius - 1 steps: radius - 1 Jacobi rounds from
 *              D0 = border ? 0 : 2 * radius reach the fixed point.
 *   Erosion    span s is kept iff D(s) >= 2 * radius (radius 0 keeps everything).  Kept spans keep their order (by column, bottom-up) and
 *              are renumbered densely; column_offsets is the prefix of the kept counts per column; height, y and clearance are copied
 *              bit for bit; link[k] becomes the new index of the old target when that target is kept and -1 otherwise (a link is never
 *              re-chosen among the column's other spans); region is NAVIGATION's Region on the new links; origin[new] = old index.  The
 *              box is unchanged.
 * OUT OF SCOPE, deliberately: Euclidean or any-angle distances (the metric is the chamfer's: octagons, not circles); radii in fractions
 * of a column; stitching of two boxes, except that the open-faces flag keeps a box from eroding at its own faces; a cost term in
 * vtmc_navfield_params (the distance array is what a host feeds one from); an update after an edit -- everything here is a snapshot, as
 * the spans are.
 *
 * Life cycle.  The distance and the origin are library-owned and grow-only.  vtmc_nav_erode REPLACES the nav result the context holds:
 * the device pointers of vtmc_nav_device_results change with it; it drops the flow field (vtmc_navfield.h) and the distance, which both
 * describe the old spans, and leaves the origin valid until the next vtmc_nav_erode or vtmc_terrain_nav_build.  vtmc_nav_locate,
 * vtmc_navfield_build and vtmc_navfield_trace then work on the eroded result unchanged.  vtmc_terrain_nav_build (also one that fails after
 * it invalidated the nav result), vtmc_terrain_init, vtmc_terrain_load and vtmc_destroy drop the distance and the origin with the nav
 * result.  Neither call changes anything else the context holds: not the grid, the history, the event counter, the dirty list, the extract
 * result, the materials, the occlusion or the scatter.  Both wait for work queued on the context's stream, as the nav build does.
 *
 * vtmc_nav_distance_build           D of every span of the nav result held; *n_border (may be NULL) is the number of border spans.  The
 *                                   nav result and the flow field stay.
 * vtmc_nav_distance_read            copies the n int32 distances; VTMC_ERR_CAPACITY when capacity is below the span count.
 * vtmc_nav_distance_device_results  the device pointer of the same; each may be NULL.
 * vtmc_nav_erode                    erodes the nav result held by the rule; *n_spans (may be NULL) is the number of spans kept.
 * vtmc_nav_erode_origin             copies origin (one int32 per kept span); VTMC_ERR_CAPACITY when capacity is below their number.
 * A nav result of 0 spans is a success with 0.
 *   VTMC_ERR_NO_RESULT     every call when the context holds no nav result; the distance read and device results before a distance
 *                          build; the origin read before an erode.
 *   VTMC_ERR_INVALID_ARG   (the nav result, the distance and the origin are kept) for a null ctx or params, a radius outside
 *                          0..VTMC_NAVERODE_MAX_RADIUS, a flag other than VTMC_NAVERODE_OPEN_BOX_FACES, a reserved word that is not 0.
 *   VTMC_ERR_DEVICE        ("labelling did not converge") should the region pass ever break its own bounds: the nav result held before
 *                          the call stands; the flow field, the distance and the origin are gone.
 */
#ifndef VTMC_NAVERODE_H
#define VTMC_NAVERODE_H

#include "vtmc_nav.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_NAVERODE_UNIT 2
#define VTMC_NAVERODE_MAX_RADIUS 255
#define VTMC_NAVERODE_OPEN_BOX_FACES 1u

typedef struct vtmc_naverode_params {
    int32_t  radius;       /* columns, 0..VTMC_NAVERODE_MAX_RADIUS */
    uint32_t flags;        /* VTMC_NAVERODE_OPEN_BOX_FACES or 0 */
    int32_t  reserved[2];  /* 0 */
} vtmc_naverode_params;    /* 16 bytes */

int32_t vtmc_nav_distance_build(vtmc_ctx *ctx, const vtmc_naverode_params *params, int32_t *n_border);
int32_t vtmc_nav_distance_read(vtmc_ctx *ctx, int32_t *dst, int32_t capacity);
int32_t vtmc_nav_distance_device_results(vtmc_ctx *ctx, const int32_t **d_dist, int32_t *n_spans);
int32_t vtmc_nav_erode(vtmc_ctx *ctx, const vtmc_naverode_params *params, int32_t *n_spans);
int32_t vtmc_nav_erode_origin(vtmc_ctx *ctx, int32_t *dst, int32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_NAVERODE_H */
