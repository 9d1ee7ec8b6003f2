/*
 * vtmc_nav.h -- the navigation layer of libvtmc.so (not in the reference): walkable spans, links and regions of a box of the resident
 * terrain, built on the device.  Same library, same context, same conventions as vtmc.h, which this header includes; a host that does
 * not walk anything on the terrain never needs it.
 *
 * The other non-local question about the terrain (the first is FRAGMENTS in vtmc.h): WHERE CAN SOMETHING WALK, AND WHICH PLACES ARE
 * CONNECTED?  A CPU navmesh builder answers it by voxelizing the triangle soup again; the resident grid is that voxelization already.
 * What the build leaves is a compact heightfield in the Recast sense -- per column the floors with enough headroom, per floor one
 * step-limited link to each of the four neighbour columns, and the connected regions -- which is what a host's A*, flow field or
 * navmesh contouring starts from.
 *
 * NAVIGATION: the rule.  All float arithmetic is FP32, one IEEE operation per step in the order written, nothing fused (the library is
 * built with -ffp-contract=off); everything else is integers.  There is no tolerance in it.
 *   Box        the clamped sample box of lower / upper: world bounds, floor / ceil, clamped to [0, dim + 1], exactly as for every modifier
 *              and for vtmc_terrain_fragments.  Box sample (ix, iy, iz) is grid sample (box_lo + (ix, iy, iz)); dx, dy, dz are the box's
 *              samples per axis.  An empty box (no sample on some axis) is a success with 0 spans and is reported with dims (0, 0, 0).
 *              Columns are the (x, z) pairs of the box; y is up (VTMC_MOD_PLANE: f = height - y).  Column index c = ix + dx * iz
 *              (box-linear, x fastest).
 *   Solid      s > 0: strict, and NaN is not solid -- the classify kernel's test and the fragments' test.
 *   Floor      sample y of a column is a floor when y and y + 1 both lie in the box, a = S(x, y, z) > 0 and b = S(x, y + 1, z) <= 0 (a NaN
 *              above is no floor).  Then t = a / (a - b) and height = (float)y + t, y the GRID index, in grid units.  This is bit for bit
 *              the marching-cubes vertex on that lattice edge (-a / (b - a) gives the same bits).  a = +inf gives a NaN height with an
 *              unspecified payload: such a span is listed and never links.
 *   Clearance  the number c of consecutive not-solid samples (NaN counts as open) at y + 1, y + 2, ... inside the box.  If the run reaches
 *              the box's top sample plane the span is OPEN: clearance = VTMC_NAV_OPEN and ceil = VTMC_NAV_OPEN.  Otherwise
 *              ceil = y + 1 + c, the first solid sample above (a grid index).
 *   Span       a floor with clearance >= agent_height (open counts); other floors are not listed.  Spans are ordered by column index and
 *              bottom-up inside a column; the span index is the position in that order.  column_offsets (dx * dz + 1 int32 entries) is
 *              the exclusive prefix of the per-column span counts; its last entry is the total.
 *   Link       for span s and direction k (0: -x, 1: +x, 2: -z, 3: +z) the neighbour column must lie inside the box, otherwise the link
 *              is -1.  A span n of that column QUALIFIES iff
 *                d = h_n - h_s  and  fabsf(d) <= max_step,  and
 *                with top = min(ceil_s, ceil_n):  top is VTMC_NAV_OPEN,  or  (float)top - (h_s > h_n ? h_s : h_n) >= (float)agent_height.
 *              link[k] is the qualifying span with the smallest fabsf(d); on a tie the lower one wins; with none it is -1.  Links need
 *              not be symmetric (the nearest span of the neighbour column may have a nearer one of its own).
 *   Region     the components of the undirected graph whose edges are the links, taken in either direction.  region is the smallest span
 *              index of the component.
 * OUT OF SCOPE, deliberately: no agent-radius erosion in the build itself (a layer of its own on top of this one does it on the device:
 * vtmc_naverode.h, border distance and span erosion; NAVEROSION.md); no slope test by normal (slope is limited through max_step, the
 * largest height difference between neighbour columns); no stitching of the results of two boxes.  Path search is not here either but in
 * a layer of its own on top of this one: vtmc_navfield.h (locate, cost field, traced paths; PATHFINDING.md), and on that one
 * vtmc_navsight.h (line of sight over the spans, smoothed traces; PATHSMOOTHING.md).
 *
 * Life cycle.  The buffers are library-owned and grow-only, valid until the next vtmc_terrain_nav_build, vtmc_terrain_init,
 * vtmc_terrain_load or vtmc_destroy, or until a vtmc_nav_erode (vtmc_naverode.h), which replaces the result held by its erosion.  The result is a snapshot of the grid at build time: later edits do not invalidate it (rebuild the
 * box an edit touched, plus a margin of a column and agent_height samples).  The build changes nothing else: not the grid, the history,
 * the event counter, the dirty list, the extract result the context holds, the materials, the occlusion bytes or the scatter instances.
 * It waits for work queued on the context's stream, as vtmc_terrain_fragments does.
 *
 * vtmc_terrain_nav_build   builds the box; *n_spans (may be NULL) is the total.
 *   VTMC_ERR_NO_RESULT     without a terrain.
 *   VTMC_ERR_INVALID_ARG   (the previous nav result is kept) for a null ctx / lower / upper / params, a bound that is NaN, agent_height
 *                          outside 1..VTMC_NAV_MAX_AGENT_HEIGHT, max_step not finite or < 0, max_spans <= 0, flags != 0.
 *   VTMC_ERR_TOO_LARGE     when the total exceeds max_spans: the total is in vtmc_last_error, nothing is emitted and the context holds no
 *                          nav result afterwards (as with vtmc_scatter_surface).
 *   VTMC_ERR_DEVICE        ("labelling did not converge") should the region pass ever break its own bounds; no result is left.
 * vtmc_nav_read            copies the spans and (when not NULL) the dx * dz + 1 offsets; VTMC_ERR_CAPACITY when capacity is below the total.
 * vtmc_nav_info            the box (first grid sample, samples per axis) and the total of the result held; each may be NULL.
 * vtmc_nav_device_results  the device pointers of the same; each may be NULL.  They change with every build and with every
 *                          vtmc_nav_erode: ask again after either.
 * The last three answer VTMC_ERR_NO_RESULT before a build.
 */
#ifndef VTMC_NAV_H
#define VTMC_NAV_H

#include "vtmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_NAV_OPEN 0x7fffffff
#define VTMC_NAV_MAX_AGENT_HEIGHT 256

typedef struct vtmc_nav_params {
    int32_t agent_height;  /* samples, 1..VTMC_NAV_MAX_AGENT_HEIGHT */
    float   max_step;      /* grid units, finite, >= 0 */
    int32_t max_spans;     /* > 0 */
    uint32_t flags;        /* reserved, 0 */
} vtmc_nav_params;         /* 16 bytes */

typedef struct vtmc_nav_span {
    float   height;        /* grid units */
    int32_t y;             /* floor sample, grid index */
    int32_t clearance;     /* open samples above, or VTMC_NAV_OPEN */
    int32_t link[4];       /* -x, +x, -z, +z: span index or -1 */
    int32_t region;        /* smallest span index of its component */
} vtmc_nav_span;           /* 32 bytes */

int32_t vtmc_terrain_nav_build(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_nav_params *params, int32_t *n_spans);
int32_t vtmc_nav_read(vtmc_ctx *ctx, vtmc_nav_span *dst, int32_t capacity, int32_t *column_offsets /* dx*dz+1, may be NULL */);
int32_t vtmc_nav_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int32_t *n_spans);
int32_t vtmc_nav_device_results(vtmc_ctx *ctx, const vtmc_nav_span **d_spans, const int32_t **d_column_offsets, int32_t *n_spans);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_NAV_H */
