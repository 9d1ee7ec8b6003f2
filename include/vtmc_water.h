/*
 * vtmc_water.h -- standing water on the resident terrain of libvtmc.so (not in the reference, which dresses its island with water meshes
 * of a package it does not vendor): flood a box of the grid from sources to their levels, on the device.  Same library, same context,
 * same conventions as vtmc.h, which this header includes; a host without water never needs it.
 *
 * It is the third non-local question about the grid: FRAGMENTS asks what still hangs on, NAVIGATION where one can walk, WATER what a pour
 * of water reaches -- a lake, a sea level, a flooded cave, the hole that fills when a player digs through a lake's rim.  The answer stays
 * on the device: a body index per sample, a density volume that a marching-cubes pass turns into the water's surface, and a probe for what
 * swims or floats.
 *
 * WATER: the rule.  Integers and 32-bit copies, plus the few FP32 steps named below; each FP32 step is one IEEE operation, in the order
 * written; no step has a tolerance.
 *   Box        the clamped sample box of lower / upper, exactly as for every modifier and for FRAGMENTS.  An empty box is a success with no
 *              bodies and dims (0, 0, 0).
 *   Open       a sample s is open when it is not solid, i.e. not s > 0.  NaN and both zeros are open.
 *   Plane      the height of sample plane j (a grid index) is y_j = (float)j * scale + origin_y, the terrain's own position formula.  Plane j
 *              is UNDER level h iff y_j <= h.  The formula is monotonic in j, so every level becomes one integer plane index (the highest
 *              plane under it, or -1) and everything after that compares integers.
 *   Source     {float position[3]; float level;}, 16 bytes.  At most VTMC_WATER_MAX_SOURCES sources and at most VTMC_WATER_MAX_LEVELS distinct
 *              level bit patterns per call.  A source's sample is the NEAREST one: per axis g = (p - origin) / scale; i = (int)floorf(g +
 *              0.5f) (saturating).  A source whose sample lies outside the box is DRY.
 *   Flood      the levels are processed from the highest to the lowest (+0 before -0).  At level h, first every source of that level whose
 *              sample is already wet JOINS that sample's body.  Then the other sources of that level are seeds in the graph of the samples of
 *              the box that are open, under h and not yet wet, with 6-connectivity inside the box.  A seed whose sample is not in that graph
 *              is dry.  Every component that holds a seed becomes one body at level h; its samples are wet.
 *              Two floods are nested or disjoint: a lower flood that overlaps a higher one has its source inside the higher one (everything
 *              it could reach lies under the higher level too, and is joined to the source), so that source joined.  Hence leaving out the
 *              wet samples changes no component of a source that is a seed.
 *   Body order descending level, then ascending grid index of the seed; the seed is the body's sample of smallest grid index.
 *              source_body[k] is the body index of source k, or -1 for a dry source.
 *   Body       the record vtmc_water_body, 64 bytes: seed, tight inclusive bounds lo / hi (grid indices), level, n_samples, n_surface (the wet
 *              samples whose +y neighbour lies in the box, is open and is not wet), flags (VTMC_WATER_AT_FACE: the body holds a sample on the
 *              bottom face or one of the four side faces of the box -- the water goes on outside, the host should enlarge the box),
 *              n_sources (seeds and joiners), two reserved words, 0.
 *   Volumes    per axis the box's dims d rounded up to 8 * ceil(max(d - 2, 1) / 8) + 2 samples, x fastest; volume sample (ix, iy, iz) is box
 *              sample (ix, iy, iz); the padding is dry.  The BODY VOLUME holds one int32 per sample: the body index, or -1.
 *              The WATER VOLUME holds one float: with L a level and j a grid plane, t = L - y_j; t = t / scale; t = clamp(t, -1, 1).
 *                a wet sample holds t(level of its body, j): in [0, 1], and 0 exactly at the level;
 *                a NEAR sample -- not wet, with a wet sample among its 26 neighbours inside the box -- takes L from the neighbour body of
 *                smallest index, which is the largest level among them; it holds t(L, j) when it is solid or t <= 0, and -1.0f otherwise
 *                (an open sample under the level that the water does not reach: diagonal contact only);
 *                every other sample holds -1.0f.
 *              The field is linear across the free surface and runs one sample into the ground, so the extracted surface lies at the level
 *              and ends inside the terrain, not half a cell short of the shore.  The volume is shaped so that vtmc_extract_volumes_device
 *              takes it as a batch of one (nx = volume dim - 2, strides 1, dim_x, dim_x * dim_y); that extract replaces the context's
 *              extract result, as any extract does.  World position of a record: origin + (box_lo + 8b + p) * scale.
 *   Probe      the nearest sample of a position by the source rule; in the box and wet: its body and depth = level - position_y (one FP32
 *              subtraction); otherwise body -1 and depth 0.  A position that is not finite gives -1.
 * OUT OF SCOPE, deliberately: no flow, no volume of water poured (a source fills its component to its level, however large); one box; a
 * snapshot of the grid at the time of the call.
 *
 * Life cycle.  The context holds one water result.  vtmc_terrain_init, vtmc_terrain_load and vtmc_destroy drop it; an edit keeps it: it is a
 * snapshot, as a nav result is.  The buffers are library-owned and grow-only.  A flood changes nothing else the context holds: not the grid,
 * the history, the event counter, the dirty list, the extract result, the materials, the occlusion, the scatter, the nav result, the flow
 * field or the crowd.  It waits for the work queued on the context's stream, as vtmc_terrain_fragments does.
 *
 * vtmc_terrain_flood          floods by the rule; source_body (n_sources words, may be NULL) and *n_bodies (may be NULL) are filled.
 *                             n_sources == 0 gives an all-dry result.  flags must be 0.
 * vtmc_water_info             the box's first sample and dims, the volume dims, the bodies, the wet samples; each may be NULL.
 * vtmc_water_bodies           the records; VTMC_ERR_CAPACITY when capacity is below the body count.
 * vtmc_water_read             the water volume and / or the body volume (each may be NULL), capacity in samples of one volume.
 * vtmc_water_device_results   the device pointers of both volumes and the volume dims; each may be NULL.
 * vtmc_water_probe            by Probe, one lane per query; body_out and depth_out may each be NULL.
 *   VTMC_ERR_NO_RESULT     flood before vtmc_terrain_init; the other five before a flood.
 *   VTMC_ERR_INVALID_ARG   (the previous result is kept) for a null pointer, a bound that is NaN, n_sources outside 0..VTMC_WATER_MAX_SOURCES,
 *                          a position or level that is not finite, more than VTMC_WATER_MAX_LEVELS levels, flags != 0, n < 0.
 *   VTMC_ERR_DEVICE        "labelling did not converge", should the labelling ever break its own bounds; no result is left.
 */
#ifndef VTMC_WATER_H
#define VTMC_WATER_H

#include "vtmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_WATER_MAX_SOURCES 4096
#define VTMC_WATER_MAX_LEVELS 8
#define VTMC_WATER_AT_FACE 1

typedef struct vtmc_water_source {
    float position[3];     /* world space; the nearest sample is the source's */
    float level;           /* world height the water stands at */
} vtmc_water_source;       /* 16 bytes */

typedef struct vtmc_water_body {
    int32_t  seed[3];      /* the body's sample of smallest grid index */
    int32_t  lo[3], hi[3]; /* tight, inclusive, grid indices */
    float    level;
    int32_t  n_samples;    /* wet samples */
    int32_t  n_surface;    /* wet samples under an open, dry sample of the box */
    uint32_t flags;        /* VTMC_WATER_AT_FACE or 0 */
    int32_t  n_sources;    /* seeds and joiners */
    uint32_t reserved[2];  /* 0 */
} vtmc_water_body;         /* 64 bytes */

int32_t vtmc_terrain_flood(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_water_source *sources, int32_t n_sources,
                           uint32_t flags, int32_t *source_body /* n_sources, may be NULL */, int32_t *n_bodies);
int32_t vtmc_water_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int32_t volume_dims[3], int32_t *n_bodies, int64_t *n_wet);
int32_t vtmc_water_bodies(vtmc_ctx *ctx, vtmc_water_body *dst, int32_t capacity);
int32_t vtmc_water_read(vtmc_ctx *ctx, float *water_dst, int32_t *body_dst, int64_t capacity_samples);
int32_t vtmc_water_device_results(vtmc_ctx *ctx, const float **d_water, const int32_t **d_body, int32_t volume_dims[3]);
int32_t vtmc_water_probe(vtmc_ctx *ctx, const float *positions, int32_t n, int32_t *body_out, float *depth_out);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_WATER_H */
