/*
 * vtmc_light.h -- voxel lighting on the resident terrain of libvtmc.so (not in the reference, whose renderer shades the island with one
 * directional light): two light channels, "sky" and "torch", flooded through the open samples of a box of the grid, on the device.  Same
 * library, same context, same conventions as vtmc.h, which this header includes; a host without lighting never needs it.
 *
 * It is the fifth non-local question about the grid: FRAGMENTS asks what still hangs on, NAVIGATION where one can walk, WATER what a pour
 * of water reaches, EROSION how slopes wear down, LIGHT how much light reaches a place -- the mouth of a cave against the end of a tunnel
 * 200 samples in, the torch a player has set down.  The ambient occlusion of vtmc.h is a local measure, a march of at most 6 cells, and
 * answers neither.  The answer stays on the device: two bytes per sample of the box, two bytes per vertex of an extract, and a probe for
 * what moves.
 *
 * LIGHT: the rule.  Integers and 32-bit copies only; the one FP32 step is the nearest-sample formula of WATER.  Nothing has a tolerance.
 *   Box        the clamped sample box of lower / upper, exactly as for every modifier, for FRAGMENTS and for WATER.  An empty box is a
 *              success with dims (0, 0, 0).
 *   Open       a sample s is open when it is not solid, i.e. not s > 0.  NaN and both zeros are open.  The grid is read once, as it is at
 *              the time of the call.
 *   Sky        a sample (ix, j, iz) of the box is SKYLIT when it is open and every sample (ix, j', iz) of the box with j' > j is open.  Its
 *              sky emission is sky_level; sky_level == 0 means no sky light at all.  Every other sample has sky emission 0.  The top face
 *              of the box is the sky: the host puts it above the ground.
 *   Source     {float position[3]; int32_t level;}, 16 bytes, level in 1..255.  At most VTMC_LIGHT_MAX_SOURCES sources per call.  A
 *              source's sample is the NEAREST one, by WATER's source rule: per axis g = (p - origin) / scale; i = (int)floorf(g + 0.5f)
 *              (saturating).  A source whose sample lies outside the box or is solid is DARK: source_lit[k] = 0.  Otherwise it is lit,
 *              source_lit[k] = 1.  The torch emission of a sample is the largest level of the lit sources that sit on it, else 0.
 *   Field      each of the two channels is flooded separately, with its own emission e and its own falloff f (sky_falloff,
 *              torch_falloff, each 1..255).  The graph is the open samples of the box, 6-connectivity, inside the box.  v is the LEAST
 *              function with v(s) = max(e(s), max over the open neighbours n of s of v(n) - f, 0); equivalently v(s) is the maximum over
 *              the open samples q of e(q) - f * d(q, s), clipped at 0, with d the hop distance in that graph.  A solid sample holds 0 in
 *              both channels.  The fixed point is unique, so the result depends neither on the launch shape nor on the order of a sweep
 *              nor on the number of rounds: the rule names none of these.
 *   Volume     the box's dims, x fastest, one vtmc_light_sample {uint8_t sky, torch;} (2 bytes) per sample.  There is no padding.
 *   Probe      the nearest sample of a position by the source rule; inside the box: that sample's two bytes; otherwise, and for a
 *              position that is not finite, (0, 0).
 *   Vertex     for the result the context holds, if and only if vtmc_ao_vertices would accept it: it came from the resident terrain and is
 *              not a level-of-detail result; both output modes.  The grid coordinate g of the vertex and the cell origin (i0, j0, k0) are
 *              found exactly as the occlusion rule's fetch finds them (vtmc.h: g = (float)(8*b) + p per axis, the clamp to [0, n-1],
 *              floorf, i0 <= n-2).  The vertex's two bytes are, per channel, the maximum over those of the cell's eight corner samples
 *              (i0 + a, j0 + b, k0 + c), a, b, c in {0, 1}, that lie inside the light box; with no corner inside, (0, 0).  It reads the
 *              light volume only, never the grid.
 * OUT OF SCOPE, deliberately: no incremental relight after an edit (light again: LIGHTING.md says what that costs); one box, and light
 * does not enter through its sides or its bottom; no coloured light; level-of-detail results are refused; nothing is saved with the
 * terrain or journaled.
 *
 * Life cycle.  The context holds one light result.  vtmc_terrain_init, vtmc_terrain_load and vtmc_destroy drop it; an edit keeps it: it is a
 * snapshot, as the water and the nav result are.  The buffers are library-owned and grow-only.  A light call changes nothing else the
 * context holds: not the grid, the history, the event counter, the dirty list, the extract result, the materials, the occlusion, the
 * scatter, the nav result, the flow field, the crowd, the water or the erosion maps.  It waits for the work queued on the context's
 * stream, as vtmc_terrain_flood does.
 *
 * vtmc_terrain_light          lights the box by the rule; source_lit (n_sources bytes, may be NULL) is filled.  n_sources == 0 leaves the
 *                             sky alone.  params->flags must be 0.
 * vtmc_light_info             the box's first sample and dims, the samples with sky > 0 and with torch > 0, and the rounds the last call's
 *                             relaxation took (at most VTMC_LIGHT_MAX_ROUNDS); each may be NULL.
 * vtmc_light_read             the volume; capacity in samples, VTMC_ERR_CAPACITY when it is below the box's sample count.
 * vtmc_light_device_results   the device pointer of the volume (NULL for an empty box) and the box's dims; each may be NULL.
 * vtmc_light_probe            by Probe, one lane per position; sky_out and torch_out (n bytes each) may each be NULL.
 * vtmc_light_vertices         by Vertex, the two bytes of every vertex of the result the context holds into a library-owned, grow-only
 *                             buffer; *n_vertices (may be NULL) receives n.  Soup: vertex 3*t + v, n = 3*T.  Indexed: n = V.
 * vtmc_light_read_vertices    copies the n samples; a capacity below n is VTMC_ERR_INVALID_ARG, as vtmc_ao_read_vertices has it.
 * vtmc_light_vertices_device_results   the device pointer of the same.
 *                             The bytes belong to one extract result and one light result: after a later extract or a later
 *                             vtmc_terrain_light the two read calls answer VTMC_ERR_NO_RESULT until vtmc_light_vertices runs again.
 *   VTMC_ERR_NO_RESULT     vtmc_terrain_light before vtmc_terrain_init; the other calls before a light call; vtmc_light_vertices also where
 *                          vtmc_ao_vertices would refuse the result.
 *   VTMC_ERR_INVALID_ARG   (the previous result is kept) for a null pointer, a bound that is NaN, n_sources outside
 *                          0..VTMC_LIGHT_MAX_SOURCES, a position that is not finite, a level outside 1..255, a falloff outside 1..255,
 *                          sky_level outside 0..255, flags != 0, n < 0.
 *   VTMC_ERR_DEVICE        "light did not settle", should the relaxation exceed VTMC_LIGHT_MAX_ROUNDS rounds; no result is left.  The bound
 *                          is a condition, not a measurement: a light of level at most 255 with falloff at least 1 travels at most 254
 *                          hops, every round that reads the previous round's values carries every cheapest path at least one hop further,
 *                          and one more round sees no change.
 */
#ifndef VTMC_LIGHT_H
#define VTMC_LIGHT_H

#include "vtmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_LIGHT_MAX_SOURCES 4096
#define VTMC_LIGHT_MAX_ROUNDS 256
#define VTMC_LIGHT_MAX_LEVEL 255

typedef struct vtmc_light_source {
    float position[3];     /* world space; the nearest sample is the source's */
    int32_t level;         /* 1..VTMC_LIGHT_MAX_LEVEL */
} vtmc_light_source;       /* 16 bytes */

typedef struct vtmc_light_params {
    int32_t sky_level;     /* 0..VTMC_LIGHT_MAX_LEVEL; 0: no sky light */
    int32_t sky_falloff;   /* 1..255, lost per hop */
    int32_t torch_falloff; /* 1..255, lost per hop */
    uint32_t flags;        /* reserved, must be 0 */
} vtmc_light_params;       /* 16 bytes */

typedef struct vtmc_light_sample {
    uint8_t sky, torch;
} vtmc_light_sample;       /* 2 bytes */

int32_t vtmc_terrain_light(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_light_params *params,
                           const vtmc_light_source *sources, int32_t n_sources, uint8_t *source_lit /* n_sources, may be NULL */);
int32_t vtmc_light_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int64_t *n_sky, int64_t *n_torch, int32_t *rounds);
int32_t vtmc_light_read(vtmc_ctx *ctx, vtmc_light_sample *dst, int64_t capacity_samples);
int32_t vtmc_light_device_results(vtmc_ctx *ctx, const vtmc_light_sample **d_volume, int32_t box_dims[3]);
int32_t vtmc_light_probe(vtmc_ctx *ctx, const float *positions, int32_t n, uint8_t *sky_out, uint8_t *torch_out);
int32_t vtmc_light_vertices(vtmc_ctx *ctx, int64_t *n_vertices);
int32_t vtmc_light_read_vertices(vtmc_ctx *ctx, vtmc_light_sample *dst, int64_t capacity_vertices);
int32_t vtmc_light_vertices_device_results(vtmc_ctx *ctx, const vtmc_light_sample **d_values, int64_t *n_vertices);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_LIGHT_H */
