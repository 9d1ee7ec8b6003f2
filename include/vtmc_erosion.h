/*
 * vtmc_erosion.h -- hydraulic and thermal erosion of the resident terrain of libvtmc.so (not in the reference, whose terrain is noise and
 * constructive solids and never weathers): a modifier kind, VTMC_MOD_EROSION, that runs a time-stepped simulation on the heightfield of a
 * box of the grid, on the device, and three readers of the maps it leaves.  Same library, same context, same conventions as vtmc.h, which
 * this header includes; a host without erosion never needs it.
 *
 * VTMC_MOD_EROSION is a kind of vtmc_modifier (vtmc.h) and is queued with vtmc_terrain_update like every other kind: its box comes from
 * lower / upper, it marks the dirty blocks of that box, it is journaled (its box, no halo, one undo step; a redo puts the values back and
 * simulates nothing), it takes one event number and draws nothing with it, and it sees what earlier modifiers of its queue wrote.
 * add_or_erode is ignored, as for the brushes.  data must be NULL and data_dims[1] must be 0.
 *   p[0] = Kr  rain depth per unit time, 0..VTMC_EROSION_MAX_RAIN        p[4] = Kd  deposit, 0..1
 *   p[1] = Ke  evaporation, >= 0, Ke * dt <= 1                           p[5] = dt  time step, in (0, 1]
 *   p[2] = Kc  sediment capacity, 0..VTMC_EROSION_MAX_CAPACITY           p[6] = T   talus: the largest stable height step between
 *   p[3] = Ks  dissolve, 0..1                                                       neighbouring columns, >= 0
 *   data_dims[0] = iterations, 1..VTMC_EROSION_MAX_ITERATIONS            p[7] = Kt  thermal rate, 0..VTMC_EROSION_MAX_THERMAL; 0: off
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error, nothing written by it): any of p[0..7] not finite, negative or outside
 * its range; Ke * dt > 1 (one FP32 product); iterations outside its range; data not NULL; data_dims[1] != 0.
 *
 * EROSION: the rule.  Everything is in grid units: sample indices, column spacing 1; the voxel scale never enters.  Every step below is
 * FP32 and one IEEE operation (the library is built without contraction; sqrtf and / are the correctly rounded ones), in the order
 * written, left to right where no parentheses stand.  Every four-way sum over the directions k = 0..3 = [-x, +x, -z, +z] is PAIRED by
 * axis, sum4(v) = (v0 + v1) + (v2 + v3), which is what makes the result of a mirrored or transposed terrain the mirrored or transposed
 * result, bit for bit.  min(a, b) is a < b ? a : b and max(a, b) is a > b ? a : b.
 *   Box        the clamped sample box [lx..ux] x [ly..uy] x [lz..uz] of lower / upper, exactly as for every modifier; nx = ux - lx + 1,
 *              nz = uz - lz + 1 columns, column (x, z) at plane index (x - lx) + nx * (z - lz).
 *   Heights    a column is ACTIVE when sample uy is not solid (!(S > 0), the classify test) and some j in [ly, uy - 1] has S_j > 0.  With
 *              the topmost such j, h0 = (float)j + S_j / (S_j - S_{j+1}).  Inactive columns -- solid through the top of the box, or
 *              open all the way down -- are WALLS: nothing flows across them and the thermal step ignores them.  The faces of the box are
 *              walls too (closed borders).  The samples are taken to be finite.
 *   State      planes of nx * nz floats: terrain b = h0, water d = 0, suspended sediment s = 0, four outflow fluxes f[k] = 0; a mask
 *              byte per column.  Every plane holds 0 on an inactive column, always.
 *   Neighbour  the neighbour n of a column in direction k COUNTS only when both columns are active and inside the box.
 *   One step   on every active column, from (b, d, f, s):
 *     Flux       d1 = d + dt * Kr;  H = b + d1.  Per direction f'_k = f_k + (dt * G) * (H - H_n), set to 0 if it is not > 0 or no
 *                neighbour counts.  out = sum4(f');  vol = out * dt.  If vol > d1: K = d1 / vol, every f'_k = f'_k * K, and
 *                out = sum4(f') again from the scaled values.
 *     Water      in_k = the flux of the neighbour in direction k towards this column (its f' of the opposite direction), 0 without one.
 *                in = sum4(in).  d2 = d1 + dt * (in - out), set to 0 if it is not > 0.
 *     Speed      wx = ((in_0 - f'_0) + (f'_1 - in_1)) * 0.5;  wz = ((in_2 - f'_2) + (f'_3 - in_3)) * 0.5;  db = (d1 + d2) * 0.5;
 *                u = db > DEPTH_EPS ? wx / db : 0;  w = db > DEPTH_EPS ? wz / db : 0;  sp = min(sqrtf(u * u + w * w), 1 / dt).
 *     Erosion    gx = (b_{+x} - b_{-x}) * 0.5, a neighbour that does not count replaced by the column's own b; gz alike.
 *                g2 = gx * gx + gz * gz;  sa = max(sqrtf(g2 / (1 + g2)), SIN_MIN);  C = Kc * sa * sp.
 *                If C > s: e = min(Ks * (C - s), d2), b1 = b - e, s1 = s + e.  Otherwise q = Kd * (s - C), b1 = b + q, s1 = s - q.
 *     Transport  conservative, no back-trace: fr_k = d1 > 0 ? (f'_k * dt) / d1 : 0;  give_k = s1 * fr_k;  gin_k = the give of the neighbour
 *                in direction k towards this column, 0 without one.  s2 = (s1 - sum4(give)) + sum4(gin).
 *     Evaporate  d3 = d2 * (1 - Ke * dt).
 *     Thermal    on b1, per direction, the same expression seen from both sides: m_k = Kt * ((max(b1, b1_n) - min(b1, b1_n)) - T), set
 *                to 0 if it is not > 0 or no neighbour counts; sign_k = -1 when b1 > b1_n, +1 when b1 < b1_n, 0 when they are equal;
 *                t_k = sign_k * m_k.  b2 = b1 + sum4(t).
 *              The next step starts from (b2, d3, f', s2).
 *   Write-back after the last step h1 = b clamped to [(float)ly + 0.5, (float)(uy - 1)]; a column the clamp changed counts in n_clamped:
 *              the box is too low, or too shallow, for what the simulation did there.  An active column with h1 != h0 (it counts in
 *              n_rewritten) is rewritten on the samples y of the box with min(h0, h1) - 1 <= (float)y <= max(h0, h1) + 1:
 *              S = clamp(h1 - (float)y, -1, 1), the flatten brush's profile.  Every other sample of the box keeps its 32 bits.  A column
 *              so written reads back to exactly h1 under Heights.  Suspended sediment left after the last step is NOT put down.
 * Why the caps.  For heights below 2^11, at most 2^20 columns and 2^16 steps: all the water ever rained is at most
 * W = 2^20 * 2^16 * dt * Kr = 2^36 * dt * Kr, and no depth exceeds it: below 2^44 at Kr <= 2^8.  A column erodes at most d2 per step, so
 * all the sediment ever taken up is below 2^16 * 2^44 = 2^60, and |b| and s stay below 2^61: gx * gx + gz * gz < 2^123 is finite, and
 * so are H and the fluxes, which grow by at most (dt * G) * 2^62 a step (below 2^82 before the scaling).  After the scaling
 * out * dt <= d1 <= W, so out <= 2^36 * Kr = 2^44 whatever dt is, and in, wx and wz stay below 2^46.  With db > DEPTH_EPS > 2^-14 the
 * speeds stay below 2^60 and u * u + w * w below 2^121; sp is finite even where 1 / dt is not.  C = Kc * sa * sp < 2^16 * 2^61.
 * Hence VTMC_EROSION_MAX_RAIN = 2^8 and VTMC_EROSION_MAX_CAPACITY = 2^16, both far above anything a terrain wants (rain of order 0.01,
 * capacity of order 1).
 * OUT OF SCOPE, deliberately: open borders, rain maps, point sources; one height per column (a surface under an overhang is not eroded,
 * and a cave roof inside the rewritten band is overwritten).
 *
 * Life cycle.  The maps of the last erosion are a snapshot: an edit, an undo or a redo keeps it, vtmc_terrain_init and vtmc_terrain_load
 * drop it, the next erosion replaces it.  The buffers are library-owned and grow-only; once they are large enough an erosion allocates
 * nothing, and all its launches -- three per step -- are queued back to back on the context's stream with no read-back between them.
 *
 * vtmc_erosion_info            fills a vtmc_erosion_report: the clamped box, nx, nz, the iterations and the three column counts (integers
 *                              counted on the device).  It waits for the work queued on the context's stream.
 * vtmc_erosion_read            one map to the host, x fastest: VTMC_EROSION_HEIGHT_BEFORE (h0), _HEIGHT_AFTER (h1), _WATER (d),
 *                              _SEDIMENT (s) are nx * nz floats, _ACTIVE is nx * nz bytes (1: active); every map holds 0 on an inactive
 *                              column.  capacity_bytes below the map's size: VTMC_ERR_CAPACITY.
 * vtmc_erosion_device_results  the device pointers of the same maps (each may be NULL), valid until the next erosion.
 *   VTMC_ERR_NO_RESULT     before any erosion, and after vtmc_terrain_init / vtmc_terrain_load.
 *   VTMC_ERR_INVALID_ARG   a null ctx, info or dst; a map that is none of the five.
 */
#ifndef VTMC_EROSION_H
#define VTMC_EROSION_H

#include "vtmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_MOD_EROSION 12

#define VTMC_EROSION_G 9.81f
#define VTMC_EROSION_SIN_MIN 0.05f
#define VTMC_EROSION_DEPTH_EPS 1.0e-4f
#define VTMC_EROSION_MAX_ITERATIONS 65536
#define VTMC_EROSION_MAX_RAIN 256.0f
#define VTMC_EROSION_MAX_CAPACITY 65536.0f
#define VTMC_EROSION_MAX_THERMAL 0.125f

#define VTMC_EROSION_HEIGHT_BEFORE 0
#define VTMC_EROSION_HEIGHT_AFTER 1
#define VTMC_EROSION_WATER 2
#define VTMC_EROSION_SEDIMENT 3
#define VTMC_EROSION_ACTIVE 4

typedef struct vtmc_erosion_report {
    int32_t lo[3];        /* first sample of the clamped box */
    int32_t hi[3];        /* last sample, inclusive */
    int32_t nx, nz;       /* columns per axis; a map holds nx * nz entries, x fastest */
    int32_t iterations;
    int32_t n_active;     /* columns that took part */
    int32_t n_rewritten;  /* active columns with h1 != h0 */
    int32_t n_clamped;    /* active columns whose final height the clamp changed */
} vtmc_erosion_report;    /* 48 bytes */

int32_t vtmc_erosion_info(vtmc_ctx *ctx, vtmc_erosion_report *info);
int32_t vtmc_erosion_read(vtmc_ctx *ctx, int32_t map, void *dst, int64_t capacity_bytes);
int32_t vtmc_erosion_device_results(vtmc_ctx *ctx, const float **d_height_before, const float **d_height_after, const float **d_water,
                                    const float **d_sediment, const uint8_t **d_active);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_EROSION_H */
