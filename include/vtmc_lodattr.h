/*
 * vtmc_lodattr.h -- per-vertex material weights and ambient occlusion of a level-of-detail extract of libvtmc.so and of its skirts (not in
 * the reference, which meshes every block at full resolution).  Same library, same context, same conventions as vtmc.h; this header
 * includes vtmc_lodskirt.h, which includes vtmc.h.  A host that shades no level-of-detail mesh never needs it.
 *
 * vtmc_material_vertices and vtmc_ao_vertices answer VTMC_ERR_NO_RESULT after vtmc_terrain_extract_lod and go on doing so: their rules
 * are written for blocks of the full-resolution grid.  This layer states the two rules for a node (o, L) and owns its buffers: it never
 * writes the values those two calls hold, and they answer for every result exactly as without it.
 *
 * LODATTR: the rule.  FP32, one IEEE operation per step in the order written (library built with -ffp-contract=off).  A node (o, L) has
 * the cell origin o, a multiple of 8 * s with s = 2^L; p is a node-local position in [0, 8] as the record holds it, n its record normal.
 *   Materials     the rule of vtmc_material_vertices with the fine grid coordinate
 *                   gx = (float)o.x + p.x * (float)s;  gy, gz alike
 *                 in place of (float)(8*bx) + p.x: the product is exact, only the sum rounds.  Everything from tx = gx * sx on is that
 *                 rule unchanged.  At L = 0 this is that rule bit for bit.  The weights are one function of the world position, so two
 *                 nodes that meet in a seam agree there up to the rounding of gx.
 *   Occlusion     the rule of vtmc_ao_vertices applied to the node's own SAMPLE LATTICE, the samples the node was meshed from, so that the
 *                 vertex lies on the isosurface the march walks away from.  With (dim_x, dim_y, dim_z) = (W+2, E+2, H+2):
 *                   S_L[i, j, k] = S[min(i*s, dim_x - 1), min(j*s, dim_y - 1), min(k*s, dim_z - 1)],  n_L = (dim - 2) / s + 2 samples per axis
 *                   gx = (float)(o.x / s) + p.x;  gy, gz alike                    (lattice coordinates: lattice sample i sits at i)
 *                   Rg = radius / voxel_scale, counted in the NODE'S OWN CELLS, as the depth of vtmc_lod_skirts is
 *                 and everything else as written there: h[], fall[], the 26 directions, fetch() with clamp-to-edge over n_L samples per
 *                 axis.  The last lattice index, n_L - 1, maps to the replicated plane dim - 1: the same clamp as tile index 9 of the
 *                 extract's rule.  radius / voxel_scale <= VTMC_AO_MAX_RADIUS_CELLS as there.  At L = 0 the lattice is the grid and this
 *                 is that rule bit for bit.
 *                 LIMIT: a coarse node's march reaches 2^L times as far in the world, so OCCLUSION IS NOT CONTINUOUS ACROSS A CHANGE OF
 *                 LEVEL: the two sides of a seam are shaded by two different radii.
 *   Skirts        the records of vtmc_lod_skirts come in pairs per quad: record 2q is (b, a, a') and record 2q + 1 is (b, a', b').  A skirt
 *                 corner takes the attribute of the mesh vertex it came from, as it takes its normal:
 *                   record 2q      attr(b), attr(a), attr(a)
 *                   record 2q + 1  attr(b), attr(a), attr(b)
 *                 where b and a are corners 0 and 1 of record 2q -- position and normal -- and the node is that record's `block`.  A
 *                 displaced corner is never evaluated at its own position: it lies inside the solid and would come out dark.
 * The rule is pointwise: the values depend neither on the output mode's order nor on how a kernel stages samples.
 *
 * Attributes and targets.  VTMC_LODATTR_MATERIAL: VTMC_MATERIAL_CHANNELS = 8 bytes per vertex; VTMC_LODATTR_AO: 1 byte per vertex.
 * VTMC_LODATTR_MESH: the vertices of the result, 3*T in soup mode (vertex 3*t + v), V in indexed mode.  VTMC_LODATTR_SKIRTS: the
 * 3 * n corners of the n skirt records, in record order, in either mode.
 *
 * Life cycle.  The values belong to ONE result and ONE set of skirts: any later extract, vtmc_terrain_update / _undo / _redo / _load /
 * _init makes all of them stale; vtmc_lod_skirts after a compute call drops the skirt target of both attributes and nothing else.  A
 * compute call covers the mesh and, when skirts of the current result exist at the time of the call, the skirts; otherwise
 * *n_skirt_vertices = 0 and the skirt target answers VTMC_ERR_NO_RESULT.  The buffers are library-owned and grow-only.  A refused call
 * keeps the previous values.  Neither attribute needs or disturbs the other.  Derived data: neither saved nor journaled.
 *
 * vtmc_lod_material_vertices   the weights of the level-of-detail result the context holds and of its skirts.
 * vtmc_lod_ao_vertices         the occlusion bytes of the same; the material layer plays no part.
 * vtmc_lodattr_info            the numbers of values an attribute holds; *n_skirt_vertices = 0 without a skirt target.
 * vtmc_lodattr_read            copies a target's values, capacity_vertices * (8 or 1) bytes at the least.
 * vtmc_lodattr_device_results  the device pointer of the same (valid until the next compute call of the attribute / destroy).
 * The count pointers may be NULL.  T = 0 is success with 0 vertices.
 *   VTMC_ERR_NO_RESULT     the context's current result is not a level-of-detail extract's; vtmc_lod_material_vertices before
 *                          vtmc_material_init; a reader before its attribute's compute call on the current result, or of the skirt
 *                          target when that call found no skirts or vtmc_lod_skirts ran since.
 *   VTMC_ERR_INVALID_ARG   null ctx or params; what vtmc_ao_vertices refuses of its params (radius not finite or <= 0, radius /
 *                          voxel_scale > VTMC_AO_MAX_RADIUS_CELLS, strength not finite or outside [0, 1], steps outside
 *                          1..VTMC_AO_MAX_STEPS, flags != 0); an unknown attribute or target; a capacity below n; dst null with n > 0.
 */
#ifndef VTMC_LODATTR_H
#define VTMC_LODATTR_H

#include "vtmc_lodskirt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_LODATTR_MATERIAL 0   /* attribute: 8 bytes per vertex */
#define VTMC_LODATTR_AO       1   /* attribute: 1 byte per vertex */
#define VTMC_LODATTR_MESH     0   /* target: the vertices of the level-of-detail result */
#define VTMC_LODATTR_SKIRTS   1   /* target: the 3 * n corners of the skirt records, record order */

int32_t vtmc_lod_material_vertices(vtmc_ctx *ctx, int64_t *n_vertices, int64_t *n_skirt_vertices);
int32_t vtmc_lod_ao_vertices(vtmc_ctx *ctx, const vtmc_ao_params *params, int64_t *n_vertices, int64_t *n_skirt_vertices);
int32_t vtmc_lodattr_info(vtmc_ctx *ctx, int32_t attribute, int64_t *n_vertices, int64_t *n_skirt_vertices);
int32_t vtmc_lodattr_read(vtmc_ctx *ctx, int32_t attribute, int32_t target, uint8_t *dst, int64_t capacity_vertices);
int32_t vtmc_lodattr_device_results(vtmc_ctx *ctx, int32_t attribute, int32_t target, const uint8_t **d_values, int64_t *n_vertices);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_LODATTR_H */
