/*
 * vtmc_lodskirt.h -- skirt triangles over the seams of a level-of-detail extract of libvtmc.so (not in the reference, which meshes every
 * block at full resolution and has no seams).  Same library, same context, same conventions as vtmc.h, which this header includes; a host
 * that draws no level-of-detail mesh never needs it.
 *
 * vtmc_terrain_extract_lod leaves the meshes of neighbouring nodes of different levels ending on their shared face in two different
 * curves; the sliver of the face between the curves is a hole a viewer looks through.  The hole lies in the plane of the face.
 * vtmc_lod_skirts hangs a strip of triangles in that same plane from each node's boundary curve towards the solid side, on the device,
 * from the records of the result the context holds.  It never reads the grid and changes nothing of the extract's result.
 *
 * LODSKIRT: the rule.  Integers and 32-bit copies, plus the FP32 steps of Displacement; each FP32 step is one IEEE operation, in the order
 * written, nothing fused; no floating-point comparison decides a count or an order.
 *   Faces         the faces of a node are numbered 0..5 = -x, +x, -y, +y, -z, +z; face f has axis f >> 1 and lies at node-local coordinate
 *                 0.0f (even f) or 8.0f (odd f) of that axis.  A node (o, L) covers n = 8 * 2^L cells per axis from the cell origin o.
 *   Flagged       face f of node (o, L) is FLAGGED when (1) the box of the same size beyond it, origin o -/+ n along the face's axis, lies
 *                 inside the terrain (0 <= origin and origin + n <= cells on that axis), and (2) the node list holds no node with that
 *                 origin at level L.  With VTMC_LODSKIRT_ALL_FACES condition (1) alone flags the face.  A face on the terrain's boundary is
 *                 never flagged.  The node's MASK is the byte with bit f set for every flagged face.  The masks are computed on the host
 *                 from the node list the context keeps, through a hash of (origin, level); the 2:1 property of the selection is not
 *                 assumed.  Where a level-L node meets a level-(L+1) node both sides are flagged: the fine node has no neighbour of its
 *                 own level there, and the coarse node's same-size neighbour was split.
 *   Quads         the triangles are taken in result order, and for each triangle the faces in ascending order.  A flagged face of the
 *                 triangle's node (its `block`) yields ONE QUAD when exactly two of the triangle's three positions have the face-axis
 *                 coordinate bitwise equal to the face's 0.0f (0x00000000) or 8.0f (0x41000000).  A vertex on a lattice edge inside the
 *                 face plane has that coordinate exact in every emit variant, because only the edge-axis component is interpolated.  Three
 *                 positions on the plane, or fewer than two, yield nothing.  Let c be the position off the plane and a, b the other two in
 *                 the triangle's cyclic order 0 -> 1 -> 2 -> 0 (a follows c, b follows a).
 *   Displacement  of a vertex p with record normal n, with (u, v) the two axes other than the face's, ascending:
 *                   d_u = -n_u, d_v = -n_v;  l2 = d_u * d_u + d_v * d_v
 *                   if !(l2 > 0) or l2 is infinite (NaN normals, flat spots):  p' = p
 *                   otherwise  p'_k = p_k + (depth * d_k) / sqrt(l2)  for k = u, v: the multiplication, then a correctly rounded division
 *                   by a correctly rounded square root, then the addition.
 *                 The face-axis component and the normal of p' are copied bitwise from p.  The record normal points to air, so p' lies
 *                 `depth` node cells from p towards the solid side, inside the face's plane.
 *   Records       two 76-byte vtmc_triangle records per quad, (b, a, a') then (b, a', b'), each normal travelling with its position,
 *                 `block` the node's index.  Because cross(p1 - p0, p2 - p0) of a triangle points to air and n points to air, (b, a, a')
 *                 faces out of the node through the face: the side a crack is seen from.  Positions are node-local and map to the world as
 *                 the node's own: terrain_origin + (o + p * 2^L) * voxel_scale.
 *   Offsets       node_offsets[i], i = 0..n_nodes, is the number of skirt records of the nodes before i.
 * The records are the same in both output modes; in indexed mode the vertices are read through the index triples.
 *
 * Life cycle.  The skirts belong to ONE result: any later extract, vtmc_terrain_update / _undo / _redo / _load / _init drops them.  The
 * buffers are library-owned and grow-only.  A call changes nothing else the context holds; the result of vtmc_terrain_extract_lod stays
 * byte for byte what it is.  A refused call keeps the previous skirts.
 *
 * vtmc_lod_skirts              builds the skirts of the level-of-detail result the context holds; *n_triangles (may be NULL) receives the
 *                              number of records.  params->depth is in the node's own cells (a coarse node's skirt is deeper in the world).
 * vtmc_lodskirt_info           nodes, nodes with a flagged face, records; each may be NULL.
 * vtmc_lodskirt_masks          the mask byte of every node.
 * vtmc_lodskirt_read           the records and (when not NULL) the n_nodes + 1 offsets.
 * vtmc_lodskirt_device_results the device pointers of the same (valid until the next vtmc_lod_skirts / destroy); each may be NULL.
 *   VTMC_ERR_NO_RESULT     vtmc_lod_skirts when the context's current result is not a level-of-detail extract's; the four readers when no
 *                          skirts were built for the current result.
 *   VTMC_ERR_INVALID_ARG   (the previous skirts are kept) params null; depth not finite, <= 0 or > VTMC_LODSKIRT_MAX_DEPTH; unknown flag bits.
 *   VTMC_ERR_TOO_LARGE     (the previous skirts are kept) more than 2^31 - 1 skirt records.
 *   VTMC_ERR_CAPACITY      a destination smaller than the records or the nodes.
 */
#ifndef VTMC_LODSKIRT_H
#define VTMC_LODSKIRT_H

#include "vtmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_LODSKIRT_ALL_FACES 1u     /* flags: every face that has a node behind it, not only faces where the level changes */
#define VTMC_LODSKIRT_MAX_DEPTH 8      /* depth above this many node cells: VTMC_ERR_INVALID_ARG */

typedef struct vtmc_lodskirt_params {
    float    depth;        /* in the node's own cells; finite, > 0, <= VTMC_LODSKIRT_MAX_DEPTH */
    uint32_t flags;        /* VTMC_LODSKIRT_ALL_FACES or 0 */
} vtmc_lodskirt_params;    /* 8 bytes */

int32_t vtmc_lod_skirts(vtmc_ctx *ctx, const vtmc_lodskirt_params *params, int64_t *n_triangles);
int32_t vtmc_lodskirt_info(vtmc_ctx *ctx, int32_t *n_nodes, int32_t *n_flagged_nodes, int64_t *n_triangles);
int32_t vtmc_lodskirt_masks(vtmc_ctx *ctx, uint8_t *dst, int32_t capacity_nodes);
int32_t vtmc_lodskirt_read(vtmc_ctx *ctx, vtmc_triangle *dst, int64_t capacity, int32_t *node_offsets /* n_nodes + 1, may be NULL */);
int32_t vtmc_lodskirt_device_results(vtmc_ctx *ctx, const vtmc_triangle **d_triangles, const int32_t **d_node_offsets, int64_t *n_triangles);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_LODSKIRT_H */
