// stamp_mesh.hip -- mesh stamps (vtmc_stamp_from_mesh; not in the reference, whose modifiers are analytic): a closed triangle mesh
// voxelized on the device into an ordinary stamp, a signed distance in stamp samples clamped to +-VTMC_MESH_BAND.  The rule, operation
// by operation, is in include/vtmc.h; the kernel follows it bit for bit (library built with -ffp-contract=off): the FP32 distance to
// the nearest triangle (closest_on_triangle, mc_cell.h: the routine of the sphere queries, here in float) and the even-odd parity of a
// ray towards +x, in double.
//
// The work is samples x triangles, so a workgroup prunes before it evaluates, as terrain_path_kernel does.  It owns a tile of the
// shared box walk (terrain_box.h: 64 x kYRun x 4 samples of the stamp, long along the parity ray's axis and thin across it, so few
// triangles project onto a tile) and takes the triangles in chunks of kMeshChunk, one per thread.  A chunk whose bounds miss the tile
// is skipped whole; otherwise each thread tests one triangle, the survivors are compacted into LDS in index order (wave ballot, prefix
// over the four waves) with a flag for each part they survived, and every thread evaluates that list for the kYRun samples of its
// run: the running minima and the parity bits stay in registers, all lanes read the same LDS record at a time (a broadcast, no bank
// conflict), and the part flags are uniform over the workgroup.  The distance part is about 70 FP32 operations per (sample, surviving
// triangle); the parity part works in FP64 only on the edges that straddle the wave's z and the samples a triangle covers.
//
// Pruning is exact, not approximate: both tests are implied by the rule itself, so the stamp is the one that evaluating every triangle
// at every sample gives.
//  - distance: the rule lets a triangle bid for a sample's minimum only inside its reach box, its AABB grown by g = 3h + slack (FP32, on
//    the host).  A sample position is (float)i * h + first, monotonic in i, so the positions of a tile's first and last sample bound every
//    sample of it exactly; a tile whose AABB lies outside the reach box on some axis holds no sample inside it, and the triangle bids
//    for none.  (The reach box costs the rule nothing: outside it a closest point found to within slack is farther than 3h, and the
//    band hides it.  It is in the rule so that no rounding of a sliver's closest point can make pruning visible.)
//  - parity: a triangle counts for a sample only when zmin <= pz < zmax (an edge straddles), ymin <= py <= ymax and px < xmax -- float
//    comparisons of the rule.  A tile with thi.z < zmin, tlo.z >= zmax, thi.y < ymin, tlo.y > ymax or tlo.x >= xmax holds no such sample.
#include "terrain_box.h"
#include "terrain_stamp.h"
#include "mc_cell.h"
#include "mesh_host.h"

namespace vtmc {

struct StampMeshArgs {
    const float4 *vert, *edge, *bound, *chunk;  // MeshRecords (mesh_host.h)
    const double *normal;
    int n_tri;
    float grow;          // g
    float first[3], h;
    int dx, dy, dz;      // the stamp's dims: the box walk's box, first sample 0
};

enum { kMeshDist = 1, kMeshParity = 2 };

// the part flags of a box [lo, hi] against the tile [tlo, thi]: kMeshDist unless the tile lies outside the reach box, kMeshParity unless no
// sample of the tile can be covered and in front
__device__ __forceinline__ int mesh_parts(const float4 &lo, const float4 &hi, float g, const float tlo[3], const float thi[3])
{
    const bool far = thi[0] < lo.x - g || tlo[0] > hi.x + g || thi[1] < lo.y - g || tlo[1] > hi.y + g || thi[2] < lo.z - g || tlo[2] > hi.z + g;
    const bool off = thi[1] < lo.y || tlo[1] > hi.y || thi[2] < lo.z || tlo[2] >= hi.z || tlo[0] >= hi.x;
    return (far ? 0 : kMeshDist) | (off ? 0 : kMeshParity);
}

// A thread outside the stamp (the tile's x / z tail) takes part in the pruning and evaluates nothing; a run's tail past the stamp along y
// is evaluated and never stored, as in terrain_path_kernel.
__global__ __launch_bounds__(256) void stamp_mesh_kernel(float *__restrict__ out, StampMeshArgs m)
{
    __shared__ float4 s_v[3][kMeshChunk], s_e[3][kMeshChunk], s_lo[kMeshChunk], s_hi[kMeshChunk];  // the surviving triangles, in index order
    __shared__ double s_n[3][kMeshChunk];
    __shared__ int s_parts[kMeshChunk];
    __shared__ int s_cnt[4];  // survivors per wave
    const BoxThread t;
    const bool live = t.inside(m);
    const int lane = threadIdx.x, wave = threadIdx.y;  // 64 x 4 threads: a wave is a row of the workgroup
    const int first[3] = {(int)blockIdx.x * 64, (int)blockIdx.z * kYRun, (int)blockIdx.y * 4};
    const int last[3] = {min(first[0] + 63, m.dx - 1), min(first[1] + kYRun - 1, m.dy - 1), min(first[2] + 3, m.dz - 1)};
    float tlo[3], thi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tlo[k] = (float)first[k] * m.h + m.first[k];
        thi[k] = (float)last[k] * m.h + m.first[k];
    }
    const float g = m.grow;
    const float px = (float)t.ix * m.h + m.first[0];
    const float pz = (float)t.iz * m.h + m.first[2];
    float py[kYRun], dmin[kYRun];
#pragma unroll
    for (int k = 0; k < kYRun; ++k) {
        py[k] = (float)(t.iy0 + k) * m.h + m.first[1];
        dmin[k] = INFINITY;
    }
    unsigned inside = 0;  // bit k: an odd number of triangles so far cover sample k of the run and lie in front of it
    for (int c0 = 0; c0 < m.n_tri; c0 += kMeshChunk) {
        const float4 *cb = m.chunk + 2 * (c0 / kMeshChunk);
        if (!mesh_parts(cb[0], cb[1], g, tlo, thi)) continue;  // uniform over the workgroup, as the barriers below need
        const int i = c0 + wave * 64 + lane;
        int parts = 0;
        float4 lo, hi;
        if (i < m.n_tri) {
            lo = m.bound[2 * i], hi = m.bound[2 * i + 1];
            parts = mesh_parts(lo, hi, g, tlo, thi);
        }
        const unsigned long long mask = __ballot(parts != 0);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();  // also: every wave has left the previous chunk's list
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = s_cnt[w];
            if (w < wave) base += c;
            total += c;
        }
        if (parts) {
            const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_v[k][at] = m.vert[3 * i + k];
                s_e[k][at] = m.edge[3 * i + k];
                s_n[k][at] = m.normal[3 * (size_t)i + k];
            }
            s_lo[at] = lo;
            s_hi[at] = hi;
            s_parts[at] = parts;
        }
        __syncthreads();
        if (!live) continue;
        const int n_live = __builtin_amdgcn_readfirstlane(total);
        for (int j = 0; j < n_live; ++j) {
            const int pj = __builtin_amdgcn_readfirstlane(s_parts[j]);
            const float4 v0 = s_v[0][j], blo = s_lo[j], bhi = s_hi[j];
            if (pj & kMeshDist) {
                const float glx = blo.x - g, ghx = bhi.x + g, gly = blo.y - g, ghy = bhi.y + g, glz = blo.z - g, ghz = bhi.z + g;
                if (px >= glx && px <= ghx && pz >= glz && pz <= ghz) {
                    const float4 v1 = s_v[1][j], v2 = s_v[2][j];
                    const float a[3] = {v0.x, v0.y, v0.z}, b[3] = {v1.x, v1.y, v1.z}, c[3] = {v2.x, v2.y, v2.z};
#pragma unroll
                    for (int k = 0; k < kYRun; ++k) {
                        if (!(py[k] >= gly && py[k] <= ghy)) continue;
                        const float p[3] = {px, py[k], pz};
                        float q[3];
                        closest_on_triangle(p, a, b, c, q);
                        const float cx = px - q[0], cy = py[k] - q[1], cz = pz - q[2];
                        const float d = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
                        if (d < dmin[k]) dmin[k] = d;  // false for a NaN (a triangle without area): it bids nothing
                    }
                }
            }
            if ((pj & kMeshParity) && px < bhi.x) {
                // bit k of `count`: an odd number of the edges seen so far straddle pz and lie on the +y side of sample k
                unsigned count = 0;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const float4 ed = s_e[e][j];  // (lo.y, lo.z, hi.y, hi.z)
                    if (!(ed.y <= pz && pz < ed.w)) continue;
                    const double ey = (double)ed.z - (double)ed.x, ez = (double)ed.w - (double)ed.y;
                    const double az = ey * ((double)pz - (double)ed.y);
#pragma unroll
                    for (int k = 0; k < kYRun; ++k) {
                        const double det = az - ((double)py[k] - (double)ed.x) * ez;
                        if (det > 0.0) count ^= 1u << k;
                    }
                }
#pragma unroll
                for (int k = 0; k < kYRun; ++k)
                    if (!(py[k] >= blo.y && py[k] <= bhi.y)) count &= ~(1u << k);
                if (count) {
                    if (px < blo.x) {
                        inside ^= count;
                    } else {
                        const double nx = s_n[0][j], ny = s_n[1][j], nz = s_n[2][j];
                        const double tx = nx * ((double)px - (double)v0.x), tz = nz * ((double)pz - (double)v0.z);
#pragma unroll
                        for (int k = 0; k < kYRun; ++k) {
                            const double tt = (tx + ny * ((double)py[k] - (double)v0.y)) + tz;
                            const bool front = (tt < 0.0 && nx > 0.0) || (tt > 0.0 && nx < 0.0);
                            if (front) inside ^= count & (1u << k);
                        }
                    }
                }
            }
        }
    }
    if (!live) return;
    const int iy1 = t.iy1(m);
    const uint64_t j0 = box_index(m, t.ix, t.iy0, t.iz);  // sample k of the run: k rows further
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) {
            const float r = dmin[k] / m.h;
            const float s = r < VTMC_MESH_BAND ? r : VTMC_MESH_BAND;
            out[j0 + (uint64_t)m.dx * k] = (inside >> k) & 1u ? s : -s;
        }
}

}  // namespace vtmc

using namespace vtmc;

extern "C" int32_t vtmc_stamp_from_mesh(vtmc_ctx *ctx, const float *positions, int32_t n_vertices, const int32_t *indices, int32_t n_triangles,
                                        const float first[3], float h, int32_t nx, int32_t ny, int32_t nz, uint32_t flags, int32_t *stamp_id)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!positions || !indices || !first || !stamp_id) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: positions, indices, first or stamp_id is null");
    if (flags & ~VTMC_MESH_TRUST_CLOSED) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: unknown flags 0x%x", flags);
    if (n_triangles < 1 || n_triangles > VTMC_MESH_MAX_TRIANGLES)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: triangle count %d not in 1..%d", n_triangles, VTMC_MESH_MAX_TRIANGLES);
    if (n_vertices < 3) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: vertex count %d below 3", n_vertices);
    if (int rc = check_stamp_dims(ctx, nx, ny, nz)) return rc;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(first[k])) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: first[%d] not finite", k);
    if (!std::isfinite(h) || !(h > 0.0f)) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: pitch %g not finite and > 0", h);
    for (size_t i = 0; i < (size_t)3 * n_triangles; ++i)
        if (indices[i] < 0 || indices[i] >= n_vertices)
            return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: triangle %zu: index %d outside the %d vertices", i / 3, indices[i], n_vertices);
    for (size_t i = 0; i < (size_t)3 * n_vertices; ++i) {
        if (!std::isfinite(positions[i])) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: vertex %zu: coordinate %zu not finite", i / 3, i % 3);
        if (std::fabs(positions[i]) > 1048576.0f)
            return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: vertex %zu: coordinate %zu is %g, above 2^20 in magnitude", i / 3, i % 3, positions[i]);
    }
    if (!(flags & VTMC_MESH_TRUST_CLOSED)) {
        int32_t edge[2], uses = 0;
        if (!mesh_closed(indices, n_triangles, edge, &uses))
            return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_from_mesh: the mesh is not closed: edge (%d, %d) is used by %d triangles, not 2", edge[0], edge[1], uses);
    }
    if (ctx->next_stamp_id == INT32_MAX) return fail(ctx, VTMC_ERR_TOO_LARGE, "stamp ids exhausted");
    const int32_t dims[3] = {nx, ny, nz};
    const MeshRecords rec = mesh_records(positions, indices, n_triangles, first, h, dims);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VtmcDevBuf d_f, d_n;  // the records live for this call only
    if (int rc = ensure(ctx, d_f, rec.f.size() * sizeof(float))) return rc;
    if (int rc = ensure(ctx, d_n, rec.n.size() * sizeof(double))) return rc;
    VtmcStamp st;
    if (int rc = new_stamp(ctx, nx, ny, nz, st)) return rc;
    VTMC_HIP(ctx, hipMemcpy(d_f.p, rec.f.data(), rec.f.size() * sizeof(float), hipMemcpyHostToDevice));
    VTMC_HIP(ctx, hipMemcpy(d_n.p, rec.n.data(), rec.n.size() * sizeof(double), hipMemcpyHostToDevice));
    StampMeshArgs a{};
    a.vert = (const float4 *)((const float *)d_f.p + rec.vert_at());
    a.edge = (const float4 *)((const float *)d_f.p + rec.edge_at());
    a.bound = (const float4 *)((const float *)d_f.p + rec.bound_at());
    a.chunk = (const float4 *)((const float *)d_f.p + rec.chunk_at());
    a.normal = (const double *)d_n.p;
    a.n_tri = n_triangles;
    a.grow = rec.grow;
    for (int k = 0; k < 3; ++k) a.first[k] = first[k];
    a.h = h;
    a.dx = nx, a.dy = ny, a.dz = nz;
    VTMC_HIP(ctx, launch_box(stamp_mesh_kernel, TerrainBox{0, 0, 0, nx, ny, nz}, ctx->stream, (float *)st.samples.p, a));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the records are freed on return
    *stamp_id = keep_stamp(ctx, st);
    return VTMC_OK;
}
