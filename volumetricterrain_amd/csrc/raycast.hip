// raycast.hip -- ray picking against the marching-cubes surface of a density grid (hand-written gfx950 / CDNA4, wave64).
//
// Replaces the Physics.Raycast of the interactive edit (paths relative to /root/reference/Unity-Project/Assets/Scripts/):
//   SceneManager.cs:114-131  Physics.Raycast(cursor ray) -> hit.point -> TerrainEngine.ModifyTerrain
//   VoxelTerrain.cs:448-465  the per-block MeshColliders that query runs against          -> raycast_kernel
// The surface is never materialised: cells along the ray are classified and their triangles rebuilt from the samples with the
// arithmetic of the exact-mode emit (CollectTriNum.compute:41-64 case, MarchingCube.compute:119-151 vertices and winding), so a
// cell's triangles equal the extracted ones bit for bit (the library is built with -ffp-contract=off; `/` is correctly rounded).
//
// One workgroup of kWaves waves per ray.  The ray is clipped to the meshed box [0,nx]x[0,ny]x[0,nz] (grid units) and the clipped
// parameter interval cut into 64 * kWaves equal sub-intervals, one per lane; a lane walks the cells of its sub-interval with a 3-D
// DDA (Amanatides & Woo), kBatch cells at a time: the kBatch * 8 corner loads of a batch are all issued before the first is
// used, so a lane waits about one memory latency per batch instead of one per cell.  After each batch the workgroup agrees
// (one barrier) on the lowest lane that has a hit: lanes after it stop -- their cells lie farther along the ray.  The answer is
// the nearest hit over all lanes (lowest lane on a tie): a wave reduction, then the kWaves wave results through LDS.
//
// Intersection: watertight ray / triangle test (Woop, Benthin & Wald 2013) in float64 on the exact grid-unit vertices 8b + p, so
// two triangles sharing an edge cannot both miss a ray crossing it.  Everything after the vertex positions is float64: the
// ray transform is the same for every triangle, and nothing depends on the grid's layout or on which lane tested a cell.
#include "surface_query.h"

namespace vtmc {

constexpr int kWaves = 4;                 // waves per ray
constexpr int kRayThreads = 64 * kWaves;  // lanes (= sub-intervals) per ray
constexpr int kBatch = 4;                 // cells a lane loads before it evaluates them

struct RaycastArgs {
    SurfaceGrid g;
    const float *ro, *rd;  // n_rays x 3 each
    vtmc_ray_hit *hits;
    int n_rays;
    float max_distance;
    int two_sided;
};

struct Best {
    double t = INFINITY;
    float u = 0.f, v = 0.f, nrm[3] = {0.f, 0.f, 0.f};
    int c[3] = {0, 0, 0};
    int tri = -1;
};

// the triangles of one cell (global cell index c, corner samples s in MarchingCube.compute order) against the ray
__device__ __forceinline__ void intersect_cell(const RaycastArgs &a, const unsigned long long *s_cases, const Ray &r, const float (&s)[8], int cx, int cy,
                                               int cz, Best &best)
{
    const unsigned cs = cell_case(s);
    if (cs == 0u || cs == 255u) return;  // the two cases without triangles (edge mask 0)
    const unsigned long long w = s_cases[cs];
#pragma unroll 1
    for (int i = 0; i < 5; ++i) {
        double P0[3], P1[3], P2[3];
        if (!cell_triangle(w, s, cx, cy, cz, i, P0, P1, P2)) continue;
        const double e1x = P1[0] - P0[0], e1y = P1[1] - P0[1], e1z = P1[2] - P0[2];
        const double e2x = P2[0] - P0[0], e2y = P2[1] - P0[1], e2z = P2[2] - P0[2];
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const double nn = nx * nx + ny * ny + nz * nz;
        if (!(nn > 0.0)) continue;  // zero area, or a NaN sample on the way
        if (!a.two_sided && !(nx * r.d[0] + ny * r.d[1] + nz * r.d[2] < 0.0)) continue;  // single-sided: the face must look at the ray
        double t, V, W, det;
        if (!ray_triangle(r, P0, P1, P2, t, V, W, det)) continue;
        if (!(t >= 0.0) || !((float)t <= a.max_distance) || !(t < best.t)) continue;
        const double inv = 1.0 / sqrt(nn);
        best.t = t;
        best.u = (float)(V / det);
        best.v = (float)(W / det);
        best.nrm[0] = (float)(nx * inv);
        best.nrm[1] = (float)(ny * inv);
        best.nrm[2] = (float)(nz * inv);
        best.c[0] = cx;
        best.c[1] = cy;
        best.c[2] = cz;
        best.tri = i;
    }
}

__global__ __launch_bounds__(kRayThreads) void raycast_kernel(RaycastArgs a)
{
    static_assert(kRayThreads == 256, "one table word per thread");
    __shared__ unsigned long long s_cases[256];  // the case table (DeviceTables::vert_packed), read by the first barrier of the walk
    __shared__ int s_first[kWaves];
    __shared__ double s_t[kWaves];
    __shared__ int s_lane[kWaves];
    const int ray = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SurfaceGrid &g = a.g;
    load_case_table(s_cases, g.vert_packed, tid);
    const float o[3] = {a.ro[3ll * ray], a.ro[3ll * ray + 1], a.ro[3ll * ray + 2]};
    const float d[3] = {a.rd[3ll * ray], a.rd[3ll * ray + 1], a.rd[3ll * ray + 2]};

    Ray r;  // grid units; d = unit world direction / voxel_scale, so the parameter is the world distance
    double dn[3] = {0.0, 0.0, 0.0};
    bool ok = finite3(o) && finite3(d);
    double t_in = 0.0, t_out = -1.0;
    if (ok) {
        const double len = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
        ok = len > 0.0;
        t_out = (double)a.max_distance;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dn[k] = (double)d[k] / len;
            r.o[k] = ((double)o[k] - g.origin[k]) / g.scale;
            r.d[k] = dn[k] / g.scale;
            // slab clip against the meshed box [0, n]: every triangle lies inside it
            if (r.d[k] != 0.0) {
                double t0 = (0.0 - r.o[k]) / r.d[k], t1 = ((double)g.n[k] - r.o[k]) / r.d[k];
                if (t0 > t1) {
                    const double x = t0;
                    t0 = t1;
                    t1 = x;
                }
                t_in = fmax(t_in, t0);
                t_out = fmin(t_out, t1);
            } else if (r.o[k] < 0.0 || r.o[k] > (double)g.n[k]) {
                ok = false;
            }
        }
        ok = ok && t_in <= t_out;
    }
    Best best;
    bool active = ok;
    int c[3] = {0, 0, 0}, step[3] = {0, 0, 0};
    double tmax[3] = {INFINITY, INFINITY, INFINITY}, inv[3] = {0.0, 0.0, 0.0}, tb = 0.0;
    if (ok) {
        ray_setup(r);
        // this lane's sub-interval [ta, tb] and the cell it starts in
        const double span = t_out - t_in;
        const double ta = t_in + span * ((double)tid / kRayThreads);
        tb = tid == kRayThreads - 1 ? t_out : t_in + span * ((double)(tid + 1) / kRayThreads);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = r.o[k] + ta * r.d[k];
            int ci = (int)fmin(fmax(floor(p), 0.0), (double)(g.n[k] - 1));
            c[k] = ci;
            step[k] = r.d[k] > 0.0 ? 1 : (r.d[k] < 0.0 ? -1 : 0);
            if (step[k]) {
                inv[k] = 1.0 / r.d[k];   // the walk multiplies: a float64 division per step costs a dozen instructions
                tmax[k] = ((double)(ci + (step[k] > 0)) - r.o[k]) * inv[k];
            }
        }
    }
    int budget = g.n[0] + g.n[1] + g.n[2] + 3;  // no lane walks more cells than a ray can cross

    const CornerOffsets corner(g);

    while (__syncthreads_or(active)) {
        float s[kBatch][8];
        int cc[kBatch][3];
        bool valid[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            valid[j] = active;
            cc[j][0] = c[0];
            cc[j][1] = c[1];
            cc[j][2] = c[2];
            if (active) {
                load_cell(g, corner, c[0], c[1], c[2], s[j]);
                // next cell: leave through the nearest face; stop past the sub-interval or the box
                const int k = tmax[0] <= tmax[1] ? (tmax[0] <= tmax[2] ? 0 : 2) : (tmax[1] <= tmax[2] ? 1 : 2);
                const double t_exit = fmin(tmax[0], fmin(tmax[1], tmax[2]));
                if (!(t_exit <= tb) || --budget <= 0) {
                    active = false;
                } else {
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk)   // axis by axis: a runtime index into c / tmax would put them in scratch
                        if (kk == k) {
                            c[kk] += step[kk];
                            tmax[kk] = ((double)(c[kk] + (step[kk] > 0)) - r.o[kk]) * inv[kk];
                            if (c[kk] < 0 || c[kk] >= g.n[kk]) active = false;
                        }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
            if (valid[j]) intersect_cell(a, s_cases, r, s[j], cc[j][0], cc[j][1], cc[j][2], best);
        // the lowest lane with a hit: every later lane's cells lie farther along the ray, so those lanes (and it) are done
        const unsigned long long hit = __ballot(best.t < INFINITY);
        if (lane == 0) s_first[wave] = hit ? wave * 64 + __builtin_ctzll(hit) : kRayThreads;
        __syncthreads();
        int first = kRayThreads;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) first = min(first, s_first[w]);
        if (tid >= first) active = false;
    }

    // nearest hit: min over the wave, then over the waves (lowest lane on a tie)
    double m = best.t;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
    const unsigned long long at = __ballot(best.t == m);
    if (lane == 0) {
        s_t[wave] = m;
        s_lane[wave] = wave * 64 + __builtin_ctzll(at);
    }
    __syncthreads();
    double gm = s_t[0];
    int winner = s_lane[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
        if (s_t[w] < gm) {
            gm = s_t[w];
            winner = s_lane[w];
        }
    if (!(gm < INFINITY)) winner = 0;
    if (tid != winner) return;
    vtmc_ray_hit h;
    if (best.t < INFINITY) {
        h.distance = (float)best.t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h.point[k] = (float)((double)o[k] + best.t * dn[k]);
            h.normal[k] = best.nrm[k];
            h.block[k] = best.c[k] >> 3;
        }
        h.barycentric[0] = best.u;
        h.barycentric[1] = best.v;
        h.cell = (best.c[0] & 7) + 8 * (best.c[1] & 7) + 64 * (best.c[2] & 7);
        h.triangle = best.tri;
    } else {
        h.distance = -1.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h.point[k] = 0.f;
            h.normal[k] = 0.f;
            h.block[k] = -1;
        }
        h.barycentric[0] = h.barycentric[1] = 0.f;
        h.cell = -1;
        h.triangle = -1;
    }
    a.hits[ray] = h;
}

static hipError_t launch_raycast(const RaycastArgs &a, hipStream_t stream)
{
    return launch(raycast_kernel, dim3((unsigned)a.n_rays), dim3(kRayThreads), 0, stream, a);
}

static int check_rays(vtmc_ctx *ctx, int32_t n_rays, bool null_arg, float max_distance, uint32_t flags)
{
    if (int rc = check_batch(ctx, n_rays, "n_rays", null_arg)) return rc;
    if (int rc = check_max_distance(ctx, max_distance)) return rc;
    if (flags & ~VTMC_RAY_TWO_SIDED) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown ray flags 0x%x", flags);
    return VTMC_OK;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_raycast_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x, int64_t stride_y,
                            int64_t stride_z, const float origin[3], float voxel_scale, const float *d_origins, const float *d_directions,
                            int32_t n_rays, float max_distance, uint32_t flags, vtmc_ray_hit *d_hits, void *stream)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = check_rays(ctx, n_rays, !d_grid || !origin || !d_origins || !d_directions || !d_hits, max_distance, flags)) return rc;
    if (n_rays == 0) return check_dims(ctx, nx, ny, nz);
    RaycastArgs a{{}, d_origins, d_directions, d_hits, n_rays, max_distance, (flags & VTMC_RAY_TWO_SIDED) ? 1 : 0};
    if (int rc = surface_of_grid(ctx, d_grid, nx, ny, nz, stride_x, stride_y, stride_z, origin, voxel_scale, &a.g)) return rc;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, launch_raycast(a, stream ? (hipStream_t)stream : ctx->stream));
    return VTMC_OK;
}

int32_t vtmc_terrain_raycast(vtmc_ctx *ctx, const float *origins, const float *directions, int32_t n_rays, float max_distance, uint32_t flags,
                             vtmc_ray_hit *hits)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = check_rays(ctx, n_rays, !origins || !directions || !hits, max_distance, flags)) return rc;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_raycast before terrain_init");
    if (n_rays == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ray_bytes = sizeof(float) * 3 * (size_t)n_rays;
    const float *const src[3] = {origins, directions, nullptr};
    const size_t bytes[3] = {ray_bytes, ray_bytes, 0};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, sizeof(vtmc_ray_hit) * (size_t)n_rays, &st)) return rc;
    const RaycastArgs a{surface_of_terrain(ctx), st.in[0], st.in[1], (vtmc_ray_hit *)st.hits, n_rays, max_distance, (flags & VTMC_RAY_TWO_SIDED) ? 1 : 0};
    VTMC_HIP(ctx, launch_raycast(a, ctx->stream));
    return fetch_hits(ctx, st, hits);
}

}  // extern "C"
