// spherequery.hip -- sphere casts and closest-point queries against the marching-cubes surface of a density grid (hand-written gfx950 /
// CDNA4, wave64).
//
// Replaces the queries a moving body makes against the per-block MeshColliders (VoxelTerrain.cs:168, 464 of the reference's Unity
// scripts cook them from the read-back mesh): Physics.SphereCast -> spherecast, and Physics.CheckSphere /
// Collider.ClosestPoint / Physics.ComputePenetration -> closest point.  The surface is the raycast's (raycast.hip): a cell's triangles
// are rebuilt from its samples by mc_cell.h, so they equal the extracted ones bit for bit.
//
// One workgroup of kSqWaves waves per query.  Broad phase: the sweep [0, max_distance] is clipped to the meshed box grown by the radius
// and cut into pieces of kPiece cells along its length.  For a piece, the lanes take the cells of its box grown by r, drop those whose
// centre lies farther than r + sqrt(3)/2 from the piece's segment (no point of such a cell is within r of it), and test the triangles
// of the rest, kBatch cells per lane at a time with all their corner loads issued before the first is used.  After each piece the
// workgroup agrees on the best (t, canonical index) so far; once that t lies inside the pieces already done it is final, because a
// contact at t involves a cell within r of the segment point at t.  A closest-point query is one such piece of zero length.
//
// Narrow phase in float64 on the exact grid-unit vertices 8b + p.  Sphere cast (Ericson, Real-Time Collision Detection §5.5): a
// triangle within r of the start answers 0; else the earliest of the face-plane contact (when its point lies in the triangle), the
// three edge cylinders and the three vertex spheres.  r = 0 is the raycast's watertight test.  Closest point: Ericson §5.1.5.  Ties in
// t or distance go to the smallest canonical index (block bx + nbx (by + nby bz), cell x + 8y + 64z, triangle i), so the answer
// depends neither on the grid's strides nor on the launch shape nor on which lane tested a cell.
#include "surface_query.h"

namespace vtmc {

constexpr int kSqWaves = 4;                   // waves per query
constexpr int kSqThreads = 64 * kSqWaves;     // lanes per query
constexpr int kSqBatch = 4;                   // cells a lane loads before it evaluates them
constexpr double kPiece = 8.0;                // sweep length per piece, cells
constexpr double kPad = 1e-3;                 // cells: slack on every conservative bound of the broad phase
constexpr unsigned long long kNoKey = ~0ull;  // the key of "no triangle"

struct SphereArgs {
    SurfaceGrid g;
    // hits before the inputs: in this order the compiler groups the argument loads so that the kernels are one s_waitcnt shorter than with
    // the case table last, and the walk's loops lie 4 bytes from where they did then; with the inputs first they lie 20 bytes off, which
    // cost the 1024-cell sweep that meets no surface 1.1 % (profiles/r10/edit_refactor/README.md)
    vtmc_sphere_hit *hits;
    const float *qo, *qd, *qr;  // per query: origin / centre (x3), direction (x3, casts only), radius
    int n_q;
    float max_distance;  // casts only
    float max_radius;    // VTMC_SPHERE_MAX_RADIUS_CELLS * voxel_scale
    int two_sided;
};

__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void sub3(const double *a, const double *b, double *c)
{
    c[0] = a[0] - b[0];
    c[1] = a[1] - b[1];
    c[2] = a[2] - b[2];
}

// closest_on_triangle (Ericson §5.1.5) is mc_cell.h's: the mesh voxelizer (stamp_mesh.hip) evaluates the same routine in FP32

// the first s >= 0 at which the point o + s u (u unit) comes within R of the line point set {a + k (b - a), k in [0, 1]}'s cylinder
// part (the end caps are the vertex spheres); INFINITY when it never does or starts inside the infinite cylinder
__device__ __forceinline__ double sweep_edge(const double *o, const double *u, const double *a, const double *b, double R)
{
    double d[3], m[3];
    sub3(b, a, d);
    sub3(o, a, m);
    const double dd = dot3(d, d), md = dot3(m, d), ud = dot3(u, d);
    const double A = dd - ud * ud, B = dd * dot3(m, u) - md * ud, C = dd * (dot3(m, m) - R * R) - md * md;
    if (!(A > 0.0) || !(C > 0.0) || !(B < 0.0)) return INFINITY;
    const double disc = B * B - A * C;
    if (!(disc >= 0.0)) return INFINITY;
    const double s = C / (-B + sqrt(disc));  // the smaller root, without cancellation
    const double k = md + s * ud;
    return k >= 0.0 && k <= dd ? s : INFINITY;
}

// the first s >= 0 at which o + s u (u unit) comes within R of point v; INFINITY when it never does or starts within R
__device__ __forceinline__ double sweep_vertex(const double *o, const double *u, const double *v, double R)
{
    double m[3];
    sub3(o, v, m);
    const double b = dot3(m, u), c = dot3(m, m) - R * R;
    if (!(c > 0.0) || !(b < 0.0)) return INFINITY;
    const double disc = b * b - c;
    if (!(disc >= 0.0)) return INFINITY;
    return c / (-b + sqrt(disc));
}

// Sphere cast of radius R > 0 from o along unit u against the triangle (P[0], P[1], P[2]) with normal n = cross(e1, e2), |n|^2 = nn:
// the first s >= 0 of contact, or INFINITY.  Grid units throughout.
__device__ __forceinline__ double sweep_triangle(const double *o, const double *u, const double (&P)[3][3], const double *n, double nn, double R)
{
    double q[3], oq[3];
    closest_on_triangle(o, P[0], P[1], P[2], q);
    sub3(o, q, oq);
    if (dot3(oq, oq) <= R * R) return 0.0;  // the ball already touches it
    const double inv = 1.0 / sqrt(nn);
    const double nh[3] = {n[0] * inv, n[1] * inv, n[2] * inv};
    double op[3];
    sub3(o, P[0], op);
    const double dist0 = dot3(nh, op), vn = dot3(nh, u);
    // face: the plane contact, when the sphere starts clear of the plane and moves towards it; if its point lies in the triangle,
    // nothing of the triangle is touched earlier
    if ((dist0 > R && vn < 0.0) || (dist0 < -R && vn > 0.0)) {
        const double side = dist0 > 0.0 ? 1.0 : -1.0;
        const double s = (dist0 - side * R) / -vn;
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = o[k] + s * u[k] - side * R * nh[k];
        bool in = true;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const double *a = P[e], *b = P[e == 2 ? 0 : e + 1];
            double ab[3], ac[3], x[3];
            sub3(b, a, ab);
            sub3(c, a, ac);
            cross3(ab, ac, x);
            in = in && dot3(x, n) >= 0.0;
        }
        if (in) return s;
    }
    double s = INFINITY;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        s = fmin(s, sweep_edge(o, u, P[e], P[e == 2 ? 0 : e + 1], R));
        s = fmin(s, sweep_vertex(o, u, P[e], R));
    }
    return s;
}

struct Query {
    double o[3];   // start / centre, grid units
    double u[3];   // unit direction (casts)
    double R;      // radius, grid units
    Ray ray;       // r = 0 casts: the raycast's ray, parameter in world units
};

// (key, t) ordering: smaller t, then the smaller canonical index
__device__ __forceinline__ bool better(double t, unsigned long long key, double bt, unsigned long long bkey)
{
    return t < bt || (t == bt && key < bkey);
}

// the triangles of one cell (global cell c, corner samples s) against the query; keeps the best (t, key).  t: the world distance of a
// cast, the squared grid-unit distance of a closest-point query
template <bool Cast>
__device__ __forceinline__ void query_cell(const SphereArgs &a, const unsigned long long *s_cases, const Query &q, const float (&s)[8], int cx,
                                           int cy, int cz, double &bt, unsigned long long &bkey)
{
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) nan = nan || s[k] != s[k];
    const unsigned cs = cell_case(s);
    if (nan || cs == 0u || cs == 255u) return;
    const unsigned long long w = s_cases[cs];
    const int nbx = a.g.n[0] >> 3, nby = a.g.n[1] >> 3;
    const unsigned long long cell_key =
        ((unsigned long long)((cx >> 3) + nbx * ((cy >> 3) + (long long)nby * (cz >> 3))) * 512ull + (unsigned)((cx & 7) + 8 * (cy & 7) + 64 * (cz & 7))) * 5ull;
#pragma unroll 1
    for (int i = 0; i < 5; ++i) {
        double P[3][3];
        if (!cell_triangle(w, s, cx, cy, cz, i, P[0], P[1], P[2])) continue;
        double e1[3], e2[3], n[3];
        sub3(P[1], P[0], e1);
        sub3(P[2], P[0], e2);
        cross3(e1, e2, n);
        const double nn = dot3(n, n);
        if (!(nn > 0.0)) continue;  // zero area
        double t;
        if (Cast) {
            if (!a.two_sided && !(dot3(n, q.u) < 0.0)) continue;  // single-sided: the face must look at the sweep
            if (q.R > 0.0) {
                t = sweep_triangle(q.o, q.u, P, n, nn, q.R) * a.g.scale;
            } else {
                double V, W, det;
                if (!ray_triangle(q.ray, P[0], P[1], P[2], t, V, W, det)) continue;
            }
            if (!(t >= 0.0 && t < INFINITY) || !((float)t <= a.max_distance)) continue;  // no contact is INFINITY; max_distance may be too
        } else {
            double c[3], d[3];
            closest_on_triangle(q.o, P[0], P[1], P[2], c);
            sub3(q.o, c, d);
            t = dot3(d, d);
            if (!(t <= q.R * q.R)) continue;
        }
        const unsigned long long key = cell_key + (unsigned)i;
        if (better(t, key, bt, bkey)) {
            bt = t;
            bkey = key;
        }
    }
}

// the workgroup's best (t, key): every thread gets it
__device__ __forceinline__ void reduce_best(double &bt, unsigned long long &bkey, double *s_t, unsigned long long *s_key, int wave, int lane)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double t = __shfl_xor(bt, off);
        const unsigned long long k = __shfl_xor(bkey, off);
        if (better(t, k, bt, bkey)) {
            bt = t;
            bkey = k;
        }
    }
    __syncthreads();  // the previous reduction's readers are done with s_t / s_key
    if (lane == 0) {
        s_t[wave] = bt;
        s_key[wave] = bkey;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kSqWaves; ++w)
        if (better(s_t[w], s_key[w], bt, bkey)) {
            bt = s_t[w];
            bkey = s_key[w];
        }
}

template <bool Cast>
__global__ __launch_bounds__(kSqThreads) void sphere_query_kernel(SphereArgs a)
{
    static_assert(kSqThreads == 256, "one table word per thread");
    __shared__ unsigned long long s_cases[256];
    __shared__ double s_t[kSqWaves];
    __shared__ unsigned long long s_key[kSqWaves];
    const int qi = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    load_case_table(s_cases, a.g.vert_packed, tid);
    const float o[3] = {a.qo[3ll * qi], a.qo[3ll * qi + 1], a.qo[3ll * qi + 2]};
    float d[3] = {0.f, 0.f, 0.f};
    if (Cast) {
        d[0] = a.qd[3ll * qi];
        d[1] = a.qd[3ll * qi + 1];
        d[2] = a.qd[3ll * qi + 2];
    }
    const float rad = a.qr[qi];

    Query q;
    double dn[3] = {0.0, 0.0, 0.0};
    // a radius outside the rule (only a device call can get here with one) and a non-finite start are misses
    bool ok = finite3(o) && rad >= 0.f && rad <= a.max_radius;
    double s_in = 0.0, s_out = 0.0;  // the sweep in grid units along u
    if (ok) {
        q.R = (double)rad / a.g.scale;
        double len = 1.0;
        if (Cast) {
            ok = finite3(d);
            len = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
            ok = ok && len > 0.0;
            s_out = (double)a.max_distance / a.g.scale * (1.0 + 1e-9) + kPad;   // (float)t <= max_distance decides exactly
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            q.o[k] = ((double)o[k] - a.g.origin[k]) / a.g.scale;
            dn[k] = Cast ? (double)d[k] / len : 0.0;
            q.u[k] = dn[k];
            q.ray.o[k] = q.o[k];
            q.ray.d[k] = dn[k] / a.g.scale;
            if (!Cast) continue;
            // slab clip against the meshed box [0, n] grown by R: no triangle is within R of a centre outside it
            const double lo = -q.R - kPad, hi = (double)a.g.n[k] + q.R + kPad;
            if (q.u[k] != 0.0) {
                double t0 = (lo - q.o[k]) / q.u[k], t1 = (hi - q.o[k]) / q.u[k];
                if (t0 > t1) {
                    const double x = t0;
                    t0 = t1;
                    t1 = x;
                }
                s_in = fmax(s_in, t0);
                s_out = fmin(s_out, t1);
            } else if (q.o[k] < lo || q.o[k] > hi) {
                ok = false;
            }
        }
        ok = ok && s_in <= s_out;
        if (Cast && ok && q.R == 0.0) ray_setup(q.ray);
    }

    double bt = INFINITY;
    unsigned long long bkey = kNoKey;
    const CornerOffsets corner(a.g);
    const double reach = q.R + 0.8660254037844387 + kPad;  // a cell centre this far from the segment: no point of the cell is within R
    double sa = s_in;
    __syncthreads();  // s_cases
    while (ok) {  // uniform across the workgroup
        const double sb = Cast ? fmin(sa + kPiece, s_out) : sa;
        double A[3], Bv[3];
        int lo[3], ext[3];
        long long count = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            A[k] = q.o[k] + sa * q.u[k];
            Bv[k] = q.o[k] + sb * q.u[k];
            const double l = fmin(A[k], Bv[k]) - q.R - kPad, h = fmax(A[k], Bv[k]) + q.R + kPad;
            lo[k] = (int)fmin(fmax(floor(l), 0.0), (double)a.g.n[k]);           // clamped before the conversion: a far centre is
            const int hi = (int)fmax(fmin(floor(h), (double)(a.g.n[k] - 1)), -1.0);  // finite but may not fit an int
            ext[k] = hi >= lo[k] ? hi - lo[k] + 1 : 0;
            count *= ext[k];
        }
        double seg[3];
        sub3(Bv, A, seg);
        const double seg2 = dot3(seg, seg);
        for (long long base = tid; base < count; base += (long long)kSqThreads * kSqBatch) {
            float s[kSqBatch][8];
            int cc[kSqBatch][3];
            bool valid[kSqBatch];
#pragma unroll
            for (int j = 0; j < kSqBatch; ++j) {
                const long long idx = base + (long long)j * kSqThreads;
                valid[j] = idx < count;
                if (!valid[j]) continue;
                const long long yz = idx / ext[0];
                cc[j][0] = lo[0] + (int)(idx - yz * ext[0]);
                cc[j][1] = lo[1] + (int)(yz % ext[1]);
                cc[j][2] = lo[2] + (int)(yz / ext[1]);
                // the cell's centre against the piece's segment
                double m[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = (double)cc[j][k] + 0.5 - A[k];
                double f = seg2 > 0.0 ? dot3(m, seg) / seg2 : 0.0;
                f = fmin(fmax(f, 0.0), 1.0);
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] -= f * seg[k];
                valid[j] = dot3(m, m) <= reach * reach;
                if (!valid[j]) continue;
                load_cell(a.g, corner, cc[j][0], cc[j][1], cc[j][2], s[j]);
            }
#pragma unroll
            for (int j = 0; j < kSqBatch; ++j)
                if (valid[j]) query_cell<Cast>(a, s_cases, q, s[j], cc[j][0], cc[j][1], cc[j][2], bt, bkey);
        }
        reduce_best(bt, bkey, s_t, s_key, wave, lane);
        // a contact at t <= sb involves a cell within R of the segment up to sb: all of those have been tested
        if (!Cast || bt <= sb * a.g.scale || sb >= s_out) break;
        sa = sb;
    }
    if (tid != 0) return;

    vtmc_sphere_hit h;
    h.distance = -1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        h.point[k] = 0.f;
        h.normal[k] = 0.f;
        h.block[k] = -1;
    }
    h.cell = -1;
    h.triangle = -1;
    if (ok && bkey != kNoKey) {
        // rebuild the winning triangle from its canonical index
        const int nbx = a.g.n[0] >> 3, nby = a.g.n[1] >> 3;
        const int tri = (int)(bkey % 5ull), cell = (int)((bkey / 5ull) % 512ull);
        const long long blk = (long long)(bkey / 2560ull);
        const int bx = (int)(blk % nbx), by = (int)((blk / nbx) % nby), bz = (int)(blk / ((long long)nbx * nby));
        const int cx = 8 * bx + (cell & 7), cy = 8 * by + ((cell >> 3) & 7), cz = 8 * bz + (cell >> 6);
        float s[8];
        load_cell(a.g, corner, cx, cy, cz, s);
        double P[3][3];
        cell_triangle(s_cases[cell_case(s)], s, cx, cy, cz, tri, P[0], P[1], P[2]);
        double e1[3], e2[3], n[3], c[3], p[3], cp[3];
        sub3(P[1], P[0], e1);
        sub3(P[2], P[0], e2);
        cross3(e1, e2, n);
        const double s_hit = Cast ? bt / a.g.scale : 0.0;  // grid units along u
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = q.o[k] + s_hit * q.u[k];
        closest_on_triangle(c, P[0], P[1], P[2], p);
        sub3(c, p, cp);
        const double dist = sqrt(dot3(cp, cp));
        const double inv = (Cast && q.R == 0.0) || !(dist > 0.0) ? 1.0 / sqrt(dot3(n, n)) : 1.0 / dist;
        const double *nv = (Cast && q.R == 0.0) || !(dist > 0.0) ? n : cp;
        h.distance = Cast ? (float)bt : (float)(dist * a.g.scale);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h.point[k] = (float)(a.g.origin[k] + p[k] * a.g.scale);
            h.normal[k] = (float)(nv[k] * inv);
        }
        h.block[0] = bx, h.block[1] = by, h.block[2] = bz;
        h.cell = cell;
        h.triangle = tri;
    }
    a.hits[qi] = h;
}

template <bool Cast>
static hipError_t launch_sphere_query(const SphereArgs &a, hipStream_t stream)
{
    return launch(sphere_query_kernel<Cast>, dim3((unsigned)a.n_q), dim3(kSqThreads), 0, stream, a);
}

// the argument rules the four entry points share (max_distance: casts only)
static int check_queries(vtmc_ctx *ctx, int32_t n, bool null_arg, bool cast, float max_distance, uint32_t flags)
{
    if (int rc = check_batch(ctx, n, "n", null_arg)) return rc;
    if (cast)
        if (int rc = check_max_distance(ctx, max_distance)) return rc;
    if (cast && (flags & ~VTMC_RAY_TWO_SIDED)) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown sphere cast flags 0x%x", flags);
    if (!cast && flags) return fail(ctx, VTMC_ERR_INVALID_ARG, "closest-point flags are reserved and must be 0 (got 0x%x)", flags);
    return VTMC_OK;
}

static float max_radius(float scale) { return (float)VTMC_SPHERE_MAX_RADIUS_CELLS * scale; }

// host radii: NaN, infinite, negative or above the limit is an error that names the query
static int check_radii(vtmc_ctx *ctx, const float *radii, int32_t n, float scale)
{
    const float lim = max_radius(scale);
    for (int32_t i = 0; i < n; ++i)
        if (!(radii[i] >= 0.0f && radii[i] <= lim))
            return fail(ctx, VTMC_ERR_INVALID_ARG, "query %d: radius %g is not in [0, %d * voxel_scale = %g]", i, (double)radii[i],
                        VTMC_SPHERE_MAX_RADIUS_CELLS, (double)lim);
    return VTMC_OK;
}

// the arguments of a batch but for its surface
static SphereArgs sphere_args(const float *o, const float *d, const float *r, vtmc_sphere_hit *hits, int32_t n, float scale, float max_distance, uint32_t flags)
{
    return SphereArgs{{}, hits, o, d, r, n, max_distance, max_radius(scale), (flags & VTMC_RAY_TWO_SIDED) ? 1 : 0};
}

static int device_query(vtmc_ctx *ctx, bool cast, const float *d_grid, int32_t nx, int32_t ny, int32_t nz, int64_t sx, int64_t sy,
                        int64_t sz, const float origin[3], float voxel_scale, const float *d_o, const float *d_d, const float *d_r, int32_t n,
                        float max_distance, uint32_t flags, vtmc_sphere_hit *d_hits, void *stream)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = check_queries(ctx, n, !d_grid || !origin || !d_o || (cast && !d_d) || !d_r || !d_hits, cast, max_distance, flags)) return rc;
    if (n == 0) return check_dims(ctx, nx, ny, nz);
    SphereArgs a = sphere_args(d_o, d_d, d_r, d_hits, n, voxel_scale, max_distance, flags);
    if (int rc = surface_of_grid(ctx, d_grid, nx, ny, nz, sx, sy, sz, origin, voxel_scale, &a.g)) return rc;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    VTMC_HIP(ctx, cast ? launch_sphere_query<true>(a, st) : launch_sphere_query<false>(a, st));
    return VTMC_OK;
}

static int terrain_query(vtmc_ctx *ctx, bool cast, const float *o, const float *d, const float *r, int32_t n, float max_distance,
                         uint32_t flags, vtmc_sphere_hit *hits)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (int rc = check_queries(ctx, n, !o || (cast && !d) || !r || !hits, cast, max_distance, flags)) return rc;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain sphere query before terrain_init");
    if (n == 0) return VTMC_OK;
    if (int rc = check_radii(ctx, r, n, ctx->tshape.scale)) return rc;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t vec_bytes = sizeof(float) * 3 * (size_t)n;
    const float *const src[3] = {o, cast ? d : nullptr, r};
    const size_t bytes[3] = {vec_bytes, cast ? vec_bytes : 0, sizeof(float) * (size_t)n};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, sizeof(vtmc_sphere_hit) * (size_t)n, &st)) return rc;
    SphereArgs a = sphere_args(st.in[0], st.in[1], st.in[2], (vtmc_sphere_hit *)st.hits, n, ctx->tshape.scale, max_distance, flags);
    a.g = surface_of_terrain(ctx);
    VTMC_HIP(ctx, cast ? launch_sphere_query<true>(a, ctx->stream) : launch_sphere_query<false>(a, ctx->stream));
    return fetch_hits(ctx, st, hits);
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_spherecast(vtmc_ctx *ctx, const float *origins, const float *directions, const float *radii, int32_t n,
                                float max_distance, uint32_t flags, vtmc_sphere_hit *hits)
{
    return terrain_query(ctx, true, origins, directions, radii, n, max_distance, flags, hits);
}

int32_t vtmc_terrain_closest_point(vtmc_ctx *ctx, const float *centers, const float *radii, int32_t n, uint32_t flags, vtmc_sphere_hit *hits)
{
    return terrain_query(ctx, false, centers, nullptr, radii, n, 1.0f, flags, hits);
}

int32_t vtmc_spherecast_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x, int64_t stride_y,
                               int64_t stride_z, const float origin[3], float voxel_scale, const float *d_origins, const float *d_directions,
                               const float *d_radii, int32_t n, float max_distance, uint32_t flags, vtmc_sphere_hit *d_hits, void *stream)
{
    return device_query(ctx, true, d_grid, nx, ny, nz, stride_x, stride_y, stride_z, origin, voxel_scale, d_origins, d_directions, d_radii, n,
                        max_distance, flags, d_hits, stream);
}

int32_t vtmc_closest_point_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x, int64_t stride_y,
                                  int64_t stride_z, const float origin[3], float voxel_scale, const float *d_centers, const float *d_radii,
                                  int32_t n, uint32_t flags, vtmc_sphere_hit *d_hits, void *stream)
{
    return device_query(ctx, false, d_grid, nx, ny, nz, stride_x, stride_y, stride_z, origin, voxel_scale, d_centers, nullptr, d_radii, n,
                        1.0f, flags, d_hits, stream);
}

}  // extern "C"
