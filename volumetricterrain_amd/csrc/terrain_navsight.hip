// terrain_navsight.hip -- any-angle paths on the navigation layer (include/vtmc_navsight.h): the line-of-sight walk over the spans, and
// the traced paths of the flow field pulled straight wherever the walk succeeds.  Not in the reference.  The rule is NAVSIGHT in
// include/vtmc_navsight.h: integers only, so the kernels are compared for equality.  The host half -- the argument checks, the column
// search, the walk itself -- is terrain_navsight.h; the kernels call the same walk.  Works on the nav result and the field the context
// holds, never reads the grid and keeps nothing between calls.  Hand-written for gfx950 / CDNA4.
//
//   nav_sight_kernel         a lane per pair: both columns by the bounded bisection of column_offsets, then the walk.
//   navsight_pack_kernel     a lane per span: the four links, packed, for the smoothed trace of the same call (see below).
//   navfield_smooth_kernel   one wave64 per start, four per workgroup; there is no barrier in it, so a wave leaves when its row is done.
//                            The spans that follow the anchor along next lie in a ring of 256 entries in the wave's LDS, with their column
//                            offsets from the START beside them (recovered from which link[k] equals next: no column search at all).
//                            The ring is why a span's next is read once per row and not once per anchor: after a pick the entries behind
//                            it stay, and the chain is only topped up to max_look.  The top-up is wave-uniform (every lane follows the
//                            same words; lane 0 stores them).  The candidates are then tested farthest first, 64 at a time, one per lane:
//                            the walk from the anchor, and the cost bound where one is asked for.  A ballot picks the highest passing lane
//                            of the first chunk that has one; lane 0 appends the pick and the anchor moves.
// Every loop is bounded by a count -- the top-up by max_look, the walk by nx + nz, the row by max_len, the bisection by 32 -- and every
// random-access index is checked against n before it is used, whatever a record says.
//
// Where the links come from was decided by tools/navsight_bench.py, the product against a build with the other source, alternating, at 1024^3
// cells and 1.36 M spans (profiles/r24/navsight).  A walk is a chain of dependent gathers, one link of one span per step.  The smoothed
// trace reads them from a packed 16-byte copy (navsight_pack_kernel): its kernel came out 6 to 9 % faster than over the 32-byte records
// on long paths (11.7 -> 11.0 ms, 29.1 -> 26.5 ms, 4.27 -> 3.98 ms) and 3 to 5 % on short ones, and the pack itself takes 0.010 ms.  That
// is little enough to make the copy anew in every call, in front of the kernel, and keep NOTHING of the nav result between calls: there
// is no cached copy to drop with the field or in vtmc_nav_erode.  The sight query reads the 32-byte spans: its kernel takes 0.04 to
// 0.07 ms for 100 000 pairs, the two sources differed by +-0.003 ms in either direction, and a pack would cost more than it could save.
// The edge costs are the 16 bytes per span the field build left in VtmcNavField::work; a walk reads them only under a cost bound.
#include "surface_query.h"
#include "terrain_navfield.h"
#include "terrain_navsight.h"
#include <cstring>

namespace vtmc {

static_assert(sizeof(vtmc_navsight_params) == 16 && sizeof(vtmc_navsight_hit) == 8, "include/vtmc_navsight.h");
constexpr int kNavSightWaves = 4;                          // starts of a workgroup of the smoothed trace
constexpr int kNavSightRing = VTMC_NAVSIGHT_MAX_LOOK;      // entries of a wave's ring: a power of two
static_assert((kNavSightRing & (kNavSightRing - 1)) == 0 && kNavSightRing % 64 == 0, "the ring wraps by a mask and is tested in whole chunks");

// LDS traffic of one wave is processed in issue order (mc_device.h: VTMC_WAVE_SYNC): a hand-off through LDS inside a wave needs only the
// compiler kept from moving LDS accesses across it
#define VTMC_NAVSIGHT_WAVE_SYNC()         \
    do {                                  \
        asm volatile("" ::: "memory");    \
        __builtin_amdgcn_wave_barrier();  \
        asm volatile("" ::: "memory");    \
    } while (0)

struct NavSightSpanLinks {   // link[k] of span s, 0 <= s < n, from the 32-byte records
    const vtmc_nav_span *spans;
    __device__ __forceinline__ int32_t operator()(int32_t s, int k) const { return spans[s].link[k]; }
};
struct NavSightPackedLinks {   // ... from the packed copy a smoothed trace makes for itself
    const int32_t *links;
    __device__ __forceinline__ int32_t operator()(int32_t s, int k) const { return links[4 * (size_t)s + k]; }
};
struct NavSightCosts {   // c(s, k), from the field build's work words
    const uint32_t *costs;
    __device__ __forceinline__ uint32_t operator()(int32_t s, int k) const { return costs[4 * (size_t)s + k]; }
};
struct NavSightNoCosts {
    __device__ __forceinline__ uint32_t operator()(int32_t, int) const { return 0u; }
};

__global__ __launch_bounds__(256) void nav_sight_kernel(NavSightSpanLinks link, const int32_t *__restrict__ offsets, int32_t dx, int32_t columns,
                                                       int32_t n, const int32_t *__restrict__ from, const int32_t *__restrict__ to, int32_t n_pairs,
                                                       vtmc_navsight_hit *__restrict__ hits)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const int32_t a = from[i], b = to[i];
    vtmc_navsight_hit hit;
    hit.last = -1, hit.steps = 0;
    if (a >= 0 && a < n && b >= 0 && b < n && columns > 0 && dx > 0) {
        const int32_t ca = navsight_column(offsets, columns, a), cb = navsight_column(offsets, columns, b);
        const NavSightWalk w = navsight_walk(a, cb % dx - ca % dx, cb / dx - ca / dx, n, link, NavSightNoCosts{});
        hit.last = w.last, hit.steps = w.steps;
    }
    hits[i] = hit;
}

// The four links of every span, 16 bytes, for the smoothed trace that follows in the same call
__global__ __launch_bounds__(256) void navsight_pack_kernel(const vtmc_nav_span *__restrict__ spans, int4 *__restrict__ links, int32_t n)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) links[s] = make_int4(spans[s].link[0], spans[s].link[1], spans[s].link[2], spans[s].link[3]);
}

// the rows are -1 already
template <bool BOUND>
__global__ __launch_bounds__(64 * kNavSightWaves) void navfield_smooth_kernel(NavSightPackedLinks link, const uint32_t *__restrict__ costs,
                                                                            const vtmc_navfield_cell *__restrict__ cells, int32_t n, const int32_t *__restrict__ starts,
                                                                            int32_t n_starts, int32_t max_len, int32_t max_look, uint32_t max_extra_cost,
                                                                            int32_t *__restrict__ paths, int32_t *__restrict__ lengths)
{
    __shared__ int32_t ring_span[kNavSightWaves][kNavSightRing];
    __shared__ uint32_t ring_at[kNavSightWaves][kNavSightRing];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kNavSightWaves + wave;
    if (i >= n_starts) return;   // the whole wave; there is no workgroup barrier below
    int32_t *chain = ring_span[wave];
    uint32_t *chain_at = ring_at[wave];
    int32_t *row = paths + (size_t)i * (size_t)max_len;
    if (max_look > kNavSightRing) max_look = kNavSightRing;   // the host has checked; keeps the ring inside the LDS whatever it says
    const int32_t s0 = starts[i];
    int len = 0;
    if (s0 >= 0 && s0 < n && cells[s0].cost != VTMC_NAVFIELD_UNREACHED) {
        if (lane == 0) row[0] = s0;
        len = 1;
        int32_t a = s0, ax = 0, az = 0;          // the anchor and its column offset from the start
        int32_t tail = s0, tx = 0, tz = 0;       // the last span of the chain (the anchor while it is empty): its next tops the chain up
        bool open = true;                        // until the chain has reached a span whose next is -1
        int head = 0, count = 0;
        while (len < max_len) {
            while (open && count < max_look) {   // wave-uniform
                const int32_t t = cells[tail].next;
                int k = -1;
                if (t >= 0 && t < n) {
#pragma unroll
                    for (int d = 3; d >= 0; --d)
                        if (link(tail, d) == t) k = d;
                }
                if (k < 0) {   // arrived; or a next that is no link of its span, which the field build never leaves
                    open = false;
                    break;
                }
                tx += k == 0 ? -1 : k == 1 ? 1 : 0, tz += k == 2 ? -1 : k == 3 ? 1 : 0;
                tail = t;
                if (lane == 0) {
                    const int slot = (head + count) & (kNavSightRing - 1);
                    chain[slot] = t, chain_at[slot] = navsight_pack(tx, tz);
                }
                ++count;
            }
            if (count == 0) break;   // next(a) is -1
            VTMC_NAVSIGHT_WAVE_SYNC();
            const uint32_t d_a = BOUND ? cells[a].cost : 0u;
            int pick = -1;
            for (int top = count; top > 0 && pick < 0; top -= 64) {   // candidates top - 64 .. top - 1, lane 63 the farthest
                const int at = top - 64 + lane;
                bool ok = false;
                if (at >= 0) {
                    const int slot = (head + at) & (kNavSightRing - 1);
                    const int32_t b = chain[slot];
                    const uint32_t where = chain_at[slot];
                    const int32_t ox = navsight_ox(where) - ax, oz = navsight_oz(where) - az;
                    if (BOUND) {
                        const NavSightWalk w = navsight_walk(a, ox, oz, n, link, NavSightCosts{costs});
                        ok = w.last == b && navsight_cost_ok(w.w, cells[b].cost, d_a, max_extra_cost);
                    } else {
                        ok = navsight_walk(a, ox, oz, n, link, NavSightNoCosts{}).last == b;
                    }
                }
                const unsigned long long m = __ballot(ok);
                if (m) pick = top - 64 + (63 - __builtin_clzll(m));
            }
            if (pick < 0) pick = 0;   // by the rule chain[0] passes; keeps the row growing whatever the records say
            const int slot = (head + pick) & (kNavSightRing - 1);
            a = chain[slot];
            ax = navsight_ox(chain_at[slot]), az = navsight_oz(chain_at[slot]);
            if (lane == 0) row[len] = a;
            ++len;
            head = (head + pick + 1) & (kNavSightRing - 1), count -= pick + 1;
            VTMC_NAVSIGHT_WAVE_SYNC();   // the picks are read before the next top-up stores
        }
    }
    if (lane == 0) lengths[i] = len;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_nav_sight(vtmc_ctx *ctx, const int32_t *from, const int32_t *to, int32_t n, vtmc_navsight_hit *hits)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_sight before terrain_nav_build");
    int32_t at = -1;
    if (const char *what = navsight_sight_fault(from, to, n, hits, nav.n, &at))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "nav_sight: %s (pair %d, %d spans)", what, at, nav.n);
    if (n == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    StageClock<3> &clock = ctx->navsight_clock;
    VTMC_HIP(ctx, clock.begin());
    const float *const src[3] = {(const float *)from, (const float *)to, nullptr};
    const size_t bytes[3] = {(size_t)n * 4u, (size_t)n * 4u, 0};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, navsight_hit_bytes(n), &st)) return rc;
    const int64_t columns = (int64_t)nav.d[0] * nav.d[2];
    VTMC_HIP(ctx, clock.mark(0, s));
    const NavSightSpanLinks link{(const vtmc_nav_span *)nav.spans.p};
    VTMC_HIP(ctx, clock.mark(1, s));   // no rows to fill
    VTMC_HIP(ctx, launch(nav_sight_kernel, lanes256(n), dim3(256), 0, s, link, (const int32_t *)nav.offsets.p, nav.d[0], (int32_t)columns,
                         nav.n, (const int32_t *)st.in[0], (const int32_t *)st.in[1], n, (vtmc_navsight_hit *)st.hits));
    VTMC_HIP(ctx, clock.mark(2, s));
    if (int rc = fetch_hits(ctx, st, hits)) return rc;
    clock.arm();
    return VTMC_OK;
}

int32_t vtmc_navfield_trace_smooth(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, const vtmc_navsight_params *params, int32_t *paths,
                                   int32_t *lengths)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid || !ctx->nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navfield_trace_smooth before navfield_build");
    if (const char *what = navsight_params_fault(params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "navfield_trace_smooth: %s", what);
    int32_t at = -1;
    if (const char *what = navfield_trace_fault(starts, n_starts, max_len, paths, lengths, nf.n, &at))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "navfield_trace_smooth: %s (start %d, %d spans)", what, at, nf.n);
    if (n_starts == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    StageClock<3> &clock = ctx->navsight_clock;
    VTMC_HIP(ctx, clock.begin());
    if (int rc = ensure(ctx, ctx->navsight_links, navsight_link_bytes(nf.n))) return rc;
    TraceRows rows;
    if (int rc = trace_rows_stage(ctx, starts, n_starts, max_len, &rows)) return rc;
    const vtmc_nav_span *spans = (const vtmc_nav_span *)ctx->nav.spans.p;
    const uint32_t *costs = (const uint32_t *)nf.work.p;   // the four edge costs of every span, as navfield_build left them
    const vtmc_navfield_cell *cells = (const vtmc_navfield_cell *)nf.cells.p;
    const dim3 grid((unsigned)(((int64_t)n_starts + kNavSightWaves - 1) / kNavSightWaves)), block(64 * kNavSightWaves);
    VTMC_HIP(ctx, clock.mark(0, s));
    VTMC_HIP(ctx, hipMemsetAsync(rows.paths, 0xff, rows.path_bytes, s));
    VTMC_HIP(ctx, launch(navsight_pack_kernel, lanes256(nf.n), dim3(256), 0, s, spans, (int4 *)ctx->navsight_links.p, nf.n));
    const NavSightPackedLinks link{(const int32_t *)ctx->navsight_links.p};
    VTMC_HIP(ctx, clock.mark(1, s));
    if (params->max_extra_cost == VTMC_NAVSIGHT_ANY_COST)
        VTMC_HIP(ctx, launch(navfield_smooth_kernel<false>, grid, block, 0, s, link, costs, cells, nf.n, rows.starts, n_starts, max_len, params->max_look, params->max_extra_cost,
                             rows.paths, rows.lengths));
    else
        VTMC_HIP(ctx, launch(navfield_smooth_kernel<true>, grid, block, 0, s, link, costs, cells, nf.n, rows.starts, n_starts, max_len, params->max_look, params->max_extra_cost,
                             rows.paths, rows.lengths));
    VTMC_HIP(ctx, clock.mark(2, s));
    if (int rc = trace_rows_fetch(ctx, rows, paths, lengths)) return rc;
    clock.arm();
    return VTMC_OK;
}

// Not part of the ABI (tools/navsight_bench.py): device time of the last vtmc_nav_sight or vtmc_navfield_trace_smooth that launched a
// kernel, ms[0] = the fill of the rows with -1 and the packing of the links (a sight query has neither: its two events follow one
// another), ms[1] = the kernel.
int32_t vtmc_debug_navsight_ms(vtmc_ctx *ctx, float ms[2])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid || !ctx->navsight_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_navsight_ms before a nav_sight or navfield_trace_smooth that launched a kernel");
    if (int rc = ctx->navsight_clock.sync_last(ctx)) return rc;
    for (int i = 0; i < 2; ++i)
        if (int rc = ctx->navsight_clock.elapsed(ctx, i, i + 1, &ms[i])) return rc;
    return VTMC_OK;
}

}  // extern "C"
