// terrain_naverode.hip -- an agent radius on the navigation layer (include/vtmc_naverode.h): every span's chamfer distance to the nearest
// border of the walkable area, and the erosion of the nav result the context holds to the spans an agent of that radius can occupy.  Not
// in the reference.  The rule is NAVERODE in include/vtmc_naverode.h: integers only, one fixed point, so the kernels are compared for
// equality.  The host half -- the argument checks, the state word and the two relaxations of a round, the counts and sizes -- is
// terrain_naverode.h.  Works on the nav result and never reads the grid.  Hand-written for gfx950 / CDNA4.
//
//   1. naverode_init_kernel    a lane per column, so the column, and with it the open-faces test, is known without a column word per
//                              span: the border test of the column's few spans, D0 into an 8-byte state word {D, Mx, Mz} per span, a
//                              packed copy of the four links (16 bytes, out-of-range links as -1) so that a round does not stride
//                              through 32-byte records, and the border count, reduced per workgroup before the atomic.
//   2. the rounds, the hot path: radius - 1 of them, two kernels each, a lane per span, a pure gather over the span graph.  Each kernel
//      loads the span's 16 bytes of links and gathers the 8-byte state word of its up to four targets; spans are ordered x-fastest, so
//      the +-x gathers are near neighbours.
//        naverode_round_kernel<false>  Mx(s) = min D over the +-x links, Mz(s) = min D over the +-z links
//        naverode_round_kernel<true>   D'(s) = min(D(s), min_k D(link k) + 2, min_{k in +-z} Mx(link k) + 3, min_{k in +-x} Mz(link k) + 3):
//                                      all twelve steps of the rule
//      A kernel reads one state array and writes the other (Jacobi: no lane reads a word another lane of the same launch writes), and
//      radius - 1 rounds reach the fixed point by the rule, so all 2 * (radius - 1) launches are queued without a flag or a read-back.
//   3. naverode_dist_kernel    the distances as int32 (vtmc_nav_distance_build only).
//   4. compaction (vtmc_nav_erode only): naverode_count_kernel, a lane per column, counts the kept spans into the scan's tile totals; the
//      scan and the offsets kernel of the nav build give the new column_offsets; naverode_write_kernel, a lane per column, writes the kept
//      records at the column's new offset, origin, the old-to-new index words and the parent words; naverode_remap_kernel, a lane per new
//      span, maps the links.  The result goes into a second span / offset buffer pair, swapped with the nav result's at the very end.
//   5. the regions of the new links: nav_label_regions, the region pass of the nav build itself.
// Every random-access read or write is bounded by the span count or the box's columns, whatever a record says.
// Traffic of a round that must reach the caches: per span and kernel 16 bytes of links and 8 bytes of state streamed, 8 bytes written, and
// four gathered state words, of which the +-x ones share the streamed lines.
#include "terrain_nav.h"
#include "terrain_naverode.h"
#include "scan_kernels.h"
#include <algorithm>

namespace vtmc {

static_assert(sizeof(vtmc_naverode_params) == 16 && sizeof(int4) == 16, "include/vtmc_naverode.h; the packed links");
enum { kNavErodeCtlBorders = 0, kNavErodeCtlWords = 1 };
constexpr int kNavErodeInitGroups = 1024;   // the most workgroups of the border test: a lane takes every (groups * 256)th column

struct NavErodeBox {
    int dx, dz;
};

__device__ __forceinline__ int link_of(const int4 &l, int k) { return k == 0 ? l.x : k == 1 ? l.y : k == 2 ? l.z : l.w; }

// Pass 1.  D0 = border ? 0 : cap.
__global__ __launch_bounds__(256) void naverode_init_kernel(const vtmc_nav_span *__restrict__ spans, const int32_t *__restrict__ offsets, NavErodeBox b, int32_t n,
                                                           uint32_t cap, uint32_t open_faces, NavErodeState *__restrict__ state, int4 *__restrict__ links,
                                                           int *__restrict__ borders)
{
    __shared__ int wave_found[4];
    int found = 0;
    const int64_t columns = (int64_t)b.dx * b.dz, stride = (int64_t)gridDim.x * 256;
    for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < columns; at += stride) {
        const int c = (int)at, ix = c % b.dx, iz = c / b.dx;
        // whether a missing link of direction k counts: always, or only towards a column of the box
        const bool counts[4] = {!open_faces || ix > 0, !open_faces || ix + 1 < b.dx, !open_faces || iz > 0, !open_faces || iz + 1 < b.dz};
        int lo = offsets[c], hi = offsets[c + 1];
        if (lo < 0) lo = 0;
        if (hi > n) hi = n;
        for (int s = lo; s < hi; ++s) {
            int l[4];
            bool border = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                l[k] = spans[s].link[k];
                if (l[k] < 0 || l[k] >= n) l[k] = -1;
                if (l[k] < 0 && counts[k]) border = true;
            }
            NavErodeState w;
            w.d = (uint16_t)(border ? 0u : cap), w.mx = kNavErodeNone, w.mz = kNavErodeNone, w.pad = 0;
            state[s] = w;
            links[s] = make_int4(l[0], l[1], l[2], l[3]);
            found += border ? 1 : 0;
        }
    }
    // one atomic per workgroup, and kNavErodeInitGroups workgroups at the most: the adds to the one word are served one after the other
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) found += __shfl_down(found, d, 64);
    if (__lane_id() == 0) wave_found[threadIdx.x >> 6] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        found = wave_found[0] + wave_found[1] + wave_found[2] + wave_found[3];
        if (found) atomicAdd(borders, found);
    }
}

// Pass 2, both halves of a round: gathers the state of the up to four targets of span s from `in`, writes the state of s to `out`
template <bool RELAX>
__global__ __launch_bounds__(256) void naverode_round_kernel(const int4 *__restrict__ links, const NavErodeState *__restrict__ in, NavErodeState *__restrict__ out,
                                                            int32_t n)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int4 l = links[s];
    const NavErodeState me = in[s];
    NavErodeState t[4];
    bool has[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = link_of(l, k);
        has[k] = i >= 0 && i < n;
        t[k] = in[has[k] ? i : s];
    }
    out[s] = RELAX ? naverode_relax(me, t, has) : naverode_pair(me, t, has);
}

// Pass 3
__global__ __launch_bounds__(256) void naverode_dist_kernel(const NavErodeState *__restrict__ state, int32_t *__restrict__ dist, int32_t n)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) dist[s] = (int32_t)state[s].d;
}

// Pass 4a: the kept spans of every column
__global__ __launch_bounds__(256) void naverode_count_kernel(const NavErodeState *__restrict__ state, const int32_t *__restrict__ offsets, int32_t columns, int32_t n,
                                                            uint32_t keep, uint32_t *__restrict__ counts)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= columns) return;
    int lo = offsets[c], hi = offsets[c + 1];
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    uint32_t kept = 0;
    for (int s = lo; s < hi; ++s) kept += state[s].d >= keep ? 1u : 0u;
    counts[c] = kept;
}

// Pass 4b: the kept records at the column's new offset, links still in old indices; origin, parent and the old-to-new words.  The new
// buffers hold n records, and a new index never exceeds the old one.
__global__ __launch_bounds__(256) void naverode_write_kernel(const vtmc_nav_span *__restrict__ spans, const NavErodeState *__restrict__ state,
                                                            const int32_t *__restrict__ offsets, const int32_t *__restrict__ new_offsets, int32_t columns, int32_t n,
                                                            uint32_t keep, vtmc_nav_span *__restrict__ out, int32_t *__restrict__ origin, int32_t *__restrict__ parent,
                                                            int32_t *__restrict__ remap)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= columns) return;
    int lo = offsets[c], hi = offsets[c + 1];
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    int slot = new_offsets[c], end = new_offsets[c + 1];
    if (end > n) end = n;
    if (slot < 0) slot = end;   // holds for the offsets of this call; keeps a store inside the buffers whatever they say
    for (int s = lo; s < hi; ++s) {
        int to = -1;
        if (state[s].d >= keep && slot < end) {
            to = slot++;
            out[to] = spans[s];
            origin[to] = s;
            parent[to] = to;
        }
        remap[s] = to;
    }
}

// Pass 4c: link[k] to the new index of its old target, or -1 when that was removed; every span its own region until the labelling.
// new_total is the last entry of the new column_offsets: the host has not read it yet.
__global__ __launch_bounds__(256) void naverode_remap_kernel(vtmc_nav_span *__restrict__ out, const int32_t *__restrict__ remap, const int32_t *__restrict__ new_total,
                                                            int32_t n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int total = *new_total;
    if (total > n) total = n;
    if (i >= total) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = out[i].link[k];
        int to = l >= 0 && l < n ? remap[l] : -1;
        if (to >= total) to = -1;
        out[i].link[k] = to;
    }
    out[i].region = i;
}

// Passes 1 and 2 over the n > 0 spans of the nav result held, queued on the context's stream: the final state lies in the first state
// array.  Events 0..2 of the clock: before the border test, after it, after the rounds.
static int naverode_distance(vtmc_ctx *ctx, const vtmc_naverode_params *p, int32_t n)
{
    const VtmcNav &nav = ctx->nav;
    VtmcNavErode &ne = ctx->naverode;
    hipStream_t s = ctx->stream;
    StageClock<5> &clock = ctx->naverode_clock;
    if (int rc = ensure(ctx, ne.state, 2 * naverode_state_bytes(n))) return rc;
    if (int rc = ensure(ctx, ne.links, naverode_link_bytes(n))) return rc;
    if (int rc = ensure(ctx, ne.ctl, kNavErodeCtlWords * sizeof(int))) return rc;
    NavErodeState *a = (NavErodeState *)ne.state.p, *b = a + n;
    int4 *links = (int4 *)ne.links.p;
    int *ctl = (int *)ne.ctl.p;
    const NavErodeBox box{nav.d[0], nav.d[2]};
    const int64_t columns = (int64_t)box.dx * box.dz;
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kNavErodeCtlWords * sizeof(int), s));
    VTMC_HIP(ctx, clock.mark(0, s));
    const dim3 init_grid(std::min<unsigned>(lanes256(columns).x, (unsigned)kNavErodeInitGroups));
    VTMC_HIP(ctx, launch(naverode_init_kernel, init_grid, dim3(256), 0, s, (const vtmc_nav_span *)nav.spans.p, (const int32_t *)nav.offsets.p, box, n,
                         naverode_clamp(p->radius), p->flags & VTMC_NAVERODE_OPEN_BOX_FACES, a, links, ctl + kNavErodeCtlBorders));
    VTMC_HIP(ctx, clock.mark(1, s));
    ne.rounds = naverode_rounds(p->radius);
    for (int r = 0; r < ne.rounds; ++r) {
        VTMC_HIP(ctx, launch(naverode_round_kernel<false>, lanes256(n), dim3(256), 0, s, (const int4 *)links, (const NavErodeState *)a, b, n));
        VTMC_HIP(ctx, launch(naverode_round_kernel<true>, lanes256(n), dim3(256), 0, s, (const int4 *)links, (const NavErodeState *)b, a, n));
    }
    VTMC_HIP(ctx, clock.mark(2, s));
    return VTMC_OK;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_nav_distance_build(vtmc_ctx *ctx, const vtmc_naverode_params *params, int32_t *n_border)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_border) *n_border = 0;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_distance_build before terrain_nav_build");
    if (const char *what = naverode_params_fault(params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "nav_distance_build: %s", what);
    VtmcNavErode &ne = ctx->naverode;
    const int32_t n = nav.n;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    ne.dist_valid = false;   // from here on the buffer no longer holds the previous distances
    StageClock<5> &clock = ctx->naverode_clock;
    VTMC_HIP(ctx, clock.begin());   // disarmed: a nav result without spans leaves it so
    int borders = 0;
    if (n > 0) {
        if (int rc = ensure(ctx, ne.dist, naverode_word_bytes(n))) return rc;
        if (int rc = naverode_distance(ctx, params, n)) return rc;
        VTMC_HIP(ctx, launch(naverode_dist_kernel, lanes256(n), dim3(256), 0, s, (const NavErodeState *)ne.state.p, (int32_t *)ne.dist.p, n));
        for (int i = 2; i < 5; ++i) VTMC_HIP(ctx, clock.mark(i, s));   // the rounds end behind the conversion; no compaction, no relabelling
        VTMC_HIP(ctx, hipMemcpyAsync(&borders, (const int *)ne.ctl.p + kNavErodeCtlBorders, sizeof borders, hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        clock.arm();
    }
    ne.dist_n = n;
    ne.dist_valid = true;
    if (n_border) *n_border = borders;
    return VTMC_OK;
}

int32_t vtmc_nav_distance_read(vtmc_ctx *ctx, int32_t *dst, int32_t capacity)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_distance_read before terrain_nav_build");
    const VtmcNavErode &ne = ctx->naverode;
    if (!ne.dist_valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_distance_read before nav_distance_build");
    if (capacity < ne.dist_n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d distances", capacity, ne.dist_n);
    if (ne.dist_n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (ne.dist_n > 0) VTMC_HIP(ctx, hipMemcpy(dst, ne.dist.p, naverode_word_bytes(ne.dist_n), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_nav_distance_device_results(vtmc_ctx *ctx, const int32_t **d_dist, int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_distance_device_results before terrain_nav_build");
    const VtmcNavErode &ne = ctx->naverode;
    if (!ne.dist_valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_distance_device_results before nav_distance_build");
    if (d_dist) *d_dist = (const int32_t *)ne.dist.p;
    if (n_spans) *n_spans = ne.dist_n;
    return VTMC_OK;
}

int32_t vtmc_nav_erode(vtmc_ctx *ctx, const vtmc_naverode_params *params, int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_spans) *n_spans = 0;
    VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_erode before terrain_nav_build");
    if (const char *what = naverode_params_fault(params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "nav_erode: %s", what);
    VtmcNavErode &ne = ctx->naverode;
    const int32_t n = nav.n;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    // from here on neither the flow field nor the distances nor the crowd describe the nav result, and the origin buffer is being rewritten
    ctx->navfield.valid = false, ne.dist_valid = false, ne.origin_valid = false, ctx->navcrowd.valid = false;
    StageClock<5> &clock = ctx->naverode_clock;
    VTMC_HIP(ctx, clock.begin());   // disarmed: a nav result without spans leaves it so
    int32_t kept = 0;
    if (n > 0) {
        const NavSizes sz = nav_sizes(nav_held_box(nav));   // n > 0: the box is not empty, and the build has sized the scan buffer and the scratch for it
        if (int rc = ensure(ctx, nav.spans_next, nav_span_bytes(n))) return rc;
        if (int rc = ensure(ctx, nav.offsets_next, sz.offsets_bytes)) return rc;
        if (int rc = ensure(ctx, nav.scan, sz.scan_bytes)) return rc;
        if (int rc = ensure(ctx, nav.scratch, nav_scratch_bytes(n))) return rc;
        if (int rc = ensure(ctx, ne.remap, naverode_word_bytes(n))) return rc;
        if (int rc = ensure(ctx, ne.origin, naverode_word_bytes(n))) return rc;
        if (int rc = naverode_distance(ctx, params, n)) return rc;
        const int32_t columns = (int32_t)sz.columns;
        const ScanLayout scan((uint64_t)columns, nav.scan.p);
        const NavErodeState *state = (const NavErodeState *)ne.state.p;
        const vtmc_nav_span *spans = (const vtmc_nav_span *)nav.spans.p;
        const int32_t *offsets = (const int32_t *)nav.offsets.p;
        vtmc_nav_span *out = (vtmc_nav_span *)nav.spans_next.p;
        int32_t *new_offsets = (int32_t *)nav.offsets_next.p, *parent = (int32_t *)nav.scratch.p;
        const uint32_t keep = naverode_clamp(params->radius);
        VTMC_HIP(ctx, launch(naverode_count_kernel, lanes256(columns), dim3(256), 0, s, state, offsets, columns, n, keep, scan.tile_totals()));
        VTMC_HIP(ctx, launch_scan(scan, s));
        VTMC_HIP(ctx, nav_launch_offsets(scan, new_offsets, s));
        VTMC_HIP(ctx, launch(naverode_write_kernel, lanes256(columns), dim3(256), 0, s, spans, state, offsets, (const int32_t *)new_offsets, columns, n, keep, out,
                             (int32_t *)ne.origin.p, parent, (int32_t *)ne.remap.p));
        VTMC_HIP(ctx, launch(naverode_remap_kernel, lanes256(n), dim3(256), 0, s, out, (const int32_t *)ne.remap.p, (const int32_t *)new_offsets + columns, n));
        VTMC_HIP(ctx, clock.mark(3, s));
        unsigned long long total = 0;
        VTMC_HIP(ctx, hipMemcpyAsync(&total, scan.total(), sizeof(total), hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        if (total > (unsigned long long)n) return fail(ctx, VTMC_ERR_DEVICE, "nav_erode: %llu spans kept of %d", total, n);
        kept = (int32_t)total;
        int rounds = 0;
        if (kept > 0) {
            VTMC_HIP(ctx, hipMemsetAsync(nav.ctl.p, 0, 2 * sizeof(int), s));   // the region pass's flag and count
            if (int rc = nav_label_regions(ctx, "nav_erode", out, parent, kept, false, &rounds)) return rc;
        }
        VTMC_HIP(ctx, clock.mark(4, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        nav.spans.swap(nav.spans_next);
        nav.offsets.swap(nav.offsets_next);
        nav.n = kept;
        clock.arm();
    }
    ne.origin_n = kept;
    ne.origin_valid = true;
    if (n_spans) *n_spans = kept;
    return VTMC_OK;
}

int32_t vtmc_nav_erode_origin(vtmc_ctx *ctx, int32_t *dst, int32_t capacity)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_erode_origin before terrain_nav_build");
    const VtmcNavErode &ne = ctx->naverode;
    if (!ne.origin_valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_erode_origin before nav_erode");
    if (capacity < ne.origin_n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d spans", capacity, ne.origin_n);
    if (ne.origin_n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (ne.origin_n > 0) VTMC_HIP(ctx, hipMemcpy(dst, ne.origin.p, naverode_word_bytes(ne.origin_n), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

// Not part of the ABI (tools/naverode_bench.py): device time of the last vtmc_nav_distance_build or vtmc_nav_erode over a nav result
// with spans, ms[0..3] = the border test, the rounds (a distance build: with the conversion to int32), the compaction, the relabelling
// (the host's read-backs of its rounds included); a distance build has neither of the last two: their events follow one another.  ms[4] = the
// rounds of the distance pass.
int32_t vtmc_debug_naverode_ms(vtmc_ctx *ctx, float ms[5])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid || !ctx->naverode_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_naverode_ms before a distance build or an erode that launched kernels");
    if (int rc = ctx->naverode_clock.sync_last(ctx)) return rc;
    for (int i = 0; i < 4; ++i)
        if (int rc = ctx->naverode_clock.elapsed(ctx, i, i + 1, &ms[i])) return rc;
    ms[4] = (float)ctx->naverode.rounds;
    return VTMC_OK;
}

}  // extern "C"
