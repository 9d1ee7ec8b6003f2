// terrain_nav.hip -- where something can walk on the resident terrain and which places are connected (vtmc_terrain_nav_build and its
// readers, include/vtmc_nav.h): per column of a box the floors with enough headroom, per floor one step-limited link to each of the four
// neighbour columns, and the connected regions.  Not in the reference.  The rule, operation by operation, is NAVIGATION in
// include/vtmc_nav.h; the kernels follow it bit for bit (library built with -ffp-contract=off).  The host half -- argument checks, the
// box as reported, the buffer sizes, the max_spans check -- is terrain_nav.h.  Hand-written for gfx950 / CDNA4.
//
// No atomic decides where a span goes: its index is a function of the grid alone.
//   1. nav_walk_kernel<false>  64 x 4 threads, a lane per column, 64 columns along x (the stride-1 axis) per wave and 4 z per workgroup.
//      A lane walks its column bottom-up; every y step is one coalesced 256-byte row per wave, kNavRows rows are requested before the
//      first is used.  The state carried across steps is the sample below, the floor that is waiting for its ceiling (height, y) and its
//      open count.  Writes the column's span count.
//   2. the exclusive scan of the counts (scan_kernels.h, shared with the scatter pass) and nav_offsets_kernel, which adds the two levels
//      into column_offsets.  The grand total goes to the host for the max_spans check and the growth of the span buffer.
//   3. nav_walk_kernel<true>   the same walk, writing height, y and clearance at the column's offset, the column of every span and the
//      span as its own parent.  A lane whose column holds no span loads nothing.
//   4. nav_link_kernel         a lane per span: for each direction it scans the neighbour column's few spans by the rule.
//   5. nav_union_kernel, nav_flatten_kernel, nav_verify_kernel   union-find over the span indices through the links (union_find.h, shared
//      with the fragment labelling: union by smaller index, bounded loops, a flag word), then every span to its root: the smallest index
//      of its component; then the regions are checked against their definition (no link crosses two regions), and the three passes run
//      again while the check fails (nav_label_regions, which the erosion of terrain_naverode.hip calls on the spans it kept).  A link that is
//      answered by the span at its other end is one union, made by the upper span.
// Every random-access read is bounded by the box or the span count and every loop by a count.
// Traffic that must reach HBM: the box twice (the emit walk skips only whole waves of empty columns), 8 bytes per column, and per span
// 32 bytes written, read by its four neighbours' lanes and written again twice (links, region), plus 8 bytes of scratch.
#include "terrain_edit.h"
#include "terrain_nav.h"
#include "scan_kernels.h"
#include "union_find.h"
#include <algorithm>

namespace vtmc {

static_assert(sizeof(vtmc_nav_span) == 32, "two 16-byte stores per span");
constexpr int kNavRows = 8;   // rows of a column in flight per lane
enum { kNavCtlFlag = 0, kNavCtlSplit = 1, kNavCtlWords = 2 };   // the control words: the loops' flag, the verify pass's count
constexpr int kNavMaxRounds = 8;   // union / flatten / verify rounds before the build gives up

__device__ __forceinline__ int nav_ceil(int y, int clearance) { return clearance == VTMC_NAV_OPEN ? VTMC_NAV_OPEN : y + 1 + clearance; }

// Passes 1 and 3.  offsets / spans / col_of / parent are read and written by the emit pass only; counts by the count pass only.
template <bool EMIT>
__global__ __launch_bounds__(256) void nav_walk_kernel(const float *__restrict__ grid, TerrainShape sh, TerrainBox b, int agent_height,
                                                       uint32_t *__restrict__ counts, const int32_t *__restrict__ offsets,
                                                       vtmc_nav_span *__restrict__ spans, int32_t *__restrict__ col_of, int32_t *__restrict__ parent,
                                                       int32_t n_spans)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iz = blockIdx.y * 4 + threadIdx.y;
    if (ix >= b.dx || iz >= b.dz) return;
    const int col = ix + b.dx * iz;
    int slot = 0, end = 0;
    if (EMIT) {
        slot = offsets[col], end = offsets[col + 1];
        if (end > n_spans) end = n_spans;   // holds for the offsets of this call; keeps a store inside the buffers whatever they say
        if (slot < 0 || slot >= end) return;
    }
    const float *column = grid + grid_index(sh, b.lx + ix, b.ly, b.lz + iz);
    const uint64_t row = (uint64_t)sh.dim_x;   // one step along y
    uint32_t n = 0;
    float below = 0.0f, height = 0.0f;   // the sample under this one; the waiting floor
    int floor_y = 0, open = 0;
    bool waiting = false;
    // a floor whose run of open samples has ended (clearance samples) or reached the top plane (VTMC_NAV_OPEN)
    auto finish = [&](int clearance) {
        if (clearance < agent_height) return;
        if (EMIT && slot < end) {
            vtmc_nav_span s;
            s.height = height, s.y = floor_y, s.clearance = clearance;
            s.link[0] = s.link[1] = s.link[2] = s.link[3] = -1;
            s.region = slot;
            spans[slot] = s;
            col_of[slot] = col;
            parent[slot] = slot;
            ++slot;
        }
        ++n;
    };
    for (int y0 = 0; y0 < b.dy; y0 += kNavRows) {
        float v[kNavRows];
#pragma unroll
        for (int j = 0; j < kNavRows; ++j) v[j] = y0 + j < b.dy ? column[(uint64_t)(y0 + j) * row] : 0.0f;
#pragma unroll
        for (int j = 0; j < kNavRows; ++j) {
            if (y0 + j >= b.dy) break;
            const float s = v[j];
            if (s > 0.0f) {
                if (waiting) finish(open);
                waiting = false;
            } else if (waiting) {
                ++open;
            } else if (below > 0.0f && s <= 0.0f) {   // a floor at the sample below; a NaN here is open but no floor
                const float t = below / (below - s);
                floor_y = b.ly + y0 + j - 1;
                height = (float)floor_y + t;
                open = 1;
                waiting = true;
            }
            below = s;
        }
    }
    if (waiting) finish(VTMC_NAV_OPEN);
    if (!EMIT) counts[col] = n;
}

// The yardstick of tools/nav_bench.py: the walk's loads and nothing else -- every lane adds up its column and leaves the sum's bits
__global__ __launch_bounds__(256) void nav_read_kernel(const float *__restrict__ grid, TerrainShape sh, TerrainBox b, uint32_t *__restrict__ sums)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iz = blockIdx.y * 4 + threadIdx.y;
    if (ix >= b.dx || iz >= b.dz) return;
    const float *column = grid + grid_index(sh, b.lx + ix, b.ly, b.lz + iz);
    const uint64_t row = (uint64_t)sh.dim_x;
    float sum = 0.0f;
    for (int y0 = 0; y0 < b.dy; y0 += kNavRows) {
        float v[kNavRows];
#pragma unroll
        for (int j = 0; j < kNavRows; ++j) v[j] = y0 + j < b.dy ? column[(uint64_t)(y0 + j) * row] : 0.0f;
#pragma unroll
        for (int j = 0; j < kNavRows; ++j) sum += v[j];
    }
    sums[ix + b.dx * iz] = __float_as_uint(sum);
}

// column_offsets from the two levels of the scan; the last entry is the total
__global__ __launch_bounds__(256) void nav_offsets_kernel(const uint32_t *__restrict__ tile_offsets, const uint32_t *__restrict__ group_offsets,
                                                         const unsigned long long *__restrict__ total, uint32_t columns, int32_t *__restrict__ offsets)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < columns) offsets[c] = (int32_t)(group_offsets[c / (uint32_t)kScanThreads] + tile_offsets[c]);
    else if (c == columns) offsets[c] = (int32_t)*total;
}

// Pass 4: link[k] of span s is the qualifying span of the neighbour column with the smallest |d|, the lower one on a tie
__global__ __launch_bounds__(256) void nav_link_kernel(vtmc_nav_span *__restrict__ spans, const int32_t *__restrict__ col_of, const int32_t *__restrict__ offsets,
                                                      int *__restrict__ flag, TerrainBox b, int32_t n, int agent_height, float max_step)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int col = col_of[s];
    if (col < 0 || col >= b.dx * b.dz) {
        atomicOr(flag, 4);
        return;
    }
    const int ix = col % b.dx, iz = col / b.dx;
    const float hs = spans[s].height;
    const int ceil_s = nav_ceil(spans[s].y, spans[s].clearance);
    const float need = (float)agent_height;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nx = ix + (k == 0 ? -1 : k == 1 ? 1 : 0), nz = iz + (k == 2 ? -1 : k == 3 ? 1 : 0);
        int best = -1;
        if (nx >= 0 && nx < b.dx && nz >= 0 && nz < b.dz) {
            const int nc = nx + b.dx * nz;
            int lo = offsets[nc], hi = offsets[nc + 1];
            if (lo < 0) lo = 0;
            if (hi > n) hi = n;
            float best_d = 0.0f;
            for (int i = lo; i < hi; ++i) {
                const float hn = spans[i].height;
                const float d = hn - hs;
                const float ad = fabsf(d);
                if (!(ad <= max_step)) continue;
                const int ceil_n = nav_ceil(spans[i].y, spans[i].clearance);
                const int top = ceil_s < ceil_n ? ceil_s : ceil_n;
                if (top != VTMC_NAV_OPEN && !((float)top - (hs > hn ? hs : hn) >= need)) continue;
                if (best < 0 || ad < best_d) best = i, best_d = ad;
            }
        }
        spans[s].link[k] = best;
    }
}

// Pass 5a: a span joins the spans it links to
__global__ __launch_bounds__(256) void nav_union_kernel(const vtmc_nav_span *__restrict__ spans, int *__restrict__ P, int *__restrict__ flag, int32_t n)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = spans[s].link[k];
        if (l < 0 || l >= n || l == s) continue;
        if (l > s && spans[l].link[k ^ 1] == s) continue;   // a link that is answered: the span at its upper end makes the union
        uf_union<kScope, true>(P, s, l, n, flag);
    }
}

// Pass 5b: every span to its root; a failed find leaves the span its own region: the flag is set, nobody reads the result
__global__ __launch_bounds__(256) void nav_flatten_kernel(vtmc_nav_span *__restrict__ spans, const int *__restrict__ P, int *__restrict__ flag, int32_t n)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int root = uf_find<kScope>(P, s, n, flag);
    spans[s].region = root < 0 ? s : root;
}

// Pass 5c: the regions against their own definition.  A span whose region differs from that of a span it links to is counted; with the
// two properties the flatten pass gives by construction (region <= index, a region's first span is its own region) a count of 0 means the
// regions ARE the components of the link graph, whatever happened in the union pass.
__global__ __launch_bounds__(256) void nav_verify_kernel(const vtmc_nav_span *__restrict__ spans, int *__restrict__ split, int32_t n)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (s < n) {
        const int r = spans[s].region;
        bad = r < 0 || r > s || spans[r].region != r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = spans[s].link[k];
            if (l >= 0 && l < n && spans[l].region != r) bad = true;
        }
    }
    const unsigned long long m = __ballot(bad);
    if (m && __lane_id() == 0) atomicAdd(split, __popcll(m));
}

// column_offsets of a scanned layout whose tiles are the columns (vtmc_ctx.h: terrain_naverode.hip compacts with it too)
hipError_t nav_launch_offsets(const ScanLayout &scan, int32_t *offsets, hipStream_t stream)
{
    const uint32_t columns = (uint32_t)scan.n_tiles;
    return launch(nav_offsets_kernel, lanes256((int64_t)columns + 1), dim3(256), 0, stream, scan.tile_offsets(), scan.group_offsets(), scan.total(), columns, offsets);
}

// Pass 5 over n > 0 spans whose links are final and whose parent words are their own indices (vtmc_ctx.h: the build, and the erosion of
// terrain_naverode.hip on the spans it kept).  Regions: union, flatten, verify -- and again while the verify pass still finds a link across
// two regions.  The union pass was seen to lose a union now and then under contention (a few per million on an MI355X, profiles/r21/nav);
// a repeat only has those few to make, and the result that is kept has passed the check.  With `timed` the nav clock's events 5..8 time
// the first round.  Uses the control words of the nav build; *rounds is the number of rounds taken.
int nav_label_regions(vtmc_ctx *ctx, const char *who, vtmc_nav_span *spans, int32_t *parent, int32_t n, bool timed, int *rounds)
{
    hipStream_t s = ctx->stream;
    StageClock<9> &clock = ctx->nav_clock;
    int *flag = (int *)ctx->nav.ctl.p;
    int h_ctl[kNavCtlWords] = {0, 0};
    *rounds = 0;
    for (int round = 0;; ++round) {
        const bool mark = timed && round == 0;
        if (mark) VTMC_HIP(ctx, clock.mark(5, s));
        VTMC_HIP(ctx, launch(nav_union_kernel, lanes256(n), dim3(256), 0, s, spans, parent, flag, n));
        if (mark) VTMC_HIP(ctx, clock.mark(6, s));
        VTMC_HIP(ctx, launch(nav_flatten_kernel, lanes256(n), dim3(256), 0, s, spans, parent, flag, n));
        if (mark) VTMC_HIP(ctx, clock.mark(7, s));
        VTMC_HIP(ctx, hipMemsetAsync(flag + kNavCtlSplit, 0, sizeof(int), s));
        VTMC_HIP(ctx, launch(nav_verify_kernel, lanes256(n), dim3(256), 0, s, spans, flag + kNavCtlSplit, n));
        if (mark) VTMC_HIP(ctx, clock.mark(8, s));
        VTMC_HIP(ctx, hipMemcpyAsync(h_ctl, flag, sizeof h_ctl, hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        *rounds = round + 1;
        if (h_ctl[kNavCtlFlag]) return fail(ctx, VTMC_ERR_DEVICE, "%s: labelling did not converge (flag %d)", who, h_ctl[kNavCtlFlag]);
        if (h_ctl[kNavCtlSplit] == 0) return VTMC_OK;
        if (round + 1 == kNavMaxRounds)
            return fail(ctx, VTMC_ERR_DEVICE, "%s: labelling did not converge (%d spans across regions after %d rounds)", who, h_ctl[kNavCtlSplit], kNavMaxRounds);
    }
}

NavBox nav_held_box(const VtmcNav &nav)
{
    NavBox nb;
    for (int k = 0; k < 3; ++k) nb.lo[k] = nav.lo[k], nb.d[k] = nav.d[k];
    return nb;
}

static dim3 walk_grid(const TerrainBox &b) { return dim3((unsigned)((b.dx + 63) / 64), (unsigned)((b.dz + 3) / 4)); }   // nav_walk_kernel, nav_read_kernel

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_nav_build(vtmc_ctx *ctx, const float lower[3], const float upper[3], const vtmc_nav_params *params, int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_spans) *n_spans = 0;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_nav_build before terrain_init");
    if (const char *what = nav_args_fault(lower, upper, params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_nav_build: %s", what);
    const TerrainShape &sh = ctx->tshape;
    const TerrainBox tb = bounds_box(sh, lower, upper);
    const int32_t first[3] = {tb.lx, tb.ly, tb.lz}, dims[3] = {tb.dx, tb.dy, tb.dz};
    const NavBox nb = nav_box(first, dims);
    const NavSizes sz = nav_sizes(nb);
    if (!sz.launchable) return fail(ctx, VTMC_ERR_TOO_LARGE, "terrain_nav_build: %lld columns", (long long)sz.columns);
    VtmcNav &nav = ctx->nav;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nav_drop(ctx);   // from here on the buffers no longer hold the previous build, nor does the flow field on it stand
    StageClock<9> &clock = ctx->nav_clock;
    VTMC_HIP(ctx, clock.begin());   // disarmed: an empty box, or a box without spans, leaves it so
    if (int rc = ensure(ctx, nav.offsets, sz.offsets_bytes)) return rc;
    int32_t *offsets = (int32_t *)nav.offsets.p;
    unsigned long long total = 0;
    if (nav_box_empty(nb)) {
        VTMC_HIP(ctx, hipMemsetAsync(offsets, 0, sz.offsets_bytes, s));
    } else {
        if (int rc = ensure(ctx, nav.scan, sz.scan_bytes)) return rc;
        if (int rc = ensure(ctx, nav.ctl, kNavCtlWords * sizeof(int))) return rc;
        const uint32_t columns = (uint32_t)sz.columns;
        const ScanLayout scan(columns, nav.scan.p);   // the tiles are the columns, their totals the span counts
        int *flag = (int *)nav.ctl.p;
        const float *grid = (const float *)ctx->terrain.p;
        const dim3 walk = walk_grid(tb);
        VTMC_HIP(ctx, hipMemsetAsync(flag, 0, kNavCtlWords * sizeof(int), s));
        VTMC_HIP(ctx, clock.mark(0, s));
        VTMC_HIP(ctx, launch(nav_walk_kernel<false>, walk, dim3(64, 4, 1), 0, s, grid, sh, tb, (int)params->agent_height, scan.tile_totals(), nullptr, nullptr,
                             nullptr, nullptr, 0));
        VTMC_HIP(ctx, clock.mark(1, s));
        VTMC_HIP(ctx, launch_scan(scan, s));
        VTMC_HIP(ctx, nav_launch_offsets(scan, offsets, s));
        VTMC_HIP(ctx, clock.mark(2, s));
        VTMC_HIP(ctx, hipMemcpyAsync(&total, scan.total(), sizeof(total), hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        if (!nav_total_fits(total, params->max_spans))
            return fail(ctx, VTMC_ERR_TOO_LARGE, "terrain_nav_build: %llu spans exceed max_spans %d", total, params->max_spans);
        const int32_t n = (int32_t)total;
        if (n > 0) {
            if (int rc = ensure(ctx, nav.spans, nav_span_bytes(n))) return rc;
            if (int rc = ensure(ctx, nav.scratch, nav_scratch_bytes(n))) return rc;
        }
        vtmc_nav_span *spans = (vtmc_nav_span *)nav.spans.p;
        int32_t *col_of = (int32_t *)nav.scratch.p, *parent = col_of + n;
        VTMC_HIP(ctx, clock.mark(3, s));
        if (n > 0) VTMC_HIP(ctx, launch(nav_walk_kernel<true>, walk, dim3(64, 4, 1), 0, s, grid, sh, tb, (int)params->agent_height, nullptr, offsets, spans, col_of, parent, n));
        VTMC_HIP(ctx, clock.mark(4, s));
        if (n > 0) VTMC_HIP(ctx, launch(nav_link_kernel, lanes256(n), dim3(256), 0, s, spans, col_of, offsets, flag, tb, n, (int)params->agent_height, params->max_step));
        nav.rounds = 0;
        if (n > 0) {
            if (int rc = nav_label_regions(ctx, "terrain_nav_build", spans, parent, n, true, &nav.rounds)) return rc;
            clock.arm();
        }
    }
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nav.n = (int32_t)total;
    for (int k = 0; k < 3; ++k) nav.lo[k] = nb.lo[k], nav.d[k] = nb.d[k];
    nav.valid = true;
    if (n_spans) *n_spans = nav.n;
    return VTMC_OK;
}

int32_t vtmc_nav_read(vtmc_ctx *ctx, vtmc_nav_span *dst, int32_t capacity, int32_t *column_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_read before terrain_nav_build");
    if (capacity < nav.n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d spans", capacity, nav.n);
    if (nav.n > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (nav.n > 0) VTMC_HIP(ctx, hipMemcpy(dst, nav.spans.p, nav_span_bytes(nav.n), hipMemcpyDeviceToHost));
    if (column_offsets) VTMC_HIP(ctx, hipMemcpy(column_offsets, nav.offsets.p, nav_sizes(nav_held_box(nav)).offsets_bytes, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_nav_info(const vtmc_ctx *ctx, int32_t box_lo[3], int32_t box_dims[3], int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_NO_RESULT, "nav_info before terrain_nav_build");
    for (int k = 0; k < 3; ++k) {
        if (box_lo) box_lo[k] = nav.lo[k];
        if (box_dims) box_dims[k] = nav.d[k];
    }
    if (n_spans) *n_spans = nav.n;
    return VTMC_OK;
}

int32_t vtmc_nav_device_results(vtmc_ctx *ctx, const vtmc_nav_span **d_spans, const int32_t **d_column_offsets, int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_device_results before terrain_nav_build");
    if (d_spans) *d_spans = (const vtmc_nav_span *)nav.spans.p;
    if (d_column_offsets) *d_column_offsets = (const int32_t *)nav.offsets.p;
    if (n_spans) *n_spans = nav.n;
    return VTMC_OK;
}

// Not part of the ABI (tools/nav_bench.py): device time of the last vtmc_terrain_nav_build that made spans, ms[0..6] = the count walk, the
// scan with the offsets, the emit walk, the links, and the first round's unions, flatten and verify; ms[7] = the rounds it took.
int32_t vtmc_debug_nav_ms(vtmc_ctx *ctx, float ms[8])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->nav.valid || !ctx->nav_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_nav_ms before a nav build that launched kernels");
    if (int rc = ctx->nav_clock.sync_last(ctx)) return rc;
    static const int pairs[7][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}};
    ms[7] = (float)ctx->nav.rounds;
    for (int i = 0; i < 7; ++i)
        if (int rc = ctx->nav_clock.elapsed(ctx, pairs[i][0], pairs[i][1], &ms[i])) return rc;
    return VTMC_OK;
}

// Not part of the ABI (tools/nav_bench.py): device time of a plain read of the box of lower / upper in the walk's own layout, the median
// of `reps` launches after one warm-up.  Uses the scan buffer of the nav build as its sink; the nav result the context holds stays.
int32_t vtmc_debug_nav_box_read_ms(vtmc_ctx *ctx, const float lower[3], const float upper[3], int32_t reps, float *ms)
{
    if (!ctx || !lower || !upper || !ms || reps < 1 || reps > 64) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_nav_box_read_ms before terrain_init");
    const TerrainBox tb = bounds_box(ctx->tshape, lower, upper);
    const int32_t first[3] = {tb.lx, tb.ly, tb.lz}, dims[3] = {tb.dx, tb.dy, tb.dz};
    const NavBox nb = nav_box(first, dims);
    const NavSizes sz = nav_sizes(nb);
    if (nav_box_empty(nb) || !sz.launchable) return fail(ctx, VTMC_ERR_INVALID_ARG, "debug_nav_box_read_ms: an empty box");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = ensure(ctx, ctx->nav.scan, sz.scan_bytes)) return rc;
    StageClock<9> &clock = ctx->nav_clock;
    VTMC_HIP(ctx, clock.begin());   // borrowed, and left disarmed: its events no longer hold the build's times
    uint32_t *sink = ScanLayout((uint64_t)sz.columns, ctx->nav.scan.p).tile_totals();   // a word per column
    float t[64];
    for (int i = -1; i < reps; ++i) {
        VTMC_HIP(ctx, clock.mark(0, s));
        VTMC_HIP(ctx, launch(nav_read_kernel, walk_grid(tb), dim3(64, 4, 1), 0, s, (const float *)ctx->terrain.p, ctx->tshape, tb, sink));
        VTMC_HIP(ctx, clock.mark(1, s));
        VTMC_HIP(ctx, hipEventSynchronize(clock.event(1)));
        if (i >= 0)
            if (int rc = clock.elapsed(ctx, 0, 1, &t[i])) return rc;
    }
    std::sort(t, t + reps);
    *ms = t[reps / 2];
    return VTMC_OK;
}

}  // extern "C"
