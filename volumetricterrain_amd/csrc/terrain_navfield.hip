// terrain_navfield.hip -- flow fields on the navigation layer (include/vtmc_navfield.h): which span a world position stands on, every
// span's cheapest cost to the nearest goal with the span to step to next, and the paths that gives.  Not in the reference.  The rule,
// operation by operation, is NAVFIELD in include/vtmc_navfield.h; the kernels follow it bit for bit (integer costs have one fixed point, so
// the order of the relaxation does not show).  The host half -- the edge cost, the argument checks, the goal validation, the sizes -- is
// terrain_navfield.h.  Works on the nav result the context holds and never reads the grid.  Hand-written for gfx950 / CDNA4.
//
//   1. navfield_init_kernel    a lane per span: the four edge costs, once, into 16 bytes per span; the cost D and the cheapest goal cost of
//                              every span to UNREACHED.  navfield_goals_kernel scatters the goals into both with atomicMin.
//   2. navfield_relax_kernel   the hot path, a pull: a span reads D of its up to four out-links and keeps the minimum.  A workgroup owns a
//                              RUN of kNavFieldRun (4096) consecutive spans, four per lane: a few rows of the largest box, since with a run
//                              shorter than a row a cost crosses one row per round (profiles/r22/navfield: 1024 took 2.8 times the rounds
//                              and twice the time at 1024^3, and was no faster on small fields).  It reads their D into LDS, folds in the links that
//                              leave the run (read from global memory once, at the start), and then sweeps the run in LDS until a sweep
//                              changes nothing in it, at most run-length times; a span that came out lower is written back.  Spans are
//                              ordered by column with x fastest, so the +-x links stay in the run and a launch carries a cost along a whole
//                              stretch of a row, not one hop.  Nothing but a span's own lane writes its word and values only fall, so a stale
//                              read of another workgroup's word (they are relaxed agent-scope loads; no fence is needed or used) costs a
//                              round at worst and never the result.  A ROUND is one launch over all runs; a workgroup that lowered anything
//                              sets the round's flag word.  The host launches kNavFieldBatch rounds per read-back of the flags, and the first
//                              round that changed nothing ends the build: every run was at its fixed point against what the round began with,
//                              which nobody changed.  Rounds are bounded by n + 1.
//   3. navfield_next_kernel    a lane per span, after convergence: next by the rule (a goal whose cost stands wins; else the smallest k that
//                              explains D), the cell, and the reached count, reduced per wave by ballot before the atomic.
//   nav_locate_kernel          a lane per position: the column, then its few spans by the rule.
//   navfield_trace_kernel      a lane per start: follows next for at most max_len entries; a next outside 0..n-1 ends the row.
// Every random-access read is bounded by the span count or the box's columns and every loop by a count.
//
// Edge costs: computed once, not per round.  Recomputing needs, per span and round, the 32-byte record plus the heights of four
// neighbours, two of which (the +-z ones) lie in other rows: two more 32-byte sectors at the least, some 100 bytes.  Kept, a round reads
// the record for its links and 16 coalesced bytes of costs: 48 bytes.  A field takes tens to hundreds of rounds, so the one pass that
// writes 16 bytes per span is repaid in the first round.
#include "surface_query.h"
#include "terrain_navfield.h"
#include <algorithm>
#include <cstring>

namespace vtmc {

static_assert(sizeof(vtmc_navfield_cell) == 8 && sizeof(vtmc_navfield_goal) == 8 && sizeof(vtmc_navfield_params) == 16, "include/vtmc_navfield.h");
constexpr int kNavFieldItems = 4;   // spans of a run per lane: a workgroup is a quarter of its run's length in lanes
constexpr int kNavFieldThreads = kNavFieldRun / kNavFieldItems;
static_assert(kNavFieldRun % (64 * kNavFieldItems) == 0 && kNavFieldRun >= 256 && kNavFieldThreads <= 1024, "a run is whole waves' worth of spans, and its lanes one workgroup");
enum { kNavFieldCtlReached = kNavFieldBatch, kNavFieldCtlWords = kNavFieldBatch + 1 };   // the control words: a flag per round of a batch, the count
constexpr uint32_t kUnreached = VTMC_NAVFIELD_UNREACHED;

__device__ __forceinline__ uint32_t cost_of(const uint4 &c, int k) { return k == 0 ? c.x : k == 1 ? c.y : k == 2 ? c.z : c.w; }

// Pass 1: the edge costs of a span's four links (0 where there is none), and both of its words to UNREACHED
__global__ __launch_bounds__(256) void navfield_init_kernel(const vtmc_nav_span *__restrict__ spans, uint4 *__restrict__ costs, uint32_t *__restrict__ D,
                                                           uint32_t *__restrict__ goal_cost, int32_t n, float climb_cost, float drop_cost)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const float hs = spans[s].height;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = spans[s].link[k];
        c[k] = l >= 0 && l < n ? navfield_edge_cost(hs, spans[l].height, climb_cost, drop_cost) : 0u;
    }
    costs[s] = make_uint4(c[0], c[1], c[2], c[3]);
    D[s] = kUnreached;
    goal_cost[s] = kUnreached;
}

__global__ __launch_bounds__(256) void navfield_goals_kernel(const vtmc_navfield_goal *__restrict__ goals, int32_t n_goals, uint32_t *__restrict__ D,
                                                            uint32_t *__restrict__ goal_cost, int32_t n)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_goals) return;
    const int s = goals[g].span;
    if (s < 0 || s >= n) return;   // the host has checked; keeps the atomics inside the buffers whatever the record says
    atomicMin(&D[s], goals[g].cost);
    atomicMin(&goal_cost[s], goals[g].cost);
}

// Pass 2, one round.  D is read and written; *flag is set when any span of any run came out lower.
__global__ __launch_bounds__(kNavFieldThreads) void navfield_relax_kernel(const vtmc_nav_span *__restrict__ spans, const uint4 *__restrict__ costs, uint32_t *D,
                                                                         int32_t n, uint32_t max_cost, int *__restrict__ flag)
{
    __shared__ uint32_t d[kNavFieldRun];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kNavFieldRun;
    int local[kNavFieldItems][4];       // the link as a position in the run, or -1: no link, or one that left the run and is folded in already
    uint32_t cost[kNavFieldItems][4];
    uint32_t before[kNavFieldItems];
#pragma unroll
    for (int j = 0; j < kNavFieldItems; ++j) {
        const int pos = j * kNavFieldThreads + tid;
        const int64_t s = base + pos;
        uint32_t best = kUnreached;
        before[j] = kUnreached;
#pragma unroll
        for (int k = 0; k < 4; ++k) local[j][k] = -1, cost[j][k] = 0u;
        if (s < n) {
            best = before[j] = D[s];
            const uint4 c = costs[s];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l = spans[s].link[k];
                if (l < 0 || l >= n) continue;
                if (l >= base && l < base + kNavFieldRun) {
                    local[j][k] = (int)(l - base), cost[j][k] = cost_of(c, k);
                    continue;
                }
                const uint32_t dt = __hip_atomic_load(&D[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (dt == kUnreached) continue;
                const uint32_t cand = dt + cost_of(c, k);   // dt <= max_cost < 2^31 and a cost is below 2^21: no wrap
                if (cand <= max_cost && cand < best) best = cand;
            }
        }
        d[pos] = best;
    }
    __syncthreads();
    // the sweeps: a lane reads what the others have written so far, in this sweep or the last; either is a valid upper bound of the
    // fixed point, so the order does not matter.  One barrier per sweep, which also takes the vote.
    for (int sweep = 0; sweep < kNavFieldRun; ++sweep) {
        int lowered = 0;
#pragma unroll
        for (int j = 0; j < kNavFieldItems; ++j) {
            const int pos = j * kNavFieldThreads + tid;
            const uint32_t cur = d[pos];
            uint32_t best = cur;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (local[j][k] < 0) continue;
                const uint32_t dt = d[local[j][k]];
                if (dt == kUnreached) continue;
                const uint32_t cand = dt + cost[j][k];
                if (cand <= max_cost && cand < best) best = cand;
            }
            if (best < cur) d[pos] = best, lowered = 1;
        }
        if (!__syncthreads_or(lowered)) break;
    }
    bool changed = false;
#pragma unroll
    for (int j = 0; j < kNavFieldItems; ++j) {
        const int pos = j * kNavFieldThreads + tid;
        const int64_t s = base + pos;
        if (s < n && d[pos] < before[j]) {
            __hip_atomic_store(&D[s], d[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            changed = true;
        }
    }
    if (__ballot(changed) && __lane_id() == 0) atomicOr(flag, 1);
}

// Pass 3: next, the cell and the reached count
__global__ __launch_bounds__(256) void navfield_next_kernel(const vtmc_nav_span *__restrict__ spans, const uint4 *__restrict__ costs, const uint32_t *__restrict__ D,
                                                           const uint32_t *__restrict__ goal_cost, vtmc_navfield_cell *__restrict__ cells, int32_t n,
                                                           int *__restrict__ reached)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    bool is_reached = false;
    if (s < n) {
        const uint32_t dv = D[s];
        int next = -1;
        if (dv != kUnreached) {
            is_reached = true;
            if (goal_cost[s] != dv) {   // not arrived: the smallest k that explains D
                const uint4 c = costs[s];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int l = spans[s].link[k];
                    if (next >= 0 || l < 0 || l >= n) continue;
                    const uint32_t dt = D[l];
                    if (dt != kUnreached && dt + cost_of(c, k) == dv) next = l;
                }
            }
        }
        vtmc_navfield_cell cell;
        cell.cost = dv, cell.next = next;
        cells[s] = cell;
    }
    const unsigned long long m = __ballot(is_reached);
    if (m && __lane_id() == 0) atomicAdd(reached, __popcll(m));
}

struct NavLocateBox {
    float origin[3], scale;
    int lox, loz, dx, dz;
};

__global__ __launch_bounds__(256) void nav_locate_kernel(const float *__restrict__ positions, int32_t n, NavLocateBox b, const int32_t *__restrict__ offsets,
                                                        const vtmc_nav_span *__restrict__ spans, int32_t n_spans, float below, float above,
                                                        int32_t *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float px = positions[3 * (size_t)i], py = positions[3 * (size_t)i + 1], pz = positions[3 * (size_t)i + 2];
    int answer = -1;
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
        const float gx = (px - b.origin[0]) / b.scale, gy = (py - b.origin[1]) / b.scale, gz = (pz - b.origin[2]) / b.scale;
        const float fx = floorf(gx + 0.5f), fz = floorf(gz + 0.5f);
        // compared as floats (a box holds at most 1026 columns per axis: exact), so the conversions below are of small integers
        if (fx >= (float)b.lox && fx <= (float)(b.lox + b.dx - 1) && fz >= (float)b.loz && fz <= (float)(b.loz + b.dz - 1)) {
            const int ix = (int)fx - b.lox, iz = (int)fz - b.loz;
            const int c = ix + b.dx * iz;
            int lo = offsets[c], hi = offsets[c + 1];
            if (lo < 0) lo = 0;
            if (hi > n_spans) hi = n_spans;
            float best = 0.0f;
            for (int s = lo; s < hi; ++s) {
                const float e = gy - spans[s].height;
                if (!(-below <= e && e <= above)) continue;
                const float ae = fabsf(e);
                if (answer < 0 || ae < best) answer = s, best = ae;
            }
        }
    }
    out[i] = answer;
}

// the rows are -1 already
__global__ __launch_bounds__(256) void navfield_trace_kernel(const vtmc_navfield_cell *__restrict__ cells, int32_t n, const int32_t *__restrict__ starts,
                                                            int32_t n_starts, int32_t max_len, int32_t *__restrict__ paths, int32_t *__restrict__ lengths)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_starts) return;
    int s = starts[i], len = 0;
    int32_t *row = paths + (size_t)i * (size_t)max_len;
    if (s >= 0 && s < n && cells[s].cost != kUnreached) {
        while (len < max_len) {
            row[len++] = s;
            const int next = cells[s].next;
            if (next < 0 || next >= n) break;
            s = next;
        }
    }
    lengths[i] = len;
}

int trace_rows_stage(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, TraceRows *rows)
{
    const float *const src[3] = {(const float *)starts, nullptr, nullptr};
    const size_t bytes[3] = {(size_t)n_starts * 4u, 0, 0};
    rows->path_bytes = navfield_path_bytes(n_starts, max_len), rows->length_bytes = (size_t)n_starts * 4u;
    QueryStage st;   // the answers: the rows, then the lengths
    if (int rc = stage_queries(ctx, src, bytes, rows->path_bytes + rows->length_bytes, &st)) return rc;
    rows->starts = (const int32_t *)st.in[0];
    rows->paths = (int32_t *)st.hits, rows->lengths = (int32_t *)((unsigned char *)st.hits + rows->path_bytes);
    rows->host_off = st.hit_off;
    return VTMC_OK;
}

int trace_rows_fetch(vtmc_ctx *ctx, const TraceRows &rows, int32_t *paths, int32_t *lengths)
{
    const unsigned char *h = ctx->h_rays.p + rows.host_off;
    VTMC_HIP(ctx, hipMemcpyAsync(ctx->h_rays.p + rows.host_off, rows.paths, rows.path_bytes + rows.length_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(paths, h, rows.path_bytes);
    memcpy(lengths, h + rows.path_bytes, rows.length_bytes);
    return VTMC_OK;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_nav_locate(vtmc_ctx *ctx, const float *positions, int32_t n, float below, float above, int32_t *spans_out)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "nav_locate before terrain_nav_build");
    if (const char *what = navfield_locate_fault(positions, n, below, above, spans_out)) return fail(ctx, VTMC_ERR_INVALID_ARG, "nav_locate: %s", what);
    if (n == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    const float *const src[3] = {positions, nullptr, nullptr};
    const size_t bytes[3] = {(size_t)n * 12u, 0, 0};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, (size_t)n * 4u, &st)) return rc;
    const TerrainShape &sh = ctx->tshape;
    const NavLocateBox b{{sh.origin[0], sh.origin[1], sh.origin[2]}, sh.scale, nav.lo[0], nav.lo[2], nav.d[0], nav.d[2]};
    VTMC_HIP(ctx, launch(nav_locate_kernel, lanes256(n), dim3(256), 0, s, st.in[0], n, b, (const int32_t *)nav.offsets.p, (const vtmc_nav_span *)nav.spans.p, nav.n,
                         below, above, (int32_t *)st.hits));
    return fetch_hits(ctx, st, spans_out);
}

int32_t vtmc_navfield_build(vtmc_ctx *ctx, const vtmc_navfield_goal *goals, int32_t n_goals, const vtmc_navfield_params *params, int32_t *n_reached)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_reached) *n_reached = 0;
    const VtmcNav &nav = ctx->nav;
    if (!nav.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navfield_build before terrain_nav_build");
    if (const char *what = navfield_params_fault(params)) return fail(ctx, VTMC_ERR_INVALID_ARG, "navfield_build: %s", what);
    int32_t at = -1;
    if (const char *what = navfield_goals_fault(goals, n_goals, nav.n, params->max_cost, &at))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "navfield_build: %s (goal %d, %d spans)", what, at, nav.n);
    const int32_t n = nav.n;   // > 0: a goal lies in 0..n-1
    VtmcNavField &nf = ctx->navfield;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nf.valid = false;   // from here on the buffers no longer hold the previous field
    StageClock<4> &clock = ctx->navfield_clock;
    if (int rc = ensure(ctx, nf.cells, navfield_cell_bytes(n))) return rc;
    if (int rc = ensure(ctx, nf.work, navfield_work_bytes(n))) return rc;
    if (int rc = ensure(ctx, nf.ctl, kNavFieldCtlWords * sizeof(int))) return rc;
    VTMC_HIP(ctx, clock.begin());
    const float *const src[3] = {(const float *)goals, nullptr, nullptr};
    const size_t bytes[3] = {(size_t)n_goals * sizeof(vtmc_navfield_goal), 0, 0};
    QueryStage st;
    if (int rc = stage_queries(ctx, src, bytes, 0, &st)) return rc;
    const vtmc_nav_span *spans = (const vtmc_nav_span *)nav.spans.p;
    uint4 *costs = (uint4 *)nf.work.p;   // then D, then the cheapest goal cost
    uint32_t *D = (uint32_t *)(costs + n), *goal_cost = D + n;
    int *ctl = (int *)nf.ctl.p;
    VTMC_HIP(ctx, clock.mark(0, s));
    VTMC_HIP(ctx, launch(navfield_init_kernel, lanes256(n), dim3(256), 0, s, spans, costs, D, goal_cost, n, params->climb_cost, params->drop_cost));
    VTMC_HIP(ctx, launch(navfield_goals_kernel, lanes256(n_goals), dim3(256), 0, s, (const vtmc_navfield_goal *)st.in[0], n_goals, D, goal_cost, n));
    VTMC_HIP(ctx, clock.mark(1, s));
    // the rounds, a batch per read-back; the first one that changed nothing is the last one counted
    const int64_t most = navfield_max_rounds(n);
    const dim3 runs((unsigned)navfield_runs(n));
    int64_t rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= most) return fail(ctx, VTMC_ERR_DEVICE, "navfield_build: relaxation did not converge (%lld rounds over %d spans)", (long long)rounds, n);
        const int batch = (int)std::min<int64_t>(kNavFieldBatch, most - rounds);
        VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kNavFieldBatch * sizeof(int), s));
        for (int b = 0; b < batch; ++b) VTMC_HIP(ctx, launch(navfield_relax_kernel, runs, dim3(kNavFieldThreads), 0, s, spans, costs, D, n, params->max_cost, ctl + b));
        int h_flags[kNavFieldBatch] = {};
        VTMC_HIP(ctx, hipMemcpyAsync(h_flags, ctl, sizeof h_flags, hipMemcpyDeviceToHost, s));
        VTMC_HIP(ctx, hipStreamSynchronize(s));
        for (int b = 0; b < batch && !done; ++b) {
            ++rounds;
            done = h_flags[b] == 0;
        }
    }
    VTMC_HIP(ctx, hipMemsetAsync(ctl + kNavFieldCtlReached, 0, sizeof(int), s));
    VTMC_HIP(ctx, clock.mark(2, s));
    VTMC_HIP(ctx, launch(navfield_next_kernel, lanes256(n), dim3(256), 0, s, spans, costs, D, goal_cost, (vtmc_navfield_cell *)nf.cells.p, n, ctl + kNavFieldCtlReached));
    VTMC_HIP(ctx, clock.mark(3, s));
    int reached = 0;
    VTMC_HIP(ctx, hipMemcpyAsync(&reached, ctl + kNavFieldCtlReached, sizeof reached, hipMemcpyDeviceToHost, s));
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    nf.n = n, nf.reached = reached, nf.rounds = (int32_t)rounds;
    nf.valid = true;
    clock.arm();
    if (n_reached) *n_reached = reached;
    return VTMC_OK;
}

int32_t vtmc_navfield_read(vtmc_ctx *ctx, vtmc_navfield_cell *dst, int32_t capacity)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navfield_read before navfield_build");
    if (capacity < nf.n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d cells", capacity, nf.n);
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipMemcpy(dst, nf.cells.p, navfield_cell_bytes(nf.n), hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int32_t vtmc_navfield_info(const vtmc_ctx *ctx, int32_t *n_spans, int32_t *n_reached, int32_t *rounds)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_NO_RESULT, "navfield_info before navfield_build");
    if (n_spans) *n_spans = nf.n;
    if (n_reached) *n_reached = nf.reached;
    if (rounds) *rounds = nf.rounds;
    return VTMC_OK;
}

int32_t vtmc_navfield_device_results(vtmc_ctx *ctx, const vtmc_navfield_cell **d_cells, int32_t *n_spans)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navfield_device_results before navfield_build");
    if (d_cells) *d_cells = (const vtmc_navfield_cell *)nf.cells.p;
    if (n_spans) *n_spans = nf.n;
    return VTMC_OK;
}

int32_t vtmc_navfield_trace(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, int32_t *paths, int32_t *lengths)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcNavField &nf = ctx->navfield;
    if (!nf.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "navfield_trace before navfield_build");
    int32_t at = -1;
    if (const char *what = navfield_trace_fault(starts, n_starts, max_len, paths, lengths, nf.n, &at))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "navfield_trace: %s (start %d, %d spans)", what, at, nf.n);
    if (n_starts == 0) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    TraceRows rows;
    if (int rc = trace_rows_stage(ctx, starts, n_starts, max_len, &rows)) return rc;
    VTMC_HIP(ctx, hipMemsetAsync(rows.paths, 0xff, rows.path_bytes, s));
    VTMC_HIP(ctx, launch(navfield_trace_kernel, lanes256(n_starts), dim3(256), 0, s, (const vtmc_navfield_cell *)nf.cells.p, nf.n, rows.starts, n_starts, max_len,
                         rows.paths, rows.lengths));
    return trace_rows_fetch(ctx, rows, paths, lengths);
}

// Not part of the ABI (tools/navfield_bench.py): device time of the last vtmc_navfield_build, ms[0..2] = the edge costs with the goals, the
// rounds (the host's read-backs between the batches included: the stream idles while the host looks at the flags), next with the count;
// ms[3] = the rounds it took.
int32_t vtmc_debug_navfield_ms(vtmc_ctx *ctx, float ms[4])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->navfield.valid || !ctx->navfield_clock.armed) return fail(ctx, VTMC_ERR_NO_RESULT, "debug_navfield_ms before navfield_build");
    if (int rc = ctx->navfield_clock.sync_last(ctx)) return rc;
    for (int i = 0; i < 3; ++i)
        if (int rc = ctx->navfield_clock.elapsed(ctx, i, i + 1, &ms[i])) return rc;
    ms[3] = (float)ctx->navfield.rounds;
    return VTMC_OK;
}

}  // extern "C"
