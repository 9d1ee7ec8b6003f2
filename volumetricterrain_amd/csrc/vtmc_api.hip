// vtmc_api.hip -- the extract entry points of include/vtmc.h, the host-side control flow that VoxelTerrain.BatchUpdate performs around
// its three dispatches (reference: Unity-Project/Assets/Scripts/VoxelTerrain.cs:330-477) and the result readers.  The context: context.hip.
//
// Differences from the reference's control flow, by design:
//  * there is no mid-pipeline read-back (VoxelTerrain.cs:394-395): classify -> scan -> emit are
//    queued back to back, {T, nActive} live in device memory, and the host reads T once at the end;
//    the emit kernel itself refuses to run past the triangle buffer's capacity, in which case the
//    buffer is grown and only the emit stage is queued again.
#include "vtmc_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>

using namespace vtmc;
typedef VtmcDevBuf DevBuf;

namespace {
// pinned tile staging a context keeps between dirty-list calls; anything larger is given back by the next small call
constexpr size_t kStageKeepBytes = (size_t)32 << 20;
constexpr int kStageTrimAfter = 8;   // an over-sized staging buffer goes after this many consecutive small calls: a host that alternates a big brush with small edits keeps it

// One launch of the emit stage on the pending extract's stream, followed by the asynchronous copy of
// the scan's totals into pinned memory.  The kernel itself refuses to run past its buffers' capacity
// (it compares the device-resident T / V with the capacities it is handed).
int queue_emit(vtmc_ctx *ctx, bool retry)
{
    const VtmcPending &pe = ctx->pending;
    hipStream_t stream = pe.stream;
    const bool indexed = pe.indexed;
    const size_t tcap = std::min<size_t>(indexed ? ctx->indices.bytes / (3 * sizeof(int32_t)) : ctx->tris.bytes / sizeof(vtmc_triangle), 0x7fffffffu);
    const size_t vcap = indexed ? std::min<size_t>(ctx->verts.bytes / sizeof(vtmc_vertex), 0x7fffffffu) : 0;
    ctx->pending.tcap = tcap;
    ctx->pending.vcap = vcap;
    uint32_t *queue = (uint32_t *)ctx->totals.p + 64;
    if (retry)   // the scan cleared the ticket queue for the first launch
        VTMC_HIP(ctx, hipMemsetAsync(queue, 0, kQueueWords * sizeof(uint32_t), stream));
    uint32_t *vc = pe.n_volumes > 0 && !pe.counts_early ? (uint32_t *)ctx->volcounts.p : nullptr;   // else the scan has left them already
    Tuning tune = ctx->tune;
    if (ctx->comm && pe.counts_early && ctx->tune.gather_beside) tune.emit_spare_wgs = 8;   // vtmc_allgather_volume_counts runs its kernel beside this one
    if (indexed)
        VTMC_HIP(ctx, launch_emit_indexed(pe.sp, ctx->tables, (const uint32_t *)ctx->offsets.p, (const uint32_t *)ctx->voffsets.p,
                                          (const BlockDesc *)ctx->active.p, (const uint32_t *)ctx->totals.p, (const uint32_t *)ctx->vtotals.p,
                                          (uint32_t)tcap, (uint32_t)vcap, ctx->verts.p, ctx->indices.p, ctx->n_cus,
                                          tune, queue, vc, pe.n_volumes, stream));
    else
        VTMC_HIP(ctx, launch_emit(pe.sp, ctx->tables, (const uint32_t *)ctx->offsets.p, (const BlockDesc *)ctx->active.p,
                                  (const uint32_t *)ctx->totals.p, (uint32_t)tcap, ctx->tris.p,
                                  ctx->n_cus, tune, queue, vc, pe.n_volumes, stream));
    VTMC_HIP(ctx, hipEventRecord(ctx->ev[3], stream));
    return VTMC_OK;
}

// Queues the device side of BatchUpdate (VoxelTerrain.cs:365-427) -- classify -> scan -> emit -- on
// `stream` and returns without waiting: {T, nActive} (and V) stay in device memory, there is no
// mid-pipeline read-back (VoxelTerrain.cs:394-395).  extract_finish() completes the call.
int extract_queue(vtmc_ctx *ctx, const BlockSpace &sp, int n_volumes, ResultSource source, uint32_t flags, hipStream_t stream)
{
    const int B = sp.n_blocks;
    const bool indexed = ctx->output_mode == VTMC_OUTPUT_INDEXED;
    ctx->result.valid = false;
    ctx->pending = VtmcPending{};
    VtmcPending pe;
    pe.sp = sp;
    pe.n_volumes = n_volumes;
    pe.indexed = indexed;
    pe.source = source;
    pe.stream = stream;
    if (B == 0) {  // the reference's early exit (VoxelTerrain.cs:396-405): empty offsets, nothing launched
        if (int rc = ensure(ctx, ctx->offsets, sizeof(uint32_t))) return rc;
        VTMC_HIP(ctx, hipMemsetAsync(ctx->offsets.p, 0, sizeof(uint32_t), stream));
        if (indexed) {
            if (int rc = ensure(ctx, ctx->voffsets, sizeof(uint32_t))) return rc;
            VTMC_HIP(ctx, hipMemsetAsync(ctx->voffsets.p, 0, sizeof(uint32_t), stream));
        }
        pe.active = true;
        ctx->pending = pe;
        return VTMC_OK;
    }
    // the emit kernel addresses a tile with 32-bit byte offsets from the block origin
    if ((9.0 * ((double)sp.sx + (double)sp.sy + (double)sp.sz) + 1.0) * 4.0 >= 4294967296.0)
        return fail(ctx, VTMC_ERR_TOO_LARGE, "strides too large: a 10x10x10 tile must span less than 4 GiB");
    if (int rc = ensure(ctx, ctx->offsets, sizeof(uint32_t) * ((size_t)B + 1))) return rc;
    if (int rc = ensure(ctx, ctx->volcounts, sizeof(uint32_t) * 2 * (size_t)std::max(n_volumes, 1))) return rc;
    if (!indexed && !ctx->tris.p) {
        if (int rc = ensure(ctx, ctx->tris, sizeof(vtmc_triangle) * ((size_t)1 << 20))) return rc;
        ctx->place_pending = true;
    }
    if (int rc = ensure(ctx, ctx->counts, sizeof(uint32_t) * (size_t)B)) return rc;
    if (int rc = ensure(ctx, ctx->active, sizeof(BlockDesc) * (size_t)B)) return rc;   // one record per non-empty block, written by the scan
    if (B >= (1 << 30)) return fail(ctx, VTMC_ERR_TOO_LARGE, "more than 2^30 blocks in one batch");   // the scan's status word holds 30 bits of non-empty blocks
    const size_t ctrl_words = scan_ctrl_words(B);
    if (int rc = ensure(ctx, ctx->partials, sizeof(unsigned long long) * 2 * ctrl_words)) return rc;   // ticket, error word, one or two status words per tile
    if (int rc = ensure(ctx, ctx->totals, sizeof(uint32_t) * (64 + kQueueWords))) return rc;  // scan totals, then the emit kernel's ticket counters
    uint8_t *d_cases = nullptr;
    if (flags & VTMC_FLAG_WANT_CASES) {
        if (int rc = ensure(ctx, ctx->cases, (size_t)B * 512)) return rc;
        d_cases = (uint8_t *)ctx->cases.p;
    }
    uint32_t *d_vcounts = nullptr;
    if (indexed) {
        if (int rc = ensure(ctx, ctx->vcounts, sizeof(uint32_t) * (size_t)B)) return rc;
        if (int rc = ensure(ctx, ctx->voffsets, sizeof(uint32_t) * ((size_t)B + 1))) return rc;
        if (int rc = ensure(ctx, ctx->vtotals, sizeof(uint32_t) * 64)) return rc;
        if (!ctx->verts.p) {
            if (int rc = ensure(ctx, ctx->verts, sizeof(vtmc_vertex) * ((size_t)1 << 19))) return rc;
            ctx->place_pending = true;
        }
        if (!ctx->indices.p) {
            if (int rc = ensure(ctx, ctx->indices, sizeof(int32_t) * 3 * ((size_t)1 << 20))) return rc;
            ctx->place_pending = true;
        }
        d_vcounts = (uint32_t *)ctx->vcounts.p;
    }
    // the streaming classify wants 32+ cells along the stride-1 axis: x, or z for the C# float[,,] order
    const bool dense = !sp.list && !(flags & (VTMC_FLAG_WANT_CASES | VTMC_FLAG_NO_DENSE_PATH)) &&
                       ((sp.sx == 1 && sp.nx >= 32) || (sp.sx != 1 && sp.sz == 1 && sp.nbz * 8 >= 32));

    ctx->h_totals.p[8] = 0u;   // the scan's look-back time-out word
    unsigned long long *ctrl = (unsigned long long *)ctx->partials.p;
    const int n_ctrl = (int)(ctrl_words * (indexed ? 2 : 1));
    VTMC_HIP(ctx, hipEventRecord(ctx->ev[0], stream));
    SignVolume sg;   // classify from the sampler's sign bits when they describe exactly this buffer (the caller vouches it is unmodified)
    {
        const auto &so = ctx->sign_of;
        if (dense && sp.sx == 1 && ctx->tune.fill_keeps_signs && so.valid && sp.base == so.d_out && sp.sy == so.dx && sp.sz == (long long)so.dx * so.dy &&
            sp.nx == so.dx - 2 && sp.nby * 8 == so.dy - 2 && sp.nbz * 8 == so.dz - 2 && (sp.sv == so.sv || n_volumes <= 1) &&
            sp.n_blocks / sp.bpv <= so.n_volumes) {
            sg.words = (const unsigned long long *)ctx->signs.p;
            sg.plane_words = density_sign_plane_words(so.dx, so.dy);
            sg.dx = so.dx;
            sg.dz = so.dz;
        }
    }
    if (dense) VTMC_HIP(ctx, launch_classify_dense(sp, ctx->tables, (uint32_t *)ctx->counts.p, d_vcounts, ctx->tune.classify_ablate, ctx->tune.classify_wgs_per_cu, ctrl, n_ctrl, sg, stream));
    else VTMC_HIP(ctx, launch_classify_blocks(sp, ctx->tables, (uint32_t *)ctx->counts.p, d_cases, d_vcounts, ctx->n_cus, ctrl, n_ctrl, stream));
    if (ctx->tune.stage_events) VTMC_HIP(ctx, hipEventRecord(ctx->ev[1], stream));
    // one launch: offsets, active list, totals (also straight into the host's pinned words), emit queue cleared; the indexed
    // output's vertex counts ride along, and so do the per-volume counts when every volume is a whole number of scan tiles
    pe.counts_early = n_volumes > 0 && scan_writes_volume_counts(sp.bpv) && (long long)sp.bpv * n_volumes == (long long)B;
    VTMC_HIP(ctx, launch_scan_fused(sp, (const uint32_t *)ctx->counts.p, B, (uint32_t *)ctx->offsets.p, (BlockDesc *)ctx->active.p, ctrl,
                                    (uint32_t *)ctx->totals.p, ctx->h_totals_dev, (uint32_t *)ctx->totals.p + 64, kQueueWords, d_vcounts,
                                    indexed ? (uint32_t *)ctx->voffsets.p : nullptr, indexed ? (uint32_t *)ctx->vtotals.p : nullptr,
                                    pe.counts_early ? (uint32_t *)ctx->volcounts.p : nullptr, sp.bpv, stream));
    if (ctx->tune.stage_events || (ctx->comm && pe.counts_early)) {
        VTMC_HIP(ctx, hipEventRecord(ctx->ev[2], stream));
        pe.scan_event = true;
    }
    pe.active = true;
    pe.launched = true;
    ctx->pending = pe;
    const int rc = queue_emit(ctx, false);
    if (rc) ctx->pending = VtmcPending{};   // nothing to finish: ev[3] was never recorded for this extract
    return rc;
}

// OUTPUT PLACEMENT (tuning key place_outputs = K > 1; round 6).  The emit kernel's time is a property of the pair (input field's allocation,
// output buffers' allocation): the identical kernel on the identical input runs 0.86 / 0.91 / 0.96 / 1.00 ms by which allocation it writes
// (profiles/r06/placement_probe.txt; the slow levels are +10 % memory latency for the identical request stream).  Which bits decide it is not
// established, so the library does what an autotuner does: when the output buffers have just been (re)allocated -- the first extract of a
// context, a growth -- the emit stage of the extract at hand is run into K - 1 further allocations of the same size, each timed, and the
// fastest set is kept (the others are freed).  Every run writes the complete, identical result; the extract's own result is in whatever set
// is kept.  Cost: 2 (K - 1) emit launches, and K allocations of the output held at once while the trial runs, once per (re)allocation.
int place_outputs(vtmc_ctx *ctx)
{
    const VtmcPending &pe = ctx->pending;
    const int K = std::min(ctx->tune.place_outputs, 16);
    // the buffers the emit stage of this extract writes: the triangle records, or (indexed output) the index and vertex buffers
    DevBuf &A = pe.indexed ? ctx->indices : ctx->tris;
    DevBuf none;
    DevBuf &B = pe.indexed ? ctx->verts : none;
    struct Set { DevBuf a, b; float ms = 0.f; };
    hipEvent_t t0 = nullptr, t1 = nullptr;
    VTMC_HIP(ctx, hipEventCreate(&t0));
    VTMC_HIP(ctx, hipEventCreate(&t1));
    auto timed_emit = [&](float *ms) -> int {   // the emit stage into the context's current buffers, twice: the second run's time counts
        for (int rep = 0; rep < 2; ++rep) {
            VTMC_HIP(ctx, hipEventRecord(t0, pe.stream));
            if (int rc = queue_emit(ctx, true)) return rc;
            VTMC_HIP(ctx, hipEventRecord(t1, pe.stream));
            VTMC_HIP(ctx, hipEventSynchronize(t1));
            VTMC_HIP(ctx, hipEventElapsedTime(ms, t0, t1));
        }
        return VTMC_OK;
    };
    auto take = [&](Set &st) { st.a = std::move(A); st.b = std::move(B); };
    ctx->place_n = 0;
    ctx->place_kept = 0;
    Set best;
    std::vector<Set> losers;   // held until the trial ends: an allocation made while the earlier ones are alive is another place in memory; one made
                               // after a loser was freed gets the loser's pages back (round 6's first form: runs of identical times)
    int rc = timed_emit(&best.ms);
    if (!rc) {
        ctx->place_ms[ctx->place_n++] = best.ms;
        take(best);
        for (int k = 1; k < K; ++k) {
            int e = ensure(ctx, A, best.a.bytes);
            if (!e && pe.indexed) e = ensure(ctx, B, best.b.bytes);
            Set cand;
            if (!e) e = timed_emit(&cand.ms);
            if (e) {   // out of memory, or a launch that failed: the trial ends here and the best so far stays
                quiet(hipStreamSynchronize(pe.stream));
                release(A);
                release(B);
                ctx->err.clear();
                break;
            }
            ctx->place_ms[ctx->place_n++] = cand.ms;
            take(cand);
            if (cand.ms < best.ms) {
                std::swap(cand, best);
                ctx->place_kept = k;
            }
            losers.push_back(std::move(cand));
        }
        losers.clear();
        A = std::move(best.a);
        B = std::move(best.b);
    }
    quiet(hipEventDestroy(t0));
    quiet(hipEventDestroy(t1));
    if (rc) return rc;
    VTMC_HIP(ctx, hipStreamSynchronize(pe.stream));   // the kept buffers hold a complete result (every candidate was emitted in full)
    return VTMC_OK;
}

// stage_ms[0..2] = classify, scan, emit (with stage_events = 1), [3] = the whole extract, from the events of the finished extract
int record_stage_ms(vtmc_ctx *ctx, bool placed)
{
    float a = 0, b = 0, c = 0;
    if (ctx->tune.stage_events) {
        VTMC_HIP(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
        VTMC_HIP(ctx, hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]));
        VTMC_HIP(ctx, hipEventElapsedTime(&c, ctx->ev[2], ctx->ev[3]));
    } else {
        VTMC_HIP(ctx, hipEventElapsedTime(&ctx->stage_ms[3], ctx->ev[0], ctx->ev[3]));
    }
    if (placed) c = ctx->place_ms[ctx->place_kept];   // ev[3] stands behind the last candidate's launch: this extract's emit stage is the kept candidate's run
    if (ctx->tune.stage_events || placed) ctx->stage_ms[3] = a + b + c;
    ctx->stage_ms[0] = a;
    ctx->stage_ms[1] = b;
    ctx->stage_ms[2] = c;
    return VTMC_OK;
}

// Completes a queued extract: waits for the stream, reads {T, V} from pinned memory and -- when the
// emit kernel found its buffers too small and did not run -- grows them (with head-room, so a slowly
// changing field does not regrow every frame) and queues only the emit stage again.
int extract_finish(vtmc_ctx *ctx, int64_t *tri_count)
{
    if (!ctx->pending.active) return fail(ctx, VTMC_ERR_NO_RESULT, "extract_finish without a queued extract");
    const VtmcPending pe = ctx->pending;
    int64_t T_found = 0, V_found = 0;
    if (!pe.launched) {
        memset(ctx->stage_ms, 0, sizeof ctx->stage_ms);
        VTMC_HIP(ctx, hipStreamSynchronize(pe.stream));
    } else {
        for (int attempt = 0;; ++attempt) {
            // the event behind the emit launch, not the whole stream: work queued behind the extract (the next batch's sampler,
            // a collective, the caller's own copies) keeps running while the host takes this result
            VTMC_HIP(ctx, hipEventSynchronize(ctx->ev[3]));
            if (ctx->h_totals.p[8]) {
                ctx->pending.active = false;
                return fail(ctx, VTMC_ERR_DEVICE, "scan: a look-back wait timed out (a predecessor tile never published)");
            }
            const uint64_t T = ((uint64_t)ctx->h_totals.p[3] << 32) | ctx->h_totals.p[2];
            const uint64_t V = pe.indexed ? (((uint64_t)ctx->h_totals.p[7] << 32) | ctx->h_totals.p[6]) : 0ull;
            if (T > 0x7fffffffull || V > 0x7fffffffull) {
                ctx->pending.active = false;
                return fail(ctx, VTMC_ERR_TOO_LARGE, "%llu triangles / %llu vertices exceed the int32 range of the ABI",
                            (unsigned long long)T, (unsigned long long)V);
            }
            T_found = (int64_t)T;
            V_found = (int64_t)V;
            if ((size_t)T <= ctx->pending.tcap && (size_t)V <= ctx->pending.vcap) break;
            if (attempt == 1) {
                ctx->pending.active = false;
                return fail(ctx, VTMC_ERR_DEVICE, "output buffers still too small after growing");
            }
            if ((size_t)T > ctx->pending.tcap) {
                const size_t want = (size_t)T + (size_t)T / 8 + 1024;
                if (int rc = pe.indexed ? ensure(ctx, ctx->indices, sizeof(int32_t) * 3 * want) : ensure(ctx, ctx->tris, sizeof(vtmc_triangle) * want)) return rc;
                ctx->place_pending = true;
            }
            if ((size_t)V > ctx->pending.vcap) {
                if (int rc = ensure(ctx, ctx->verts, sizeof(vtmc_vertex) * ((size_t)V + (size_t)V / 8 + 1024))) return rc;
                ctx->place_pending = true;
            }
            VTMC_HIP(ctx, hipEventRecord(ctx->ev[2], pe.stream));
            if (int rc = queue_emit(ctx, true)) return rc;
        }
        bool placed = false;
        if (ctx->place_pending && ctx->tune.place_outputs > 1 && T_found > 0) {
            if (int rc = place_outputs(ctx)) return rc;
            placed = ctx->place_n > 0;
        }
        ctx->place_pending = false;
        if (int rc = record_stage_ms(ctx, placed)) return rc;
    }
    ctx->pending.active = false;
    const uint32_t n_active = pe.launched ? ctx->h_totals.p[1] : 0u;   // the scan's count of non-empty blocks: the entries of `active`
    ctx->result = VtmcResult{true, ctx->result.epoch + 1, pe.source, pe.sp, pe.sp.n_blocks, n_active, pe.n_volumes, T_found, V_found, pe.indexed};
    if (tri_count) *tri_count = T_found;
    return VTMC_OK;
}

// upload the memory span a strided host grid occupies; returns device pointer in ctx->input
int upload_grid(vtmc_ctx *ctx, const float *grid, int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz)
{
    if (sx <= 0 || sy <= 0 || sz <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    const size_t span = (size_t)(nx + 1) * sx + (size_t)(ny + 1) * sy + (size_t)(nz + 1) * sz + 1;
    if (int rc = ensure(ctx, ctx->input, span * sizeof(float))) return rc;
    VTMC_HIP(ctx, hipMemcpyAsync(ctx->input.p, grid, span * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return VTMC_OK;
}

// the last result's per-block offsets (n_blocks + 1 words) into dst, when the caller asked for them
int copy_offsets(vtmc_ctx *ctx, int32_t *dst, const DevBuf &offsets)
{
    if (!dst) return VTMC_OK;
    if (ctx->result.blocks > 0) VTMC_HIP(ctx, hipMemcpy(dst, offsets.p, sizeof(uint32_t) * ((size_t)ctx->result.blocks + 1), hipMemcpyDeviceToHost));
    else dst[0] = 0;
    return VTMC_OK;
}

// Pinned staging of `bytes` of gathered tiles, or null (none to be had, or a huge dirty set: the caller takes the pageable route).  A
// larger one than kStageKeepBytes is trimmed back to it once kStageTrimAfter calls in a row were small (freeing and re-pinning tens of MB
// costs milliseconds and a device sync each way).
float *stage_buffer(vtmc_ctx *ctx, size_t bytes)
{
    if (bytes > ((size_t)256 << 20)) return nullptr;
    const bool small = ctx->h_stage.bytes > kStageKeepBytes && bytes <= kStageKeepBytes / 4;
    ctx->h_stage_small_calls = small ? ctx->h_stage_small_calls + 1 : 0;
    const bool trim = small && ctx->h_stage_small_calls >= kStageTrimAfter;
    if (bytes > ctx->h_stage.bytes || trim) {
        ctx->h_stage_small_calls = 0;
        quiet(pin(ctx->h_stage, trim ? kStageKeepBytes : std::max(bytes + bytes / 4, (size_t)1 << 20)));   // optional: null goes pageable
    }
    return ctx->h_stage.p;
}

// The 10x10x10 sample tile of every listed block, gathered out of the strided host grid as BatchUpdate does (VoxelTerrain.cs:341-361), into
// pinned staging when it can be had (one DMA straight from where the gather wrote instead of the runtime's staged copy of a pageable
// vector, profiles/r03/dropin_route.txt), else into `pageable`; null when out of host memory.
const float *gather_tiles(vtmc_ctx *ctx, const float *grid, int64_t sx, int64_t sy, int64_t sz, const int32_t *block_list, int32_t n_blocks,
                          std::vector<float> &pageable)
{
    float *tiles = stage_buffer(ctx, (size_t)n_blocks * VTMC_TILE_SAMPLES * sizeof(float));
    if (!tiles) {   // no pinned memory to be had (or a huge dirty set): the pageable route
        try {
            pageable.resize((size_t)n_blocks * VTMC_TILE_SAMPLES);
        } catch (const std::bad_alloc &) {
            return nullptr;
        }
        tiles = pageable.data();
    }
    for (int32_t b = 0; b < n_blocks; ++b) {
        const int32_t *p = block_list + 3 * (size_t)b;
        const float *org = grid + 8 * ((int64_t)p[0] * sx + (int64_t)p[1] * sy + (int64_t)p[2] * sz);
        float *t = tiles + (size_t)b * VTMC_TILE_SAMPLES;
        // the innermost loop walks the grid axis with the smallest stride (z for a C# float[,,]): the reads stay in one or two cache lines
        if (sz < sx) {
            for (int ix = 0; ix < 10; ++ix)
                for (int iy = 0; iy < 10; ++iy)
                    for (int iz = 0; iz < 10; ++iz) t[ix + 10 * iy + 100 * iz] = org[ix * sx + iy * sy + iz * sz];
        } else {
            for (int iz = 0; iz < 10; ++iz)
                for (int iy = 0; iy < 10; ++iy)
                    for (int ix = 0; ix < 10; ++ix) t[ix + 10 * iy + 100 * iz] = org[ix * sx + iy * sy + iz * sz];
        }
    }
    return tiles;
}

}  // namespace

namespace vtmc {

int extract_core(vtmc_ctx *ctx, const BlockSpace &sp, int n_volumes, ResultSource source, int32_t *tri_count)
{
    int64_t T = 0;
    if (int rc = extract_queue(ctx, sp, n_volumes, source, 0, ctx->stream)) return rc;
    if (int rc = extract_finish(ctx, &T)) return rc;
    if (tri_count) *tri_count = (int32_t)T;
    return VTMC_OK;
}

int attr_gate(vtmc_ctx *ctx, const char *who)
{
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "%s before terrain_init", who);
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "%s before any extract", who);
    if (ctx->result.source != ResultSource::TerrainDirty)
        return fail(ctx, VTMC_ERR_NO_RESULT, "%s: the last result did not come from the resident terrain", who);
    return VTMC_OK;
}

// an attribute is the current result's when it was computed at the epoch of a result that still stands (a standing result's epoch is >= 1)
static bool attr_current(const vtmc_ctx *ctx, const VertexAttr &a) { return ctx->result.valid && a.epoch == ctx->result.epoch; }

int attr_read(vtmc_ctx *ctx, const VertexAttr &a, const char *stale, size_t bytes_per_vertex, uint8_t *dst, int64_t capacity_vertices)
{
    if (!attr_current(ctx, a)) return fail(ctx, VTMC_ERR_NO_RESULT, "%s", stale);
    if (capacity_vertices < a.n) return fail(ctx, VTMC_ERR_INVALID_ARG, "capacity %lld < %lld vertices", (long long)capacity_vertices, (long long)a.n);
    if (a.n == 0) return VTMC_OK;
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipMemcpy(dst, a.values.p, (size_t)a.n * bytes_per_vertex, hipMemcpyDeviceToHost));
    return VTMC_OK;
}

int attr_device_results(vtmc_ctx *ctx, const VertexAttr &a, const char *stale, const uint8_t **d_values, int64_t *n_vertices)
{
    if (!attr_current(ctx, a)) return fail(ctx, VTMC_ERR_NO_RESULT, "%s", stale);
    if (d_values) *d_values = (const uint8_t *)a.values.p;
    if (n_vertices) *n_vertices = a.n;
    return VTMC_OK;
}

float *pinned_stage(vtmc_ctx *ctx, size_t bytes) { return stage_buffer(ctx, bytes); }

int check_dims(vtmc_ctx *ctx, int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(ctx, VTMC_ERR_DIMS, "non-positive grid size %dx%dx%d", nx, ny, nz);
    // VoxelTerrain.cs:138-139 "block size must align to terrain size"
    if (nx % 8 || ny % 8 || nz % 8)
        return fail(ctx, VTMC_ERR_DIMS, "block size must align to terrain size (%dx%dx%d is not a multiple of 8)", nx, ny, nz);
    return VTMC_OK;
}

BlockSpace dense_space(const float *d_base, int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz, int n_volumes,
                       int64_t sv)
{
    BlockSpace sp{};
    sp.base = d_base;
    sp.sx = sx;
    sp.sy = sy;
    sp.sz = sz;
    sp.sv = sv;
    sp.nbx = nx / 8;
    sp.nby = ny / 8;
    sp.nbz = nz / 8;
    sp.bpv = sp.nbx * sp.nby * sp.nbz;
    sp.n_blocks = sp.bpv * n_volumes;
    sp.list = nullptr;
    sp.zfast = (sz == 1 && sx != 1) ? 1 : 0;
    sp.nx = nx;
    sp.d_bpv = FastDiv((unsigned)std::max(sp.bpv, 1));
    sp.d_nbx = FastDiv((unsigned)std::max(sp.nbx, 1));
    sp.d_nby = FastDiv((unsigned)std::max(sp.nby, 1));
    return sp;
}

int upload_block_list(vtmc_ctx *ctx, const int32_t *xyz, int n, BlockSpace &sp)
{
    if (int rc = ensure(ctx, ctx->list, sizeof(int32_t) * 3 * (size_t)std::max(n, 1))) return rc;
    if (n > 0) VTMC_HIP(ctx, hipMemcpyAsync(ctx->list.p, xyz, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    sp.list = (const int *)ctx->list.p;
    sp.n_blocks = n;
    return VTMC_OK;
}

}  // namespace vtmc

extern "C" {

int32_t vtmc_extract_blocks(vtmc_ctx *ctx, const float *samples, int32_t n_blocks, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_blocks < 0 || (n_blocks > 0 && !samples)) return fail(ctx, VTMC_ERR_INVALID_ARG, "samples is null or n_blocks < 0");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_blocks * VTMC_TILE_SAMPLES * sizeof(float);
    if (n_blocks > 0) {
        if (int rc = ensure(ctx, ctx->input, bytes)) return rc;
        VTMC_HIP(ctx, hipMemcpyAsync(ctx->input.p, samples, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    // the tile buffer is a batch of n_blocks volumes of one 8^3 block each
    BlockSpace sp = dense_space((const float *)ctx->input.p, 8, 8, 8, 1, 10, 100, n_blocks, VTMC_TILE_SAMPLES);
    const int rc = extract_core(ctx, sp, 0, ResultSource::Caller, tri_count);
    // the caller's `samples` are only borrowed for this call: a failure behind the asynchronous upload must not return while the DMA still reads them
    if (rc && n_blocks > 0) quiet(hipStreamSynchronize(ctx->stream));
    return rc;
}

int32_t vtmc_extract_grid(vtmc_ctx *ctx, const float *grid, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x,
                          int64_t stride_y, int64_t stride_z, const int32_t *block_list, int32_t n_blocks,
                          int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!grid) return fail(ctx, VTMC_ERR_INVALID_ARG, "grid is null");
    if (int rc = check_dims(ctx, nx, ny, nz)) return rc;
    if (block_list && n_blocks < 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "n_blocks < 0");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    BlockSpace sp = dense_space(nullptr, nx, ny, nz, stride_x, stride_y, stride_z, 1, 0);
    if (block_list) {
        for (int32_t b = 0; b < n_blocks; ++b) {
            const int32_t *p = block_list + 3 * (size_t)b;
            if (p[0] < 0 || p[0] >= sp.nbx || p[1] < 0 || p[1] >= sp.nby || p[2] < 0 || p[2] >= sp.nbz)
                return fail(ctx, VTMC_ERR_DIMS, "block %d = (%d,%d,%d) outside the %dx%dx%d block grid", b, p[0], p[1], p[2],
                            sp.nbx, sp.nby, sp.nbz);
        }
        const size_t span = (size_t)(nx + 1) * stride_x + (size_t)(ny + 1) * stride_y + (size_t)(nz + 1) * stride_z + 1;
        if ((size_t)n_blocks * VTMC_TILE_SAMPLES * 2 < span) {   // small dirty set on a large grid: only B*4000 bytes cross PCIe
            if (stride_x <= 0 || stride_y <= 0 || stride_z <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
            std::vector<float> pageable;
            const float *tiles = gather_tiles(ctx, grid, stride_x, stride_y, stride_z, block_list, n_blocks, pageable);
            if (!tiles) return fail(ctx, VTMC_ERR_DEVICE, "out of host memory gathering %d tiles", n_blocks);
            // blocking: the staging buffer is free again when it returns -- also when it fails behind its upload (extract_blocks drains the stream then)
            return vtmc_extract_blocks(ctx, tiles, n_blocks, tri_count);
        }
    }
    if (int rc = upload_grid(ctx, grid, nx, ny, nz, stride_x, stride_y, stride_z)) return rc;
    if (block_list)
        if (int rc = upload_block_list(ctx, block_list, n_blocks, sp)) return rc;
    sp.base = (const float *)ctx->input.p;
    const int rc = extract_core(ctx, sp, block_list ? 0 : 1, ResultSource::Caller, tri_count);
    if (rc) quiet(hipStreamSynchronize(ctx->stream));   // the uploads above borrow the caller's arrays: nothing of them is in flight when an error returns
    return rc;
}

int32_t vtmc_extract_grid_sharded(vtmc_ctx *ctx, const float *grid, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x,
                                  int64_t stride_y, int64_t stride_z, int32_t chunk_cells, int32_t rank, int32_t world_size,
                                  uint32_t *chunk_counts, int32_t chunk_counts_capacity, int32_t *n_local_chunks,
                                  int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!grid) return fail(ctx, VTMC_ERR_INVALID_ARG, "grid is null");
    if (int rc = check_dims(ctx, nx, ny, nz)) return rc;
    if (chunk_cells <= 0 || chunk_cells % 8 || nx % chunk_cells || ny % chunk_cells || nz % chunk_cells)
        return fail(ctx, VTMC_ERR_DIMS, "chunk size %d must be a multiple of 8 dividing %dx%dx%d", chunk_cells, nx, ny, nz);
    if (world_size <= 0 || rank < 0 || rank >= world_size) return fail(ctx, VTMC_ERR_INVALID_ARG, "bad rank %d / world %d", rank, world_size);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    const int ncx = nx / chunk_cells, ncy = ny / chunk_cells, ncz = nz / chunk_cells;
    const int cb = chunk_cells / 8, bpc = cb * cb * cb;
    std::vector<int32_t> list;
    int n_local = 0;
    for (int c = 0; c < ncx * ncy * ncz; ++c) {
        if (c % world_size != rank) continue;
        const int cx = c % ncx, cy = (c / ncx) % ncy, cz = c / (ncx * ncy);
        for (int bz = 0; bz < cb; ++bz)
            for (int by = 0; by < cb; ++by)
                for (int bx = 0; bx < cb; ++bx) list.insert(list.end(), {cx * cb + bx, cy * cb + by, cz * cb + bz});
        ++n_local;
    }
    if (n_local_chunks) *n_local_chunks = n_local;
    if (chunk_counts && chunk_counts_capacity < n_local)
        return fail(ctx, VTMC_ERR_CAPACITY, "chunk_counts holds %d chunks, need %d", chunk_counts_capacity, n_local);
    if (int rc = upload_grid(ctx, grid, nx, ny, nz, stride_x, stride_y, stride_z)) return rc;
    const int n_blocks = n_local * bpc;
    BlockSpace sp = dense_space((const float *)ctx->input.p, nx, ny, nz, stride_x, stride_y, stride_z, 1, 0);
    if (int rc = upload_block_list(ctx, list.data(), n_blocks, sp)) return rc;
    sp.bpv = bpc;  // chunk-major list: each local chunk is a contiguous run of bpc blocks
    int32_t T = 0;
    if (int rc = extract_core(ctx, sp, n_local, ResultSource::Caller, &T)) return rc;
    if (chunk_counts && n_local > 0 && n_blocks > 0)
        VTMC_HIP(ctx, hipMemcpy(chunk_counts, ctx->volcounts.p, sizeof(uint32_t) * 2 * (size_t)n_local, hipMemcpyDeviceToHost));
    if (tri_count) *tri_count = T;
    return VTMC_OK;
}

int32_t vtmc_set_output_mode(vtmc_ctx *ctx, int32_t mode)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (mode != VTMC_OUTPUT_SOUP && mode != VTMC_OUTPUT_INDEXED) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown output mode %d", mode);
    ctx->output_mode = mode;
    return VTMC_OK;
}

int32_t vtmc_last_vertex_count(const vtmc_ctx *ctx, int32_t *vertex_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid || !ctx->result.indexed) return VTMC_ERR_NO_RESULT;
    if (vertex_count) *vertex_count = (int32_t)ctx->result.verts;
    return VTMC_OK;
}

int32_t vtmc_read_indexed_mesh(vtmc_ctx *ctx, vtmc_vertex *vertices, int64_t vertex_capacity, int32_t *indices, int64_t tri_capacity,
                               int32_t *block_vertex_offsets, int32_t *block_tri_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid || !ctx->result.indexed) return fail(ctx, VTMC_ERR_NO_RESULT, "read_indexed_mesh: the last extract did not run in indexed mode");
    if (vertex_capacity < ctx->result.verts || tri_capacity < ctx->result.tris)
        return fail(ctx, VTMC_ERR_CAPACITY, "capacity (%lld vertices, %lld triangles) < (%lld, %lld)", (long long)vertex_capacity,
                    (long long)tri_capacity, (long long)ctx->result.verts, (long long)ctx->result.tris);
    if ((ctx->result.verts > 0 && !vertices) || (ctx->result.tris > 0 && !indices)) return fail(ctx, VTMC_ERR_INVALID_ARG, "destination is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->result.verts > 0) VTMC_HIP(ctx, hipMemcpy(vertices, ctx->verts.p, sizeof(vtmc_vertex) * (size_t)ctx->result.verts, hipMemcpyDeviceToHost));
    if (ctx->result.tris > 0) VTMC_HIP(ctx, hipMemcpy(indices, ctx->indices.p, sizeof(int32_t) * 3 * (size_t)ctx->result.tris, hipMemcpyDeviceToHost));
    if (int rc = copy_offsets(ctx, block_vertex_offsets, ctx->voffsets)) return rc;
    return copy_offsets(ctx, block_tri_offsets, ctx->offsets);
}

int32_t vtmc_device_indexed_results(vtmc_ctx *ctx, const vtmc_vertex **d_vertices, const int32_t **d_indices,
                                    const uint32_t **d_block_vertex_offsets, const uint32_t **d_block_tri_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid || !ctx->result.indexed) return fail(ctx, VTMC_ERR_NO_RESULT, "device_indexed_results: the last extract did not run in indexed mode");
    if (d_vertices) *d_vertices = (const vtmc_vertex *)ctx->verts.p;
    if (d_indices) *d_indices = (const int32_t *)ctx->indices.p;
    if (d_block_vertex_offsets) *d_block_vertex_offsets = (const uint32_t *)ctx->voffsets.p;
    if (d_block_tri_offsets) *d_block_tri_offsets = (const uint32_t *)ctx->offsets.p;
    return VTMC_OK;
}

int32_t vtmc_read_triangles(vtmc_ctx *ctx, vtmc_triangle *dst, int64_t capacity, int32_t *block_tri_offsets)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "read_triangles before any extract");
    if (ctx->result.indexed) return fail(ctx, VTMC_ERR_NO_RESULT, "read_triangles: the last extract ran in indexed mode (use vtmc_read_indexed_mesh)");
    if (capacity < ctx->result.tris) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %lld triangles", (long long)capacity, (long long)ctx->result.tris);
    if (ctx->result.tris > 0 && !dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->result.tris > 0)
        VTMC_HIP(ctx, hipMemcpy(dst, ctx->tris.p, sizeof(vtmc_triangle) * (size_t)ctx->result.tris, hipMemcpyDeviceToHost));
    return copy_offsets(ctx, block_tri_offsets, ctx->offsets);
}

int32_t vtmc_read_cases(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "read_cases before any extract");
    const int64_t need = (int64_t)ctx->result.blocks * 512;
    if (capacity < need) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %lld < %lld bytes", (long long)capacity, (long long)need);
    if (need == 0) return VTMC_OK;
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    // materialise _CornerFlags on demand with the per-block classify kernel (the input of the last
    // extract is still resident: ctx-owned for host entry points, caller-owned for device ones)
    if (int rc = ensure(ctx, ctx->cases, (size_t)need)) return rc;
    DevBuf tmp;   // freed on every path out
    if (int rc = ensure(ctx, tmp, sizeof(uint32_t) * (size_t)ctx->result.blocks)) return rc;
    hipError_t e = launch_classify_blocks(ctx->result.space, ctx->tables, (uint32_t *)tmp.p, (uint8_t *)ctx->cases.p, nullptr, ctx->n_cus, nullptr, 0, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(dst, ctx->cases.p, (size_t)need, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, VTMC_ERR_DEVICE, "read_cases: %s", hipGetErrorString(e));
    return VTMC_OK;
}

int32_t vtmc_last_counts(const vtmc_ctx *ctx, int32_t *n_blocks, int32_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return VTMC_ERR_NO_RESULT;
    if (n_blocks) *n_blocks = ctx->result.blocks;
    if (tri_count) *tri_count = (int32_t)ctx->result.tris;
    return VTMC_OK;
}

int32_t vtmc_extract_volumes_device(vtmc_ctx *ctx, const vtmc_volume_batch *batch, void *stream, uint32_t flags,
                                    int64_t *tri_count)
{
    if (int32_t rc = vtmc_extract_volumes_device_async(ctx, batch, stream, flags)) return rc;
    return extract_finish(ctx, tri_count);
}

int32_t vtmc_extract_volumes_device_async(vtmc_ctx *ctx, const vtmc_volume_batch *batch, void *stream, uint32_t flags)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!batch || !batch->d_samples) return fail(ctx, VTMC_ERR_INVALID_ARG, "batch or batch->d_samples is null");
    if (int rc = check_dims(ctx, batch->nx, batch->ny, batch->nz)) return rc;
    if (batch->n_volumes < 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "n_volumes < 0");
    if (batch->stride_x <= 0 || batch->stride_y <= 0 || batch->stride_z <= 0 || batch->volume_stride < 0)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    const long long bpv = (long long)(batch->nx / 8) * (batch->ny / 8) * (batch->nz / 8);
    if (bpv * batch->n_volumes > 0x7fffffffll) return fail(ctx, VTMC_ERR_TOO_LARGE, "more than 2^31-1 blocks");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    BlockSpace sp = dense_space(batch->d_samples, batch->nx, batch->ny, batch->nz, batch->stride_x, batch->stride_y,
                                batch->stride_z, batch->n_volumes, batch->volume_stride);
    return extract_queue(ctx, sp, batch->n_volumes, ResultSource::Caller, flags, stream ? (hipStream_t)stream : ctx->stream);
}

int32_t vtmc_extract_finish(vtmc_ctx *ctx, int64_t *tri_count)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    return extract_finish(ctx, tri_count);
}

int32_t vtmc_device_results(vtmc_ctx *ctx, const vtmc_triangle **d_triangles, const uint32_t **d_block_tri_offsets,
                            const uint32_t **d_volume_counts)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "device_results before any extract");
    if (d_triangles) *d_triangles = (const vtmc_triangle *)ctx->tris.p;
    if (d_block_tri_offsets) *d_block_tri_offsets = (const uint32_t *)ctx->offsets.p;
    if (d_volume_counts) *d_volume_counts = (const uint32_t *)ctx->volcounts.p;
    return VTMC_OK;
}

int32_t vtmc_copy_volume_counts_device(vtmc_ctx *ctx, uint32_t *d_dst, int32_t capacity_volumes, void *stream)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    // the counts are final once the scan has run: valid for a finished extract and for a queued one
    if (!ctx->result.valid && !ctx->pending.active) return fail(ctx, VTMC_ERR_NO_RESULT, "copy_volume_counts before any extract");
    const int n_vol = ctx->pending.active ? ctx->pending.n_volumes : ctx->result.volumes;
    const int n_blk = ctx->pending.active ? ctx->pending.sp.n_blocks : ctx->result.blocks;
    if (capacity_volumes < n_vol) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d volumes", capacity_volumes, n_vol);
    if (n_vol == 0 || n_blk == 0) return VTMC_OK;
    if (!d_dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "d_dst is null");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    // a queued extract on another stream: the copy is ordered behind its emit launch (whose first workgroup may write the counts)
    if (ctx->pending.active && ctx->pending.launched && st != ctx->pending.stream) VTMC_HIP(ctx, hipStreamWaitEvent(st, ctx->ev[3], 0));
    VTMC_HIP(ctx, hipMemcpyAsync(d_dst, ctx->volcounts.p, sizeof(uint32_t) * 2 * (size_t)n_vol, hipMemcpyDeviceToDevice, st));
    return VTMC_OK;
}

int32_t vtmc_reserve_triangles(vtmc_ctx *ctx, int64_t capacity)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (capacity < 0 || capacity > 0x7fffffffll) return fail(ctx, VTMC_ERR_INVALID_ARG, "capacity out of range");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->result.valid = false;  // the old triangle buffer may be released
    const size_t bytes = sizeof(vtmc_triangle) * (size_t)std::max<int64_t>(capacity, 1);
    if (ctx->tris.p && ctx->tris.bytes > std::max<size_t>(bytes, 256)) release(ctx->tris);  // exact size: shrinking is allowed
    const void *before = ctx->tris.p;
    const int rc = ensure(ctx, ctx->tris, bytes);
    if (!rc && ctx->tris.p != before) ctx->place_pending = true;   // a new allocation: the next extract may try others beside it (place_outputs)
    return rc;
}

int32_t vtmc_last_placement(const vtmc_ctx *ctx, float ms[16], int32_t *n_candidates, int32_t *kept)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (ms) memcpy(ms, ctx->place_ms, sizeof ctx->place_ms);
    if (n_candidates) *n_candidates = ctx->place_n;
    if (kept) *kept = ctx->place_kept;
    return VTMC_OK;
}

int32_t vtmc_last_stage_ms(vtmc_ctx *ctx, float ms[4])
{
    if (!ctx || !ms) return VTMC_ERR_INVALID_ARG;
    if (!ctx->result.valid) return fail(ctx, VTMC_ERR_NO_RESULT, "last_stage_ms before any extract");
    memcpy(ms, ctx->stage_ms, sizeof ctx->stage_ms);
    return VTMC_OK;
}

}  // extern "C"
