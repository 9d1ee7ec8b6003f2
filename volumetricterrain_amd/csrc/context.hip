// context.hip -- the context of include/vtmc.h: creation and teardown, its stream pool, the tuning keys, the shared error text and
// grow-only device buffers (the reference allocates and releases six ComputeBuffers per call, VoxelTerrain.cs:368-414, 469-476).
// There is no CPU fallback of any kind: without a HIP device vtmc_create fails.
#include "mc_tables_packed.h"
#include "vtmc_ctx.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

using namespace vtmc;

static thread_local std::string g_create_error;

namespace vtmc {

// STREAMS OUTLIVE THEIR CONTEXTS (round 6).  vtmc_context_stream hands raw hipStream_t handles to the host, and host-side objects keep
// referring to them after vtmc_destroy -- events recorded on them, a framework's stream wrapper, a caching allocator that records an event on
// the stream when it frees a pinned buffer that was copied on it: round 5's aborts in the interpreter's tear-down.  A context therefore does
// not destroy its streams: vtmc_destroy drains them and parks them here, per device and kind, and the next context on that device takes a
// parked one.  Bounded by the largest number of contexts alive at once.  At process exit they are left to the runtime, as a framework's own
// streams are: an atexit handler that destroyed them (tried in round 6) runs after a profiler's tool library has torn its stream
// bookkeeping down -- rocprofv3 then aborts inside hipStreamDestroy -- and is not what decides how a process ends under ROCm 7.2 anyway
// ("Streams": copies on a CU-mask stream do, whatever is destroyed when).  VTMC_STREAM_POOL=0 in the environment (test
// switch) restores destruction in vtmc_destroy.
namespace {
struct StreamPool {
    std::mutex m;
    std::vector<std::pair<int, hipStream_t>> parked[2];   // [0] ordinary non-blocking streams, [1] streams on a hardware queue of their own
};
StreamPool &stream_pool()
{
    static StreamPool *p = new StreamPool;   // never destructed: no static destructor that could run beside the HIP runtime's own at exit
    return *p;
}
bool env_is(const char *name, const char *value)
{
    const char *v = getenv(name);
    return v && !strcmp(v, value);
}
bool stream_pool_enabled()
{
    static const bool on = !env_is("VTMC_STREAM_POOL", "0");
    return on;
}
}  // namespace

// A stream of `device` (current): own_queue = made by hipExtStreamCreateWithCUMask with every CU named -- such a stream always sits on a
// hardware queue of its own, ordinary streams share a handful (profiles/r05/stream_overlap.txt).
hipError_t take_stream(int device, bool own_queue, int n_cus, hipStream_t *out)
{
    if (stream_pool_enabled()) {
        StreamPool &sp = stream_pool();
        std::lock_guard<std::mutex> g(sp.m);
        auto &v = sp.parked[own_queue ? 1 : 0];
        for (size_t i = v.size(); i-- > 0;)   // the one parked last
            if (v[i].first == device) {
                *out = v[i].second;
                v.erase(v.begin() + (long)i);
                return hipSuccess;
            }
    }
    if (!own_queue) return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    std::vector<uint32_t> mask((size_t)(n_cus + 31) / 32, 0xFFFFFFFFu);
    if (n_cus % 32) mask.back() = (1u << (n_cus % 32)) - 1u;
    return hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data());
}

// the stream is idle (the caller synchronised it)
void park_stream(int device, bool own_queue, hipStream_t s)
{
    if (!s) return;
    if (!stream_pool_enabled()) {
        quiet(hipStreamDestroy(s));
        return;
    }
    StreamPool &sp = stream_pool();
    std::lock_guard<std::mutex> g(sp.m);
    sp.parked[own_queue ? 1 : 0].emplace_back(device, s);
}

int fail(vtmc_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

int ensure(vtmc_ctx *ctx, VtmcDevBuf &b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return VTMC_OK;
    if (b.p) VTMC_HIP(ctx, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    size_t want = std::max<size_t>(bytes, 256);
    VTMC_HIP(ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    return VTMC_OK;
}

}  // namespace vtmc

extern "C" {

const char *vtmc_version(void) { return "vtmc 0.1 gfx950"; }

int32_t vtmc_create(int32_t device, vtmc_ctx **out_ctx)
{
    if (!out_ctx) return fail(nullptr, VTMC_ERR_INVALID_ARG, "out_ctx is null");
    *out_ctx = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, VTMC_ERR_DEVICE, "no HIP device available (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n_dev) return fail(nullptr, VTMC_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, n_dev);
    vtmc_ctx *ctx = new (std::nothrow) vtmc_ctx();
    if (!ctx) return fail(nullptr, VTMC_ERR_DEVICE, "out of host memory");
    ctx->device = device;
    auto bail = [&](const char *what, hipError_t err) {
        std::string msg = std::string(what) + ": " + hipGetErrorString(err);
        vtmc_destroy(ctx);
        return fail(nullptr, VTMC_ERR_DEVICE, "%s", msg.c_str());
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    ctx->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // test switch (tests/test_own_queue_cpp_host.py): the context's MAIN stream on a hardware queue of its own, pinned staging and read-backs
    // included -- the configuration whose C++ host hung at process exit in round 5 ("Streams")
    ctx->stream_own_queue = env_is("VTMC_TEST_MAIN_STREAM_OWN_QUEUE", "1");
    if ((e = take_stream(device, ctx->stream_own_queue, ctx->n_cus, &ctx->stream)) != hipSuccess) return bail("hipStreamCreate", e);
    for (auto &ev : ctx->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&ctx->ev_origins, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = pin(ctx->h_totals, 64 * sizeof(uint32_t))) != hipSuccess) return bail("hipHostMalloc", e);
    memset(ctx->h_totals.p, 0, 64 * sizeof(uint32_t));
    if ((e = hipHostGetDevicePointer((void **)&ctx->h_totals_dev, ctx->h_totals.p, 0)) != hipSuccess) return bail("hipHostGetDevicePointer", e);

    // tables: VoxelTerrain.cs:151-156 uploads three int tables; here the packed 2 KB vert table and a
    // 256-byte triangle-count table (the edge-mask table is implied by the vert table)
    static const unsigned long long packed[VTMC_MC_TABLE_WORDS] = VTMC_MC_TABLE_INIT;
    unsigned char tri_num[256];
    for (int c = 0; c < 256; ++c) tri_num[c] = (unsigned char)(packed[c] >> 60);
    if (ensure(ctx, ctx->d_vert, sizeof packed) || ensure(ctx, ctx->d_trinum, sizeof tri_num)) {
        std::string msg = ctx->err;
        vtmc_destroy(ctx);
        return fail(nullptr, VTMC_ERR_DEVICE, "%s", msg.c_str());
    }
    if ((e = hipMemcpy(ctx->d_vert.p, packed, sizeof packed, hipMemcpyHostToDevice)) != hipSuccess) return bail("table upload", e);
    if ((e = hipMemcpy(ctx->d_trinum.p, tri_num, sizeof tri_num, hipMemcpyHostToDevice)) != hipSuccess) return bail("table upload", e);
    ctx->tables.vert_packed = (const unsigned long long *)ctx->d_vert.p;
    ctx->tables.tri_num = (const unsigned char *)ctx->d_trinum.p;
    *out_ctx = ctx;
    return VTMC_OK;
}

int32_t vtmc_destroy(vtmc_ctx *ctx)
{
    if (!ctx) return VTMC_OK;
    quiet(hipSetDevice(ctx->device));
    // 1. nothing of this context is still running: a queued extract nobody finished (on whatever stream the caller named), the own-queue
    //    stream, the collective's stream, the ordinary stream -- BEFORE anything they use is released (round 5 freed device and pinned memory
    //    first and synchronised the own-queue stream last)
    if (ctx->pending.active && ctx->pending.stream) quiet(hipStreamSynchronize(ctx->pending.stream));
    if (ctx->queue_stream) quiet(hipStreamSynchronize(ctx->queue_stream));
    if (ctx->comm_stream) quiet(hipStreamSynchronize(ctx->comm_stream));
    if (ctx->stream) quiet(hipStreamSynchronize(ctx->stream));
    comm_release(ctx);   // drains the collectives queued through the communicator (also on a stream of the caller's), then lets go of it
    // 2. the streams: parked for the next context of this device, never destroyed -- handles from vtmc_context_stream stay valid for host-side
    //    objects that outlive the context (see StreamPool above; VTMC_STREAM_POOL=0: destroyed here, ahead of the events and the memory)
    park_stream(ctx->device, false, ctx->comm_stream);
    park_stream(ctx->device, true, ctx->queue_stream);
    park_stream(ctx->device, ctx->stream_own_queue, ctx->stream);
    ctx->comm_stream = ctx->queue_stream = ctx->stream = nullptr;
    // 3. events: those named here; the stage clocks of the passes (StageClock) destroy theirs in `delete ctx` below -- after steps 1 and 2
    //    like these, so no stream of the context can still be recording into one
    if (ctx->ev_origins) quiet(hipEventDestroy(ctx->ev_origins));
    for (auto &ev : ctx->ev)
        if (ev) quiet(hipEventDestroy(ev));
    if (ctx->ev_gather) quiet(hipEventDestroy(ctx->ev_gather));
    if (ctx->ev_last_gather) quiet(hipEventDestroy(ctx->ev_last_gather));
    if (ctx->ev_comm_chain) quiet(hipEventDestroy(ctx->ev_comm_chain));
    // 4. device buffers, pinned memory and the stage clocks' events: the members free their own
    delete ctx;
    return VTMC_OK;
}

const char *vtmc_last_error(const vtmc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t vtmc_context_stream(vtmc_ctx *ctx, int32_t own_queue, void **stream)
{
    if (!ctx || !stream) return VTMC_ERR_INVALID_ARG;
    *stream = nullptr;
    if (!own_queue) {
        *stream = (void *)ctx->stream;
        return VTMC_OK;
    }
    // A stream on a HARDWARE QUEUE OF ITS OWN.  Ordinary HIP streams share a handful of queues, and two contexts whose streams land on one
    // queue run their steps strictly one behind the other; on queues of their own, step k + 1's classify kernel starts on the CUs step k's
    // emit kernel leaves as it drains (profiles/r05/stream_overlap.txt: -4..5 % of a 1024^3 step, -20 % of a rank's step of an 8-rank run).
    // A stream made with a CU mask always gets its queue; the mask names every CU.  Taken on first request (a parked one of an earlier
    // context, or a new one); parked again, not destroyed, by vtmc_destroy: the handle stays valid until the process exits.
    if (!ctx->queue_stream) {
        VTMC_HIP(ctx, hipSetDevice(ctx->device));
        const hipError_t e = take_stream(ctx->device, true, ctx->n_cus, &ctx->queue_stream);
        if (e != hipSuccess) {
            quiet(e);
            ctx->queue_stream = nullptr;
            return fail(ctx, VTMC_ERR_DEVICE, "hipExtStreamCreateWithCUMask failed: %s", hipGetErrorString(e));
        }
    }
    *stream = (void *)ctx->queue_stream;
    return VTMC_OK;
}

// every parked stream of every device is destroyed now; the contexts alive keep theirs
int32_t vtmc_release_streams(void)
{
    StreamPool &sp = stream_pool();
    std::vector<std::pair<int, hipStream_t>> all;
    {
        std::lock_guard<std::mutex> g(sp.m);
        for (auto &v : sp.parked) {
            all.insert(all.end(), v.begin(), v.end());
            v.clear();
        }
    }
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (auto &ds : all) {
        if (hipSetDevice(ds.first) != hipSuccess) continue;
        quiet(hipStreamSynchronize(ds.second));
        quiet(hipStreamDestroy(ds.second));
    }
    if (have_prev) quiet(hipSetDevice(prev));
    return (int)all.size();
}

int32_t vtmc_set_tuning(vtmc_ctx *ctx, const char *key, int32_t value)
{
    if (!ctx || !key) return VTMC_ERR_INVALID_ARG;
    const std::string k(key);
    // every key below selects code that tests/test_tuning_matrix.py compares with the oracle; a value outside a key's range is refused
    auto ranged = [&](int &field, int lo, int hi) {
        if (value < lo || value > hi) return fail(ctx, VTMC_ERR_INVALID_ARG, "tuning key '%s': %d is outside [%d, %d]", key, value, lo, hi);
        field = value;
        return (int)VTMC_OK;
    };
    if (k == "emit_fast_math") return ranged(ctx->tune.emit_fast_math, 0, 1);
    if (k == "emit_once") return ranged(ctx->tune.emit_once, 0, 1);
    if (k == "emit_dynamic") return ranged(ctx->tune.emit_dynamic, 0, 1);
    if (k == "emit_sub_log2") return ranged(ctx->tune.emit_sub_log2, 0, 4);
    if (k == "emit_row_masks") return ranged(ctx->tune.emit_row_masks, 0, 1);
    if (k == "emit_wgs_per_cu") return ranged(ctx->tune.emit_wgs_per_cu, 0, 8);
    // residency caps work by unused dynamic LDS; ONE workgroup per CU would ask for the whole 160 KB, which the runtime answers with abort(): refused
    if ((k == "classify_wgs_per_cu" || k == "density_wgs_per_cu") && value == 1)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "tuning key '%s': a cap of one workgroup per CU is not supported (0: none, or 2 and more)", key);
    if (k == "classify_wgs_per_cu") return ranged(ctx->tune.classify_wgs_per_cu, 0, 7);
    if (k == "density_wgs_per_cu") return ranged(ctx->tune.density_wgs_per_cu, 0, 3);
    if (k == "gather_beside") return ranged(ctx->tune.gather_beside, 0, 1);
    if (k == "place_outputs") return ranged(ctx->tune.place_outputs, 0, 16);
    if (k == "stage_events") return ranged(ctx->tune.stage_events, 0, 1);
    if (k == "invalidate_signs") {   // the caller wrote to (or re-used the address of) a buffer the last fill left sign bits for
        ctx->sign_of.valid = false;
        return VTMC_OK;
    }
    if (k == "fill_keeps_signs") {
        ctx->sign_of.valid = false;
        return ranged(ctx->tune.fill_keeps_signs, 0, 1);
    }
#ifdef VTMC_DIAGNOSTICS   // output INVALID: diagnostic builds only (the product's kernels do not contain these branches)
    if (k == "emit_ablate") ctx->tune.emit_ablate = value;
    else if (k == "classify_ablate") ctx->tune.classify_ablate = value;
    else if (k == "density_ablate") ctx->tune.density_ablate = value;
    else
#endif
    return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown tuning key '%s'", key);
    return VTMC_OK;
}

}  // extern "C"
