// vtmc_ctx.h -- the context object behind include/vtmc.h and the small host helpers every translation unit of the C-ABI layer shares
// (every .hip file but the two of extract kernels): the owned buffers, the stage clocks that time a pass's kernels (StageClock), fail /
// VTMC_HIP, and the one kernel launch of the layer (launch, with the lanes256 grid).  Not installed.
#ifndef VTMC_CTX_H
#define VTMC_CTX_H
#include "../../include/vtmc.h"
#include "vtmc_internal.h"
struct vtmc_nav_span;   // include/vtmc_nav.h
#include "../../include/vtmc_water.h"
#include "../../include/vtmc_erosion.h"

#include <deque>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace vtmc {
struct TerrainBox {
    int lx, ly, lz;  // first sample
    int dx, dy, dz;  // samples per axis (0 on some axis: the modifier wrote nothing)
};
// Memory a context owns: device memory (VtmcDevBuf, grown by ensure) or pinned host memory (VtmcPinnedBuf, allocated by pin).  Move-only, so
// one object names one allocation, and freed by its destructor.  Pointer and size are always cleared together: a buffer freed with its size
// left standing is written to by the next call that finds it "large enough" (round 3's double free).
template <typename T, hipError_t (*Free)(void *)>
struct OwnedBuf {
    T *p = nullptr;
    size_t bytes = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
    OwnedBuf &operator=(OwnedBuf o) noexcept { return swap(o); }   // `o` takes what this held and frees it
    ~OwnedBuf() { release(); }
    OwnedBuf &swap(OwnedBuf &o) noexcept
    {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    void release()
    {
        if (p) quiet(Free(p));
        p = nullptr;
        bytes = 0;
    }
};
// The N timing events around the kernels of one pass, and whether they hold a whole run of it.  A pass calls begin() (the first one creates
// the events; every one disarms the clock), mark(i, stream) between its kernels, and arm() once the last mark is queued; a reader refuses
// while !armed, then sync_last() and elapsed().  Neither copied nor moved: the events are destroyed with the context that holds the clock.
template <int N>
struct StageClock {
    hipEvent_t ev[N] = {};
    bool armed = false;
    StageClock() = default;
    StageClock(const StageClock &) = delete;
    StageClock &operator=(const StageClock &) = delete;
    ~StageClock()
    {
        for (hipEvent_t e : ev)
            if (e) quiet(hipEventDestroy(e));
    }
    hipError_t begin()
    {
        armed = false;
        for (hipEvent_t &e : ev)
            if (!e)
                if (hipError_t rc = hipEventCreate(&e)) return rc;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t stream) { return hipEventRecord(ev[i], stream); }
    void arm() { armed = true; }
    hipEvent_t event(int i) const { return ev[i]; }
    int sync_last(vtmc_ctx *ctx) const;                           // on the context's device: waits for event N - 1
    int elapsed(vtmc_ctx *ctx, int i, int j, float *ms) const;    // milliseconds from event i to event j
};
}  // namespace vtmc
typedef vtmc::OwnedBuf<void, hipFree> VtmcDevBuf;
template <typename T>
using VtmcPinnedBuf = vtmc::OwnedBuf<T, hipHostFree>;

// One modifier of a recorded vtmc_terrain_update: its sample box, where the box's image lies in the journal arena, and the clamped
// AABB the dirty-block rule reads (kept for every modifier, also those whose box is empty, so an undo dirties what the update did).
struct VtmcHistoryBox {
    vtmc::TerrainBox box;
    int low[3], up[3];
    size_t off = 0;  // bytes into the arena
};
// One recorded update: its boxes in queue order, laid out back to back in [off, off + bytes) of the arena.  The images hold the
// samples as they were before the step while it is done, and as they were after it while it is undone.
struct VtmcHistoryStep {
    std::vector<VtmcHistoryBox> boxes;
    size_t off = 0, bytes = 0;
};

// One stamp (vtmc_stamp_create / _capture): nx * ny * nz FP32 samples in device memory, x fastest.
struct VtmcStamp {
    VtmcDevBuf samples;
    int nx = 0, ny = 0, nz = 0;
};

// Who produced an extract's blocks: the caller's own samples, the resident terrain's dirty list (terrain.hip) or a level-of-detail
// selection of the terrain (terrain_lod.hip: the blocks are nodes, tiles in lod_tiles, node list in lod_nodes)
enum class ResultSource { Caller, TerrainDirty, TerrainLod };

// The result the context holds.  extract_finish() writes it whole and is the only writer of a valid one; everything that overwrites or
// may release what it names clears `valid` and leaves `epoch` alone, so no epoch ever names two results.
struct VtmcResult {
    bool valid = false;
    uint64_t epoch = 0;          // counts the finished extracts
    ResultSource source = ResultSource::Caller;
    vtmc::BlockSpace space{};
    int blocks = 0;
    uint32_t active = 0;         // non-empty blocks: the BlockDesc records the scan left in `active`, in list order
    int volumes = 0;
    int64_t tris = 0, verts = 0;
    bool indexed = false;
    int64_t vertices() const { return indexed ? verts : 3 * tris; }
};

// One value per vertex of the result `epoch` names (material weights, occlusion): library-owned, computed on demand, stale after the
// next extract
struct VertexAttr {
    VtmcDevBuf values;
    int64_t n = 0;
    uint64_t epoch = 0;
};

// What a pass over the triangles of the result `epoch` names holds (tri_stream_kernels.h): library-owned, grow-only, stale after the next
// extract.  records: the n records the pass emitted; block_offsets: blocks + 1 entries; masks: one byte per triangle, whole tiles; scan:
// the ScanLayout of the tiles' totals.
struct VtmcTriStream {
    VtmcDevBuf records, block_offsets, masks, scan;
    int64_t n = 0;
    int blocks = 0;
    uint64_t epoch = 0;
};

// The navigation build the context holds (terrain_nav.hip): library-owned, grow-only; a snapshot of the grid at build time, dropped by
// vtmc_terrain_init / _load.  offsets: the columns + 1 span offsets; scan: the grand total (64 bits), the column counts and their prefixes
// inside a group of columns, the group totals and their prefixes; scratch: a column word and a parent word per span; ctl: the flag word
// and the verify pass's count.
struct VtmcNav {
    VtmcDevBuf spans, offsets, scan, scratch, ctl;
    VtmcDevBuf spans_next, offsets_next;           // what vtmc_nav_erode writes its result into before it swaps them with spans / offsets
    bool valid = false;
    int32_t n = 0;
    int32_t lo[3] = {0, 0, 0}, d[3] = {0, 0, 0};   // the box as reported: first sample, samples per axis
    int rounds = 0;                                // union / flatten / verify rounds of the last build
};

// The flow field the context holds (terrain_navfield.hip), built on the nav result above and dropped with it: library-owned, grow-only.
// cells: the result; work: per span the four edge costs (16 bytes), then the cost D and the cheapest goal cost (4 bytes each); ctl: the
// flag word of every round of a batch, then the reached count.
struct VtmcNavField {
    VtmcDevBuf cells, work, ctl;
    bool valid = false;
    int32_t n = 0, reached = 0, rounds = 0;
};

// The agent radius on the nav result above (terrain_naverode.hip): library-owned, grow-only.  state: two arrays of 8-byte state words, a
// round reads one and writes the other; links: the four links of every span, packed; dist: the distances of vtmc_nav_distance_build, which
// describe the nav result they were built on and are dropped when an erode replaces it; remap: the old-to-new index words of an erode;
// origin: its result beside the spans, valid until the next erode or nav build; ctl: the border count.
struct VtmcNavErode {
    VtmcDevBuf state, links, dist, remap, origin, ctl;
    bool dist_valid = false, origin_valid = false;
    int32_t dist_n = 0, origin_n = 0;
    int32_t rounds = 0;        // of the last distance pass
};

// The crowd the context holds (terrain_navcrowd.hip), spawned on the nav result above and dropped with it; a new flow field keeps it:
// library-owned, grow-only.  agents: the records; pending: per agent the {target, cost} words a tick's claim kernel leaves for its resolve
// kernel; occupancy, claims: a word per span; links: the four links of every span, packed at the spawn; ctl: the counters of a spawn or of
// the last tick of a step.  The counts are the host's copy of what the last spawn or step left.
struct VtmcNavCrowd {
    VtmcDevBuf agents, pending, occupancy, claims, links, ctl;
    bool valid = false;
    int32_t n_agents = 0, n_spans = 0;
    int32_t occupying = 0, arrived = 0, ticks = 0, moved_last = 0;
};

// The water result the context holds (terrain_water.hip): library-owned, grow-only; a snapshot of the grid at flood time, dropped by
// vtmc_terrain_init / _load.  water, body: the two volumes (vd samples per axis); labels: a parent word per sample of the box; records:
// VTMC_WATER_MAX_SOURCES body records; seeds: the sources of the call, level by level; source_body: a word per source; ctl: the flag
// word and the body count; probe: the positions and answers of vtmc_water_probe.  bodies: the host's copy of the records.
struct VtmcWater {
    VtmcDevBuf water, body, labels, records, seeds, source_body, ctl, probe;
    bool valid = false;
    int32_t lo[3] = {0, 0, 0}, d[3] = {0, 0, 0}, vd[3] = {0, 0, 0};   // the box as reported, and the volume dims
    int64_t wet = 0;
    std::vector<vtmc_water_body> bodies;
};

// The maps of the last VTMC_MOD_EROSION (terrain_erosion.hip): library-owned, grow-only; a snapshot, kept by edits, undo and redo, dropped
// by vtmc_terrain_init / _load, replaced by the next erosion.  state: the planes of the simulation, the mask bytes and the three counters
// (terrain_erosion.h: ErosionLayout), in which the maps lie where the last step left them.  info: the host's copy of the report; its three
// counts are fetched from the device by the first vtmc_erosion_info that asks (counts_pending).
struct VtmcErosion {
    VtmcDevBuf state;
    bool valid = false, counts_pending = false;
    bool has_state = false;   // the planes are those of info's nx x nz box, whether or not the maps still are a snapshot (vtmc_debug_erosion_step_ms)
    bool lds = false;         // the step's variant (vtmc_debug_erosion_lds)
    vtmc_erosion_report info{};
};

// The light result the context holds (terrain_light.hip): library-owned, grow-only; a snapshot of the grid at the time of the call, dropped
// by vtmc_terrain_init / _load.  volume: the two volumes a round reads and writes in turn, equal once the relaxation has settled, [0]
// the result; mask: the open mask, a 64-bit word per row of up to 64 samples along x; tiles: a changed byte per tile and round parity;
// seeds: the sources of the call; lit: a byte per source; ctl: the changed word of every round, then the two counts; probe: the positions
// and answers of vtmc_light_probe.  serial counts the light results, so the vertex bytes know which one they were read from.  plain,
// batch: the relaxation's variant and the rounds queued between two read-backs (vtmc_debug_light_variant).
struct VtmcLight {
    VtmcDevBuf volume[2], mask, tiles, seeds, lit, ctl, probe;
    bool valid = false;
    int32_t lo[3] = {0, 0, 0}, d[3] = {0, 0, 0};
    int64_t n_sky = 0, n_torch = 0;
    int32_t rounds = 0;
    uint64_t serial = 0;
    bool plain = false;
    int32_t batch = 4;
    VertexAttr vertices;           // two bytes per vertex of the result vertices.epoch names ...
    uint64_t vertices_serial = 0;  // ... read from the light result of this serial
};

// The skirts over the seams of a level-of-detail result (terrain_lodskirt.hip): the records are vtmc_triangle, the blocks are nodes, a
// mask byte holds a triangle's faces.  node_masks: the face masks of the nodes as the kernels read them, face_masks the host's copy of
// those of the skirts held; sink: what vtmc_debug_lodskirt_read_ms's kernel leaves.  staged: the emit kernel's store variant
// (vtmc_debug_lodskirt_store).
struct VtmcLodSkirt {
    VtmcTriStream pass;
    VtmcDevBuf node_masks, sink;
    std::vector<uint8_t> face_masks;
    int32_t flagged = 0;
    bool staged = false;
};

// The materials and the occlusion of a level-of-detail result and of its skirts (terrain_lodattr.hip), the layer's own: values[attribute]
// [target], each current while its epoch is the result's; vtmc_lod_skirts clears the epochs of the skirt targets.  stats: the two route
// counters of the last occlusion call (vtmc_debug_lodattr_routes); direct_max: vertices up to which a node takes the direct route, -1 the
// library's default; skirts_in_node: the occlusion of a node's skirt corners comes from the node's own workgroup (the library's choice), not
// from a pass of its own (vtmc_debug_lodattr_skirts_in_node).
struct VtmcLodAttr {
    VertexAttr values[2][2];
    VtmcDevBuf stats;
    int32_t direct_max = -1;
    bool skirts_in_node = true;
};

// An extract that has been queued on a stream and not yet completed by extract_finish().
struct VtmcPending {
    bool active = false;    // queued, extract_finish() not yet called
    bool launched = false;  // false: the empty-batch early exit (nothing to wait for but the memsets)
    vtmc::BlockSpace sp{};
    int n_volumes = 0;
    bool indexed = false;
    ResultSource source = ResultSource::Caller;
    hipStream_t stream = nullptr;
    size_t tcap = 0, vcap = 0;  // capacities the last emit launch was given
    bool scan_event = false;    // ev[2] was recorded behind this extract's scan
    bool counts_early = false;  // the per-volume counts were final when ev[2] (end of the scan) was recorded
};

struct vtmc_ctx {
    int device = 0;
    int n_cus = 256;
    hipStream_t stream = nullptr;         // the context's own stream (what `stream` = NULL means in the ABI)
    bool stream_own_queue = false;        // test switch VTMC_TEST_MAIN_STREAM_OWN_QUEUE=1: `stream` itself sits on a hardware queue of its own
    hipStream_t queue_stream = nullptr;   // vtmc_context_stream(own_queue = 1): a stream on a hardware queue of its own, made on request
    vtmc::DeviceTables tables{nullptr, nullptr};
    VtmcDevBuf d_vert, d_trinum;
    VtmcDevBuf counts, offsets, active, partials, totals, volcounts, cases, tris, input, list, perm, origins, yrows;
    VtmcDevBuf vcounts, voffsets, vtotals, verts, indices;  // indexed output
    int output_mode = VTMC_OUTPUT_SOUP;
    uint32_t *h_totals_dev = nullptr;  // the same pinned words as the device sees them (the fused scan writes its totals there)
    VtmcPinnedBuf<uint32_t> h_totals;  // pinned: the scan's totals ({T sat, nActive, T lo, T hi}, then the vertex scan's), 64 words
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // [0..3] stage timing, [4] staging copies
    VtmcDevBuf signs;               // the sign volume of the last z-walk fill (tuning key "fill_keeps_signs")
    struct {
        bool valid = false;
        const float *d_out = nullptr;
        int dx = 0, dy = 0, dz = 0, n_volumes = 0;
        long long sv = 0;
    } sign_of;                      // which buffer / layout `signs` describes
    VtmcPinnedBuf<float> h_stage;   // pinned staging of host-gathered tiles (vtmc_extract_grid with a dirty list)
    int h_stage_small_calls = 0;    // consecutive calls that needed far less than an over-sized staging buffer holds (the trim waits for kStageTrimAfter of them)
    VtmcPinnedBuf<int32_t> h_origins;   // pinned staging of the sampler's chunk origins
    hipEvent_t ev_origins = nullptr;   // behind the upload from h_origins
    bool origins_upload_pending = false;
    float stage_ms[4] = {0, 0, 0, 0};
    bool place_pending = false;     // the output buffers were (re)allocated since the last placement trial (tuning key place_outputs)
    float place_ms[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // emit stage per candidate of the last trial ([0]: the buffer that was there), place_n of them
    int place_n = 0, place_kept = 0;
    vtmc::StageClock<2> fill_clock;   // around the last density kernel (vtmc_last_fill_ms)
    VtmcPending pending;
    VtmcResult result;
    vtmc::Tuning tune;
    // device-resident terrain (vtmc_terrain_*)
    VtmcDevBuf terrain, heightmap;
    vtmc::TerrainShape tshape{};
    bool has_terrain = false;
    uint32_t terrain_events = 0;
    std::vector<int32_t> dirty;  // (bx,by,bz) of the last vtmc_terrain_update, ordered by block id
    bool dirty_is_all = false;   // ... or every block (the list is then materialised on demand only)
    // terrain.hip: the edit journal (vtmc_terrain_set_history / _undo / _redo).  `journal` is the arena, max_bytes long, allocated by
    // set_history only; the steps are placed in it as a ring, oldest first.  hist[0, hist_done) can be undone, hist[hist_done, end) redone.
    VtmcDevBuf journal;
    std::deque<VtmcHistoryStep> hist;
    size_t hist_done = 0;
    // terrain_brush.hip: the stage of a VTMC_MOD_SMOOTH brush (its box plus a one-sample halo, before the brush), grow-only; grown only after
    // the stream has drained, since an earlier smooth of the same queue may still be reading it
    VtmcDevBuf brush;
    // terrain_stamp.hip: the stamps by id; ids count up from 1 and are never reused.  No part of the terrain: vtmc_terrain_init / _load and the
    // history leave them alone, vtmc_destroy frees them.
    std::map<int32_t, VtmcStamp> stamps;
    int32_t next_stamp_id = 1;
    // terrain_path.hip: the segment records of the VTMC_MOD_PATH modifier being applied, grow-only; written only after the stream has
    // drained, since an earlier path modifier of the same queue may still be reading it
    VtmcDevBuf path;
    // terrain_fragments.hip: the scratch of a labelling pass (a parent word and an auxiliary word per sample of the box: 8 bytes per sample), its
    // control words (the convergence flag, the fragment count, the slot counter) and the query's fragment records; all grow-only, grown only
    // after the stream has drained
    VtmcDevBuf frag_labels, frag_ctl, frag_records;
    // terrain_material.hip: the material layer (mat_c^3 texels of 8 bytes; mat_c = 0: none), the float image of a set_control_map on its way
    // to the quantising kernel, the strokes of a paint call, and the vertex weights (8 bytes per vertex)
    VtmcDevBuf material, mat_image, mat_strokes;
    int mat_c = 0;
    VertexAttr mat_weights;
    // terrain_ao.hip: the ambient-occlusion byte of every vertex, and the two route counters of the last call (workgroups that staged a
    // tile, workgroups that fetched from global memory: vtmc_debug_ao_routes)
    VertexAttr ao;
    VtmcDevBuf ao_stats;
    int32_t ao_direct_max = -1;         // vertices up to which a block takes the direct route; -1: the library's default
    // terrain_scatter.hip: the instances of the last vtmc_scatter_surface (the records are vtmc_instance, a mask byte holds a triangle's
    // survivors) and the clock of its kernels (armed by a call that launched them)
    VtmcTriStream scatter;
    vtmc::StageClock<6> scatter_clock;
    // terrain_nav.hip: the last navigation build and the clock of its kernels (armed by a build that made spans)
    VtmcNav nav;
    vtmc::StageClock<9> nav_clock;
    // terrain_navfield.hip: the flow field on that build and the clock of its kernels (edge costs and goals, relaxation, next)
    VtmcNavField navfield;
    vtmc::StageClock<4> navfield_clock;
    // terrain_naverode.hip: the distance to the border and the origin of an erosion of that build, and the clock of its kernels (border
    // test, rounds, compaction, relabelling)
    VtmcNavErode naverode;
    vtmc::StageClock<5> naverode_clock;
    // terrain_navsight.hip: the packed links a smoothed trace makes for itself in every call (scratch, grow-only: the layer keeps nothing
    // of the nav result or the field between calls), and the clock of the last call (the fill of the rows with the packing, the kernel)
    VtmcDevBuf navsight_links;
    vtmc::StageClock<3> navsight_clock;
    // terrain_navcrowd.hip: the crowd on that build, and the clock around the ticks of the last step that ran any
    VtmcNavCrowd navcrowd;
    vtmc::StageClock<2> navcrowd_clock;
    // terrain_water.hip: the last flood, and the clock of its kernels (the levels' labelling, the statistics, the volume)
    VtmcWater water;
    vtmc::StageClock<4> water_clock;
    // terrain_erosion.hip: the state and the maps of the last erosion
    VtmcErosion erosion;
    vtmc::StageClock<4> erosion_clock;   // around the height pass, the steps, and the finish with the write-back of the last erosion
    // terrain_light.hip: the last light result, and the clock of its kernels (the seed passes, the relaxation, the count)
    VtmcLight light;
    vtmc::StageClock<4> light_clock;
    // terrain_lod.hip: the node list of the last level-of-detail result (host, and the copy the gather kernel reads), the packed
    // tiles the kernel gathers (VTMC_TILE_SAMPLES floats per node: the BlockSpace of that result points into them), and the clock around
    // the gather launch of the last extract that succeeded (vtmc_debug_lod_gather_ms)
    std::vector<vtmc_lod_node> lod_nodes;
    VtmcDevBuf lod_nodes_dev, lod_tiles;
    vtmc::StageClock<2> lod_clock;
    // terrain_lodskirt.hip: the skirts of the last vtmc_lod_skirts and the clock of its kernels (armed by a call that launched them)
    VtmcLodSkirt lodskirt;
    vtmc::StageClock<6> lodskirt_clock;
    // terrain_lodattr.hip: per-vertex materials and occlusion of that result and of those skirts, and the clock around the occlusion kernels
    // of the last call that launched them (the nodes' pass, the skirts' pass)
    VtmcLodAttr lodattr;
    vtmc::StageClock<3> lodattr_clock;
    // raycast.hip, spherequery.hip: the queries and hits of vtmc_terrain_raycast / _spherecast / _closest_point (device, then their pinned staging)
    VtmcDevBuf rays;
    VtmcPinnedBuf<unsigned char> h_rays;
    uint64_t perm_seed = 0;
    bool perm_valid = false;
    // terrain_io.hip (vtmc_terrain_save / _load): per-brick flags, kinds, RAW counts, slots and RAW list, the scan's control words, and the
    // two halves of the slice stage on the device and (pinned) on the host; all grow-only, the stages a fixed size
    VtmcDevBuf tio_bricks, tio_stage;
    VtmcPinnedBuf<unsigned char> h_tio;
    // chunk_io.hip: file image being assembled / last image read
    VtmcDevBuf chunk_image;
    // comm.hip: RCCL communicator (opaque ncclComm_t) + the padded send buffer of the counts all-gather
    bool comm_borrowed = false;   // comm belongs to another context (vtmc_comm_share): never destroyed through this one
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    VtmcDevBuf comm_send;
    hipStream_t comm_stream = nullptr;   // the all-gather runs here, beside the emit kernel, when the counts leave the scan
    hipEvent_t ev_gather = nullptr;
    hipEvent_t ev_last_gather = nullptr;   // behind the last all-gather this context queued, on the stream it went to
    bool gather_recorded = false;
    hipEvent_t ev_comm_chain = nullptr;    // owner of a communicator: behind the LAST collective anybody issued through it (the chain of comm.hip)
    hipStream_t comm_chain_stream = nullptr;
    bool comm_chain_recorded = false;
    vtmc_ctx *comm_owner = nullptr;              // borrowed: whose communicator this is
    std::vector<vtmc_ctx *> comm_borrowers;      // owned: the contexts that borrowed it (detached when the owner lets go)
    std::string err;
};

namespace vtmc {
// sets the context's (or, with ctx == nullptr, the thread's create-) error text and returns `code`
int fail(vtmc_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
int ensure(vtmc_ctx *ctx, VtmcDevBuf &b, size_t bytes);  // grow-only device buffer
inline void release(VtmcDevBuf &b) { b.release(); }
template <typename T>
hipError_t pin(VtmcPinnedBuf<T> &b, size_t bytes)   // replaces the buffer; empty when it fails
{
    b.release();
    const hipError_t e = hipHostMalloc((void **)&b.p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) b.bytes = bytes;
    else b.p = nullptr;
    return e;
}
// a context's streams come from (and return to) a per-device pool and are never destroyed -- see StreamPool there
hipError_t take_stream(int device, bool own_queue, int n_cus, hipStream_t *out);
void comm_release(vtmc_ctx *ctx);  // comm.hip: called by vtmc_destroy
int check_dims(vtmc_ctx *ctx, int nx, int ny, int nz);
BlockSpace dense_space(const float *d_base, int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz, int n_volumes, int64_t sv);
float *pinned_stage(vtmc_ctx *ctx, size_t bytes);   // the pinned stage of host-gathered data (vtmc_api.hip), grown to `bytes`; null: none to be had, go pageable
void material_drop(vtmc_ctx *ctx);   // terrain_material.hip: vtmc_terrain_init / _load drop the layer
// whatever invalidates the nav result drops what describes it, the flow field, the border distance and the origin of an erosion, and the
// crowd that stands on it: vtmc_terrain_init / _load and every vtmc_terrain_nav_build
inline void nav_drop(vtmc_ctx *ctx) { ctx->nav.valid = false, ctx->navfield.valid = false, ctx->naverode.dist_valid = false, ctx->naverode.origin_valid = false, ctx->navcrowd.valid = false; }
// vtmc_lod_skirts replaces the skirts: what was computed for the corners of the previous ones names nothing any more
inline void lodattr_drop_skirts(vtmc_ctx *ctx) { ctx->lodattr.values[0][1].epoch = 0, ctx->lodattr.values[1][1].epoch = 0; }
inline void water_drop(vtmc_ctx *ctx) { ctx->water.valid = false; }   // vtmc_terrain_init / _load: the snapshot's grid is gone
inline void erosion_drop(vtmc_ctx *ctx) { ctx->erosion.valid = false; }   // vtmc_terrain_init / _load: the snapshot's grid is gone
inline void light_drop(vtmc_ctx *ctx) { ctx->light.valid = false; }       // vtmc_terrain_init / _load: the snapshot's grid is gone
int upload_block_list(vtmc_ctx *ctx, const int32_t *xyz, int n, BlockSpace &sp);   // sp then walks the (bx,by,bz) list
int extract_core(vtmc_ctx *ctx, const BlockSpace &sp, int n_volumes, ResultSource source, int32_t *tri_count);   // queued on the context's stream and finished
// The vertex attributes of a terrain result (terrain_material.hip, terrain_ao.hip), in vtmc_api.hip.  attr_gate: may `who` compute one for
// the result the context holds (terrain, then result, then its blocks are the dirty list's)?  attr_read / attr_device_results: the
// attribute of the current result to the host / as it lies in device memory; `stale` is the refusal when it is not the current result's.
int attr_gate(vtmc_ctx *ctx, const char *who);
int attr_read(vtmc_ctx *ctx, const VertexAttr &a, const char *stale, size_t bytes_per_vertex, uint8_t *dst, int64_t capacity_vertices);
int attr_device_results(vtmc_ctx *ctx, const VertexAttr &a, const char *stale, const uint8_t **d_values, int64_t *n_vertices);
// terrain.hip, for terrain_io.hip
void history_clear(vtmc_ctx *ctx);
int terrain_extract_all(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count);   // extracts every block of the resident terrain, as an update that dirtied all of them

// terrain_nav.hip, for terrain_naverode.hip: column_offsets from a scanned layout whose tiles are the columns, and the region pass over
// n > 0 spans with final links and parent[i] == i (union, flatten, verify, repeated while the check fails)
struct ScanLayout;
hipError_t nav_launch_offsets(const ScanLayout &scan, int32_t *offsets, hipStream_t stream);
int nav_label_regions(vtmc_ctx *ctx, const char *who, vtmc_nav_span *spans, int32_t *parent, int32_t n, bool timed, int *rounds);
// ... and the box a nav result holds, as terrain_nav.h's sizes take it
struct NavBox;
NavBox nav_held_box(const VtmcNav &nav);

// terrain_navfield.hip, for terrain_navsight.hip: the rows of a trace, plain or smoothed, on their way through the context's query stage
// (surface_query.h): n_starts rows of max_len spans, then n_starts lengths, one block on the device and in pinned memory.
struct TraceRows {
    const int32_t *starts;      // device: the staged starts
    int32_t *paths, *lengths;   // device
    size_t path_bytes, length_bytes, host_off;   // host_off: of the block in ctx->h_rays
};
// stages the starts (their upload is queued on the context's stream) and carves the block; between this and the fetch the caller queues
// the fill of the rows with -1 (0xff bytes over path_bytes) and its kernel
int trace_rows_stage(vtmc_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t max_len, TraceRows *rows);
// behind the kernel: the block comes back, the stream is drained, and the rows and lengths go to the caller's arrays
int trace_rows_fetch(vtmc_ctx *ctx, const TraceRows &rows, int32_t *paths, int32_t *lengths);

// The one kernel launch of this layer: clears the runtime's sticky error word, launches, and returns what this launch left (the rule of
// launch_begin / launch_end in vtmc_internal.h, whose own wrappers in the two files of extract kernels keep the hand-written form).
template <class... Params, class... Args>
hipError_t launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args)
{
    launch_begin();
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    return launch_end();
}
// the grid of a kernel with one lane per element and 256 lanes per workgroup
inline dim3 lanes256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
}  // namespace vtmc

#define VTMC_HIP(ctx, expr)                                                                                \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return vtmc::fail(ctx, VTMC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                                         \
    } while (0)

template <int N>
int vtmc::StageClock<N>::sync_last(vtmc_ctx *ctx) const
{
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipEventSynchronize(ev[N - 1]));
    return VTMC_OK;
}
template <int N>
int vtmc::StageClock<N>::elapsed(vtmc_ctx *ctx, int i, int j, float *ms) const
{
    VTMC_HIP(ctx, hipEventElapsedTime(ms, ev[i], ev[j]));
    return VTMC_OK;
}

#endif
