// terrain_fragments.hip -- what is still attached to the ground: connected-component labelling of the solid samples (s > 0) of a box of
// the resident grid, behind the fragment query (vtmc_terrain_fragments) and the modifier that removes fragments (VTMC_MOD_DETACH).  Not in
// the reference.  The rule -- 6-connectivity inside the box, anchored = touches a face of the box, seed = smallest grid index -- is in
// include/vtmc.h; everything here is integers and 32-bit copies.  Hand-written for gfx950 / CDNA4.
//
// Labels are box-linear int32 indices (1026^3 < 2^31); box-linear order is grid-index order, so "root = smallest index" is the seed.
// Scratch: a parent word and an auxiliary word per sample of the box (8 bytes per sample, grow-only, vtmc_ctx.h).  Three phases, each a
// kernel of its own, so that a kernel boundary stands between every phase and the next one's reads:
//   1. frag_local_kernel   tiles of 64 x 8 x 8 samples (long in x, the stride-1 axis: a wave reads 256 contiguous bytes), union-find in
//                          LDS over the runs along x (a run is one ballot); leaves every solid sample pointing at the smallest index of
//                          its piece of the tile, -1 in the others.  The one read of the grid.
//   2. frag_merge_kernel   the samples on a tile's low faces join their neighbour across the face: union by smaller index on the global
//                          parent array (tile_label.h, shared with terrain_water.hip, as are the tile constants and the row walk).
//   3. frag_flatten_kernel every sample to its root; fused with the per-root sample counts (reduced per run of a wave before the atomic).
// Between 2 and 3, frag_anchor_kernel walks the six faces of the box and marks the roots it meets.
//
// VISIBILITY inside the merge kernel: the parent array is written by workgroups on other XCDs while it is read.  The union (union_find.h)
// is written so that ONLY THE VALUE THE ATTACHING ATOMIC RETURNS DECIDES whether it is done: a root a is attached under a smaller root b by
// a compare-and-swap of parent[a] from a to b, and the union is complete only if that succeeds (a was still a root at that moment);
// otherwise it goes on with (old, b), which must still meet.  Every parent value ever written is a smaller index of the same tree, so a
// stale read names an older ancestor: it can cost a retry, never a wrong answer.  The reads are relaxed agent-scope atomic loads all the
// same, which keeps the retries few.  Path compression is an atomicMin, on nodes that are no roots.
//
// EVERY LOOP IS BOUNDED, twice: a walk up the parents must strictly decrease the index and a union's retry must strictly decrease its
// larger root (both hold on any valid input), and each loop also counts against the number of samples.  A violation sets a
// flag word and ends the loop; the query answers VTMC_ERR_DEVICE ("labelling did not converge"), the detach kernel writes nothing.
#include "terrain_edit.h"
#include "terrain_fragments.h"
#include "terrain_stamp.h"
#include "tile_label.h"
#include <climits>
#include <cstring>
#include <vector>

namespace vtmc {

constexpr uint32_t kAnchoredBit = 0x80000000u;   // aux[root]: anchored; the bits below it count the samples of an unanchored root (<= 2^30)
enum { kCtlFlag = 0, kCtlCount = 1, kCtlSlots = 2, kCtlWords = 16 };

// Phase 1.  64 x 4 threads; thread (tx, tq) owns the 16 samples (tx, r & 7, r >> 3), r = tq + 4 k, of the tile, so a wave holds one row
// of 64 samples along x at a time.  A row's solid mask is one ballot: every sample starts out pointing at the first sample of its run
// along x (no union along x at all), and two neighbouring rows need one union per stretch in which both are solid, made by the
// stretch's first lane -- within a stretch both rows are one run each.
__global__ __launch_bounds__(256) void frag_local_kernel(const float *__restrict__ grid, int *__restrict__ P, uint32_t *__restrict__ aux,
                                                         int *__restrict__ flag, TerrainShape sh, TerrainBox b)
{
    __shared__ int L[kTileSamples];
    __shared__ unsigned long long M[kTileY * kTileZ];   // the solid mask of row r
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int tx = threadIdx.x, tq = threadIdx.y;
    const int ix = blockIdx.x * kTileX + tx, y0 = blockIdx.y * kTileY, z0 = blockIdx.z * kTileZ;
    unsigned solid = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        bool s = false;
        if (ix < b.dx && y0 + ly < b.dy && z0 + lz < b.dz) s = grid[grid_index(sh, b.lx + ix, b.ly + y0 + ly, b.lz + z0 + lz)] > 0.0f;
        const unsigned long long mask = __ballot(s);
        if (tx == 0) M[r] = mask;
        const unsigned long long air_below = ~mask & ((1ull << tx) - 1ull);   // the lanes below tx that are not solid
        L[li] = s ? kTileX * r + (air_below ? 64 - __clzll((long long)air_below) : 0) : -1;
        solid |= (unsigned)s << k;
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        if (!(solid >> k & 1)) continue;
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        const unsigned long long here = M[r];
        if (ly > 0) {
            const unsigned long long both = here & M[r - 1];
            if ((both >> tx & 1) && !(tx > 0 && (both >> (tx - 1) & 1))) uf_union<kScope, false>(L, li, li - kTileX, kTileSamples, flag);
        }
        if (lz > 0) {
            const unsigned long long both = here & M[r - kTileY];
            if ((both >> tx & 1) && !(tx > 0 && (both >> (tx - 1) & 1))) uf_union<kScope, false>(L, li, li - kTileX * kTileY, kTileSamples, flag);
        }
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int r = tq + 4 * k, ly = r & 7, lz = r >> 3, li = tx + kTileX * r;
        if (!(ix < b.dx && y0 + ly < b.dy && z0 + lz < b.dz)) continue;
        int label = -1;
        if (solid >> k & 1) {
            const int root = uf_find<kScope>(L, li, kTileSamples, flag);
            // a failed find leaves the sample its own root: the flag is set, nothing reads the labels
            const int rl = root < 0 ? li : root;
            label = frag_index(b, blockIdx.x * kTileX + (rl & (kTileX - 1)), y0 + (rl / kTileX & (kTileY - 1)), z0 + rl / (kTileX * kTileY));
        }
        const int j = frag_index(b, ix, y0 + ly, z0 + lz);
        P[j] = label;
        aux[j] = 0u;
    }
}

// Phase 2 (tile_label.h).
__global__ __launch_bounds__(256) void frag_merge_kernel(int *__restrict__ P, int *__restrict__ flag, TerrainBox b, int n) { label_merge(P, flag, b, n); }

// The six faces of the box, one thread per face sample (edges twice): the root above a solid one is anchored.
__global__ __launch_bounds__(256) void frag_anchor_kernel(const int *__restrict__ P, uint32_t *__restrict__ aux, int *__restrict__ flag, TerrainBox b, int n)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const long long xy = (long long)b.dx * b.dy, xz = (long long)b.dx * b.dz, yz = (long long)b.dy * b.dz;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int x, y, z;
    bool in = true;
    if (i < 2 * xy) {
        const int r = (int)(i % xy);
        x = r % b.dx, y = r / b.dx, z = i < xy ? 0 : b.dz - 1;
    } else if ((i -= 2 * xy) < 2 * xz) {
        const int r = (int)(i % xz);
        x = r % b.dx, z = r / b.dx, y = i < xz ? 0 : b.dy - 1;
    } else if ((i -= 2 * xz) < 2 * yz) {
        const int r = (int)(i % yz);
        y = r % b.dy, z = r / b.dy, x = i < yz ? 0 : b.dx - 1;
    } else {
        x = y = z = 0;
        in = false;
    }
    int root = -1;
    if (in) {
        const int j = frag_index(b, x, y, z);
        if (uf_load<kScope>(P, j) >= 0) root = uf_find<kScope>(P, j, n, flag);
    }
    if (run_length(root) > 0 && !(aux[root] & kAnchoredBit)) atomicOr(aux + root, kAnchoredBit);
}

// Phase 3, and the counts: a run of a wave that shares an unanchored root adds its length with one atomic.  Anchored roots -- the ground,
// most of the samples -- are not counted at all.
__global__ __launch_bounds__(256) void frag_flatten_kernel(int *__restrict__ P, uint32_t *__restrict__ aux, int *__restrict__ flag, TerrainBox b, int n)
{
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const RowThread t;
    int key = -1;
    if (t.inside(b)) {
        const int j = frag_index(b, t.ix, t.iy, t.iz);
        if (uf_load<kScope>(P, j) >= 0) {
            const int root = uf_find<kScope>(P, j, n, flag);
            if (root >= 0) {
                P[j] = root;
                if (!(aux[root] & kAnchoredBit)) key = root;
            }
        }
    }
    const int len = run_length(key);
    if (len > 0) atomicAdd(aux + key, (uint32_t)len);
}

__device__ __forceinline__ bool is_fragment(uint32_t a, int max_samples) { return !(a & kAnchoredBit) && (max_samples == 0 || a <= (uint32_t)max_samples); }

// VTMC_MOD_DETACH on the shared box walk: every sample of every fragment takes the erode write of a clamped density 2.
template <bool kJournal>
__global__ __launch_bounds__(256) void frag_detach_kernel(float *__restrict__ grid, float *__restrict__ image, const int *__restrict__ P,
                                                          const uint32_t *__restrict__ aux, const int *__restrict__ ctl, TerrainShape sh,
                                                          TerrainBox b, uint32_t event, int max_samples)
{
    const BoxThread t;
    if (!t.inside(b)) return;
    const bool sound = ctl[kCtlFlag] == 0;
    for (int iy = t.iy0, iy1 = t.iy1(b); iy < iy1; ++iy) {
        const int j = frag_index(b, t.ix, iy, t.iz);
        const uint64_t sample = grid_index(sh, b.lx + t.ix, b.ly + iy, b.lz + t.iz);
        const int root = P[j];
        if (!kJournal && root < 0) continue;
        const float s = grid[sample];
        if (kJournal) image[j] = s;
        if (root >= 0 && sound && is_fragment(aux[root], max_samples)) grid[sample] = csg_combine(sh, event, sample, 0, 2.0f, s);
    }
}

// the query: how many roots are fragments
__global__ __launch_bounds__(256) void frag_count_kernel(const int *__restrict__ P, const uint32_t *__restrict__ aux, int *__restrict__ ctl, TerrainBox b,
                                                        int max_samples)
{
    const RowThread t;
    bool frag = false;
    if (t.inside(b)) {
        const int j = frag_index(b, t.ix, t.iy, t.iz);
        frag = P[j] == j && is_fragment(aux[j], max_samples);
    }
    const unsigned long long m = __ballot(frag);
    if (m && __lane_id() == 0) atomicAdd(ctl + kCtlCount, __popcll(m));
}

// the query: every fragment's root takes a slot of the record list (one atomic per wave); aux[root] becomes slot + 1, 0 for the other roots
__global__ __launch_bounds__(256) void frag_select_kernel(const int *__restrict__ P, uint32_t *__restrict__ aux, int *__restrict__ ctl,
                                                         FragmentRecord *__restrict__ recs, TerrainBox b, int max_samples, int capacity)
{
    const RowThread t;
    bool frag = false, root = false;
    int j = 0;
    uint32_t a = 0;
    if (t.inside(b)) {
        j = frag_index(b, t.ix, t.iy, t.iz);
        root = P[j] == j;
        a = aux[j];
        frag = root && is_fragment(a, max_samples);
    }
    const unsigned long long m = __ballot(frag);
    const int lane = __lane_id();
    int base = 0;
    if (m && lane == 0) base = atomicAdd(ctl + kCtlSlots, __popcll(m));
    base = __shfl(base, 0);
    if (frag) {
        const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < capacity) {
            FragmentRecord r;
            r.root = j, r.n_samples = (int)a;
            r.lo[0] = r.lo[1] = r.lo[2] = INT_MAX;
            r.hi[0] = r.hi[1] = r.hi[2] = INT_MIN;
            recs[slot] = r;
            aux[j] = (uint32_t)slot + 1u;
        } else {
            aux[j] = 0u;
        }
    } else if (root) {
        aux[j] = 0u;
    }
}

// the query: tight bounds, in grid samples; a run of a wave lies in one row, so its first lane reduces for all of it
__global__ __launch_bounds__(256) void frag_bounds_kernel(const int *__restrict__ P, const uint32_t *__restrict__ aux, FragmentRecord *__restrict__ recs,
                                                         TerrainBox b)
{
    const RowThread t;
    int key = -1;
    if (t.inside(b)) {
        const int root = P[frag_index(b, t.ix, t.iy, t.iz)];
        if (root >= 0) key = (int)aux[root] - 1;
    }
    const int len = run_length(key);
    if (len > 0) {
        FragmentRecord *r = recs + key;
        const int x = b.lx + t.ix, y = b.ly + t.iy, z = b.lz + t.iz;
        atomicMin(&r->lo[0], x);
        atomicMax(&r->hi[0], x + len - 1);
        atomicMin(&r->lo[1], y);
        atomicMax(&r->hi[1], y);
        atomicMin(&r->lo[2], z);
        atomicMax(&r->hi[2], z);
    }
}

// the query's capture: the stamp box sb (inside the query box b) with every other solid piece turned into equally deep air
__global__ __launch_bounds__(256) void frag_capture_kernel(const float *__restrict__ grid, const int *__restrict__ P, float *__restrict__ stamp,
                                                          TerrainShape sh, TerrainBox b, TerrainBox sb, int root)
{
    const BoxThread t;
    if (!t.inside(sb)) return;
    for (int iy = t.iy0, iy1 = t.iy1(sb); iy < iy1; ++iy) {
        const int x = sb.lx + t.ix, y = sb.ly + iy, z = sb.lz + t.iz;
        const float s = grid[grid_index(sh, x, y, z)];
        const int r = P[frag_index(b, x - b.lx, y - b.ly, z - b.lz)];
        stamp[box_index(sb, t.ix, iy, t.iz)] = r < 0 || r == root ? s : -s;
    }
}

// The scratch of a box of n samples.  Grown only after the stream has drained: an earlier detach of the same queue may still be reading it.
static int fragment_scratch(vtmc_ctx *ctx, size_t n)
{
    if (ctx->frag_labels.bytes < 8 * n || ctx->frag_ctl.bytes < kCtlWords * sizeof(int)) {
        VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (int rc = ensure(ctx, ctx->frag_labels, 8 * n)) return rc;
        if (int rc = ensure(ctx, ctx->frag_ctl, kCtlWords * sizeof(int))) return rc;
    }
    return VTMC_OK;
}

// Queues the labelling of the non-empty box b on ctx->stream: afterwards P[j] is the root of every solid sample j (-1: not solid) and
// aux[root] holds the anchored bit or, without it, the sample count.  ctl is cleared first.
static int label_box(vtmc_ctx *ctx, const float *grid, const TerrainBox &b, int **P_out, uint32_t **aux_out, int **ctl_out)
{
    const size_t n = (size_t)b.dx * b.dy * b.dz;
    if (int rc = fragment_scratch(ctx, n)) return rc;
    int *P = (int *)ctx->frag_labels.p, *ctl = (int *)ctx->frag_ctl.p;
    uint32_t *aux = (uint32_t *)ctx->frag_labels.p + n;
    const TerrainShape &sh = ctx->tshape;
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, hipMemsetAsync(ctl, 0, kCtlWords * sizeof(int), s));
    VTMC_HIP(ctx, launch(frag_local_kernel, tile_grid(b), dim3(64, 4, 1), 0, s, grid, P, aux, ctl + kCtlFlag, sh, b));
    VTMC_HIP(ctx, launch_rows(frag_merge_kernel, b, s, P, ctl + kCtlFlag, b, (int)n));
    const long long faces = 2 * ((long long)b.dx * b.dy + (long long)b.dx * b.dz + (long long)b.dy * b.dz);
    VTMC_HIP(ctx, launch(frag_anchor_kernel, lanes256(faces), dim3(256), 0, s, P, aux, ctl + kCtlFlag, b, (int)n));
    VTMC_HIP(ctx, launch_rows(frag_flatten_kernel, b, s, P, aux, ctl + kCtlFlag, b, (int)n));
    *P_out = P, *aux_out = aux, *ctl_out = ctl;
    return VTMC_OK;
}

int check_detach(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    if (const char *what = detach_fault(md)) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: %s", i, what);
    return VTMC_OK;
}

// No host read-back: should the labelling fail its bounds (a defect, never an input), the write kernel sees the flag and writes nothing.
int apply_detach(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image)
{
    const TerrainBox b = box_of(a);
    int *P, *ctl;
    uint32_t *aux;
    if (int rc = label_box(ctx, grid, b, &P, &aux, &ctl)) return rc;
    VTMC_HIP(ctx, launch_box(image ? frag_detach_kernel<true> : frag_detach_kernel<false>, b, ctx->stream, grid, image, (const int *)P, (const uint32_t *)aux,
                             (const int *)ctl, ctx->tshape, b, a.event, (int)md.data_dims[0]));
    return VTMC_OK;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_terrain_fragments(vtmc_ctx *ctx, const float lower[3], const float upper[3], int32_t max_samples, int32_t capture_min_samples,
                               vtmc_fragment *dst, int32_t capacity, int32_t *n_fragments)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (n_fragments) *n_fragments = 0;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "terrain_fragments before terrain_init");
    if (const char *what = fragments_args_fault(lower, upper, max_samples, capture_min_samples)) return fail(ctx, VTMC_ERR_INVALID_ARG, "terrain_fragments: %s", what);
    const TerrainShape &sh = ctx->tshape;
    const TerrainBox b = bounds_box(sh, lower, upper);
    if (box_empty(b)) return VTMC_OK;
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    int *P, *ctl;
    uint32_t *aux;
    if (int rc = label_box(ctx, (const float *)ctx->terrain.p, b, &P, &aux, &ctl)) return rc;
    hipStream_t s = ctx->stream;
    VTMC_HIP(ctx, launch_rows(frag_count_kernel, b, s, (const int *)P, (const uint32_t *)aux, ctl, b, (int)max_samples));
    int h_ctl[kCtlWords];
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    VTMC_HIP(ctx, hipMemcpy(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost));
    if (h_ctl[kCtlFlag]) return fail(ctx, VTMC_ERR_DEVICE, "terrain_fragments: labelling did not converge (flag %d)", h_ctl[kCtlFlag]);
    const int32_t n = h_ctl[kCtlCount];
    if (n_fragments) *n_fragments = n;
    if (!dst) return VTMC_OK;   // count only
    if (capacity < n) return fail(ctx, VTMC_ERR_CAPACITY, "capacity %d < %d fragments", capacity, n);
    if (n == 0) return VTMC_OK;
    if (int rc = ensure(ctx, ctx->frag_records, sizeof(FragmentRecord) * (size_t)n)) return rc;
    FragmentRecord *d_recs = (FragmentRecord *)ctx->frag_records.p;
    VTMC_HIP(ctx, launch_rows(frag_select_kernel, b, s, (const int *)P, aux, ctl, d_recs, b, (int)max_samples, (int)n));
    VTMC_HIP(ctx, launch_rows(frag_bounds_kernel, b, s, (const int *)P, (const uint32_t *)aux, d_recs, b));
    std::vector<FragmentRecord> recs((size_t)n);
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    VTMC_HIP(ctx, hipMemcpy(recs.data(), d_recs, sizeof(FragmentRecord) * (size_t)n, hipMemcpyDeviceToHost));
    const int32_t box_lo[3] = {b.lx, b.ly, b.lz}, box_d[3] = {b.dx, b.dy, b.dz};
    fragments_order(recs, box_lo, box_d, dst);
    if (capture_min_samples <= 0) return VTMC_OK;
    // capture: the stamps enter the context's table only once nothing can fail any more; until then they free themselves
    std::vector<std::pair<int32_t, VtmcStamp>> made;
    for (int32_t i = 0; i < n; ++i) {
        int32_t first[3], dims[3];
        if (dst[i].n_samples < capture_min_samples || !fragment_stamp_box(dst[i], box_lo, box_d, first, dims)) continue;
        if ((int64_t)ctx->next_stamp_id + (int64_t)made.size() >= INT32_MAX) return fail(ctx, VTMC_ERR_TOO_LARGE, "stamp ids exhausted");
        VtmcStamp st;
        if (int rc = new_stamp(ctx, dims[0], dims[1], dims[2], st)) return rc;
        const TerrainBox sb{first[0], first[1], first[2], dims[0], dims[1], dims[2]};
        VTMC_HIP(ctx, launch_box(frag_capture_kernel, sb, s, (const float *)ctx->terrain.p, (const int *)P, (float *)st.samples.p, sh, b, sb, recs[i].root));
        made.emplace_back(i, std::move(st));
    }
    VTMC_HIP(ctx, hipStreamSynchronize(s));
    for (auto &m : made) dst[m.first].stamp_id = keep_stamp(ctx, m.second);
    return VTMC_OK;
}

}  // extern "C"
