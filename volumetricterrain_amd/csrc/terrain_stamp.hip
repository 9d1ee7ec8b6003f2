// terrain_stamp.hip -- stamps: density volumes a context keeps in HBM (vtmc_stamp_create / _capture / _info / _read / _destroy) and the
// modifier that pastes one into the resident terrain through a rotation and a uniform pitch (VTMC_MOD_STAMP; not in the reference, whose
// modifiers are analytic).  The 3-D form of the heightmap modifier: a trilinear fetch of the stamp at the sample's position in stamp
// coordinates, then the CSG write of kinds 0-3 or a replacing write.  The rule, operation by operation, is in include/vtmc.h; the kernel
// follows it bit for bit (library built with -ffp-contract=off).
//
// The paste runs on the shared box walk (terrain_box.h): 64 x 4 lanes over (x, z), kYRun samples along y per lane.  Per sample it reads 8
// stamp samples, reads the grid sample and writes it: the 8 reads are gathers whose coalescing depends on the rotation (with the identity a
// wave reads rows of the stamp, x fastest in both), served by L2 for stamps of the sizes an editor pastes (64^3 is 1 MB).  Plain global
// loads, no LDS stage: a workgroup's footprint in the stamp under a free rotation is a slanted slab, not a tile (profiles/r13/stamp).
#include "terrain_edit.h"
#include "terrain_stamp.h"
#include <cmath>
#include <vector>

namespace vtmc {

constexpr int kStampMinDim = 2, kStampMaxDim = 1026;
constexpr long long kStampMaxSamples = 1ll << 27;  // 32-bit indices inside a stamp

struct TerrainStampArgs {
    const float *s;              // the stamp, nx * ny * nz samples, x fastest
    int nx, ny, nz;
    float t[3];                  // p[0..2]: world position of the stamp's centre
    float m[9];                  // M[i][j] at m[3 * i + j]: world offset -> stamp coordinates (inverse rotation over the pitch)
    float c[3];                  // (n_k - 1) / 2: the centre in stamp coordinates
    int lx, ly, lz, dx, dy, dz;  // the clamped sample box, as TerrainModifierArgs
    uint32_t event;
};

enum { kStampAdd = 0, kStampErode = 1, kStampReplace = 2 };

// i = floor(u) and the neighbour above it, clamped to the last sample: at u = n - 1 exactly the weight is 0 and both name sample n - 1
__device__ __forceinline__ void stamp_cell(float u, int n, int &i0, int &i1, float &f)
{
    i0 = (int)floorf(u);
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    f = u - (float)i0;
}

// a + (b - a) * f on the x-pair (i0, i1) of row `row` (the index of its sample 0)
__device__ __forceinline__ float stamp_row(const float *__restrict__ s, int row, int i0, int i1, float f)
{
    const float a = s[row + i0], b = s[row + i1];
    return a + (b - a) * f;
}

// kJournal as terrain_modify_kernel; kMode: kStampAdd / kStampErode (mode 0 with add_or_erode 1 / 0) or kStampReplace (mode 1).
// Along a thread's y-run only the M?1 * dy terms change: the M?0 * dx and M?2 * dz products are formed once (the sums keep the header's
// order).  History off: a sample outside the footprint is neither read nor written; history on: it still goes to the image.
template <bool kJournal, int kMode>
__global__ __launch_bounds__(256) void terrain_stamp_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainStampArgs m)
{
    const BoxThread t;
    if (!t.inside(m)) return;
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    const float dx = px - m.t[0], dz = pz - m.t[2];
    const float ux = m.m[0] * dx, uz = m.m[2] * dz, vx = m.m[3] * dx, vz = m.m[5] * dz, wx = m.m[6] * dx, wz = m.m[8] * dz;
    const float umax = (float)(m.nx - 1), vmax = (float)(m.ny - 1), wmax = (float)(m.nz - 1);
    const float *__restrict__ s = m.s;
    const uint64_t row = box_index(m, t.ix, 0, t.iz);  // image index of (ix, 0, iz); sample iy lies iy rows of dx further
#pragma unroll 4
    for (int iy = t.iy0, iy1 = t.iy1(m); iy < iy1; ++iy) {
        const int y = m.ly + iy;
        const float py = (float)y * sh.scale + sh.origin[1];
        const float dy = py - m.t[1];
        const float u = ((ux + m.m[1] * dy) + uz) + m.c[0];
        const float v = ((vx + m.m[4] * dy) + vz) + m.c[1];
        const float w = ((wx + m.m[7] * dy) + wz) + m.c[2];
        const bool in = u >= 0.0f && u <= umax && v >= 0.0f && v <= vmax && w >= 0.0f && w <= wmax;  // false for a NaN
        if (!kJournal && !in) continue;
        const uint64_t sample = grid_index(sh, x, y, z);
        const float old = kJournal || kMode != kStampReplace ? grid[sample] : 0.0f;
        if (kJournal) image[row + (uint64_t)m.dx * (uint64_t)iy] = old;
        if (!in) continue;
        int i0, i1, j0, j1, k0, k1;
        float fu, fv, fw;
        stamp_cell(u, m.nx, i0, i1, fu);
        stamp_cell(v, m.ny, j0, j1, fv);
        stamp_cell(w, m.nz, k0, k1, fw);
        const int r00 = m.nx * (j0 + m.ny * k0), r10 = m.nx * (j1 + m.ny * k0), r01 = m.nx * (j0 + m.ny * k1), r11 = m.nx * (j1 + m.ny * k1);
        const float a00 = stamp_row(s, r00, i0, i1, fu), a10 = stamp_row(s, r10, i0, i1, fu);
        const float a01 = stamp_row(s, r01, i0, i1, fu), a11 = stamp_row(s, r11, i0, i1, fu);
        const float b0 = a00 + (a10 - a00) * fv, b1 = a01 + (a11 - a01) * fv;
        const float q = b0 + (b1 - b0) * fw;
        float r;
        if (kMode == kStampReplace) {
            r = fabsf(q) <= 2.0f ? q : clamp_drawn(q, sh.seed, m.event, sample, 0u);
        } else {
            const float md = clamp_drawn(q, sh.seed, m.event, sample, 0u);
            r = csg_combine(sh, m.event, sample, kMode == kStampAdd, md, old);
        }
        grid[sample] = r;
    }
}

using StampKernel = void (*)(float *, float *, TerrainShape, TerrainStampArgs);
static StampKernel stamp_kernel(bool journal, int mode)
{
    static const StampKernel k[2][3] = {
        {terrain_stamp_kernel<false, kStampAdd>, terrain_stamp_kernel<false, kStampErode>, terrain_stamp_kernel<false, kStampReplace>},
        {terrain_stamp_kernel<true, kStampAdd>, terrain_stamp_kernel<true, kStampErode>, terrain_stamp_kernel<true, kStampReplace>}};
    return k[journal][mode];
}

static const VtmcStamp *find_stamp(const vtmc_ctx *ctx, int32_t id)
{
    const auto it = ctx->stamps.find(id);
    return it == ctx->stamps.end() ? nullptr : &it->second;
}

// The host half of the rule (include/vtmc.h), in double from the floats of p: the quaternion normalised, its rotation matrix R (stamp
// axes -> world), M = R^T / h rounded once, and the centre in stamp coordinates.
static void stamp_map(const float p[8], const VtmcStamp &st, TerrainStampArgs &a)
{
    double x = p[3], y = p[4], z = p[5], w = p[6];
    const double n = std::sqrt(x * x + y * y + z * z + w * w);
    x /= n, y /= n, z /= n, w /= n;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    const double h = (double)p[7];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a.m[3 * i + j] = (float)(R[j][i] / h);
    const int dims[3] = {st.nx, st.ny, st.nz};
    for (int k = 0; k < 3; ++k) {
        a.t[k] = p[k];
        a.c[k] = (float)(dims[k] - 1) * 0.5f;
    }
}

int check_stamp(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    const float *p = md.p;
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(p[k])) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: stamp parameter p[%d] not finite", i, k);
    const double x = p[3], y = p[4], z = p[5], w = p[6];
    if (!(std::sqrt(x * x + y * y + z * z + w * w) > 0.0)) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: stamp quaternion has length 0", i);
    if (!(p[7] > 0.0f)) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: stamp pitch %g not > 0", i, p[7]);
    if (!find_stamp(ctx, md.data_dims[0])) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: unknown stamp id %d", i, md.data_dims[0]);
    if (md.data_dims[1] < 0 || md.data_dims[1] > 1) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: stamp mode %d not in 0..1", i, md.data_dims[1]);
    return VTMC_OK;
}

int apply_stamp(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image)
{
    const VtmcStamp *st = find_stamp(ctx, md.data_dims[0]);
    if (!st) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown stamp id %d", md.data_dims[0]);  // check_stamp has run: not reached
    TerrainStampArgs s{};
    s.s = (const float *)st->samples.p;
    s.nx = st->nx, s.ny = st->ny, s.nz = st->nz;
    stamp_map(md.p, *st, s);
    s.lx = a.lx, s.ly = a.ly, s.lz = a.lz, s.dx = a.dx, s.dy = a.dy, s.dz = a.dz;
    s.event = a.event;
    const int mode = md.data_dims[1] == 1 ? kStampReplace : (a.add_or_erode ? kStampAdd : kStampErode);
    VTMC_HIP(ctx, launch_box(stamp_kernel(image != nullptr, mode), box_of(a), ctx->stream, grid, image, ctx->tshape, s));
    return VTMC_OK;
}

int check_stamp_dims(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz)
{
    for (int32_t n : {nx, ny, nz})
        if (n < kStampMinDim || n > kStampMaxDim)
            return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp dims %d x %d x %d: each must lie in %d..%d", nx, ny, nz, kStampMinDim, kStampMaxDim);
    if ((long long)nx * ny * nz > kStampMaxSamples)
        return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp dims %d x %d x %d: more than 2^27 samples", nx, ny, nz);
    return VTMC_OK;
}

// a new stamp of the given (checked) dims with its device memory allocated; the id is taken only when that succeeded
int new_stamp(vtmc_ctx *ctx, int32_t nx, int32_t ny, int32_t nz, VtmcStamp &st)
{
    st.nx = nx, st.ny = ny, st.nz = nz;
    return ensure(ctx, st.samples, sizeof(float) * (size_t)nx * (size_t)ny * (size_t)nz);
}

int32_t keep_stamp(vtmc_ctx *ctx, VtmcStamp &st)
{
    const int32_t id = ctx->next_stamp_id++;
    ctx->stamps.emplace(id, std::move(st));
    return id;
}

}  // namespace vtmc

using namespace vtmc;

extern "C" {

int32_t vtmc_stamp_create(vtmc_ctx *ctx, const float *src, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x, int64_t stride_y,
                          int64_t stride_z, int32_t *stamp_id)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!src || !stamp_id) return fail(ctx, VTMC_ERR_INVALID_ARG, "src or stamp_id is null");
    if (int rc = check_stamp_dims(ctx, nx, ny, nz)) return rc;
    if (stride_x <= 0 || stride_y <= 0 || stride_z <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    if (ctx->next_stamp_id == INT32_MAX) return fail(ctx, VTMC_ERR_TOO_LARGE, "stamp ids exhausted");
    std::vector<float> tmp((size_t)nx * ny * nz);
    size_t i = 0;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const float v = src[x * stride_x + y * stride_y + z * stride_z];
                if (!std::isfinite(v)) return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp sample (%d, %d, %d) not finite", x, y, z);
                tmp[i++] = v;
            }
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VtmcStamp st;
    if (int rc = new_stamp(ctx, nx, ny, nz, st)) return rc;
    VTMC_HIP(ctx, hipMemcpy(st.samples.p, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice));
    *stamp_id = keep_stamp(ctx, st);
    return VTMC_OK;
}

int32_t vtmc_stamp_capture(vtmc_ctx *ctx, const int32_t first_sample[3], int32_t nx, int32_t ny, int32_t nz, int32_t *stamp_id)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    if (!ctx->has_terrain) return fail(ctx, VTMC_ERR_NO_RESULT, "stamp_capture before terrain_init");
    if (!first_sample || !stamp_id) return fail(ctx, VTMC_ERR_INVALID_ARG, "first_sample or stamp_id is null");
    if (int rc = check_stamp_dims(ctx, nx, ny, nz)) return rc;
    const TerrainShape &sh = ctx->tshape;
    const int dims[3] = {sh.dim_x, sh.dim_y, sh.dim_z}, n[3] = {nx, ny, nz};
    for (int k = 0; k < 3; ++k)
        if (first_sample[k] < 0 || (long long)first_sample[k] + n[k] > dims[k])
            return fail(ctx, VTMC_ERR_INVALID_ARG, "stamp_capture: samples [%d, %lld) of axis %d reach outside the grid's %d", first_sample[k],
                        (long long)first_sample[k] + n[k], k, dims[k]);
    if (ctx->next_stamp_id == INT32_MAX) return fail(ctx, VTMC_ERR_TOO_LARGE, "stamp ids exhausted");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VtmcStamp st;
    if (int rc = new_stamp(ctx, nx, ny, nz, st)) return rc;
    const TerrainBox b{first_sample[0], first_sample[1], first_sample[2], nx, ny, nz};
    VTMC_HIP(ctx, launch_terrain_copy_box((const float *)ctx->terrain.p, (float *)st.samples.p, sh, b, ctx->stream));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *stamp_id = keep_stamp(ctx, st);
    return VTMC_OK;
}

int32_t vtmc_stamp_info(const vtmc_ctx *ctx, int32_t stamp_id, int32_t dims[3])
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcStamp *st = find_stamp(ctx, stamp_id);
    if (!st) return fail(const_cast<vtmc_ctx *>(ctx), VTMC_ERR_INVALID_ARG, "unknown stamp id %d", stamp_id);
    if (dims) dims[0] = st->nx, dims[1] = st->ny, dims[2] = st->nz;
    return VTMC_OK;
}

int32_t vtmc_stamp_read(vtmc_ctx *ctx, int32_t stamp_id, float *dst, int64_t stride_x, int64_t stride_y, int64_t stride_z)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const VtmcStamp *st = find_stamp(ctx, stamp_id);
    if (!st) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown stamp id %d", stamp_id);
    if (!dst) return fail(ctx, VTMC_ERR_INVALID_ARG, "dst is null");
    if (stride_x <= 0 || stride_y <= 0 || stride_z <= 0) return fail(ctx, VTMC_ERR_INVALID_ARG, "strides must be positive");
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> tmp((size_t)st->nx * st->ny * st->nz);
    VTMC_HIP(ctx, hipMemcpy(tmp.data(), st->samples.p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    size_t i = 0;
    for (int z = 0; z < st->nz; ++z)
        for (int y = 0; y < st->ny; ++y)
            for (int x = 0; x < st->nx; ++x) dst[x * stride_x + y * stride_y + z * stride_z] = tmp[i++];
    return VTMC_OK;
}

int32_t vtmc_stamp_destroy(vtmc_ctx *ctx, int32_t stamp_id)
{
    if (!ctx) return VTMC_ERR_INVALID_ARG;
    const auto it = ctx->stamps.find(stamp_id);
    if (it == ctx->stamps.end()) return fail(ctx, VTMC_ERR_INVALID_ARG, "unknown stamp id %d", stamp_id);
    VTMC_HIP(ctx, hipSetDevice(ctx->device));
    VTMC_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a paste of a queued update may still be reading it
    ctx->stamps.erase(it);
    return VTMC_OK;
}

}  // extern "C"
