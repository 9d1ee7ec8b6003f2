// terrain_noise.hip -- the noise modifier of the resident terrain (VTMC_MOD_NOISE: fBm, billow, ridged multifractal; the reference's
// RidgedMultifractalModifier wraps LibNoise, which it does not vendor: the values here are the library's own Perlin, perlin_device.h): its
// kernel, check and apply, an entry of the modifier table (terrain_edit.h).  The CSG write is that of kinds 0-3 (terrain_box.h).
#include "perlin_device.h"
#include "terrain_edit.h"
#include <algorithm>
#include <cmath>

namespace vtmc {

// Its own kernel arguments, not TerrainModifierArgs (which every other kernel carries): the 256-byte permutation travels by value, so an
// edit needs no device allocation, no upload and no host wait.
struct TerrainNoiseArgs {
    int add_or_erode;
    float frequency, lacunarity, gain, amplitude, bias, ramp_scale, ramp_center, ridge_offset;  // vtmc_modifier.p[0..7]
    int octaves;
    int lx, ly, lz, dx, dy, dz;  // the clamped sample box, as TerrainModifierArgs
    uint32_t event;
    unsigned char perm[256];     // density_permutation((uint64_t)(uint32_t)seed)
};

// one octave's contribution: sum and the ridged basis' running weight w, from the octave's noise value n
template <int kBasis>
__device__ __forceinline__ void noise_octave(float n, float amp, float ridge_offset, float &sum, float &w)
{
    if (kBasis == 0) {          // fBm
        sum = sum + amp * n;
    } else if (kBasis == 1) {   // billow
        float t = fabsf(n);
        t = t + t;
        t = t - 1.0f;
        sum = sum + amp * t;
    } else {                    // ridged multifractal
        float r = ridge_offset - fabsf(n);
        r = r * r;
        r = r * w;
        w = r + r;
        w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
        sum = sum + amp * r;
    }
}

// what a sample becomes: q from its octave sum, its clamp draws, then the CSG write
__device__ __forceinline__ float noise_write(const TerrainShape &sh, const TerrainNoiseArgs &m, float sum, float py, uint64_t sample, float s)
{
    float q = m.amplitude * sum;
    q = q + m.bias;
    q = q - (py - m.ramp_center) * m.ramp_scale;
    const float md = clamp_drawn(q, sh.seed, m.event, sample, 0u);
    return csg_combine(sh, m.event, sample, m.add_or_erode, md, s);
}

// VALU-bound (octaves x ~100 FP32 operations against 8-12 bytes per sample), unlike the other edit kernels.  The octave loop is the OUTER one:
// what an octave needs of x and z (perlin_column) is evaluated once and serves the kYRun samples of the thread's run, whose octave
// coordinates, sums and ridge weights stay in registers (3 x kYRun).  Every sample still sees its own operations in the header's order,
// so the interchange keeps the bits.  A run's tail past the box is evaluated and never loaded or stored.
// VTMC_NOISE_PER_SAMPLE builds the plain form (noise3 per sample and octave) for the comparison in profiles/r11/noise/README.md.
template <bool kJournal, int kBasis>
__global__ __launch_bounds__(256) void terrain_noise_kernel(float *__restrict__ grid, float *__restrict__ image, TerrainShape sh, TerrainNoiseArgs m)
{
    __shared__ unsigned s_perm[512];  // 32-bit entries, the table twice: a lookup is one ds_read_b32 with no index wrap
    {
        const int t = threadIdx.y * 64 + threadIdx.x;
        const unsigned v = m.perm[t];
        s_perm[t] = v;
        s_perm[t + 256] = v;
    }
    __syncthreads();
    const PermWords P{s_perm};
    const BoxThread t;
    if (!t.inside(m)) return;
    const int x = m.lx + t.ix, z = m.lz + t.iz;
    const float px = (float)x * sh.scale + sh.origin[0];
    const float pz = (float)z * sh.scale + sh.origin[2];
    const int iy1 = t.iy1(m);
    const uint64_t s0 = grid_index(sh, x, m.ly + t.iy0, z), j0 = box_index(m, t.ix, t.iy0, t.iz);  // sample k of the run: k rows further
#ifndef VTMC_NOISE_PER_SAMPLE
    float yo[kYRun], sum[kYRun], w[kYRun];
#pragma unroll
    for (int k = 0; k < kYRun; ++k) {
        const float py = (float)(m.ly + t.iy0 + k) * sh.scale + sh.origin[1];
        yo[k] = py * m.frequency;
        sum[k] = 0.0f;
        w[k] = 1.0f;
    }
    float xo = px * m.frequency, zo = pz * m.frequency, amp = 1.0f;
    for (int o = 0; o < m.octaves; ++o) {
        const PerlinColumn c = perlin_column(P, xo, zo);
#pragma unroll
        for (int k = 0; k < kYRun; ++k) {
            noise_octave<kBasis>(perlin_at(P, c, yo[k]), amp, m.ridge_offset, sum[k], w[k]);
            yo[k] = yo[k] * m.lacunarity;
        }
        xo = xo * m.lacunarity;
        zo = zo * m.lacunarity;
        amp = amp * m.gain;
    }
    float old[kYRun];  // every load of the run is issued before the first store, as terrain_swap_kernel
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) old[k] = grid[s0 + (uint64_t)sh.dim_x * k];
#pragma unroll
    for (int k = 0; k < kYRun; ++k)
        if (t.iy0 + k < iy1) {
            const float py = (float)(m.ly + t.iy0 + k) * sh.scale + sh.origin[1];  // again rather than kept: kYRun registers
            const uint64_t sample = s0 + (uint64_t)sh.dim_x * k;
            if (kJournal) image[j0 + (uint64_t)m.dx * k] = old[k];
            grid[sample] = noise_write(sh, m, sum[k], py, sample, old[k]);
        }
#else
    for (int k = 0; t.iy0 + k < iy1; ++k) {
        const float py = (float)(m.ly + t.iy0 + k) * sh.scale + sh.origin[1];
        float xo = px * m.frequency, yo = py * m.frequency, zo = pz * m.frequency, amp = 1.0f, sum = 0.0f, w = 1.0f;
        for (int o = 0; o < m.octaves; ++o) {
            noise_octave<kBasis>(noise3(P, xo, yo, zo), amp, m.ridge_offset, sum, w);
            xo = xo * m.lacunarity;
            yo = yo * m.lacunarity;
            zo = zo * m.lacunarity;
            amp = amp * m.gain;
        }
        const uint64_t sample = s0 + (uint64_t)sh.dim_x * k;
        const float s = grid[sample];
        if (kJournal) image[j0 + (uint64_t)m.dx * k] = s;
        grid[sample] = noise_write(sh, m, sum, py, sample, s);
    }
#endif
}

// VTMC_MOD_NOISE: data_dims[1] = octaves | basis << 8
static int noise_octaves(const vtmc_modifier &md) { return md.data_dims[1] & 255; }
static int noise_basis(const vtmc_modifier &md) { return md.data_dims[1] >> 8; }

// The largest magnitude a lattice coordinate of a (checked: finite parameters, octaves 1..16) noise modifier can take inside its clamped
// sample box: the box's world corners (positions are monotonic in the index) times |f| * max(1, |L|)^(octaves - 1).  From 2^24 on the
// lattice fraction carries no information, and further out the float -> int conversion differs between targets.
static double noise_lattice_reach(const TerrainShape &sh, const vtmc_modifier &md)
{
    int low[3], up[3];
    const TerrainModifierArgs a = sample_range(sh, md, low, up);
    if (box_empty(box_of(a))) return 0.0;  // no sample is evaluated
    const int first[3] = {a.lx, a.ly, a.lz}, ext[3] = {a.dx, a.dy, a.dz};
    double reach = 0.0;
    for (int k = 0; k < 3; ++k)
        for (int idx : {first[k], first[k] + ext[k] - 1}) reach = std::max(reach, (double)std::fabs((float)idx * sh.scale + sh.origin[k]));
    return reach * std::fabs((double)md.p[0]) * std::pow(std::max(1.0, std::fabs((double)md.p[1])), noise_octaves(md) - 1);
}

static TerrainNoiseArgs noise_args(const vtmc_modifier &md, const TerrainModifierArgs &a)
{
    TerrainNoiseArgs n{};
    n.add_or_erode = a.add_or_erode;
    n.frequency = md.p[0], n.lacunarity = md.p[1], n.gain = md.p[2], n.amplitude = md.p[3], n.bias = md.p[4];
    n.ramp_scale = md.p[5], n.ramp_center = md.p[6], n.ridge_offset = md.p[7];
    n.octaves = noise_octaves(md);
    n.lx = a.lx, n.ly = a.ly, n.lz = a.lz, n.dx = a.dx, n.dy = a.dy, n.dz = a.dz;
    n.event = a.event;
    density_permutation((uint64_t)(uint32_t)md.data_dims[0], n.perm);  // the C# int _seed
    return n;
}

using NoiseKernel = void (*)(float *, float *, TerrainShape, TerrainNoiseArgs);
static NoiseKernel noise_kernel(bool journal, int basis)
{
    static const NoiseKernel k[2][3] = {{terrain_noise_kernel<false, 0>, terrain_noise_kernel<false, 1>, terrain_noise_kernel<false, 2>},
                                        {terrain_noise_kernel<true, 0>, terrain_noise_kernel<true, 1>, terrain_noise_kernel<true, 2>}};
    return k[journal][basis];
}

int check_noise(vtmc_ctx *ctx, const vtmc_modifier &md, int32_t i)
{
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(md.p[k])) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: noise parameter p[%d] not finite", i, k);
    const int octaves = noise_octaves(md), basis = noise_basis(md);
    if (octaves < 1 || octaves > 16) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: noise octaves %d not in 1..16", i, octaves);
    if (basis < 0 || basis > 2) return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: noise basis %d not in 0..2", i, basis);
    const double reach = noise_lattice_reach(ctx->tshape, md);
    if (!(reach < 16777216.0))
        return fail(ctx, VTMC_ERR_INVALID_ARG, "modifier %d: noise lattice coordinates reach %g in its box (limit 2^24)", i, reach);
    return VTMC_OK;
}

int apply_noise(vtmc_ctx *ctx, const vtmc_modifier &md, const TerrainModifierArgs &a, float *grid, float *image)
{
    VTMC_HIP(ctx, launch_box(noise_kernel(image != nullptr, noise_basis(md)), box_of(a), ctx->stream, grid, image, ctx->tshape, noise_args(md, a)));
    return VTMC_OK;
}

}  // namespace vtmc
