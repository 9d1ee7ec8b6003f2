// perlin_device.h -- the library's one Perlin: Ken Perlin's 2002 improved noise over a 256-entry permutation (density_permutation), as
// oracle/density_ref.c states it.  Shared by density.hip (the benchmark volumes' per-sample kernel) and terrain_noise.hip (VTMC_MOD_NOISE).
// FP32, one IEEE operation per step (the library is built with -ffp-contract=off), so a sample's bits depend on its position alone.
//
// A sample is split where the terrain's box walk splits it: perlin_column is everything that depends on x and z only (lattice cell,
// fractions, fade weights, the P(X) / P(X + 1) stage of the hash), perlin_at finishes one y of that column.  noise3 is the two in a
// row; a kernel that walks a run of y evaluates the column once and reuses identical values, which keeps the bits.
#ifndef VTMC_PERLIN_DEVICE_H
#define VTMC_PERLIN_DEVICE_H
#include <hip/hip_runtime.h>

namespace vtmc {

__device__ __forceinline__ float fade(float t) { return t * t * t * (t * (t * 6.0f - 15.0f) + 10.0f); }
__device__ __forceinline__ float mixf(float t, float a, float b) { return a + t * (b - a); }
__device__ __forceinline__ float gradf(int hash, float x, float y, float z)
{
    int h = hash & 15;
    float u = h < 8 ? x : y;
    float v = h < 4 ? y : ((h == 12 || h == 14) ? x : z);
    return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}

// P(i) of the definition, i >= 0: the permutation as it lies in memory
struct PermBytes {   // 256 bytes, the index wrapped
    const unsigned char *p;
    __device__ __forceinline__ int operator()(int i) const { return (int)p[i & 255]; }
};
struct PermWords {   // 512 dwords, entry i = perm[i & 255]: no index of a sample exceeds 255 + 255 + 1, so nothing is wrapped
    const unsigned *p;
    __device__ __forceinline__ int operator()(int i) const { return (int)p[i]; }
};

struct PerlinColumn {
    float x, x1, z, z1;  // fractions along x and z, and the same minus one
    float u, w;          // fade(x), fade(z)
    int a, b;            // P(X), P(X + 1)
    int Z;               // lattice cell along z, & 255
};

template <class Perm>
__device__ __forceinline__ PerlinColumn perlin_column(const Perm &P, float x, float z)
{
    PerlinColumn c;
    const float fx = floorf(x), fz = floorf(z);
    const int X = (int)fx & 255;
    c.Z = (int)fz & 255;
    c.x = x - fx;
    c.z = z - fz;
    c.x1 = c.x - 1;
    c.z1 = c.z - 1;
    c.u = fade(c.x);
    c.w = fade(c.z);
    c.a = P(X);
    c.b = P(X + 1);
    return c;
}

template <class Perm>
__device__ __forceinline__ float perlin_at(const Perm &P, const PerlinColumn &c, float y)
{
    const float fy = floorf(y);
    const int Y = (int)fy & 255;
    y -= fy;
    const float v = fade(y), y1 = y - 1;
    const int A = c.a + Y, AA = P(A) + c.Z, AB = P(A + 1) + c.Z;
    const int B = c.b + Y, BA = P(B) + c.Z, BB = P(B + 1) + c.Z;
    return mixf(c.w,
                mixf(v, mixf(c.u, gradf(P(AA), c.x, y, c.z), gradf(P(BA), c.x1, y, c.z)),
                     mixf(c.u, gradf(P(AB), c.x, y1, c.z), gradf(P(BB), c.x1, y1, c.z))),
                mixf(v, mixf(c.u, gradf(P(AA + 1), c.x, y, c.z1), gradf(P(BA + 1), c.x1, y, c.z1)),
                     mixf(c.u, gradf(P(AB + 1), c.x, y1, c.z1), gradf(P(BB + 1), c.x1, y1, c.z1))));
}

template <class Perm>
__device__ __forceinline__ float noise3(const Perm &P, float x, float y, float z)
{
    return perlin_at(P, perlin_column(P, x, z), y);
}

}  // namespace vtmc
#endif
