// terrain_erosion.h -- the host half of VTMC_MOD_EROSION (terrain_erosion.hip): the argument checks, the constants a step's kernels take
// (each one FP32 operation of the rule, made once on the host), and the layout of the state buffer.  Plain C++ with no device code and no
// HIP header, so a stand-alone program compiles it for the CPU (tools/erosion_host_check.cpp runs it under the host sanitizers).  The
// rule is EROSION in include/vtmc_erosion.h.
#ifndef VTMC_TERRAIN_EROSION_H
#define VTMC_TERRAIN_EROSION_H
#include "../../include/vtmc_erosion.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vtmc {

static_assert(sizeof(vtmc_erosion_report) == 48, "include/vtmc_erosion.h");

// What is wrong with a VTMC_MOD_EROSION modifier by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG) behind
// "modifier <i>: erosion "
inline const char *erosion_args_fault(const vtmc_modifier &md)
{
    const float *p = md.p;
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(p[k])) return "parameter not finite";
    for (int k = 0; k < 8; ++k)
        if (p[k] < 0.0f) return "parameter negative";
    if (p[0] > VTMC_EROSION_MAX_RAIN) return "rain above VTMC_EROSION_MAX_RAIN";
    if (p[2] > VTMC_EROSION_MAX_CAPACITY) return "capacity above VTMC_EROSION_MAX_CAPACITY";
    if (p[3] > 1.0f) return "dissolve outside 0..1";
    if (p[4] > 1.0f) return "deposit outside 0..1";
    if (!(p[5] > 0.0f) || p[5] > 1.0f) return "dt outside (0, 1]";
    if (p[7] > VTMC_EROSION_MAX_THERMAL) return "thermal rate above VTMC_EROSION_MAX_THERMAL";
    if (p[1] * p[5] > 1.0f) return "evaporation * dt above 1";
    if (md.data_dims[0] < 1 || md.data_dims[0] > VTMC_EROSION_MAX_ITERATIONS) return "iterations outside 1..VTMC_EROSION_MAX_ITERATIONS";
    if (md.data) return "data must be NULL";
    if (md.data_dims[1] != 0) return "data_dims[1] must be 0";
    return nullptr;
}

// What the kernels of a step take: the parameters, and the products of the rule that depend on nothing else (one FP32 operation each)
struct ErosionStep {
    float dt, dt_rain, dt_g, inv_dt, keep;   // dt; dt * Kr; dt * G; 1 / dt; 1 - Ke * dt
    float kc, ks, kd, talus, kt;
};
inline ErosionStep erosion_step(const float p[8])
{
    ErosionStep s;
    s.dt = p[5];
    s.dt_rain = p[5] * p[0];
    s.dt_g = p[5] * VTMC_EROSION_G;
    s.inv_dt = 1.0f / p[5];
    const float ke_dt = p[1] * p[5];
    s.keep = 1.0f - ke_dt;
    s.kc = p[2], s.ks = p[3], s.kd = p[4], s.talus = p[6], s.kt = p[7];
    return s;
}

// The state buffer of an nx x nz box: eleven planes of `stride` floats (the columns rounded up to whole 256-byte lines), then the mask
// bytes, then the three counters.  b, s and d each have two planes: a step's kernels read one and write the other where a lane needs
// what its neighbour holds (terrain_erosion.hip).
enum ErosionPlane { kBefore = 0, kB0, kB1, kS0, kS1, kD0, kD1, kF0, kF1, kF2, kF3, kErosionPlanes };
struct ErosionLayout {
    int64_t columns, stride;   // nx * nz; floats per plane
    size_t mask_off, ctl_off, bytes;
};
inline ErosionLayout erosion_layout(int32_t nx, int32_t nz)
{
    ErosionLayout l;
    l.columns = (int64_t)nx * (int64_t)nz;
    l.stride = (l.columns + 63) / 64 * 64;
    l.mask_off = sizeof(float) * (size_t)kErosionPlanes * (size_t)l.stride;
    l.ctl_off = l.mask_off + (size_t)l.stride;
    l.bytes = l.ctl_off + 256;
    return l;
}
// where water and sediment lie after `iterations` steps: d and s change planes once a step
inline int erosion_final_parity(int32_t iterations) { return iterations & 1; }

// the bytes of one map of vtmc_erosion_read, or 0 for a map that is none of the five
inline int64_t erosion_map_bytes(int32_t map, int64_t columns)
{
    if (map < VTMC_EROSION_HEIGHT_BEFORE || map > VTMC_EROSION_ACTIVE) return 0;
    return map == VTMC_EROSION_ACTIVE ? columns : 4 * columns;
}

// the clamp of the write-back: [(float)ly + 0.5, (float)(uy - 1)]
inline float erosion_clamp_lo(int32_t ly) { return (float)ly + 0.5f; }
inline float erosion_clamp_hi(int32_t uy) { return (float)(uy - 1); }

}  // namespace vtmc
#endif
