// terrain_nav.h -- the host half of the navigation build (terrain_nav.hip): the argument checks, the box as the result reports it, the
// buffer sizes and the max_spans check.  Plain C++ with no device code and no HIP header, so a stand-alone program compiles it for the CPU
// (tools/nav_host_check.cpp runs it under the host sanitizers).  Every size is 64-bit arithmetic.
#ifndef VTMC_TERRAIN_NAV_H
#define VTMC_TERRAIN_NAV_H
#include "../../include/vtmc_nav.h"
#include "scan_layout.h"
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vtmc {

// What is wrong with the arguments of vtmc_terrain_nav_build by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *nav_args_fault(const float *lower, const float *upper, const vtmc_nav_params *p)
{
    if (!lower || !upper) return "lower or upper is null";
    if (!p) return "params is null";
    for (int k = 0; k < 3; ++k)
        if (std::isnan(lower[k]) || std::isnan(upper[k])) return "a bound is NaN";
    if (p->agent_height < 1 || p->agent_height > VTMC_NAV_MAX_AGENT_HEIGHT) return "agent_height outside 1..VTMC_NAV_MAX_AGENT_HEIGHT";
    if (!std::isfinite(p->max_step) || p->max_step < 0.0f) return "max_step must be finite and >= 0";
    if (p->max_spans <= 0) return "max_spans <= 0";
    if (p->flags != 0u) return "flags != 0";
    return nullptr;
}

// The box as the result reports it: first sample and samples per axis of a clamped sample box, (0, 0, 0) samples when any axis has none
struct NavBox {
    int32_t lo[3], d[3];
};
inline NavBox nav_box(const int32_t first[3], const int32_t dims[3])
{
    NavBox b;
    const bool empty = dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0;
    for (int k = 0; k < 3; ++k) b.lo[k] = first[k], b.d[k] = empty ? 0 : dims[k];
    return b;
}
inline bool nav_box_empty(const NavBox &b) { return b.d[0] == 0; }

// The sizes of a build over the box: columns = dx * dz (64 bits: 1026^2 today, but nothing here relies on it), the groups of the scan
// and the bytes of the buffers that depend on the columns alone.
struct NavSizes {
    int64_t columns;         // dx * dz
    int64_t groups;          // the groups of the scan over the columns' counts (scan_layout.h)
    size_t offsets_bytes;    // column_offsets: (columns + 1) int32
    size_t scan_bytes;       // that scan's buffer: a ScanLayout of `columns` tiles
    bool launchable;         // the columns fit a uint32 tile count and a kernel grid
};
inline NavSizes nav_sizes(const NavBox &b)
{
    NavSizes s;
    s.columns = (int64_t)b.d[0] * (int64_t)b.d[2];
    const ScanLayout scan((uint64_t)s.columns);
    s.groups = (int64_t)scan.groups();
    s.offsets_bytes = (size_t)(s.columns + 1) * 4u;
    s.scan_bytes = scan.bytes();
    s.launchable = s.columns < (int64_t)1 << 31 && ((int64_t)b.d[2] + 3) / 4 <= 65535;
    return s;
}

// The bytes that depend on the spans: the records, and the scratch (a column word and a parent word per span)
inline size_t nav_span_bytes(int64_t n) { return (size_t)n * sizeof(vtmc_nav_span); }
inline size_t nav_scratch_bytes(int64_t n) { return (size_t)n * 8u; }

// The max_spans check, before anything is emitted: true when the build may go on (the total then fits an int32, since max_spans does)
inline bool nav_total_fits(uint64_t total, int32_t max_spans) { return max_spans > 0 && total <= (uint64_t)max_spans; }

}  // namespace vtmc
#endif
