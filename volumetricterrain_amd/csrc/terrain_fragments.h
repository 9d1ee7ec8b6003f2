// terrain_fragments.h -- the host half of the fragment query and the detach modifier (terrain_fragments.hip): the argument checks, the
// stamp box of a captured fragment and the ordering of the list.  Plain C++ with no device code and no HIP header, so a stand-alone program
// compiles it for the CPU (tools/fragments_host_check.cpp runs it under the host sanitizers).  Everything here is integer arithmetic.
#ifndef VTMC_TERRAIN_FRAGMENTS_H
#define VTMC_TERRAIN_FRAGMENTS_H
#include "../../include/vtmc.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vtmc {

// What is wrong with a VTMC_MOD_DETACH modifier by value, or null: the texts of vtmc_last_error (VTMC_ERR_INVALID_ARG)
inline const char *detach_fault(const vtmc_modifier &md)
{
    if (md.add_or_erode != 0) return "detach: add_or_erode must be 0";
    if (md.data != nullptr) return "detach: data must be null";
    if (md.data_dims[0] < 0) return "detach: max_samples (data_dims[0]) < 0";
    if (md.data_dims[1] != 0) return "detach: data_dims[1] must be 0";
    return nullptr;
}

// What is wrong with the arguments of vtmc_terrain_fragments by value, or null
inline const char *fragments_args_fault(const float *lower, const float *upper, int32_t max_samples, int32_t capture_min_samples)
{
    if (!lower || !upper) return "lower or upper is null";
    for (int k = 0; k < 3; ++k)
        if (std::isnan(lower[k]) || std::isnan(upper[k])) return "a bound is NaN";
    if (max_samples < 0) return "max_samples < 0";
    if (capture_min_samples < 0) return "capture_min_samples < 0";
    return nullptr;
}

// One unanchored root as the device leaves it: the root's box-linear index (the seed: the smallest index of the fragment), the solid
// sample count and the tight bounds in grid samples.  32 bytes.
struct FragmentRecord {
    int32_t root, n_samples;
    int32_t lo[3], hi[3];
};
static_assert(sizeof(FragmentRecord) == 32, "copied from the device as it lies");

// The list of the query from the device's records (any order): increasing seed, which is increasing box-linear root, since the box-linear
// order of two samples of the box is their grid-index order.  box_lo / box_d: first sample and samples per axis of the query box.
inline void fragments_order(std::vector<FragmentRecord> &recs, const int32_t box_lo[3], const int32_t box_d[3], vtmc_fragment *dst)
{
    std::sort(recs.begin(), recs.end(), [](const FragmentRecord &a, const FragmentRecord &b) { return a.root < b.root; });
    for (size_t i = 0; i < recs.size(); ++i) {
        const FragmentRecord &r = recs[i];
        vtmc_fragment &f = dst[i];
        f.seed[0] = box_lo[0] + r.root % box_d[0];
        f.seed[1] = box_lo[1] + r.root / box_d[0] % box_d[1];
        f.seed[2] = box_lo[2] + r.root / box_d[0] / box_d[1];
        for (int k = 0; k < 3; ++k) f.lo[k] = r.lo[k], f.hi[k] = r.hi[k];
        f.n_samples = r.n_samples;
        f.stamp_id = 0;
        f.reserved = 0;
    }
}

// The stamp box of a fragment: [max(lo - 2, box lo), min(hi + 2, box hi)] per axis, as first sample and dims.  False when the box breaks
// the stamp limits (a dim outside 2..1026 or more than 2^27 samples): the fragment is then listed without a stamp.
inline bool fragment_stamp_box(const vtmc_fragment &f, const int32_t box_lo[3], const int32_t box_d[3], int32_t first[3], int32_t dims[3])
{
    long long n = 1;
    for (int k = 0; k < 3; ++k) {
        const int32_t a = std::max(f.lo[k] - 2, box_lo[k]), b = std::min(f.hi[k] + 2, box_lo[k] + box_d[k] - 1);
        first[k] = a;
        dims[k] = b - a + 1;
        if (dims[k] < 2 || dims[k] > 1026) return false;
        n *= dims[k];
    }
    return n <= (1ll << 27);
}

}  // namespace vtmc
#endif
