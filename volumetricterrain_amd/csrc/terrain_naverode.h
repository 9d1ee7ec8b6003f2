// terrain_naverode.h -- the host half of the agent radius (terrain_naverode.hip): the argument checks, the state word of a span and the
// two relaxations of a round (the functions the kernels share with it), the round and launch counts and the buffer sizes.  Plain C++ with
// no device code and no HIP header, so a stand-alone program compiles it for the CPU (tools/naverode_host_check.cpp runs it under the
// host sanitizers).  Every size is 64-bit arithmetic.
#ifndef VTMC_TERRAIN_NAVERODE_H
#define VTMC_TERRAIN_NAVERODE_H
#include "../../include/vtmc_naverode.h"
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTMC_NAVERODE_HD __host__ __device__
#else
#define VTMC_NAVERODE_HD
#endif

namespace vtmc {

// What is wrong with the parameters of vtmc_nav_distance_build / vtmc_nav_erode by value, or null: the texts of vtmc_last_error
inline const char *naverode_params_fault(const vtmc_naverode_params *p)
{
    if (!p) return "params is null";
    if (p->radius < 0 || p->radius > VTMC_NAVERODE_MAX_RADIUS) return "radius outside 0..VTMC_NAVERODE_MAX_RADIUS";
    if (p->flags & ~(uint32_t)VTMC_NAVERODE_OPEN_BOX_FACES) return "an unknown flag";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "a reserved word is not 0";
    return nullptr;
}

// The state of a span between two kernels of a round, 8 bytes: its distance D (at most 2 * 255 = 510) and the smallest D among the
// spans its +-x links (mx) and its +-z links (mz) lead to; kNavErodeNone where there is no such span.
struct alignas(8) NavErodeState {
    uint16_t d, mx, mz, pad;
};
static_assert(sizeof(NavErodeState) == 8, "one 8-byte load per gather");
constexpr uint16_t kNavErodeNone = 0xffffu;
static_assert(VTMC_NAVERODE_UNIT * VTMC_NAVERODE_MAX_RADIUS < kNavErodeNone - 3, "a distance plus a step stays under the sentinel");

VTMC_NAVERODE_HD inline uint32_t naverode_clamp(int32_t radius) { return (uint32_t)(VTMC_NAVERODE_UNIT * radius); }   // 2 * radius: D's cap, and the least D of a kept span
VTMC_NAVERODE_HD inline uint32_t naverode_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// NAVERODE, Steps, one round for one span.  t[k] is the state of the span link[k] leads to, has[k] whether there is one.
// First half: the smallest D one hop away along each axis.
VTMC_NAVERODE_HD inline NavErodeState naverode_pair(NavErodeState me, const NavErodeState t[4], const bool has[4])
{
    uint32_t mx = kNavErodeNone, mz = kNavErodeNone;
    if (has[0]) mx = naverode_min(mx, t[0].d);
    if (has[1]) mx = naverode_min(mx, t[1].d);
    if (has[2]) mz = naverode_min(mz, t[2].d);
    if (has[3]) mz = naverode_min(mz, t[3].d);
    NavErodeState out;
    out.d = me.d, out.mx = (uint16_t)mx, out.mz = (uint16_t)mz, out.pad = 0;
    return out;
}
// Second half: the one-hop steps (weight 2) and, through the first half's minima of the span one hop away, the two-hop steps that turn
// onto the other axis (weight 3): all twelve steps.  D never rises, so the cap of D0 holds.
VTMC_NAVERODE_HD inline NavErodeState naverode_relax(NavErodeState me, const NavErodeState t[4], const bool has[4])
{
    uint32_t best = me.d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!has[k]) continue;
        best = naverode_min(best, (uint32_t)t[k].d + 2u);
        best = naverode_min(best, (uint32_t)(k < 2 ? t[k].mz : t[k].mx) + 3u);
    }
    NavErodeState out;
    out.d = (uint16_t)best, out.mx = kNavErodeNone, out.mz = kNavErodeNone, out.pad = 0;
    return out;
}

// Rounds to the fixed point, and the kernel launches they take (two per round): none for radius 0 and 1, where D0 is D already
inline int32_t naverode_rounds(int32_t radius) { return radius > 1 ? radius - 1 : 0; }
inline int32_t naverode_launches(int32_t radius) { return 2 * naverode_rounds(radius); }

// The bytes over n spans: one state array (there are two, a round reads one and writes the other), the packed links, the distances,
// the old-to-new index words and the origin
inline size_t naverode_state_bytes(int64_t n) { return (size_t)n * sizeof(NavErodeState); }
inline size_t naverode_link_bytes(int64_t n) { return (size_t)n * 16u; }
inline size_t naverode_word_bytes(int64_t n) { return (size_t)n * 4u; }

}  // namespace vtmc
#endif
