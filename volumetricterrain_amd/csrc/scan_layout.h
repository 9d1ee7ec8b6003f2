// scan_layout.h -- the buffer the two-level scan of scan_kernels.h works in, for n_tiles uint32 totals: the grand total (64 bits), the tile
// totals, their prefixes inside a group of kScanThreads tiles, the group totals and their prefixes.  Plain C++ with no HIP header, so the
// host halves that size the buffer (terrain_nav.h) and the stand-alone host checks (tools/nav_host_check.cpp, tools/scatter_host_check.cpp,
// tools/lodskirt_host_check.cpp) read the one layout the launches use.  Every size is 64-bit arithmetic.
#ifndef VTMC_SCAN_LAYOUT_H
#define VTMC_SCAN_LAYOUT_H
#include <cstddef>
#include <cstdint>

namespace vtmc {

constexpr int kScanThreads = 1024;   // threads of a scan workgroup = tiles of a group

struct ScanLayout {
    uint64_t n_tiles;
    unsigned char *base;   // null while only the sizes are asked
    explicit ScanLayout(uint64_t tiles, void *at = nullptr) : n_tiles(tiles), base((unsigned char *)at) {}
    uint64_t groups() const { return (n_tiles + kScanThreads - 1) / kScanThreads; }
    size_t bytes() const { return 8u + 4u * 2u * (size_t)(n_tiles + groups()); }
    unsigned long long *total() const { return (unsigned long long *)base; }
    uint32_t *tile_totals() const { return (uint32_t *)(base + 8); }
    uint32_t *tile_offsets() const { return tile_totals() + n_tiles; }
    uint32_t *group_totals() const { return tile_offsets() + n_tiles; }
    uint32_t *group_offsets() const { return group_totals() + groups(); }
};

}  // namespace vtmc
#endif
