// tri_stream.h -- the sizes of a pass that streams the triangles of a result in tiles, one lane per triangle (tri_stream_kernels.h; the
// surface scatter and the level-of-detail skirts are such passes): the tile, the tiles of T triangles and their mask bytes.  Plain C++ with
// no HIP header, so the host halves (terrain_scatter.h, terrain_lodskirt.h) and the stand-alone host checks (tools/scatter_host_check.cpp,
// tools/lodskirt_host_check.cpp) read the sizes the launches use.
#ifndef VTMC_TRI_STREAM_H
#define VTMC_TRI_STREAM_H
#include <cstddef>
#include <cstdint>

namespace vtmc {

constexpr int kTriTile = 256;   // triangles per workgroup, one lane each

// workgroups of a pass over T triangles (T >= 0)
inline uint32_t tri_tiles(int64_t n_tris) { return (uint32_t)((n_tris + kTriTile - 1) / kTriTile); }

// the mask bytes of T triangles, padded so that every tile's bytes are whole dwords
inline size_t tri_mask_bytes(int64_t n_tris) { return (size_t)tri_tiles(n_tris) * kTriTile; }

}  // namespace vtmc
#endif
