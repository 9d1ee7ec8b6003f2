// record_tile.h -- how the passes over an extract's records (per vertex: material_filter.h, ao_march.h; per triangle: the stream of
// tri_stream_kernels.h, for terrain_scatter.hip and terrain_lodskirt.hip) bring a run of records into LDS: a soup record is 19 dwords and
// a lane that read "its" record would walk memory at a 76-byte stride, so a workgroup of 256 threads loads the run as consecutive
// 16-byte pieces instead.  Device code only.
#ifndef VTMC_RECORD_TILE_H
#define VTMC_RECORD_TILE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vtmc {

// `nd` consecutive dwords from src (16-byte aligned) into LDS: 16-byte pieces, the last one dword by dword where it is not whole
__device__ __forceinline__ void load_record_tile(uint32_t *lds, const uint32_t *__restrict__ src, uint32_t nd)
{
    for (uint32_t q = threadIdx.x; 4 * q < nd; q += 256) {
        if (4 * q + 4 <= nd) {
            *reinterpret_cast<uint4 *>(lds + 4 * q) = *reinterpret_cast<const uint4 *>(src + 4 * q);
        } else {
            for (uint32_t d = 4 * q; d < nd; ++d) lds[d] = src[d];
        }
    }
}

}  // namespace vtmc
#endif
