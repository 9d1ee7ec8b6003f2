/*
 * vtmc.h -- C ABI of the MI355X-native marching-cubes extractor (libvtmc.so).
 *
 * Drop-in boundary for the GPU section of PGRTerrain.Render.VoxelTerrain.BatchUpdate
 * (reference: Unity-Project/Assets/Scripts/VoxelTerrain.cs:330-477), which today drives three
 * Unity compute shaders (Shaders/SampleNormal.compute, CollectTriNum.compute, MarchingCube.compute)
 * through nine ComputeBuffer bindings (VoxelTerrain.cs:370-421).  Every entry point is cdecl,
 * `extern "C"`, takes only plain pointers / integers / the 76-byte POD below, and never throws:
 * the return value is a status (0 = OK, negative = error, text via vtmc_last_error).
 *
 * Ownership: host memory passed in is borrowed for the duration of the call only; all device
 * memory is owned by the context.  Calls on one context are serialised by the caller
 * (the reference calls from the Unity main thread only, TerrainEngine.cs:145-149); different
 * contexts may be used from different threads.  Host entry points block until results are complete.
 *
 * Canonical triangle order (the reference's order is whatever its atomic append produces,
 * MarchingCube.compute:160-162): (block index in the submitted list, cell x + 8y + 64z, table
 * triangle i).  The host can therefore slice per block with block_tri_offsets instead of binning
 * (VoxelTerrain.cs:437-446).
 */
#ifndef VTMC_H
#define VTMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTMC_BLOCK_SIZE 8          /* VoxelTerrain.cs:54  blockSize */
#define VTMC_TILE_SAMPLES 1000     /* (blockSize+2)^3, VoxelTerrain.cs:337-341 */
#define VTMC_MAX_TRIS_PER_CELL 5   /* VoxelTerrain.cs:480 maxTriNumPerCell */

/* status codes */
#define VTMC_OK 0
#define VTMC_ERR_INVALID_ARG (-1)  /* null pointer, negative count ... */
#define VTMC_ERR_DIMS (-2)         /* dims not a multiple of 8 (VoxelTerrain.cs:138-139) or block out of range */
#define VTMC_ERR_CAPACITY (-3)     /* destination smaller than the triangle count */
#define VTMC_ERR_DEVICE (-4)       /* HIP runtime error (text in vtmc_last_error) */
#define VTMC_ERR_NO_RESULT (-5)    /* read_* before any extract_* */
#define VTMC_ERR_TOO_LARGE (-6)    /* more than 2^31-1 triangles or blocks */

/* Wire format of one triangle -- replaces the private CSTriangle read-back struct
 * (VoxelTerrain.cs:23-37; HLSL twin MarchingCube.compute:18-27).  76 bytes, packed.  Positions
 * are block-local in cell units [0,8]; `block` is the index into the submitted block list. */
typedef struct vtmc_triangle {
    float position0[3];
    float position1[3];
    float position2[3];
    float normal0[3];
    float normal1[3];
    float normal2[3];
    int32_t block;
} vtmc_triangle;

typedef struct vtmc_ctx vtmc_ctx;

/* Replaces the table uploads of VoxelTerrain.Init (VoxelTerrain.cs:151-156): binds HIP device
 * `device`, uploads the lookup tables, creates the stream and reusable scratch. */
int32_t vtmc_create(int32_t device, vtmc_ctx **out_ctx);

/* Replaces the ComputeBuffer.Release calls of VoxelTerrain.Free (VoxelTerrain.cs:228-244) and of
 * BatchUpdate's epilogue (VoxelTerrain.cs:469-476). */
int32_t vtmc_destroy(vtmc_ctx *ctx);

/* UTF-8 text of the last error on this context ("" if none).  ctx may be NULL (global create error). */
const char *vtmc_last_error(const vtmc_ctx *ctx);

/* Replaces bufferSamples.SetData + the three Dispatch calls + bufferTriNum.GetData
 * (VoxelTerrain.cs:365-395).  `samples` = n_blocks tiles of 10x10x10 floats, x fastest, exactly the
 * array BatchUpdate builds (VoxelTerrain.cs:341-361).  *tri_count receives T (0 is success, the
 * reference's early-out VoxelTerrain.cs:396-405). */
int32_t vtmc_extract_blocks(vtmc_ctx *ctx, const float *samples, int32_t n_blocks, int32_t *tri_count);

/* New: removes the tile gather (VoxelTerrain.cs:337-361).  Reads the (nx+2, ny+2, nz+2)-sample
 * grid in place: sample (x,y,z) = grid[x*stride_x + y*stride_y + z*stride_z] (element strides), so
 * a pinned C# float[W+2,E+2,H+2] (z fastest, VoxelTerrain.cs:145) is passed with strides
 * ((E+2)*(H+2), H+2, 1).  block_list = n_blocks (bx,by,bz) triples (the dirty list
 * VoxelTerrain.cs:321); NULL = every block, ordered bx + nbx*(by + nby*bz), n_blocks ignored. */
int32_t vtmc_extract_grid(vtmc_ctx *ctx, const float *grid, int32_t nx, int32_t ny, int32_t nz,
                          int64_t stride_x, int64_t stride_y, int64_t stride_z,
                          const int32_t *block_list, int32_t n_blocks, int32_t *tri_count);

/* Multi-GPU host entry: the grid is cut into chunks of chunk_cells^3 cells, chunk c
 * (c = cx + ncx*(cy + ncy*cz)) belongs to rank c % world_size.  Extracts this rank's chunks only,
 * chunk-major, blocks in canonical order inside each chunk.  chunk_counts receives for each LOCAL
 * chunk {vertex count, triangle count}; *n_local_chunks how many.  No collective is issued here:
 * vtmc_allgather_volume_counts (below) is the RCCL all-gather that follows it. */
int32_t vtmc_extract_grid_sharded(vtmc_ctx *ctx, const float *grid, int32_t nx, int32_t ny, int32_t nz,
                                  int64_t stride_x, int64_t stride_y, int64_t stride_z,
                                  int32_t chunk_cells, int32_t rank, int32_t world_size,
                                  uint32_t *chunk_counts, int32_t chunk_counts_capacity,
                                  int32_t *n_local_chunks, int32_t *tri_count);

/* Replaces bufferMeshes.GetData(csTriangles) (VoxelTerrain.cs:426-427).  Copies the T triangles of
 * the last extract_* in canonical order.  block_tri_offsets (optional, n_blocks+1 entries) receives
 * the exclusive prefix of per-block triangle counts. */
int32_t vtmc_read_triangles(vtmc_ctx *ctx, vtmc_triangle *dst, int64_t capacity, int32_t *block_tri_offsets);

/* The _CornerFlags buffer of the last extract_* (CollectTriNum.compute:56-62) as one byte per
 * cell: dst[512*b + x + 8y + 64z].  Parity / debugging aid; capacity in bytes. */
int32_t vtmc_read_cases(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity);

/* Number of blocks / triangles of the last extract_*. */
int32_t vtmc_last_counts(const vtmc_ctx *ctx, int32_t *n_blocks, int32_t *tri_count);

/* ------------------------------------------------------------------------------------------
 * Device-resident entry points: same extraction, inputs already in HBM (what a GPU-resident host,
 * the sharded driver and bench.py use).  Pointers prefixed d_ are device pointers on ctx's device.
 * ------------------------------------------------------------------------------------------ */

/* A batch of equally shaped volumes: volume v starts at d_samples + v*volume_stride and holds
 * (nx+2, ny+2, nz+2) samples addressed with the element strides.  One 1026^3 grid is a batch of 1;
 * the reference's tile buffer is a batch of n_blocks volumes with nx=ny=nz=8, strides (1,10,100),
 * volume_stride 1000; "1024^3 as 8^3 chunks of 128^3" is a batch of 512 with nx=ny=nz=128. */
typedef struct vtmc_volume_batch {
    const float *d_samples;
    int32_t nx, ny, nz;
    int64_t stride_x, stride_y, stride_z;
    int32_t n_volumes;
    int64_t volume_stride;
} vtmc_volume_batch;

#define VTMC_FLAG_WANT_CASES 1u    /* also materialise the per-cell case bytes (slower generic classify) */
#define VTMC_FLAG_NO_DENSE_PATH 2u /* force the per-block classify kernel (A/B testing) */

/* Extract every block of every volume (block id = v*blocks_per_volume + bx + nbx*(by + nby*bz)).
 * `stream` is a hipStream_t (NULL = the context's own stream).  Blocks until T is known. */
int32_t vtmc_extract_volumes_device(vtmc_ctx *ctx, const vtmc_volume_batch *batch, void *stream,
                                    uint32_t flags, int64_t *tri_count);

/* The same extract in two halves, for hosts that keep the CPU out of the step (the multi-GPU driver):
 * _async queues classify -> scan -> emit on `stream` and returns at once -- {T, nActive} stay in
 * device memory, there is no mid-pipeline read-back (VoxelTerrain.cs:394-395) --; after it the per-
 * volume counts are final on the stream, so vtmc_copy_volume_counts_device / vtmc_allgather_volume_counts
 * may be queued behind it.  vtmc_extract_finish waits for THIS extract (an event behind its emit
 * launch -- not for work the caller queued behind it on the stream: the next batch's sampler, a
 * collective, copies; a caller that wants those too synchronises its stream), returns T and -- when
 * the triangle buffer turned out too small and the emit kernel refused to run -- grows it and runs
 * the emit stage again.  Exactly one _finish per _async; no other extract_* of this context in between. */
int32_t vtmc_extract_volumes_device_async(vtmc_ctx *ctx, const vtmc_volume_batch *batch, void *stream, uint32_t flags);
int32_t vtmc_extract_finish(vtmc_ctx *ctx, int64_t *tri_count);

/* A stream of the context (a hipStream_t).  own_queue = 0: the context's own stream, what `stream` = NULL means everywhere above.
 * own_queue = 1: a second stream that sits on a HARDWARE QUEUE OF ITS OWN (taken on first request): ordinary HIP streams share a handful
 * of hardware queues, and two contexts whose streams land on one queue run their steps strictly in turn; a host that keeps several steps
 * in flight passes each context's own-queue stream to vtmc_extract_volumes_device_async and the steps overlap where one kernel drains and
 * the next ramps up (bench.py --streams 2).
 * LIFETIME: the context stops using the stream at vtmc_destroy (which drains it), but the HANDLE stays valid until the process exits: the
 * library never destroys a stream, it parks it and gives it to the next context created on that device.  Host-side objects that still refer
 * to it after vtmc_destroy -- events recorded on it, a framework's stream wrapper, a caching allocator that records on it when it frees a
 * pinned buffer -- are therefore safe, whatever order they are released in.  Work the HOST queues on the handle after vtmc_destroy simply
 * shares the stream with that next context.  See INTEGRATION.md ("Streams").
 * (The reference has one queue: every Dispatch / GetData of BatchUpdate is in program order on Unity's graphics device,
 * VoxelTerrain.cs:365-427.) */
int32_t vtmc_context_stream(vtmc_ctx *ctx, int32_t own_queue, void **stream);

/* Destroys the streams the library holds for contexts that no longer exist (the parked ones; a live context keeps its own).  Optional: a host
 * calls it at a point where nothing of its own refers to a handle of a destroyed context any more -- typically once, before it exits.  Needed
 * in one situation only: under a profiler (rocprofv3) a process that ends with streams on hardware queues of their own still alive crashes in
 * the profiler's finalisation and loses the profile; bench.py and the tools that are run under rocprofv3 call it for that reason.  Returns the
 * number of streams destroyed. */
int32_t vtmc_release_streams(void);

/* Device pointers to the results of the last extract_* (valid until the next extract_* / destroy):
 * triangles (T x 76 B), block_tri_offsets (n_blocks+1 x u32), volume_counts (n_volumes x
 * {vertices, triangles} u32 -- the array SURVEY.md 8e all-gathers).  Any out pointer may be NULL. */
int32_t vtmc_device_results(vtmc_ctx *ctx, const vtmc_triangle **d_triangles,
                            const uint32_t **d_block_tri_offsets, const uint32_t **d_volume_counts);

/* Copies volume_counts of the last extract_* (n_volumes x {vertices, triangles} u32) into a
 * caller-owned DEVICE buffer on `stream` (NULL = the context's stream), asynchronously: the buffer a
 * multi-GPU caller hands to its all-gather (RCCL), SURVEY.md 8e. */
int32_t vtmc_copy_volume_counts_device(vtmc_ctx *ctx, uint32_t *d_dst, int32_t capacity_volumes, void *stream);

/* Pre-size the triangle buffer (otherwise it grows on demand and the emit stage is re-run once). */
int32_t vtmc_reserve_triangles(vtmc_ctx *ctx, int64_t capacity);

/* Per-stage device time of the last extract_* in milliseconds, measured with HIP events on the
 * stream the kernels ran on: ms[0] classify+count, ms[1] scan,
 * ms[2] emit, ms[3] whole call.
 * The reference's only timing hook is the commented-out timer at VoxelTerrain.cs:363/467. */
int32_t vtmc_last_stage_ms(vtmc_ctx *ctx, float ms[4]);

/* Selects a kernel variant / launch shape, mainly for A/B measurements in one process.  Every key and value the library accepts keeps
 * results within the parity bar and is compared with the CPU oracle by tests/test_tuning_matrix.py; an unknown key or a value outside
 * a key's range answers VTMC_ERR_INVALID_ARG and changes nothing.  Keys: "emit_fast_math" (1: v_rcp / v_rsq / fma, default; 0: correctly
 * rounded, bit-compatible with the CPU oracle), "emit_once" (default 1: with emit_fast_math, every welded vertex of a block is evaluated
 * once and the 76-byte records are expanded from LDS; 0: per triangle corner), "emit_dynamic" (default 1: per-XCD ticket counters; 0: a
 * static round-robin over the list of non-empty blocks), "emit_sub_log2" (0-4, default 1: 2^s ticket counters per XCD),
 * "emit_row_masks" (default 1: only tile rows next to cells with triangles are fetched), "emit_wgs_per_cu" (0-8; 0, default: the
 * kernel's own residency),
 * "classify_wgs_per_cu" (0 or 2-7, default 3: residency cap of the streaming classify kernel; 0: none), "density_wgs_per_cu" (0, 2 or 3:
 * residency cap of the synthetic sampler), "stage_events" (default 1: HIP events between the three kernels for vtmc_last_stage_ms; 0: only around
 * the step), "gather_beside" (default 0: the all-gather of a queued extract runs behind the emit kernel on the caller's stream; 1: beside
 * it on the context's second stream), "place_outputs" (0-16, default 0: see vtmc_last_placement below).  The diagnostic keys "emit_ablate" / "classify_ablate" / "density_ablate" (parts of a kernel
 * switched off, output INVALID) exist only in -DVTMC_DIAGNOSTICS builds of the library (tools/build_diagnostics.py).
 * "fill_keeps_signs" (default 0) is a contract, not a variant: with 1, vtmc_density_fill_device[_async] also leaves
 * one sign bit per sample in context memory, and an extract by the SAME context of exactly that buffer (pointer,
 * dims, strides, volume count) classifies from those bits instead of the samples (1/32 of the bytes; results are
 * identical).  The caller vouches that nothing wrote to the buffer between the fill and the extract; any other
 * fill by the context, setting the key again, or "invalidate_signs" (any value) drops the bits -- a caller whose allocator may hand the
 * same address to a new buffer of the same shape calls that when it frees the old one.  streaming.ChunkStream sets it. */
int32_t vtmc_set_tuning(vtmc_ctx *ctx, const char *key, int32_t value);

/* OUTPUT PLACEMENT (tuning key "place_outputs" = K, 2-16; default 0 = off).  The emit kernel's time is a property of the pair (allocation of the
 * input field, allocation of the output buffers): the identical kernel on the identical input runs 0.86 ... 1.00 ms by which allocation it
 * writes (profiles/r06/placement_probe.txt).  With K > 1, whenever the library has just (re)allocated its output buffers -- a context's first
 * extract, a growth -- it runs the emit stage of the extract at hand into K - 1 further allocations of the same size, times each and keeps the
 * fastest (an autotuner's move; the result is complete and identical in every candidate).  Cost: 2 (K - 1) emit launches and K allocations of the
 * output held at once while the trial runs (they must differ: one freed and made again gets its old pages back), once per (re)allocation.  vtmc_last_placement reports the last trial: the emit stage's milliseconds per candidate (ms[0] = the
 * allocation that was there), how many were tried (0: no trial yet) and which one was kept. */
int32_t vtmc_last_placement(const vtmc_ctx *ctx, float ms[16], int32_t *n_candidates, int32_t *kept);

/* Synthetic density sampler (the reference has no noise field of its own):
 * density = sum_{o<octaves} gain^o * perlin(p*frequency*lacunarity^o) - (p.y - ramp_center)*ramp_scale,
 * p = volume origin + sample index, FP32, Perlin 2002 improved noise with a SplitMix64 permutation.
 * The lattice coordinate of octave o is the FP32 chain x = (float)(origin + index) * frequency, then x = x * lacunarity per octave; its
 * cell is (int)floorf(x), which is defined only below 2^31.  Any frequency, lacunarity and gain are accepted (negative, zero, below 1)
 * as long as the chain stays inside that range: VTMC_ERR_INVALID_ARG, nothing written, when the largest |origin + index| of any volume
 * and axis times |frequency| * max(1, |lacunarity|)^(octaves - 1), evaluated in double with 2^-19 on top for the chain's own roundings,
 * is not below 2^31 (frequency or lacunarity that are not finite included), or when origin + dim - 1 leaves int32.  From 2^24 on a
 * coordinate has no fraction left: that octave is 0, which is the definition's value there, not an error. */
typedef struct vtmc_density_params {
    uint64_t seed;
    float frequency;
    int32_t octaves;
    float lacunarity;
    float gain;
    float ramp_scale;
    float ramp_center;
} vtmc_density_params;

/* Fill n_volumes volumes of (dim_x, dim_y, dim_z) samples; volume v has global sample origin
 * origins[3v..3v+2] (host array) and is written at d_out + v*volume_stride with element strides. */
int32_t vtmc_density_fill_device(vtmc_ctx *ctx, const vtmc_density_params *params,
                                 const int32_t *origins, int32_t n_volumes,
                                 int32_t dim_x, int32_t dim_y, int32_t dim_z,
                                 int64_t stride_x, int64_t stride_y, int64_t stride_z,
                                 int64_t volume_stride, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Indexed (welded) output -- new; the reference welds on the CPU afterwards with Mesh.Optimize()
 * (VoxelTerrain.cs:460).  Per block: one vertex per lattice edge with a sign change (all cells
 * around the edge share it).  Every such edge is a cube edge of exactly one OWNER cell -- the cell
 * whose corner 0 is the edge's low point (cube edges 0, 3, 8 of MarchingCube.compute:40-43) or, on the
 * block's x = 8 / y = 8 / z = 8 faces, the boundary cell next to it -- and vertices are ordered by owner
 * cell x + 8y + 64z, then cube edge id; three block-local int32 indices per triangle in the canonical
 * triangle order.  ~27 bytes per triangle instead of 76.  De-indexing reproduces the 76-byte records
 * within the 1e-5 bar (the reference evaluates an edge from either end depending on the cell; here
 * always from its low end).  Faster than the soup on the benchmark field.
 * ------------------------------------------------------------------------------------------ */
typedef struct vtmc_vertex {
    float position[3]; /* block-local, cell units [0,8] */
    float normal[3];
} vtmc_vertex;

#define VTMC_OUTPUT_SOUP 0    /* 76-byte CSTriangle records (default) */
#define VTMC_OUTPUT_INDEXED 1 /* vtmc_vertex + index buffers */

/* Selects what the following extract_* / terrain_update calls produce. */
int32_t vtmc_set_output_mode(vtmc_ctx *ctx, int32_t mode);

/* Vertex count of the last extract in indexed mode (tri count: vtmc_last_counts). */
int32_t vtmc_last_vertex_count(const vtmc_ctx *ctx, int32_t *vertex_count);

/* Copies the indexed mesh of the last extract: V vertices, 3*T indices (block-local: add nothing,
 * a block's vertices are vertices[block_vertex_offsets[b] .. block_vertex_offsets[b+1])), and the
 * two per-block exclusive prefixes (n_blocks+1 entries each, optional). */
int32_t vtmc_read_indexed_mesh(vtmc_ctx *ctx, vtmc_vertex *vertices, int64_t vertex_capacity, int32_t *indices,
                               int64_t tri_capacity, int32_t *block_vertex_offsets, int32_t *block_tri_offsets);

/* Device pointers of the same (valid until the next extract_* / destroy). */
int32_t vtmc_device_indexed_results(vtmc_ctx *ctx, const vtmc_vertex **d_vertices, const int32_t **d_indices,
                                    const uint32_t **d_block_vertex_offsets, const uint32_t **d_block_tri_offsets);

/* ------------------------------------------------------------------------------------------
 * Device-resident terrain: the density grid of VoxelTerrain and its Update() on the GPU.
 * Replaces _voxelSamples (VoxelTerrain.cs:42,145), the per-sample CSG loop of Update
 * (VoxelTerrain.cs:284-305), the dirty-block selection (VoxelTerrain.cs:307-317) and the hand-off to
 * BatchUpdate (VoxelTerrain.cs:321-324) without the grid ever crossing PCIe.
 * ------------------------------------------------------------------------------------------ */

#define VTMC_MOD_PLANE 0     /* TerrainModifier.cs:38-65   f = _height - y            p[0] = _height */
#define VTMC_MOD_SPHERE 1    /* TerrainModifier.cs:70-91   f = _radius - |pos - c|    p[0..2] = _center, p[3] = _radius */
#define VTMC_MOD_CYLINDER 2  /* TerrainModifier.cs:96-152  p[0..2] = _axisStart, p[3..5] = _axisDir (normalised),
                                                           p[6] = _axisLength, p[7] = _radius */
#define VTMC_MOD_HEIGHTMAP 3 /* IslandModifier.cs:34-73    f = bilinear(_heightmap)(x, z) - y; p[0] = _island.width,
                                                           p[1] = _island.height; data = _heightmap (host pointer,
                                                           float[data_dims[0], data_dims[1]] row-major as the C# float[,]) */
#define VTMC_MOD_SMOOTH 4    /* sculpt brush (not in the reference): p[0..2] = centre c (world), p[3] = radius r, p[4] = strength s */
#define VTMC_MOD_FLATTEN 5   /* sculpt brush (not in the reference): p[0..2] = centre c (a point of the plane), p[3] = radius r,
                                                           p[4] = strength s, p[5..7] = plane normal n (the mirrors normalise it;
                                                           used as given) */
/* The brushes (kinds 4 and 5) take their box from lower / upper as kinds 0-3 do (the mirrors pass c -/+ r), mark dirty blocks by the
 * same rule and take one event number each (they draw nothing with it); add_or_erode is ignored.  A brush sees what the earlier
 * modifiers of its queue wrote.  Per sample of the box, FP32 in this order (px, py, pz as for kinds 0-3: (float)x * scale + origin):
 *   d = sqrtf((dx*dx + dy*dy) + dz*dz) with dx = px - c0 ...;  t = 1 - d / r;  t = t + t;  t = clamp(t, 0, 1);  w = s * t
 *   w == 0: the sample keeps its 32 bits;  otherwise S' = S + (T - S) * w
 * VTMC_MOD_SMOOTH: T = the 27-point box mean of the samples as they were before this modifier (none of its own writes is visible to
 *   it), a neighbour index outside the grid clamped to [0, dim-1] on its axis:  R(y,z) = (s[x-1] + s[x]) + s[x+1];
 *   P(z) = (R(y-1,z) + R(y,z)) + R(y+1,z);  T = ((P(z-1) + P(z)) + P(z+1)) / 27.
 * VTMC_MOD_FLATTEN: g = ((n0*(c0-px) + n1*(c1-py)) + n2*(c2-pz)) / scale;  T = clamp(g, -1, 1): solid below the plane (n up), air
 *   above it, linear in grid units within one sample of it, so with s = 1 the surface lies on the plane where a cell's corners are
 *   all within r/2 of c.
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error) for c not finite, r not finite or <= 0, s not finite or outside
 * [0, 1], and for flatten n not finite or dot(n, n) == 0.  The journal records a brush's box (no halo), as any modifier's. */

#define VTMC_MOD_NOISE 8     /* fractal noise: the device form of RidgedMultifractalModifier (TerrainModifier.cs:158-196) and its fBm and
                                                           billow relatives.  p[0] = frequency f (per world unit), p[1] = lacunarity L,
                                                           p[2] = gain g, p[3] = amplitude a, p[4] = bias b, p[5] = ramp scale rs,
                                                           p[6] = ramp centre rc (world y), p[7] = ridge offset h (ridged only;
                                                           LibNoise's is 1); data_dims[0] = seed (the C# int _seed),
                                                           data_dims[1] = octaves | basis << 8 (octaves 1..16; basis 0 fBm, 1 billow,
                                                           2 ridged multifractal); data is not read.  Kinds 6 and 7 are not defined. */
/* The noise is THE LIBRARY'S OWN: Ken Perlin's 2002 improved noise over the 256-entry permutation of the density sampler (a Fisher-Yates
 * shuffle driven by SplitMix64 of (uint64_t)(uint32_t)seed, as vtmc_density_fill_device uses for vtmc_density_params.seed).  The
 * reference's modifier wraps LibNoise, which it does not vendor: no value here is LibNoise's and parity with it is not claimed.
 * A noise modifier takes its box from lower / upper, marks dirty blocks, is journaled and takes one event number exactly as kinds 0-3,
 * in queue order with every other kind.  Per sample of the box, FP32, one IEEE operation per step, in this order (px, py, pz as for
 * kinds 0-3: (float)x * scale + origin; noise3 = the improved noise, value in about [-1, 1]):
 *   x = px * f;  y = py * f;  z = pz * f;  amp = 1;  sum = 0;  w = 1
 *   for o in 0 .. octaves-1:
 *     n = noise3(x, y, z)
 *     fBm:     sum = sum + amp * n
 *     billow:  t = fabsf(n);  t = t + t;  t = t - 1;  sum = sum + amp * t
 *     ridged:  r = h - fabsf(n);  r = r * r;  r = r * w;  w = r + r;  w = w < 0 ? 0 : (w > 1 ? 1 : w);  sum = sum + amp * r
 *     x = x * L;  y = y * L;  z = z * L;  amp = amp * g
 *   q = a * sum;  q = q + b;  q = q - (py - rc) * rs
 *   md = Clamp(q, void, full) with draws 0 / 1; then add_or_erode 1: S = max(S, md); 0: S = Clamp(min(S, -md), void, full), draws 2 / 3:
 *   the write of kinds 0-3.
 * With basis 0, a = 1, b = 0, scale 1 and origin 0 the value q is what vtmc_density_fill_device's definition gives for the same
 * vtmc_density_params at integer positions.
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error, nothing written by it): any of p[0..7] not finite; octaves outside
 * 1..16; basis outside 0..2; or lattice coordinates that can reach 2^24 in magnitude inside the modifier's clamped sample box: the
 * largest |world coordinate| of the box's corner samples times |f| * max(1, |L|)^(octaves - 1), evaluated in double, must be below
 * 2^24 (beyond it the lattice fraction carries no information and the float -> int conversion differs between targets). */

#define VTMC_MOD_STAMP 9     /* pastes a stamp (vtmc_stamp_create / _capture below), turned and resized: p[0..2] = t, the world position
                                                           of the stamp's centre; p[3..6] = quaternion (x, y, z, w) of any non-zero
                                                           length, stamp axes -> world; p[7] = h, world units between neighbouring
                                                           stamp samples (> 0); data_dims[0] = stamp id; data_dims[1] = mode: 0 CSG
                                                           (add_or_erode decides, as for kinds 0-3), 1 replace (add_or_erode ignored);
                                                           data is not read.  Not in the reference. */
/* A stamp modifier takes its box from lower / upper (the mirrors pass the world AABB of the turned stamp box; the box only has to contain
 * the footprint, which the kernel tests per sample), marks dirty blocks, is journaled (its box, no halo) and takes one event number exactly
 * as kinds 0-3, in queue order with every other kind, and sees what the earlier modifiers of its queue wrote.  Undo and redo swap the
 * journal's images and never read the stamp again: a stamp destroyed after a paste breaks neither.  Densities are not rescaled with h.
 * On the host, in double, from the floats of p:
 *   n = sqrt(x*x + y*y + z*z + w*w);  x /= n;  y /= n;  z /= n;  w /= n
 *   R00 = 1 - 2*(y*y + z*z);  R01 = 2*(x*y - z*w);      R02 = 2*(x*z + y*w)
 *   R10 = 2*(x*y + z*w);      R11 = 1 - 2*(x*x + z*z);  R12 = 2*(y*z - x*w)
 *   R20 = 2*(x*z - y*w);      R21 = 2*(y*z + x*w);      R22 = 1 - 2*(x*x + y*y)
 *   M[i][j] = (float)(R[j][i] / (double)h)   (the inverse rotation over the pitch, rounded once);  c_k = (float)(n_k - 1) * 0.5f
 * Per sample of the box, FP32, one IEEE operation per step, in this order (px, py, pz as for kinds 0-3: (float)x * scale + origin; s the
 * stamp, (nx, ny, nz) its dims):
 *   dx = px - t0;  dy = py - t1;  dz = pz - t2
 *   u = ((M00*dx + M01*dy) + M02*dz) + c0;   v and w alike with rows 1 and 2 of M and c1, c2
 *   outside the footprint -- !(u >= 0 && u <= nx-1), or the same for v or w (a NaN included): the sample keeps its 32 bits
 *   i = (int)floorf(u);  i' = min(i + 1, nx - 1);  fu = u - (float)i;     j, j', fv from v and k, k', fw from w alike
 *   a00 = s[i,j,k] + (s[i',j,k] - s[i,j,k]) * fu;   a10 the same at j';  a01 at k';  a11 at j', k'
 *   b0 = a00 + (a10 - a00) * fv;  b1 = a01 + (a11 - a01) * fv;  q = b0 + (b1 - b0) * fw
 *   mode 0: md = Clamp(q, void, full) with draws 0 / 1; then add_or_erode 1: S = max(S, md); 0: S = Clamp(min(S, -md), void, full), draws
 *           2 / 3: the write of kinds 0-3
 *   mode 1: fabsf(q) <= 2: S = q;  otherwise S = Clamp(q, void, full), draws 0 / 1
 * (i' is clamped rather than i: on the footprint's upper faces, u = nx-1 exactly, the weight is 0 and the value is s[nx-1] itself, not
 * s[nx-2] + (s[nx-1] - s[nx-2]) * 1, which rounds.)
 * Mode 1 makes copy and paste exact.  A stamp captured from the grid and pasted with the identity quaternion (0, 0, 0, 1), h = the voxel
 * scale, its centre a whole number of samples from where it was taken, and positions for which u, v, w come out as whole numbers (a
 * power-of-two scale with an origin on its lattice, for one), has every weight 0: a + (b - a) * 0 is a for the finite values a grid holds,
 * the 32 bits of the captured samples are written back, and the blocks the box covers mesh exactly as the source's did.  The one exception
 * is the sign of a zero: -0 comes back as +0 where (b - a) * 0 is +0.
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error, nothing written by it): any of p[0..7] not finite; a quaternion of
 * length 0; h <= 0; an unknown (or destroyed) stamp id; a mode outside 0..1. */

#define VTMC_MOD_PATH 10     /* carves or builds along curves: the union of tapered capsules over a segment soup (rivers, tunnels, roads,
                                                           shafts; polylines, trees and disjoint pieces alike).  data = host pointer,
                                                           borrowed for the call and copied to the device: data_dims[0] = n_seg
                                                           segments (1..65536) of data_dims[1] = 8 floats each,
                                                           ax, ay, az, ra, bx, by, bz, rb: the world-space end points and the radius
                                                           at each end (round ends, radius linear along the segment).  p[0..7] are
                                                           not read.  add_or_erode as for kinds 0-3 (a river or a tunnel is erode). */
/* The shape is THE LIBRARY'S OWN.  The reference carves its rivers with one flat-ended eroding CylinderModifier per segment
 * (RiverRenderer.cs:151-170, TerrainEngine.cs:97-99), which leaves wedge-shaped gaps on the outside of every bend; a path is one modifier,
 * one event number and one journal box, and its values are not those of that cylinder queue.
 * A path modifier takes its box from lower / upper (the mirrors pass the AABB of all end points grown by their radii), writes EVERY sample
 * of the box, marks dirty blocks, is journaled (its box, no halo) and takes one event number exactly as kinds 0-3, in queue order with every
 * other kind, and sees what the earlier modifiers of its queue wrote.  Two path modifiers of one queue each read their own data.
 * On the host, per segment, FP32, one IEEE operation per step:
 *   ex = bx - ax;  ey = by - ay;  ez = bz - az
 *   ll = (ex*ex + ey*ey) + ez*ez;  il = ll >= 1e-30f ? 1.0f / ll : 0.0f;  dr = rb - ra
 * Per sample of the box, FP32, one IEEE operation per step, segments in increasing index (px, py, pz as for kinds 0-3:
 * (float)x * scale + origin):
 *   q = -inf
 *   per segment:
 *     dx = px - ax;  dy = py - ay;  dz = pz - az
 *     t = ((dx*ex + dy*ey) + dz*ez) * il;  t = t < 0 ? 0 : (t > 1 ? 1 : t)
 *     cx = dx - ex*t;  cy = dy - ey*t;  cz = dz - ez*t
 *     d = sqrtf((cx*cx + cy*cy) + cz*cz);  r = ra + dr*t;  f = r - d
 *     if (f > q) q = f
 *   md = Clamp(q, void, full) with draws 0 / 1; then add_or_erode 1: S = max(S, md); 0: S = Clamp(min(S, -md), void, full), draws 2 / 3:
 *   the write of kinds 0-3.
 * (The increasing order matters only for the sign of a zero.)  Two properties:
 *  - a single segment with a == b and ra == rb == r, given SphereModifier's box, writes what VTMC_MOD_SPHERE with centre a and radius r
 *    writes, bit for bit: il = 0, t = +-0, c = d, f = r - |p - a|;
 *  - the result never depends on how the kernel prunes segments.  A workgroup skips a segment only when f < -2 on every sample of its
 *    tile, and any q < -2 (the initial -inf included) clamps to the same drawn void value.
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error, nothing written by it): data null; n_seg outside 1..65536;
 * data_dims[1] != 8; any of a segment's 8 floats not finite; a radius below 0; a coordinate or radius above 2^20 in magnitude (so every
 * product above stays finite for sample positions of that size). */

#define VTMC_MOD_DETACH 11   /* removes what no longer hangs on anything: every floating fragment of the box (not in the reference).
                                                           data_dims[0] = max_samples (>= 0; 0: no limit), an integer in data_dims
                                                           as VTMC_MOD_STAMP's id is.  add_or_erode must be 0, data NULL,
                                                           data_dims[1] 0; p[0..7] are not read. */
/* FRAGMENTS: the one question about the terrain that is not local -- after this dig, what is still attached to the ground?  The rule below
 * is shared by VTMC_MOD_DETACH and vtmc_terrain_fragments (further down); it is integers and 32-bit copies only, there is no tolerance in
 * it, and nothing in it depends on how the labelling is done.
 *   Box        the clamped sample box of lower / upper: world bounds, floor / ceil, clamped to [0, dim + 1], exactly as for every modifier.
 *              An empty box: nothing to do.
 *   Solid      a sample is solid when s > 0: strict, and NaN is not solid -- the classify kernel's test.
 *   Component  two solid samples of the box are joined when they are neighbours along x, y or z (6-connectivity); a component is a class
 *              of that relation, taken inside the box only.  Diagonal contact does not join.  This is THE LIBRARY'S OWN rule and the safe
 *              side: two solid samples across an edge of the lattice are always one piece of the mesh, whatever the case tables choose,
 *              while what the tables do with two solid samples that touch only diagonally depends on the case (the ambiguous faces).  A
 *              piece that hangs on by a diagonal alone is therefore treated as loose, never the other way round.
 *   Anchored   a component that holds at least one sample on any of the six faces of the box.  What reaches the edge of the box may go on
 *              outside it; where a face of the box is a face of the grid, the world's border holds it.
 *   Fragment   every other component.  Its seed is its sample of smallest grid index x + dim_x * (y + dim_y * z); lo / hi are its tight
 *              inclusive sample bounds; n_samples is its solid sample count.
 *   Size limit with max_samples > 0 a fragment of n_samples > max_samples is left alone and not listed (a sky island that is meant to
 *              float); 0: no limit.
 *   Order      fragments are listed in increasing grid index of the seed.
 * VTMC_MOD_DETACH writes every sample of every fragment as an erode whose clamped density is 2 does: with the event number e the modifier
 * takes and the sample's grid index i, s becomes Clamp(min(s, -2), void, full) = uniform(seed, e, i, 2) - 2, a void value in [-2, -1).
 * Every other sample keeps its bits.  The modifier takes its box from lower / upper, marks the dirty blocks of that box (also when nothing
 * was removed), is journaled (its box: undo restores it bit for bit, redo puts the values back without labelling again) and takes one event
 * number exactly as kinds 0-3, in queue order with every other kind, and sees what the earlier modifiers of its queue wrote: in a queue
 * [erode sphere, detach(box around it)] the dig and what falls off are ONE undo step.
 * VTMC_ERR_INVALID_ARG (the modifier's index in vtmc_last_error, nothing written by it): add_or_erode != 0; data not NULL;
 * data_dims[0] < 0; data_dims[1] != 0. */

/* One queued TerrainModifier (TerrainModifier.cs:19-33).  lower / upper are the values the C#
 * LowerBound / UpperBound properties return (world space): the shim copies them, so Unity's
 * Vector3.ProjectOnPlane stays on the C# side. */
typedef struct vtmc_modifier {
    int32_t kind;
    int32_t add_or_erode; /* 1: add (union, max), 0: erode (difference, clamped min of the negation) */
    float lower[3];
    float upper[3];
    float p[8];
    const float *data;    /* VTMC_MOD_HEIGHTMAP and VTMC_MOD_PATH only: borrowed for the call, copied to the device */
    int32_t data_dims[2];
} vtmc_modifier;

/* Replaces the grid allocation + fill of VoxelTerrain.Init (VoxelTerrain.cs:121-149): a
 * (width+2, elevation+2, height+2)-sample grid in HBM, every sample a "void" value in [-2,-1].
 * The reference draws voidDensity / fullDensity from UnityEngine.Random on every read
 * (VoxelTerrain.cs:50-51); here they are a counter-based hash of (seed, event, sample, draw) with
 * the same ranges and the same number of draws, so results are reproducible.  Errors as the
 * reference's: dims not a multiple of 8, more than 1025 samples per axis (VoxelTerrain.cs:138-142). */
int32_t vtmc_terrain_init(vtmc_ctx *ctx, int32_t width, int32_t elevation, int32_t height, float voxel_scale,
                          const float terrain_origin[3], uint64_t seed);

/* Replaces VoxelTerrain.Update (VoxelTerrain.cs:262-325) for a queue of n_mods modifiers, applied
 * in order: AABB -> sample range (floor / ceil, clamped to [0, dim+1]), per-sample density write,
 * union of dirty blocks (a block is dirty on an axis when up >= 8b && low <= 8b+8), then
 * BatchUpdate on that set.  The dirty list is ordered by bx + nbx*(by + nby*bz) (the reference's
 * HashSet order is arbitrary); `block` of a triangle indexes it.  *n_dirty_blocks and *tri_count may
 * be NULL.  Triangles are read with vtmc_read_triangles / vtmc_device_results as after any extract. */
int32_t vtmc_terrain_update(vtmc_ctx *ctx, const vtmc_modifier *mods, int32_t n_mods, int32_t *n_dirty_blocks,
                            int32_t *tri_count);

/* The dirty list of the last vtmc_terrain_update: n (bx,by,bz) triples (_nextUpdateblocks,
 * VoxelTerrain.cs:321). */
int32_t vtmc_terrain_dirty_blocks(vtmc_ctx *ctx, int32_t *dst, int32_t capacity_blocks, int32_t *n_blocks);

/* Copies the density grid to the host: dst[x*stride_x + y*stride_y + z*stride_z] (element strides;
 * a C# float[W+2,E+2,H+2] is ((E+2)*(H+2), H+2, 1)).  Parity / debugging / persistence. */
int32_t vtmc_terrain_read_samples(vtmc_ctx *ctx, float *dst, int64_t stride_x, int64_t stride_y, int64_t stride_z);

/* Device pointer + element strides of the grid (x fastest), for GPU-resident callers. */
int32_t vtmc_terrain_device_grid(vtmc_ctx *ctx, const float **d_samples, int64_t strides[3], int32_t dims[3]);

/* Undo / redo of terrain edits (off by default; not in the reference).  vtmc_terrain_set_history(ctx, max_bytes) allocates a device
 * journal of max_bytes and clears the history; 0 turns history off and frees it.  While history is on, a vtmc_terrain_update that
 * writes at least one sample records one step: per modifier, the samples of its clamped sample box as they were before (4 bytes per
 * sample, each box rounded up to 256 bytes) and the bounds its dirty blocks were found from.  A call that writes no sample (an empty
 * queue, modifiers wholly outside the grid) records nothing and keeps both stacks.  A step discards every undone step; the oldest
 * steps are dropped until it fits (steps of equal size S: floor(max_bytes / S) are kept; the journal is a ring).  A step larger than
 * max_bytes, or an update that fails after writing, clears the history.  vtmc_terrain_init clears it and keeps the budget.
 * Where a step lies: its bytes are one contiguous range of the journal.  After the undone steps are discarded it begins where the
 * newest remaining step ends (at offset 0 when none remains), or at offset 0 when it would reach past max_bytes from there; the bytes
 * it leaves behind at the journal's end stay unused until the ring comes round.  Then the oldest steps are dropped until no remaining
 * step shares a byte with the new one and the offsets of the remaining steps and the new one, read oldest to newest, fall at most once
 * (the ring wraps once): a step stranded at the journal's end behind a step that wrapped goes before any step in front of it does.
 *
 * vtmc_terrain_undo restores the newest step's boxes bit for bit in reverse modifier order, vtmc_terrain_redo puts the newest undone
 * step's values back in modifier order (no modifier is evaluated again); each then extracts that step's dirty set as its update did,
 * and returns, lists (vtmc_terrain_dirty_blocks) and leaves for the read_* / raycast calls exactly what vtmc_terrain_update does.
 * Neither changes the event counter the clamp draws of later updates hash.  VTMC_ERR_NO_RESULT when there is nothing to undo / redo,
 * with nothing changed.  vtmc_terrain_history reports the steps that can be undone / redone and the journal bytes they hold. */
int32_t vtmc_terrain_set_history(vtmc_ctx *ctx, int64_t max_bytes);
int32_t vtmc_terrain_undo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count);
int32_t vtmc_terrain_redo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count);
int32_t vtmc_terrain_history(const vtmc_ctx *ctx, int32_t *n_undo, int32_t *n_redo, int64_t *bytes_used);

/* Saving a session: the resident terrain as a sparse brick file (not in the reference, which has no persistence; layout:
 * volumetricterrain_amd/terrainfile.py -- 64-byte header {magic "VTMT", version 1, flags, W, E, H, voxel_scale, origin, seed, events,
 * n_raw}, one kind byte per brick padded to 16 bytes, then the RAW bricks, 2048 bytes each, in increasing brick index; the file is
 * exactly 64 + pad16(bricks) + 2048 * n_raw bytes).
 *
 * The (W+2, E+2, H+2) sample grid is cut into disjoint 8x8x8-sample bricks, W/8 + 1 along x and likewise along y and z (the last brick
 * of an axis holds 2 sample planes), brick index bx + nbx*(by + nby*bz).  A brick's kind is
 *   1 VOID  every sample of it satisfies s <= -1, and every sample of the up-to-27 bricks around it (clipped at the grid) !(s > 0);
 *   2 FULL  every sample of it satisfies s >= 1, and every sample of those bricks s > 0;
 *   0 RAW   everything else, including any brick that holds a NaN.
 * RAW bricks are stored and restored as 32-bit copies (sample (i,j,k) of a brick at i + 8j + 64k, +0.0f outside the grid): NaN payloads
 * and -0 survive.  VOID / FULL bricks are elided, and vtmc_terrain_load redraws them from the hash vtmc_terrain_init's void values come
 * from, under one new event number e = saved events + 1: a VOID sample becomes uniform(seed, e, grid index, 0) - 2 in [-2,-1), a FULL
 * sample uniform(seed, e, grid index, 1) + 1 in [1,2).  With VTMC_TERRAIN_SAVE_EXACT every brick is RAW.
 *
 * Why the rule is safe: the extract path reads a sample only as a corner of an active cell, or as the forward neighbour of such a
 * corner (the normal's forward difference, SampleNormal.compute:27-30).  Such a sample lies within 2 samples of a sign change, that
 * is of a sample with s > 0 and of one without; the neighbourhood test is a conservative whole-brick dilation of that distance, so
 * the brick of a sample that is read is neither VOID nor FULL.  A redrawn sample keeps its sign class, so no cell changes its case.
 * Elided samples therefore never reach a triangle, a ray hit or a sphere query: the mesh after a load is the mesh before the save, bit
 * for bit.  What is lost by contract are the random mantissa bits of saturated samples away from the surface.
 *
 * vtmc_terrain_save changes nothing in the context (grid, history, last result, event counter); it waits for work queued on the
 * context's stream as vtmc_terrain_read_samples does.  Classify, compact and pack run on the device; only the kind table and the RAW
 * bricks cross PCIe, in slices of a fixed pinned stage.  *bytes_written (may be NULL) is the size of the file.
 *
 * vtmc_terrain_load (re)initialises the terrain from the file alone (dims, voxel_scale, origin, seed), with or without an earlier
 * vtmc_terrain_init; it clears the history and keeps its budget, and the event counter becomes e.  It then extracts every block, and
 * returns, lists and leaves for the read_* and query calls what a vtmc_terrain_update that dirtied every block does; with
 * VTMC_TERRAIN_LOAD_NO_EXTRACT it extracts nothing and leaves no result.  The file is untrusted: wrong magic or version, dims not a
 * multiple of 8 or above 1024, a scale not finite or <= 0, an origin not finite, an unknown kind byte, n_raw different from the number
 * of kind-0 bytes, or a file size different from the one the header implies are answered with VTMC_ERR_INVALID_ARG before the resident
 * terrain is touched (file faults: the codes of vtmc_chunk_read).  A read that fails after that check leaves the context without a
 * terrain, and vtmc_last_error says so.
 *
 * vtmc_terrain_write_samples is the inverse of vtmc_terrain_read_samples (same element strides, 32-bit copies) on an initialised
 * terrain: it clears the history, takes no event number and extracts nothing -- for hosts migrating a C# _voxelSamples.
 * VTMC_ERR_NO_RESULT from save / write_samples without a terrain; VTMC_ERR_INVALID_ARG for null, range or flag errors. */
#define VTMC_TERRAIN_SAVE_EXACT 1u      /* every brick stored raw: load restores all samples bit for bit */
int32_t vtmc_terrain_save(vtmc_ctx *ctx, const char *path, uint32_t flags, int64_t *bytes_written);

#define VTMC_TERRAIN_LOAD_NO_EXTRACT 1u
int32_t vtmc_terrain_load(vtmc_ctx *ctx, const char *path, uint32_t flags, int32_t *n_dirty_blocks, int32_t *tri_count);

int32_t vtmc_terrain_write_samples(vtmc_ctx *ctx, const float *src, int64_t stride_x, int64_t stride_y, int64_t stride_z);

/* Stamps: density volumes the context keeps in device memory, for VTMC_MOD_STAMP to paste (not in the reference, whose modifiers are
 * analytic): authored content -- a sculpted rock, a prefab tunnel section -- or a captured piece of the terrain, caves and overhangs included,
 * pasted as often as wanted without another upload.  A stamp is nx * ny * nz FP32 samples, x fastest; each of nx, ny, nz lies in 2..1026
 * and nx * ny * nz is at most 2^27 (anything else: VTMC_ERR_INVALID_ARG).  Ids are positive, count up per context and are never reused in
 * it.  Stamps are no part of the terrain: they survive vtmc_terrain_init, vtmc_terrain_load, undo and redo, they are not written to the
 * terrain file (a host that wants to keep one reads it with vtmc_stamp_read), and vtmc_destroy frees them.  An unknown or destroyed id
 * answers VTMC_ERR_INVALID_ARG.
 *   vtmc_stamp_create   uploads host samples, sample (x, y, z) = src[x*stride_x + y*stride_y + z*stride_z] (element strides, all positive).
 *                       A sample that is not finite is refused with VTMC_ERR_INVALID_ARG before anything is uploaded.
 *   vtmc_stamp_capture  copies the box [first_sample, first_sample + n) of the resident grid on the device, as 32-bit copies: nothing crosses
 *                       PCIe.  The box must lie inside the (W+2, E+2, H+2) grid (VTMC_ERR_INVALID_ARG); VTMC_ERR_NO_RESULT without a terrain.
 *                       It changes nothing in the terrain: not the grid, the history, the event counter or the last result.
 *   vtmc_stamp_info     the dims of a stamp.
 *   vtmc_stamp_read     copies a stamp to the host with element strides as vtmc_stamp_create's.
 *   vtmc_stamp_destroy  frees it; a step of the history that pasted it is still undone and redone. */
int32_t vtmc_stamp_create(vtmc_ctx *ctx, const float *src, int32_t nx, int32_t ny, int32_t nz, int64_t stride_x, int64_t stride_y,
                          int64_t stride_z, int32_t *stamp_id);
int32_t vtmc_stamp_capture(vtmc_ctx *ctx, const int32_t first_sample[3], int32_t nx, int32_t ny, int32_t nz, int32_t *stamp_id);
int32_t vtmc_stamp_info(const vtmc_ctx *ctx, int32_t stamp_id, int32_t dims[3]);
int32_t vtmc_stamp_read(vtmc_ctx *ctx, int32_t stamp_id, float *dst, int64_t stride_x, int64_t stride_y, int64_t stride_z);
int32_t vtmc_stamp_destroy(vtmc_ctx *ctx, int32_t stamp_id);

/* The fragment query (not in the reference): lists, and optionally captures as stamps, exactly the fragments a VTMC_MOD_DETACH with the same
 * lower / upper and max_samples would remove now (the rule: FRAGMENTS, at VTMC_MOD_DETACH above), in the rule's order.  It changes nothing:
 * not the grid, the history, the event counter, the dirty list or the result the context holds; it waits for work queued on the context's
 * stream as vtmc_terrain_read_samples does.  Labelling, counting, bounds and capture run on the device; only the records cross PCIe.
 *   dst = NULL            count only: *n_fragments is set, nothing is captured.
 *   capacity < n          VTMC_ERR_CAPACITY with *n_fragments set and nothing captured.
 *   capture_min_samples   > 0: every listed fragment with n_samples >= capture_min_samples also becomes a stamp, its id in stamp_id.  The
 *                         stamp box is [max(lo - 2, box lo), min(hi + 2, box hi)] per axis: it never leaves the query box, and since a
 *                         fragment touches no face of that box the margin is at least 1 on every side and every dim at least 3.  A stamp
 *                         sample is the grid's 32-bit value where the grid sample is not solid or belongs to this fragment, and -s where
 *                         it is solid but belongs to something else: another piece in the box becomes equally deep air, so the stamp
 *                         meshes to this fragment alone.  A fragment whose stamp box breaks the stamp limits (2^27 samples) keeps
 *                         stamp_id 0.  If an allocation fails, the stamps this call made are destroyed and the call returns
 *                         VTMC_ERR_DEVICE.  The stamps are ordinary stamps: vtmc_stamp_info / _read / _destroy and VTMC_MOD_STAMP work
 *                         on them (pasted unturned in replace mode at its own box, one puts its fragment back bit for bit).
 * VTMC_ERR_NO_RESULT without a terrain; VTMC_ERR_INVALID_ARG for null bounds, a bound that is NaN, or a negative max_samples or
 * capture_min_samples; VTMC_ERR_DEVICE ("labelling did not converge") should the labelling ever break its own bounds.
 * A host's flow for a dig: vtmc_terrain_update [erode]; vtmc_terrain_fragments with capture; spawn the debris from the stamps;
 * vtmc_terrain_update [detach]. */
typedef struct vtmc_fragment {
    int32_t seed[3];     /* sample of smallest grid index */
    int32_t lo[3];       /* tight bounds, inclusive */
    int32_t hi[3];
    int32_t n_samples;   /* solid samples */
    int32_t stamp_id;    /* 0: not captured */
    int32_t reserved;    /* 0 */
} vtmc_fragment;         /* 48 bytes */

int32_t vtmc_terrain_fragments(vtmc_ctx *ctx, const float lower[3], const float upper[3], int32_t max_samples, int32_t capture_min_samples,
                               vtmc_fragment *dst, int32_t capacity, int32_t *n_fragments);

/* NAVIGATION: the other non-local question -- where can something walk, and which places are connected? -- is answered by a layer with a
 * header of its own, include/vtmc_nav.h (walkable spans, links and regions of a box of the resident terrain; same library, same context).
 * It includes this header and adds nothing to it. */

/* Mesh stamps: a closed triangle mesh -- a rock, an arch, a prefab tunnel mouth -- voxelized on the device into an ordinary stamp (not in
 * the reference).  positions = n_vertices x 3 floats, indices = n_triangles x 3 vertex numbers; both are host pointers, borrowed for the
 * call and copied to the device.  Stamp sample (i, j, k) lies at px = (float)i * h + first[0], py = (float)j * h + first[1],
 * pz = (float)k * h + first[2] (the form terrain positions take; monotonic in the index).  The result is a stamp like any other: an id from
 * the context's counter, the dims limits above, x fastest, read by vtmc_stamp_read, pasted by VTMC_MOD_STAMP, freed by vtmc_stamp_destroy
 * or vtmc_destroy.  The call needs no terrain and changes nothing in one: not the grid, the history, the event counter or the last result.
 *
 * A sample's value is s = sigma * min(dmin / h, VTMC_MESH_BAND): the distance to the nearest triangle in stamp samples, positive inside
 * (solid, the library's sign), saturating at +-3.  A paste clamps by its own rule and anything beyond +-2 draws a void or full value, so
 * the band loses nothing.  THE RULE, one IEEE operation per step in the order written (library built with -ffp-contract=off):
 *
 * On the host, FP32:  reach = the largest of h, |first[k]|, |(float)(n_k - 1) * h + first[k]| and every |coordinate| of a triangle's
 * vertices;  g = 3.0f * h + 1e-4f * reach.
 *
 * Per triangle, v0, v1, v2 are its three vertices in ascending order of (x, then y, then z) of their values, so neither the order in
 * which a triangle names its vertices nor the order of the triangles changes a bit of the result; min_k, max_k are their float extremes
 * per axis.
 *
 * Distance, FP32.  dmin = +inf; per triangle (a, b, c) = (v0, v1, v2):
 *   the triangle bids only inside its reach box: px >= min_x - g && px <= max_x + g, and the same for y and z; there
 *   ab = b - a;  ac = c - a;  ap = p - a;  bp = p - b;  cp = p - c                    (per component)
 *   d1 = ab.ap;  d2 = ac.ap;  d3 = ab.bp;  d4 = ac.bp;  d5 = ab.cp;  d6 = ac.cp       (u.v = (ux*vx + uy*vy) + uz*vz)
 *   vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *   the first region that holds (Voronoi regions of the triangle, Ericson 5.1.5), q = (a + ab*wb) + ac*wc per component unless said:
 *     d1 <= 0 && d2 <= 0:                           wb = 0, wc = 0                      (vertex a)
 *     d3 >= 0 && d4 <= d3:                          wb = 1, wc = 0                      (vertex b)
 *     vc <= 0 && d1 >= 0 && d3 <= 0:                wb = d1 / (d1 - d3), wc = 0         (edge ab)
 *     d6 >= 0 && d5 <= d6:                          wb = 0, wc = 1                      (vertex c)
 *     vb <= 0 && d2 >= 0 && d6 <= 0:                wb = 0, wc = d2 / (d2 - d6)         (edge ac)
 *     va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0:      w = (d4 - d3) / ((d4 - d3) + (d5 - d6));  q = b + w*(c - b)   (edge bc)
 *     otherwise:                                    den = 1 / ((va + vb) + vc);  wb = vb*den;  wc = vc*den         (face)
 *   cx = px - qx;  cy = py - qy;  cz = pz - qz;  d = sqrtf((cx*cx + cy*cy) + cz*cz);  if (d < dmin) dmin = d
 * A d that is NaN (a triangle without area can give one) bids nothing, so dmin does not depend on the order of the triangles.  The reach
 * box hides nothing the band would show: outside it a closest point found to within 1e-4 * reach is farther than 3h.  It is part of the
 * rule so that the result never depends on how the kernel prunes triangles, whatever the rounding does to a sliver's closest point.
 *
 * Sign: sigma = +1 iff an odd number of triangles cover p and lie in front of it, along a ray from p towards +x; else -1.  Even-odd, so
 * the winding order is irrelevant and a self-intersecting closed mesh gets even-odd semantics.  FP64 from the float inputs (each float
 * converted exactly), comparisons of floats as they are:
 *   covers:  per edge (v0 v1), (v1 v2), (v2 v0) of the triangle, its end points ordered lo, hi by (z, then y) of their values (hi is the
 *     one with the larger z, or with equal z the larger y):  the edge straddles iff lo.z <= pz && pz < hi.z (half-open: a horizontal edge
 *     never does);  a straddling edge counts iff  (hi.y - lo.y)*(pz - lo.z) - (py - lo.y)*(hi.z - lo.z) > 0.
 *     The triangle covers p iff an odd number of its edges count and min_y <= py && py <= max_y.
 *     (The order is by value, so both triangles at a shared edge compute the same determinant: a ray through an edge or a vertex is
 *     claimed by exactly one of them.)
 *   in front:  px >= max_x: no;  px < min_x: yes;  otherwise with u = v1 - v0, w = v2 - v0,
 *     n.x = u.y*w.z - u.z*w.y;  n.y = u.z*w.x - u.x*w.z;  n.z = u.x*w.y - u.y*w.x
 *     t = (n.x*(px - v0.x) + n.y*(py - v0.y)) + n.z*(pz - v0.z);   in front iff (t < 0 && n.x > 0) || (t > 0 && n.x < 0)
 *     (a triangle with n.x == 0 never counts).
 * Then r = dmin / h;  m = r < 3.0f ? r : 3.0f;  s = sigma > 0 ? m : -m  (no triangle in reach: +-3; on the surface: +-0).
 *
 * VTMC_ERR_INVALID_ARG, with nothing allocated and no id taken: a null pointer; n_triangles outside 1..VTMC_MESH_MAX_TRIANGLES;
 * n_vertices < 3; an index outside 0..n_vertices-1; a position that is not finite or above 2^20 in magnitude; first not finite; h not
 * finite or <= 0; dims outside the stamp limits; flags other than VTMC_MESH_TRUST_CLOSED; a mesh that is not closed, unless that flag
 * is set.  Closed means: after dropping the triangles that repeat an index, every undirected index pair is used by exactly two
 * triangles (checked on the host; vtmc_last_error names the first offending edge).  Vertices are told apart by index, not by position:
 * weld duplicates first.  With VTMC_MESH_TRUST_CLOSED the rule is applied to whatever triangles are given. */
#define VTMC_MESH_MAX_TRIANGLES (1 << 20)
#define VTMC_MESH_BAND 3.0f              /* stamp values saturate at +-3 grid units */
#define VTMC_MESH_TRUST_CLOSED 1u        /* skip the host's closed-mesh check */
int32_t vtmc_stamp_from_mesh(vtmc_ctx *ctx, const float *positions, int32_t n_vertices, const int32_t *indices, int32_t n_triangles,
                             const float first[3], float h, int32_t nx, int32_t ny, int32_t nz, uint32_t flags, int32_t *stamp_id);

/* ------------------------------------------------------------------------------------------
 * Material layer -- the device form of VoxelTerrain.SetControlMap (VoxelTerrain.cs:186-209, filled by TerrainEngine.cs:107-142): the two
 * 3-D RGBA8 splat textures the triplanar shaders sample at (worldPos - _Offset) * _Scale (Triplanar8Tex.shader:97,193), kept in HBM beside
 * the density grid, a paint brush on them (not in the reference, which can only replace a texture whole, from the CPU), and the material
 * weights of every vertex of an extracted mesh, so that a consumer that is not Unity's sampler -- a collider's surface type, a footstep
 * sound, an exporter, vertex colours -- needs no 3-D texture.
 *
 * The layer is a cube of C = 16 * fineness texels per axis, fineness 1..8 (the reference clamps it so, VoxelTerrain.cs:191).  A texel
 * holds VTMC_MATERIAL_CHANNELS = 8 bytes at byte offset 8 * (i + C*(j + C*k)), x fastest as the reference's map[x + y*C + z*C*C]:
 * channels 0..3 are group 1's r, g, b, a (_matControlTex1), channels 4..7 group 2's.  The cube spans the terrain's W x E x H cells,
 * stretched per axis, as _Scale = 1 / TerrainSize does.  All arithmetic below is FP32, one IEEE operation per step in the order written
 * (library built with -ffp-contract=off); rintf rounds ties to even, as Mathf.Round.
 *
 * vtmc_material_init  needs a terrain (VTMC_ERR_NO_RESULT without one); fineness outside 1..8 is VTMC_ERR_INVALID_ARG.  Allocates the cube
 *   and sets every texel to (255,0,0,0, 0,0,0,0), as TerrainSample starts with _matComponents[0] = 1.  Calling it again replaces the layer.
 *   vtmc_terrain_init and vtmc_terrain_load drop the layer (the dims may change); every other material call without a layer answers
 *   VTMC_ERR_NO_RESULT.  The layer is no part of the terrain file, whose format stays as it is: a host persists it with
 *   vtmc_material_read / _write.
 * vtmc_material_set_control_map  group is 1 or 2; rgba is C^3 x 4 floats, a Color[] in the texel order above.  Each channel becomes
 *   (uint8)rintf(clamp(c, 0, 1) * 255.0f); the other group's four bytes are kept.  The float image crosses PCIe and is quantised on the
 *   device.  A NaN anywhere in the image is VTMC_ERR_INVALID_ARG, with nothing written.
 * vtmc_material_write / _read  copy the whole C^3 x 8 bytes; *size (may be NULL) receives C.  vtmc_material_read with dst = NULL is the
 *   size query.
 *
 * vtmc_material_paint  applies n_strokes strokes in order.  On the host, per axis:  ts_x = ((float)W * voxel_scale) / (float)C, with E and
 *   H for y and z.  Per texel (i, j, k) and stroke (c, r, s, channel):
 *     px = ((float)i + 0.5f) * ts_x + origin_x;  py, pz alike;  dx = px - c0;  dy, dz alike
 *     d = sqrtf((dx*dx + dy*dy) + dz*dz);  t = 1 - d / r;  t = t + t;  t = clamp(t, 0, 1);  w = s * t      (the sculpt brushes' falloff)
 *     w == 0: the texel keeps its bytes;  otherwise per channel k:
 *       v = (float)old[k];  T = (k == channel) ? 255.0f : 0.0f;  v = v + (T - v) * w;  new[k] = (uint8)rintf(v)     (in [0, 255] unclamped)
 *   A stroke does not wrap: texels are 0..C-1 per axis, paint near one face never reaches the opposite one.  The rule is pointwise, so the
 *   result does not depend on which box of texels the kernel walks or on its applying every stroke of the call to a texel in one pass.
 *   VTMC_ERR_INVALID_ARG (the stroke's index in vtmc_last_error, nothing written by the call): a centre that is not finite; r not finite or
 *   <= 0; s not finite or outside [0, 1]; a channel outside 0..7; n_strokes outside 0..VTMC_MATERIAL_MAX_STROKES; null strokes with
 *   n_strokes > 0.
 *   Paint is NOT journaled: vtmc_terrain_undo / _redo restore densities and leave the layer alone (an editor that wants to undo paint
 *   keeps the bytes of vtmc_material_read, 8 C^3 of them at most 16 MB).  Paint takes no event number, marks no block dirty, extracts
 *   nothing and leaves the last result and its vertex weights as they are.
 *
 * vtmc_material_vertices  computes the weights of every vertex of the result the context holds, 8 bytes per vertex, into a library-owned,
 *   grow-only buffer; *n_vertices (may be NULL) receives n.  The result must come from the resident terrain -- vtmc_terrain_update, _undo,
 *   _redo, or _load with extraction -- in either output mode.  Soup: vertex 3*t + v of triangle t in record order, n = 3*T.  Indexed: one
 *   per vtmc_vertex, n = V.  Per vertex, with (bx, by, bz) the block of the dirty list its `block` field (soup) or the block vertex
 *   offsets (indexed) name, and sx = (float)C / (float)W computed once on the host (E and H for y and z):
 *     gx = (float)(8*bx) + position.x;  tx = gx * sx;  tx = tx - 0.5f
 *     i0 = (int)floorf(tx);  fx = tx - (float)i0;  i0 = ((i0 % C) + C) % C;  i1 = (i0 + 1) % C
 *       (the texture's Repeat wrap: tx = -0.5 at gx = 0 reads texels C-1 and 0);  j0, j1, fy and k0, k1, fz alike
 *     per channel, bytes converted to float, in the stamp's lerp form:
 *       a00 = m[i0,j0,k0] + (m[i1,j0,k0] - m[i0,j0,k0]) * fx;  a10 the same at j1;  a01 at k1;  a11 at j1, k1
 *       b0 = a00 + (a10 - a00) * fy;  b1 = a01 + (a11 - a01) * fy;  q = b0 + (b1 - b0) * fz;  out = (uint8)rintf(q)
 *   The filter is THE LIBRARY'S OWN: a trilinear filter in FP32.  A texture unit filters with fixed-point weights of a few bits; its
 *   values are not reproduced and parity with a GPU sampler is not claimed.
 *   VTMC_ERR_NO_RESULT without a layer, without a result, or when the result did not come from the terrain (vtmc_extract_*).  T = 0 is
 *   success with 0 vertices.  The weights belong to one result: after any later extract they are stale, and vtmc_material_read_vertices /
 *   _device_results answer VTMC_ERR_NO_RESULT until vtmc_material_vertices runs again.
 * vtmc_material_read_vertices  copies the n x 8 bytes; a capacity below n is VTMC_ERR_INVALID_ARG.
 * vtmc_material_device_results  the device pointer of the same (valid until the next vtmc_material_vertices / destroy).
 * ------------------------------------------------------------------------------------------ */
#define VTMC_MATERIAL_CHANNELS 8
#define VTMC_MATERIAL_MAX_STROKES 4096

typedef struct vtmc_material_stroke {
    float center[3];   /* world */
    float radius;
    float strength;    /* [0, 1] */
    int32_t channel;   /* 0..7 */
} vtmc_material_stroke;

int32_t vtmc_material_init(vtmc_ctx *ctx, int32_t fineness);
int32_t vtmc_material_set_control_map(vtmc_ctx *ctx, const float *rgba, int32_t group);
int32_t vtmc_material_write(vtmc_ctx *ctx, const uint8_t *src);
int32_t vtmc_material_read(vtmc_ctx *ctx, uint8_t *dst, int32_t *size);
int32_t vtmc_material_paint(vtmc_ctx *ctx, const vtmc_material_stroke *strokes, int32_t n_strokes);
int32_t vtmc_material_vertices(vtmc_ctx *ctx, int64_t *n_vertices);
int32_t vtmc_material_read_vertices(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity_vertices);
int32_t vtmc_material_device_results(vtmc_ctx *ctx, const uint8_t **d_weights, int64_t *n_vertices);

/* ------------------------------------------------------------------------------------------
 * Ambient occlusion -- the second per-vertex attribute of a terrain extract (not in the reference): one byte per vertex, computed on the
 * device from the resident density grid, in either output mode.  255 = fully open, 0 = fully occluded at strength 1.  It is THE LIBRARY'S
 * OWN measure, a clamped-density march along 26 lattice directions; it is no ray-traced visibility integral and parity with any
 * renderer's AO is not claimed.  Density above 0 is solid; the CSG clamp saturates the interior to [1, 2), hence the clamp to 1.  Its
 * life cycle is that of the vertex material weights: computed on demand for the result the context holds, library-owned, stale after the
 * next extract.  Derived data: neither saved with the terrain nor journaled.
 *
 * All arithmetic is FP32, one IEEE operation per step in the order written (library built with -ffp-contract=off); / and sqrtf are
 * correctly rounded, rintf rounds ties to even.
 *
 * Host, once per call, S = steps:   Rg = radius / voxel_scale;   for s = 1..S:  h[s] = Rg * ((float)s / (float)S);
 *   fall[s] = 1.0f - (float)(s - 1) / (float)S.
 * Directions: the 26 lattice directions (i, j, k) in {-1, 0, 1}^3 without (0, 0, 0), numbered m = 0..25 in ascending order of
 *   (i+1) + 3*(j+1) + 9*(k+1);  d_m = ((float)i * len, (float)j * len, (float)k * len), len by the number of non-zero components:
 *   one 1.0f, two 0.70710678f, three 0.57735027f (the literals are part of the rule).
 * Per vertex: position p and normal n as the record holds them (soup corner 3t + v, or vtmc_vertex v; the normal is the un-normalised
 *   gradient normal the extract wrote), block (bx, by, bz) found as vtmc_material_vertices finds it.
 *     gx = (float)(8*bx) + p.x;  gy, gz alike                            (grid sample coordinates: sample i sits at i)
 *     l = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z)
 *     if (!(l > 0) || !(l < INFINITY)):  out = 255                       (the NaN normal of a flat gradient: unoccluded)
 *     else  N = n / l per component;  num = 0;  den = 0;  for m = 0..25 in order:
 *       c = (N.x*d.x + N.y*d.y) + N.z*d.z;   if (!(c > 0)) skip this direction
 *       o = 0;  for s = 1..S:
 *         qx = gx + d.x*h[s];  qy, qz alike;   r = fetch(q);   r = r > 0 ? (r < 1 ? r : 1) : 0      (a NaN sample occludes nothing)
 *         r = r * fall[s];   if (r > o) o = r
 *       num = num + c*o;   den = den + c
 *     a = 1.0f - strength * (num / den);   a = a > 0 ? (a < 1 ? a : 1) : 0;   out = (uint8)rintf(a * 255.0f)
 *   den > 0 always holds: some lattice direction makes less than 55 degrees with any unit vector.
 * fetch(q) reads the (W+2, E+2, H+2) grid with clamp-to-edge.  Per axis with n samples:
 *     t = q < 0 ? 0 : (q > (float)(n-1) ? (float)(n-1) : q);   i0 = (int)floorf(t);   if (i0 > n-2) i0 = n-2;   f = t - (float)i0
 *   and the eight samples are combined in the material rule's lerp form a + (b - a)*f, along x, then y, then z.
 * The grid is read as it is at the time of the call.  The rule is pointwise: the result depends neither on the launch shape nor on how
 * the kernel stages samples.
 *
 * vtmc_ao_vertices  computes the byte of every vertex of the result the context holds into a library-owned, grow-only buffer;
 *   *n_vertices (may be NULL) receives n.  Soup: vertex 3*t + v, n = 3*T.  Indexed: n = V.  VTMC_ERR_NO_RESULT without a terrain, without
 *   a result, or when the result did not come from the resident terrain.  T = 0 is success with 0 vertices.  VTMC_ERR_INVALID_ARG, with
 *   nothing computed and the previous values kept: null ctx or params; radius not finite or <= 0; radius / voxel_scale >
 *   VTMC_AO_MAX_RADIUS_CELLS; strength not finite or outside [0, 1]; steps outside 1..VTMC_AO_MAX_STEPS; flags != 0.
 *   The values belong to one result: after any later extract vtmc_ao_read_vertices / _device_results answer VTMC_ERR_NO_RESULT until
 *   vtmc_ao_vertices runs again.  The material layer plays no part: neither call needs or disturbs the other's values.
 * vtmc_ao_read_vertices  copies the n bytes; a capacity below n is VTMC_ERR_INVALID_ARG.
 * vtmc_ao_device_results  the device pointer of the same (valid until the next vtmc_ao_vertices / destroy).
 * ------------------------------------------------------------------------------------------ */
#define VTMC_AO_MAX_STEPS 8
#define VTMC_AO_MAX_RADIUS_CELLS 6      /* radius / voxel_scale above this: VTMC_ERR_INVALID_ARG */

typedef struct vtmc_ao_params {
    float radius;      /* world units, > 0 */
    float strength;    /* [0, 1] */
    int32_t steps;     /* 1..VTMC_AO_MAX_STEPS */
    uint32_t flags;    /* reserved, must be 0 */
} vtmc_ao_params;      /* 16 bytes */

int32_t vtmc_ao_vertices(vtmc_ctx *ctx, const vtmc_ao_params *params, int64_t *n_vertices);
int32_t vtmc_ao_read_vertices(vtmc_ctx *ctx, uint8_t *dst, int64_t capacity_vertices);
int32_t vtmc_ao_device_results(vtmc_ctx *ctx, const uint8_t **d_ao, int64_t *n_vertices);

/* ------------------------------------------------------------------------------------------
 * Surface scatter -- the third consumer of a terrain extract (not in the reference): instances (grass, rocks, trees) distributed over the
 * triangles of the result by area, filtered by slope, world height and one channel of the material layer, on the device, in either
 * output mode.  It is STABLE UNDER EDITS: every random draw is keyed on the triangle's own vertex coordinates in the grid, not on its
 * index in the result, so a block whose triangles an edit left as they were gets exactly the instances it had; a host replaces the
 * instances of the dirty blocks only.  The life cycle is that of the vertex attributes: computed on demand for the result the context
 * holds, library-owned, stale after the next extract.
 *
 * All arithmetic is FP32, one IEEE operation per step in the order written (library built with -ffp-contract=off); / and sqrtf are
 * correctly rounded; 64-bit integer arithmetic wraps.
 *
 * Hash:  fin(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31   (the finaliser of
 *   the terrain's own counter hash);  G = 0x9E3779B97F4A7C15;  step(k, w) = fin((k ^ (uint64)w) + G).
 * Triangle key:  per corner c and axis a:  g[c][a] = ((float)(8*b_a) + p[c][a]) + 0.0f, with (bx, by, bz) the block as
 *   vtmc_material_vertices finds it and p the block-local position in the record (indexed: of the vtmc_vertex the index names; the
 *   + 0.0f turns -0 into +0);  k = fin((uint64)seed + G);  then for c = 0..2, a = 0..2 in that order:  k = step(k, bits(g[c][a])).
 * Draws:  word(k, i, d) = step(k, ((uint64)i << 8) | d);  U(k, i, d) = (float)(uint32)(word >> 40) * 2^-24;
 *   rnd = (uint32)(word(k, i, 4) >> 32).
 * Per triangle, from the block-local positions p0, p1, p2 and normals n0, n1, n2:
 *     e1 = p1 - p0;  e2 = p2 - p0
 *     cx = e1.y*e2.z - e1.z*e2.y;  cy = e1.z*e2.x - e1.x*e2.z;  cz = e1.x*e2.y - e1.y*e2.x
 *     L = sqrtf((cx*cx + cy*cy) + cz*cz);   if (!(L > 0) || !(L < INFINITY)):  no instances      (degenerate triangles exist in every terrain)
 *     up = cy / L;   if (!(min_up <= up && up <= max_up)):  no instances
 *       (cross(p1 - p0, p2 - p0) points out of the solid, as the record normals do: flat ground under a plane modifier has up = 1)
 *     dc = density * (voxel_scale * voxel_scale), computed on the host;   lam = (0.5f * L) * dc;   fl = floorf(lam)
 *     n = (int)fl + (U(k, 0, 0) < lam - fl ? 1 : 0);   n = min(n, VTMC_SCATTER_MAX_PER_TRIANGLE)
 *       (a triangle inside a unit cell has area at most sqrt(3)/2, so with dc <= 8 the cap never binds)
 * Per candidate i = 0..n-1:
 *     u = U(k, i, 1);  v = U(k, i, 2);   if (u + v > 1.0f):  u = 1.0f - u;  v = 1.0f - v
 *     q = (p0 + e1*u) + e2*v per component;   nrm = (n0 + (n1 - n0)*u) + (n2 - n0)*v per component
 *     world_a = origin_a + ((float)(8*b_a) + q_a) * voxel_scale;   keep iff min_y <= world_y && world_y <= max_y
 *     if material_channel >= 0:  w = the byte vtmc_material_vertices would give a vertex of this block at block-local position q, in that
 *       channel;  keep iff U(k, i, 3) * 255.0f < (float)w
 * Output: the survivors in triangle order, then by ascending i.  block_instance_offsets[b] = the number of instances on blocks before b of
 *   the result's block list; entry B is the total.
 *
 * vtmc_scatter_surface  computes the instances of the result the context holds into library-owned, grow-only buffers; *n_instances (may
 *   be NULL) receives their number.  VTMC_ERR_NO_RESULT without a terrain, without a result, when the result did not come from the
 *   terrain's dirty list (vtmc_extract_*, vtmc_terrain_extract_lod), or with material_channel >= 0 and no material layer.
 *   VTMC_ERR_INVALID_ARG, with nothing computed and the previous instances kept: null ctx or params; density not finite or <= 0;
 *   dc > VTMC_SCATTER_MAX_DENSITY_CELLS; a NaN in, or min > max of, either band; material_channel outside -1..7; max_instances <= 0;
 *   flags != 0.  VTMC_ERR_TOO_LARGE when the total exceeds max_instances: nothing is emitted, the context then holds no scatter, and
 *   vtmc_last_error carries the total, so a host can retry.  T = 0 is success with 0 instances and an all-zero offsets array.
 *   The instances belong to one result: after any later extract vtmc_scatter_read / _device_results answer VTMC_ERR_NO_RESULT until
 *   vtmc_scatter_surface runs again.  Painting or editing afterwards does not change instances already made; the vertex weights and
 *   occlusion bytes of the same result are not disturbed, nor do they disturb the instances.
 * vtmc_scatter_read  copies the instances and (when not NULL) the B + 1 offsets; a capacity below the total is VTMC_ERR_INVALID_ARG.
 * vtmc_scatter_device_results  the device pointers of the same (valid until the next vtmc_scatter_surface / destroy); each may be NULL.
 * ------------------------------------------------------------------------------------------ */
#define VTMC_SCATTER_MAX_DENSITY_CELLS 8.0f   /* density * voxel_scale^2 above this: VTMC_ERR_INVALID_ARG */
#define VTMC_SCATTER_MAX_PER_TRIANGLE 8

typedef struct vtmc_scatter_params {
    float density;            /* instances per world unit^2, finite, > 0 */
    float min_up, max_up;     /* keep a triangle when min_up <= up <= max_up (up: y of its unit face normal); not NaN, min <= max */
    float min_y, max_y;       /* world height band of an instance; not NaN (infinities = no bound), min <= max */
    int32_t material_channel; /* -1: no material filter; 0..7: keep with probability weight/255 of that channel */
    uint32_t seed;
    int32_t max_instances;    /* > 0 */
    uint32_t flags;           /* reserved, 0 */
} vtmc_scatter_params;        /* 36 bytes */

typedef struct vtmc_instance {
    float position[3];        /* world */
    float normal[3];          /* the record normals interpolated, un-normalised */
    uint32_t triangle;        /* index of the triangle in the result (soup record / index triple) */
    uint32_t rnd;             /* 32 random bits of the instance (rotation, scale, variant are the host's to derive) */
} vtmc_instance;              /* 32 bytes */

int32_t vtmc_scatter_surface(vtmc_ctx *ctx, const vtmc_scatter_params *params, int64_t *n_instances);
int32_t vtmc_scatter_read(vtmc_ctx *ctx, vtmc_instance *dst, int64_t capacity, int32_t *block_instance_offsets /* B+1, may be NULL */);
int32_t vtmc_scatter_device_results(vtmc_ctx *ctx, const vtmc_instance **d_instances, const int32_t **d_block_offsets, int64_t *n_instances);

/* ------------------------------------------------------------------------------------------
 * Level of detail -- meshing the resident terrain coarsely far from a viewer (not in the reference, which meshes every block at full
 * resolution and is capped at 1025 samples per axis for it).  vtmc_terrain_extract_lod chooses an octree of NODES around a viewer on the
 * host, gathers every node's 10x10x10 tile from the resident grid on the device and runs the ordinary extraction on the packed tiles.
 *
 * NODE.  A node of level L has stride s = 2^L and a cell origin o, every component of o a multiple of 8 s.  It covers the cells
 * [o, o + 8 s) per axis and is meshed as ONE ordinary 8^3-cell block whose cells are s fine cells wide.  Its tile is the point subsample
 * of the resident grid S (sample counts dim = (W+2, E+2, H+2)) with edge replication:
 *   T[i, j, k] = S[min(o.x + i s, dim_x - 1), min(o.y + j s, dim_y - 1), min(o.z + k s, dim_z - 1)],   i, j, k in 0..9.
 * The largest index of a node is o + 9 s <= dim - 2 + s, so only index 9 can ever clamp, and that sample feeds normals only (the forward
 * difference of the vertices on the node's upper faces).  At L = 0 nothing clamps and the tile is the block's own: a level-0 node is
 * byte for byte the block the ordinary terrain extract produces.
 * The mesh of a node is what the extraction makes of T as a tile of vtmc_extract_blocks: cases, counts, 76-byte records or welded
 * vertices, positions node-local in [0, 8], forward-difference normals of T (in units of the node's own cells).  `block` of a triangle,
 * and the block of the per-block offsets, is the node's index in the node list.  World position of a node-local position p:
 *   terrain_origin + (o + p * s) * voxel_scale        (the ordinary extract's mapping for a block at cell origin o, p scaled by s).
 *
 * SELECTION, on the host, deterministic, in double arithmetic, no operation fused (no fma):
 *   c_k = ((double)viewer[k] - (double)terrain_origin[k]) / (double)voxel_scale                  the viewer in cells
 *   the roots are all nodes of level max_level, x fastest (o = 8 * 2^max_level * (rx, ry, rz), rx running first, then ry, then rz)
 *   a node of level L > 0 and size n = 8 * 2^L is replaced by its 8 children of level L - 1 when  d < (double)split * n,  where
 *     d = max over the axes of max(o_k - c_k, 0, c_k - (o_k + n)): the Chebyshev distance from c to the box [o, o + n], 0 inside;
 *   child k has origin o + (n / 2) * (k & 1, (k >> 1) & 1, (k >> 2) & 1) (bit 0 = x, bit 1 = y, bit 2 = z); children are visited in
 *   increasing k and tested by the same rule; the node list is the depth-first order of that descent.
 * The nodes tile the terrain's cells exactly once.  With split >= 1, nodes that share a face differ by at most one level: for boxes A
 * and P that touch, d(A) <= d(P) + size(P); a node A two or more levels above a face neighbour would have had to stay whole, d(A) >=
 * split * size(A), beside a box P of at most half its size (the neighbour's ancestor) that split, d(P) < split * size(A) / 2, which
 * needs split * size(A) / 2 < size(A) / 2, that is split < 1.  (The tests check the 2:1 property and do not assume it.)
 *
 * SEAMS BETWEEN LEVELS ARE NOT STITCHED.  Where a level-L node meets a level-(L+1) node the two meshes are built from different samples
 * and can differ on the shared face by up to the coarse cell's interpolation error: cracks are possible there.  No skirts are added and
 * no sample is snapped.  The 2:1 property above is what a later transition pass needs.  That holds for this call's own result, which stays
 * as it is; vtmc_lod_skirts (include/vtmc_lodskirt.h, an optional layer) covers the seams with skirt triangles built from this result on
 * the device, to be drawn beside it.
 *
 * vtmc_terrain_extract_lod  works in both output modes and leaves its result for vtmc_read_triangles, vtmc_read_indexed_mesh,
 *   vtmc_read_cases, vtmc_device_results, vtmc_device_indexed_results and vtmc_last_counts (n_blocks = the number of nodes) exactly as any
 *   extract does.  It changes nothing in the terrain: not the grid, the dirty list, the history or the event counter.  Its result is NOT a
 *   result of the dirty list: vtmc_material_vertices and vtmc_ao_vertices answer VTMC_ERR_NO_RESULT after it, until the next
 *   vtmc_terrain_update / _undo / _redo / _load.  Those two entry points keep refusing: per-vertex materials and occlusion of this result
 *   and of its skirts are vtmc_lod_material_vertices and vtmc_lod_ao_vertices (include/vtmc_lodattr.h, an optional layer with its own buffers).
 *   *n_nodes and *tri_count may be NULL.
 *   VTMC_ERR_NO_RESULT before vtmc_terrain_init.  VTMC_ERR_INVALID_ARG: params null; viewer or split not finite; split < 1; max_level
 *   outside 0..VTMC_LOD_MAX_LEVEL; max_nodes <= 0.  VTMC_ERR_DIMS: 8 * 2^max_level does not divide W, E and H.  VTMC_ERR_TOO_LARGE: the
 *   selection holds more than max_nodes nodes.  All of these leave the context as it was, the previous result included.
 * vtmc_terrain_lod_nodes  the node list of the result the context holds (dst = NULL: only *n_nodes).  VTMC_ERR_NO_RESULT when that result
 *   is not a level-of-detail extract's (none yet, or another extract since); VTMC_ERR_CAPACITY when capacity_nodes is too small.
 * ------------------------------------------------------------------------------------------ */
#define VTMC_LOD_MAX_LEVEL 7

typedef struct vtmc_lod_params {
    float viewer[3];     /* world space */
    float split;         /* >= 1: a node splits when the viewer is nearer than split * its size (in cells) */
    int32_t max_level;   /* 0..VTMC_LOD_MAX_LEVEL: the level of the roots */
    int32_t max_nodes;   /* > 0 */
} vtmc_lod_params;       /* 24 bytes */

typedef struct vtmc_lod_node {
    int32_t origin[3];   /* cells; multiples of 8 * 2^level */
    int32_t level;
} vtmc_lod_node;         /* 16 bytes */

int32_t vtmc_terrain_extract_lod(vtmc_ctx *ctx, const vtmc_lod_params *params, int32_t *n_nodes, int32_t *tri_count);
int32_t vtmc_terrain_lod_nodes(vtmc_ctx *ctx, vtmc_lod_node *dst, int32_t capacity_nodes, int32_t *n_nodes);

/* ------------------------------------------------------------------------------------------
 * Ray picking -- replaces the Physics.Raycast of the interactive edit (SceneManager.cs:114-131)
 * against the MeshColliders that BatchUpdate cooks from the extracted mesh (VoxelTerrain.cs:448-465),
 * without any mesh on the host.  The surface is the triangle set vtmc_extract_grid emits for every
 * block with emit_fast_math = 0 (positions bit for bit), a block-local vertex p of block b lying at
 * world origin + (8b + p) * voxel_scale.  A ray is (o, d) in world space, d of any non-zero length;
 * the nearest triangle with 0 <= distance <= max_distance along d/|d| is reported.  Faces are
 * single-sided as a MeshCollider's: a triangle counts when dot(d, cross(p1-p0, p2-p0)) < 0 (its normal
 * points from solid to air); VTMC_RAY_TWO_SIDED counts both sides.  Zero-area triangles are never hit.
 * A ray with a zero or non-finite direction or a non-finite origin is a miss.  max_distance may be
 * +inf; NaN or <= 0 is VTMC_ERR_INVALID_ARG.  Results are deterministic and do not depend on the
 * grid's strides.
 * ------------------------------------------------------------------------------------------ */
typedef struct vtmc_ray_hit {
    float distance;        /* world units along the normalised direction; -1: no hit */
    float point[3];        /* world */
    float normal[3];       /* unit face normal cross(p1-p0, p2-p0) of the hit triangle (world) */
    float barycentric[2];  /* (u, v): point = (1-u-v) p0 + u p1 + v p2 */
    int32_t block[3];      /* (bx, by, bz); -1 on a miss */
    int32_t cell;          /* x + 8y + 64z inside the block; -1 on a miss */
    int32_t triangle;      /* i of the case's triangle list, 0..4; -1: no hit */
} vtmc_ray_hit;            /* 56 bytes; (block, cell, triangle) names one triangle of the canonical order */

#define VTMC_RAY_TWO_SIDED 1u

/* Physics.Raycast against the terrain of vtmc_terrain_init / _update: host arrays (n_rays x 3 floats each),
 * synchronous, hits[n_rays].  VTMC_ERR_NO_RESULT before vtmc_terrain_init. */
int32_t vtmc_terrain_raycast(vtmc_ctx *ctx, const float *origins, const float *directions, int32_t n_rays,
                             float max_distance, uint32_t flags, vtmc_ray_hit *hits);

/* The same query on any device grid of (nx+2, ny+2, nz+2) samples (element strides as vtmc_extract_grid), device
 * rays and hits, queued on `stream` (NULL = the context's stream) without synchronising. */
int32_t vtmc_raycast_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z,
                            const float origin[3], float voxel_scale,
                            const float *d_origins, const float *d_directions, int32_t n_rays,
                            float max_distance, uint32_t flags, vtmc_ray_hit *d_hits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sphere casts and closest points -- the queries a moving body makes against the MeshColliders that
 * BatchUpdate cooks from the read-back mesh (VoxelTerrain.cs:168, 464): Physics.SphereCast, and
 * Physics.CheckSphere / Collider.ClosestPoint / Physics.ComputePenetration.  The surface is the ray
 * picking's: the triangles vtmc_extract_grid emits in exact mode, vertex p of block b at world
 * origin + (8b + p) * voxel_scale.  Zero-area triangles and cells with a NaN corner never count.  All
 * distances are world units.
 *
 * Sphere cast: a ball of radius r >= 0 centred at o, swept along d/|d|.  The answer is the smallest
 * t in [0, max_distance] at which the closed ball around o + t d/|d| meets a closed triangle; a
 * triangle the ball touches at the start gives t = 0.  The face rule is the raycast's, per triangle
 * and for face, edge and vertex contacts alike: a triangle counts when dot(d, cross(p1-p0, p2-p0)) < 0,
 * or always with VTMC_RAY_TWO_SIDED.  r = 0 is the ray of vtmc_terrain_raycast.
 *
 * Closest point: the point q of the surface nearest to a centre c among the triangles within r of it,
 * every triangle counting (no face rule); flags are reserved and must be 0.
 *
 * Ties (equal t, or equal distance) go to the smallest canonical index (block bx + nbx (by + nby bz),
 * cell x + 8y + 64z, triangle i): results depend neither on the grid's strides nor on the launch.
 * A query with a zero or non-finite direction, or a non-finite origin / centre, is a miss.
 * VTMC_ERR_INVALID_ARG: n < 0; a null pointer with n > 0; max_distance NaN or <= 0 (+inf allowed);
 * unknown flags; a host radius that is NaN, infinite, negative or above
 * VTMC_SPHERE_MAX_RADIUS_CELLS * voxel_scale (the error text names the query).  The _device calls do not
 * read their device radii on the host: there such a query is a miss.  n = 0 does nothing.
 * ------------------------------------------------------------------------------------------ */
typedef struct vtmc_sphere_hit {
    float distance;   /* sphere cast: centre travel along d/|d|; closest point: |c - q|; -1 = miss */
    float point[3];   /* contact / closest point on the surface (world) */
    float normal[3];  /* unit, from `point` towards the centre at contact; the triangle's unit face normal when that is 0 */
    int32_t block[3]; /* -1 on a miss */
    int32_t cell;     /* x + 8y + 64z; -1 on a miss */
    int32_t triangle; /* 0..4; -1 on a miss */
} vtmc_sphere_hit;    /* 48 bytes */

#define VTMC_SPHERE_MAX_RADIUS_CELLS 16   /* r / voxel_scale above this: VTMC_ERR_INVALID_ARG */

/* On the terrain of vtmc_terrain_init / _update: host arrays (origins, directions, centers: n x 3 floats;
 * radii: n floats), synchronous, hits[n].  VTMC_ERR_NO_RESULT before vtmc_terrain_init. */
int32_t vtmc_terrain_spherecast(vtmc_ctx *ctx, const float *origins, const float *directions, const float *radii,
                                int32_t n, float max_distance, uint32_t flags, vtmc_sphere_hit *hits);
int32_t vtmc_terrain_closest_point(vtmc_ctx *ctx, const float *centers, const float *radii, int32_t n, uint32_t flags,
                                   vtmc_sphere_hit *hits);

/* The same queries on any device grid (as vtmc_raycast_device), device arrays, queued on `stream`
 * (NULL = the context's stream) without synchronising. */
int32_t vtmc_spherecast_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz,
                               int64_t stride_x, int64_t stride_y, int64_t stride_z, const float origin[3], float voxel_scale,
                               const float *d_origins, const float *d_directions, const float *d_radii, int32_t n,
                               float max_distance, uint32_t flags, vtmc_sphere_hit *d_hits, void *stream);
int32_t vtmc_closest_point_device(vtmc_ctx *ctx, const float *d_grid, int32_t nx, int32_t ny, int32_t nz,
                                  int64_t stride_x, int64_t stride_y, int64_t stride_z, const float origin[3], float voxel_scale,
                                  const float *d_centers, const float *d_radii, int32_t n, uint32_t flags,
                                  vtmc_sphere_hit *d_hits, void *stream);

/* The same fill without the final synchronisation: queued on `stream` (NULL = the context's stream)
 * and ordered only by it, so a streaming driver can generate batch k+1 on one context / stream while
 * batch k is extracted on another (BASELINE config "2048^3 streaming grid, double-buffered chunks").
 * The origins are staged in context-owned device memory: issue fills of ONE context on one stream. */
int32_t vtmc_density_fill_device_async(vtmc_ctx *ctx, const vtmc_density_params *params,
                                       const int32_t *origins, int32_t n_volumes,
                                       int32_t dim_x, int32_t dim_y, int32_t dim_z,
                                       int64_t stride_x, int64_t stride_y, int64_t stride_z,
                                       int64_t volume_stride, float *d_out, void *stream);

/* Device time in milliseconds of the density kernel the last vtmc_density_fill_device[_async] queued
 * (HIP events on the stream it ran on; waits for that kernel only). */
int32_t vtmc_last_fill_ms(vtmc_ctx *ctx, float *ms);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: one context per GPU / process, chunk c -> rank c % world_size, and ONE collective --
 * an RCCL all-gather (over xGMI) of the per-chunk {vertices, triangles} pairs -- after which every
 * rank derives the global offsets with a local exclusive scan.  New in the build: the
 * reference is single-process / single-GPU; the call sits where BatchUpdate hands its results to the
 * host (VoxelTerrain.cs:426-446).  librccl is bound at run time on the first vtmc_comm_* call.
 * ------------------------------------------------------------------------------------------ */
#define VTMC_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

/* Rank 0 draws the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by the host's own
 * means (the C# host: its launcher's socket / file; bench.py: torch.distributed broadcast). */
int32_t vtmc_comm_unique_id(uint8_t id[VTMC_COMM_ID_BYTES]);

/* Collective over all ranks: creates this context's communicator on its device (ncclCommInitRank). */
int32_t vtmc_comm_init_rank(vtmc_ctx *ctx, const uint8_t id[VTMC_COMM_ID_BYTES], int32_t rank, int32_t world_size);
int32_t vtmc_comm_destroy(vtmc_ctx *ctx);

/* `ctx` uses the communicator of `owner` (same device, same process) for vtmc_allgather_volume_counts from now on: contexts that take
 * turns (a step in flight while the host takes the previous one) issue all their collectives through ONE communicator.  ORDER: the
 * collectives of a communicator -- its owner's and every borrower's -- form one chain kept by the owner: a collective queued on another
 * stream than the one before it first waits, on the device, for the previous one's event, so RCCL sees them one after the other, in host
 * call order, exactly as on one stream -- and that order must be the same on every rank.  ONE HOST THREAD drives all contexts that share a
 * communicator (the chain's state on the owner is updated by the borrowers without a lock); contexts with communicators of their own may
 * live on different threads.  `ctx` never destroys the communicator; `owner` must stay alive, and keep it, as long as `ctx` uses it
 * (vtmc_comm_destroy(ctx) or another vtmc_comm_* call on ctx ends the sharing; an owner that goes first detaches its borrowers). */
int32_t vtmc_comm_share(vtmc_ctx *ctx, vtmc_ctx *owner);

/* All-gather of volume_counts of the last extract_* on `stream` (NULL = the context's stream),
 * asynchronously: d_all_counts (device, world_size x volumes_per_rank x {vertices, triangles} u32)
 * receives rank r's pairs at [r * volumes_per_rank ...), zero-padded where a rank owns fewer volumes.
 * No host synchronisation: the caller orders later work on the same stream.
 * Queued behind vtmc_extract_volumes_device_async (before vtmc_extract_finish) whose chunks are whole
 * scan tiles (a multiple of 2048 blocks, e.g. 128^3 cells), the counts have already left the scan
 * kernel: the collective then runs on the context's second stream BESIDE the emit kernel (launched a
 * workgroup per XCD short for it) and `stream` merely waits for its end -- only with the tuning key "gather_beside" = 1
 * (default 0).  Otherwise, and by default, it runs on `stream`, behind the emit kernel. */
int32_t vtmc_allgather_volume_counts(vtmc_ctx *ctx, uint32_t *d_all_counts, int32_t volumes_per_rank, void *stream);

/* Blocking device -> host copy on `stream` (NULL = the context's stream) through the library's own
 * HIP runtime: for hosts that hold device pointers from vtmc_device_results and no HIP binding. */
int32_t vtmc_copy_to_host(vtmc_ctx *ctx, const void *d_src, void *dst, int64_t bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Persisted chunks (layout: volumetricterrain_amd/chunkfile.py -- 64-byte
 * header, then 16-byte aligned sections).  New in the build: the reference keeps its grid in memory
 * only (VoxelTerrain.cs:145-149).  The file image is assembled on the device.
 * ------------------------------------------------------------------------------------------ */
#define VTMC_CHUNK_SAMPLES 1u /* f32[(cells+2)^3], x fastest */
#define VTMC_CHUNK_SOUP 2u    /* 76-byte records, `block` relative to the chunk */
#define VTMC_CHUNK_INDEXED 4u /* vert_offsets, vertices, indices */

/* Writes volume `volume` of the last vtmc_extract_volumes_device / vtmc_extract_grid (its samples when
 * with_samples != 0 -- the input of that extract must still be resident --, its block offsets rebased to
 * 0 and its mesh in the output mode that extract ran in).  origin = global sample index of the chunk. */
int32_t vtmc_chunk_write(vtmc_ctx *ctx, const char *path, int32_t volume, const int32_t origin[3], int32_t with_samples);

typedef struct vtmc_chunk_view {
    int32_t origin[3];
    int32_t cells[3];
    uint32_t flags, n_blocks, n_triangles, n_vertices;
    const float *d_samples;            /* NULL when the section is absent; strides (1, cells[0]+2, (cells[0]+2)*(cells[1]+2)) */
    const uint32_t *d_tri_offsets;     /* n_blocks + 1 */
    const vtmc_triangle *d_triangles;
    const uint32_t *d_vert_offsets;
    const vtmc_vertex *d_vertices;
    const int32_t *d_indices;
} vtmc_chunk_view;

/* Uploads a chunk file as one image and returns DEVICE pointers to its sections (owned by the
 * context, valid until the next vtmc_chunk_read / vtmc_chunk_write / vtmc_destroy): d_samples can be
 * handed straight back to vtmc_extract_volumes_device. */
int32_t vtmc_chunk_read(vtmc_ctx *ctx, const char *path, vtmc_chunk_view *out);

/* Library / build identification: "vtmc <version> gfx950". */
const char *vtmc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VTMC_H */
