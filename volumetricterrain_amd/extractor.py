"""Extractor -- thin Python owner of one vtmc context (one per GPU / process).

Mirrors the call sequence of VoxelTerrain.BatchUpdate (VoxelTerrain.cs:365-427):
extract_* (upload + three dispatches + count read-back) then read_triangles (GetData).
numpy arrays stand in for the pinned C# arrays; nothing here computes -- every result
comes out of libvtmc.so.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import COMM_ID_BYTES, FRAGMENT_DTYPE, INSTANCE_DTYPE, LIGHT_SAMPLE_DTYPE, LIGHT_SOURCE_DTYPE, MATERIAL_CHANNELS, MESH_TRUST_CLOSED, NAV_SPAN_DTYPE, NAVCROWD_AGENT_DTYPE, NAVFIELD_CELL_DTYPE, NAVFIELD_GOAL_DTYPE, NAVSIGHT_HIT_DTYPE, RAY_HIT_DTYPE, RAY_TWO_SIDED, SPHERE_HIT_DTYPE, TRI_DTYPE, VERTEX_DTYPE, WATER_BODY_DTYPE, WATER_SOURCE_DTYPE, ChunkView, DensityParams, Modifier, VolumeBatch, VtmcError
from .modifiers import AmbientOcclusion, LodParams, LodSkirtParams, NavErodeParams, NavParams, ScatterParams, fragment_bounds, fragment_count, mesh_stamp_args


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _struct(x):
    """The ctypes struct of a mirror object of modifiers.py (anything with to_struct); a struct is passed through."""
    return x.to_struct() if hasattr(x, "to_struct") else x


def _struct_array(items, kind):
    """(a ctypes array of `kind` with the items' structs copied into it -- one element when there are none --, their number)"""
    structs = [_struct(x) for x in items]
    arr = (kind * max(len(structs), 1))()
    for i, s in enumerate(structs):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(s), ctypes.sizeof(kind))
    arr._structs = structs   # what a struct keeps alive (a path's segments) lives as long as the array
    return arr, len(structs)


def elem_strides(grid):
    if grid.dtype != np.float32 or grid.ndim != 3:
        raise ValueError("grid must be a 3-D float32 array indexed [x, y, z]")
    if any(s % 4 for s in grid.strides):
        raise ValueError("grid strides must be multiples of 4 bytes")
    return tuple(int(s) // 4 for s in grid.strides)


def nav_world_positions(spans, column_offsets, box_lo, dims, origin, scale):
    """World positions (float64, (n, 3)) of the spans of Extractor.terrain_nav: origin + (x, height, z) * scale, with (x, z) the grid
    column of each span, found from column_offsets (column c = ix + dx * iz of the box at box_lo with dims samples per axis)."""
    counts = np.diff(np.asarray(column_offsets, np.int64))
    col = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    dx = max(int(dims[0]), 1)
    g = np.stack([box_lo[0] + col % dx, np.asarray(spans["height"], np.float64), box_lo[2] + col // dx], axis=1)
    return np.asarray(origin, np.float64) + g * float(scale)


def density_params(kind, n, seed=1337):
    """perlin3d f = 8/N; fbm8 = 8 octaves, lacunarity 2, gain 0.5, f = 4/N, minus a ramp."""
    if kind == "perlin3d":
        return DensityParams(seed, 8.0 / n, 1, 2.0, 0.5, 0.0, 0.0)
    if kind == "fbm8":
        return DensityParams(seed, 4.0 / n, 8, 2.0, 0.5, 2.0 / n, n / 2.0)
    raise ValueError("unknown density kind %r" % (kind,))


class Extractor:
    def __init__(self, device=0, lib_path=None):
        self._L = _lib.load(lib_path)   # lib_path: another build of the library beside the product's (A/B tools)
        h = ctypes.c_void_p()
        rc = self._L.vtmc_create(device, ctypes.byref(h))
        if rc != 0:
            raise VtmcError(rc, self._L.vtmc_last_error(None).decode())
        self._h = h
        self.device = device

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise VtmcError(rc, self._L.vtmc_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.vtmc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host entry points (what the C# shim P/Invokes) --------------------------------------
    def extract_blocks(self, samples):
        """samples: (B, 1000) float32 tiles laid out as VoxelTerrain.cs:341-361.  Returns T."""
        samples = np.ascontiguousarray(samples, np.float32).reshape(-1, 1000)
        t = ctypes.c_int32()
        self._check(self._L.vtmc_extract_blocks(self._h, _ptr(samples), samples.shape[0], ctypes.byref(t)))
        return t.value

    def extract_grid(self, grid, block_list=None):
        """grid indexed [x, y, z], shape (nx+2, ny+2, nz+2), any positive strides.  Returns T."""
        sx, sy, sz = elem_strides(grid)
        nx, ny, nz = (d - 2 for d in grid.shape)
        n = 0
        if block_list is not None:
            block_list = np.ascontiguousarray(block_list, np.int32).reshape(-1, 3)
            n = len(block_list)
        t = ctypes.c_int32()
        self._check(self._L.vtmc_extract_grid(self._h, _ptr(grid), nx, ny, nz, sx, sy, sz,
                                              _ptr(block_list), n, ctypes.byref(t)))
        return t.value

    def extract_grid_sharded(self, grid, chunk_cells, rank, world_size):
        """Returns (T_local, chunk_counts[n_local, 2] = {vertices, triangles})."""
        sx, sy, sz = elem_strides(grid)
        nx, ny, nz = (d - 2 for d in grid.shape)
        n_chunks = max(1, (nx // chunk_cells) * (ny // chunk_cells) * (nz // chunk_cells)) if chunk_cells > 0 else 1
        counts = np.zeros((n_chunks, 2), np.uint32)
        n_local, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_extract_grid_sharded(self._h, _ptr(grid), nx, ny, nz, sx, sy, sz,
                                                      chunk_cells, rank, world_size, _ptr(counts),
                                                      n_chunks, ctypes.byref(n_local), ctypes.byref(t)))
        return t.value, counts[:n_local.value].copy()

    def last_counts(self):
        b, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_last_counts(self._h, ctypes.byref(b), ctypes.byref(t)))
        return b.value, t.value

    def read_triangles(self, with_offsets=True):
        n_blocks, n_tris = self.last_counts()
        tris = np.zeros(n_tris, TRI_DTYPE)
        offs = np.zeros(n_blocks + 1, np.int32) if with_offsets else None
        self._check(self._L.vtmc_read_triangles(self._h, _ptr(tris), n_tris, _ptr(offs)))
        return (tris, offs) if with_offsets else tris

    # -- indexed (welded) output ---------------------------------------------------------------
    def set_output_mode(self, indexed):
        """indexed=True: the following extract_* / terrain_update calls produce vtmc_vertex + index
        buffers (read_indexed_mesh) instead of 76-byte records (read_triangles)."""
        self._check(self._L.vtmc_set_output_mode(self._h, 1 if indexed else 0))

    def last_vertex_count(self):
        nv = ctypes.c_int32()
        self._check(self._L.vtmc_last_vertex_count(self._h, ctypes.byref(nv)))
        return nv.value

    def read_indexed_mesh(self):
        """(vertices[V], indices[T,3] block-local, block_vertex_offsets[B+1], block_tri_offsets[B+1])."""
        n_blocks, n_tris = self.last_counts()
        nv = ctypes.c_int32()
        self._check(self._L.vtmc_last_vertex_count(self._h, ctypes.byref(nv)))
        verts = np.zeros(nv.value, VERTEX_DTYPE)
        idx = np.zeros((n_tris, 3), np.int32)
        voffs, toffs = np.zeros(n_blocks + 1, np.int32), np.zeros(n_blocks + 1, np.int32)
        self._check(self._L.vtmc_read_indexed_mesh(self._h, _ptr(verts), nv.value, _ptr(idx), n_tris, _ptr(voffs), _ptr(toffs)))
        return verts, idx, voffs, toffs

    def device_indexed_results(self):
        a, b, c, d = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._L.vtmc_device_indexed_results(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return a.value, b.value, c.value, d.value

    def read_cases(self):
        n_blocks, _ = self.last_counts()
        cases = np.zeros((n_blocks, 512), np.uint8)
        self._check(self._L.vtmc_read_cases(self._h, _ptr(cases), cases.nbytes))
        return cases

    # -- device-resident entry points ---------------------------------------------------------
    def extract_volumes_device(self, d_ptr, n, strides, n_volumes=1, volume_stride=0, stream=None, flags=0):
        """d_ptr: device address (int) of the first sample; n = (nx, ny, nz) cells per volume;
        strides = element strides (sx, sy, sz).  Returns T."""
        vb = VolumeBatch(d_ptr, n[0], n[1], n[2], strides[0], strides[1], strides[2], n_volumes, volume_stride)
        t = ctypes.c_int64()
        self._check(self._L.vtmc_extract_volumes_device(self._h, ctypes.byref(vb), stream, flags, ctypes.byref(t)))
        return t.value

    def extract_volumes_device_async(self, d_ptr, n, strides, n_volumes=1, volume_stride=0, stream=None, flags=0):
        """Queues the extract on `stream` and returns at once; extract_finish() completes it."""
        vb = VolumeBatch(d_ptr, n[0], n[1], n[2], strides[0], strides[1], strides[2], n_volumes, volume_stride)
        self._check(self._L.vtmc_extract_volumes_device_async(self._h, ctypes.byref(vb), stream, flags))

    def extract_finish(self):
        t = ctypes.c_int64()
        self._check(self._L.vtmc_extract_finish(self._h, ctypes.byref(t)))
        return t.value

    def device_results(self):
        """(triangles, block_tri_offsets, volume_counts) device addresses of the last extract."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._L.vtmc_device_results(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def copy_volume_counts_device(self, d_dst, capacity_volumes, stream=None):
        """Per-volume {vertices, triangles} of the last extract into a caller-owned device buffer
        (async on `stream`): what the multi-GPU driver all-gathers."""
        self._check(self._L.vtmc_copy_volume_counts_device(self._h, d_dst, capacity_volumes, stream))

    def copy_to_host(self, d_ptr, nbytes, stream=None):
        """Blocking device -> host copy through the library's own HIP runtime (vtmc_copy_to_host)."""
        out = np.empty(int(nbytes), np.uint8)
        self._check(self._L.vtmc_copy_to_host(self._h, d_ptr, _ptr(out), int(nbytes), stream))
        return out

    def copy_into_host(self, d_ptr, host_ptr, nbytes, stream=None):
        """The same copy into memory the caller owns (an address, e.g. of pinned words): nothing is allocated per call."""
        self._check(self._L.vtmc_copy_to_host(self._h, d_ptr, ctypes.c_void_p(host_ptr), int(nbytes), stream))

    def copy_u32(self, d_ptr, count, stream=None):
        return self.copy_to_host(d_ptr, 4 * int(count), stream).view(np.uint32)

    # -- multi-GPU: the RCCL all-gather of per-chunk counts behind the C ABI ---------------------
    def comm_unique_id(self):
        """128 opaque bytes drawn by rank 0 (ncclGetUniqueId); the caller distributes them."""
        buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
        rc = self._L.vtmc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p))
        if rc != 0:
            raise VtmcError(rc, self._L.vtmc_last_error(None).decode())
        return bytes(buf)

    def comm_init_rank(self, unique_id, rank, world_size):
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self._L.vtmc_comm_init_rank(self._h, ctypes.cast(buf, ctypes.c_void_p), rank, world_size))

    def comm_destroy(self):
        self._check(self._L.vtmc_comm_destroy(self._h))

    def comm_share(self, owner):
        """This context issues its all-gathers through `owner`'s communicator (two contexts taking turns on one stream)."""
        self._check(self._L.vtmc_comm_share(self._h, owner._h))

    def allgather_volume_counts(self, d_all_counts, volumes_per_rank, stream=None):
        """Queues the all-gather of the last extract's per-volume {vertices, triangles} on `stream`:
        d_all_counts (device, world x volumes_per_rank x 2 u32).  Asynchronous."""
        self._check(self._L.vtmc_allgather_volume_counts(self._h, d_all_counts, volumes_per_rank, stream))

    # -- persisted chunks (device-side packer / loader) -------------------------------------------
    def chunk_write(self, path, volume, origin, with_samples=True):
        o = (ctypes.c_int32 * 3)(*[int(v) for v in origin])
        self._check(self._L.vtmc_chunk_write(self._h, str(path).encode(), volume, ctypes.byref(o), 1 if with_samples else 0))

    def chunk_read(self, path):
        """Uploads a chunk file; returns the ChunkView of device pointers (valid until the next chunk_* call)."""
        v = ChunkView()
        self._check(self._L.vtmc_chunk_read(self._h, str(path).encode(), ctypes.byref(v)))
        return v

    def reserve_triangles(self, capacity):
        self._check(self._L.vtmc_reserve_triangles(self._h, int(capacity)))

    def stream_handle(self, own_queue=True):
        """A hipStream_t of the context as an integer.  own_queue=True: the stream on a hardware queue of its own (two contexts, two steps in
        flight, steps that overlap); False: the context's own stream (what stream = None means).  Wrap it with torch.cuda.ExternalStream to
        queue torch work behind a step -- and release every torch object that touched it (events, pinned tensors copied on it: PyTorch
        records an event on the stream when it FREES such a tensor) before the context is closed: the stream dies with it."""
        h = ctypes.c_void_p()
        self._check(self._L.vtmc_context_stream(self._h, 1 if own_queue else 0, ctypes.byref(h)))
        return h.value or 0

    def last_stage_ms(self):
        ms = (ctypes.c_float * 4)()
        self._check(self._L.vtmc_last_stage_ms(self._h, ctypes.byref(ms)))
        return {"classify": ms[0], "scan": ms[1], "emit": ms[2], "total": ms[3]}

    def last_placement(self):
        """The last output-placement trial (tuning key place_outputs): ([emit ms per candidate], index kept); ([], 0) when none has run."""
        ms, n, kept = (ctypes.c_float * 16)(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_last_placement(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(kept)))
        return [round(float(ms[i]), 4) for i in range(n.value)], kept.value

    def last_fill_ms(self):
        ms = ctypes.c_float()
        self._check(self._L.vtmc_last_fill_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def set_tuning(self, **kv):
        for k, v in kv.items():
            self._check(self._L.vtmc_set_tuning(self._h, k.encode(), int(v)))

    # -- device-resident terrain: VoxelTerrain.Init / Update on the GPU ------------------------
    def terrain_init(self, width, elevation, height, voxel_scale=1.0, origin=(0.0, 0.0, 0.0), seed=1):
        """VoxelTerrain.Init's grid (VoxelTerrain.cs:121-149) in HBM."""
        o = (ctypes.c_float * 3)(*origin)
        self._check(self._L.vtmc_terrain_init(self._h, width, elevation, height, voxel_scale, ctypes.byref(o), seed))
        self._terrain_dims = (width, elevation, height)
        self._terrain_placement = (tuple(float(np.float32(v)) for v in origin), float(np.float32(voxel_scale)))   # for lod_world_positions

    def terrain_update(self, mods):
        """VoxelTerrain.Update (VoxelTerrain.cs:262-325) for a queue of Modifier structs.
        Returns (number of dirty blocks, T)."""
        nd, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_update(self._h, *_struct_array(mods, Modifier), ctypes.byref(nd), ctypes.byref(t)))
        return nd.value, t.value

    def terrain_set_history(self, max_bytes):
        """Undo / redo of terrain_update calls in a device journal of max_bytes (0: history off, the default)."""
        self._check(self._L.vtmc_terrain_set_history(self._h, int(max_bytes)))

    def terrain_undo(self):
        """Takes the newest recorded terrain_update back and extracts its dirty blocks.  Returns (number of dirty blocks, T);
        VtmcError ERR_NO_RESULT when there is nothing to undo."""
        nd, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_undo(self._h, ctypes.byref(nd), ctypes.byref(t)))
        return nd.value, t.value

    def terrain_redo(self):
        """Re-applies the newest undone step, as terrain_undo.  Returns (number of dirty blocks, T)."""
        nd, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_redo(self._h, ctypes.byref(nd), ctypes.byref(t)))
        return nd.value, t.value

    def terrain_history(self):
        """(steps that can be undone, steps that can be redone, journal bytes they hold)."""
        nu, nr, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self._L.vtmc_terrain_history(self._h, ctypes.byref(nu), ctypes.byref(nr), ctypes.byref(b)))
        return nu.value, nr.value, b.value

    def terrain_dirty_blocks(self):
        n = ctypes.c_int32()
        self._check(self._L.vtmc_terrain_dirty_blocks(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 3), np.int32)
        self._check(self._L.vtmc_terrain_dirty_blocks(self._h, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def terrain_read_samples(self, order="x"):
        """The density grid indexed [x, y, z]; order='x': x fastest in memory, 'z': a C# float[,,]."""
        w, e, h = self._terrain_dims
        if order == "x":
            mem = np.empty((h + 2, e + 2, w + 2), np.float32)
            grid = mem.transpose(2, 1, 0)
        else:
            grid = np.empty((w + 2, e + 2, h + 2), np.float32)
        sx, sy, sz = elem_strides(grid)
        self._check(self._L.vtmc_terrain_read_samples(self._h, _ptr(grid), sx, sy, sz))
        return grid

    # -- saving a session: the resident terrain as a sparse brick file (terrainfile.py) ---------------------------
    def terrain_save(self, path, exact=False):
        """Writes the resident terrain to `path` (classified, compacted and packed on the device); exact=True stores every brick raw.
        Changes nothing in the context.  Returns the file's size in bytes."""
        n = ctypes.c_int64()
        self._check(self._L.vtmc_terrain_save(self._h, str(path).encode(), _lib.TERRAIN_SAVE_EXACT if exact else 0, ctypes.byref(n)))
        return n.value

    def terrain_load(self, path, extract=True):
        """(Re)initialises the terrain from a file of terrain_save / terrainfile.write_terrain, with or without an earlier terrain_init,
        and extracts every block unless extract=False.  Returns (number of dirty blocks, T)."""
        nd, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_load(self._h, str(path).encode(), 0 if extract else _lib.TERRAIN_LOAD_NO_EXTRACT,
                                              ctypes.byref(nd), ctypes.byref(t)))
        dims = (ctypes.c_int32 * 3)()
        self._check(self._L.vtmc_terrain_device_grid(self._h, None, None, ctypes.byref(dims)))
        self._terrain_dims = tuple(d - 2 for d in dims)   # for terrain_read_samples
        from .terrainfile import read_header
        meta = read_header(path)
        self._terrain_placement = (tuple(float(v) for v in meta["origin"]), float(meta["scale"]))   # for lod_world_positions
        return nd.value, t.value

    def terrain_write_samples(self, grid):
        """The inverse of terrain_read_samples: grid indexed [x, y, z], shape (W+2, E+2, H+2), any positive strides.  Clears the history,
        extracts nothing."""
        if tuple(grid.shape) != tuple(d + 2 for d in self._terrain_dims):
            raise ValueError("grid shape %r does not match the terrain's samples" % (tuple(grid.shape),))
        sx, sy, sz = elem_strides(grid)
        self._check(self._L.vtmc_terrain_write_samples(self._h, _ptr(grid), sx, sy, sz))

    # -- stamps: density volumes the context keeps in HBM for StampModifier to paste ---------------------------------
    def stamp_create(self, samples):
        """A stamp from host samples: a float32 array indexed [x, y, z] (any positive strides), every sample finite.  Returns its id."""
        samples = np.asarray(samples)
        sx, sy, sz = elem_strides(samples)
        if min(sx, sy, sz) <= 0:
            raise ValueError("stamp strides must be positive")
        sid = ctypes.c_int32()
        self._check(self._L.vtmc_stamp_create(self._h, _ptr(samples), *samples.shape, sx, sy, sz, ctypes.byref(sid)))
        return sid.value

    def stamp_capture(self, first, dims):
        """A stamp copied on the device from the resident grid: the samples [first, first + dims) per axis.  Returns its id."""
        f = (ctypes.c_int32 * 3)(*(int(v) for v in first))
        sid = ctypes.c_int32()
        self._check(self._L.vtmc_stamp_capture(self._h, ctypes.byref(f), *(int(n) for n in dims), ctypes.byref(sid)))
        return sid.value

    def stamp_from_mesh(self, vertices, triangles, first, pitch, dims, trust_closed=False):
        """A stamp voxelized on the device from a closed triangle mesh: vertices (n, 3), triangles (m, 3) vertex numbers; sample (i, j, k)
        lies at first + pitch * (i, j, k) (modifiers.mesh_stamp_box gives first and dims for a mesh).  The values are the signed distance
        to the surface in stamp samples, positive inside, clamped to +-MESH_BAND.  trust_closed skips the closed-mesh check.  Returns its id."""
        v, t, f, h, dims = mesh_stamp_args(vertices, triangles, first, pitch, dims)
        sid = ctypes.c_int32()
        self._check(self._L.vtmc_stamp_from_mesh(self._h, _ptr(v), len(v), _ptr(t), len(t), ctypes.byref((ctypes.c_float * 3)(*f)), float(h), *dims,
                                                 MESH_TRUST_CLOSED if trust_closed else 0, ctypes.byref(sid)))
        return sid.value

    def stamp_dims(self, stamp_id):
        d = (ctypes.c_int32 * 3)()
        self._check(self._L.vtmc_stamp_info(self._h, int(stamp_id), ctypes.byref(d)))
        return tuple(d)

    def stamp_read(self, stamp_id):
        """The stamp's samples indexed [x, y, z] (x fastest in memory): what a host stores to keep a stamp."""
        nx, ny, nz = self.stamp_dims(stamp_id)
        out = np.empty((nz, ny, nx), np.float32).transpose(2, 1, 0)
        sx, sy, sz = elem_strides(out)
        self._check(self._L.vtmc_stamp_read(self._h, int(stamp_id), _ptr(out), sx, sy, sz))
        return out

    def stamp_destroy(self, stamp_id):
        self._check(self._L.vtmc_stamp_destroy(self._h, int(stamp_id)))

    # -- fragments: what no longer hangs on anything, listed (and captured as stamps) without touching the terrain --------
    def terrain_fragments(self, lower=None, upper=None, max_samples=0, capture_min_samples=0):
        """The floating fragments of the box lower..upper (world bounds; None: the whole terrain) that DetachModifier with the same bounds
        and max_samples would remove now: a FRAGMENT_DTYPE array in increasing grid index of the seed.  capture_min_samples > 0: every
        fragment of at least that many samples also becomes a stamp (its id in stamp_id; its place: fragment_stamp_box).  Changes nothing
        in the terrain."""
        lo, up = fragment_bounds(lower, upper)
        most, least = fragment_count(max_samples, "max_samples"), fragment_count(capture_min_samples, "capture_min_samples")
        lo_c, up_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*up)
        n = ctypes.c_int32()
        self._check(self._L.vtmc_terrain_fragments(self._h, ctypes.byref(lo_c), ctypes.byref(up_c), most, 0, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, FRAGMENT_DTYPE)
        if n.value:
            self._check(self._L.vtmc_terrain_fragments(self._h, ctypes.byref(lo_c), ctypes.byref(up_c), most, least, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def terrain_sample_box(self, lower=None, upper=None):
        """The clamped sample box of world bounds, (first sample, samples per axis), as the library finds it for a modifier or a fragment
        query: floor / ceil of (bound - origin) / scale in float32, clamped to the grid; an axis of 0 samples: empty."""
        lo, up = fragment_bounds(lower, upper)
        origin, scale = self._terrain_placement
        first, dims = [], []
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(3):
                top = self._terrain_dims[k] + 1
                a = float(np.floor((lo[k] - np.float32(origin[k])) / np.float32(scale)))
                b = float(np.ceil((up[k] - np.float32(origin[k])) / np.float32(scale)))
                a, b = int(max(min(a, 2.0 ** 31 - 1), 0.0)), int(min(max(b, -2.0 ** 31), float(top)))
                first.append(a)
                dims.append(max(0, b - a + 1) if a <= top else 0)
        return tuple(first), tuple(dims)

    def fragment_stamp_box(self, fragment, lower=None, upper=None):
        """(first sample, dims) of the stamp a fragment record of terrain_fragments(lower, upper, ...) was captured into: its bounds grown
        by 2 samples, cut to the query box.  StampModifier(stamp_id, dims, world centre of that box, mode="replace") pastes it back."""
        first, dims = self.terrain_sample_box(lower, upper)
        a = [max(int(fragment["lo"][k]) - 2, first[k]) for k in range(3)]
        b = [min(int(fragment["hi"][k]) + 2, first[k] + dims[k] - 1) for k in range(3)]
        return tuple(a), tuple(b[k] - a[k] + 1 for k in range(3))

    # -- navigation: walkable spans, links and regions of a box of the resident terrain (include/vtmc_nav.h) ----------
    def terrain_nav(self, lower=None, upper=None, params=None):
        """Builds the navigation layer of the box lower..upper (world bounds; None: the whole terrain) for a NavParams (world units; or a
        vtmc_nav_params struct, in samples and grid units).  Returns (spans, column_offsets, box_lo, box_dims): a NAV_SPAN_DTYPE array
        ordered by column (ix + dx * iz) and bottom-up inside a column, the dx * dz + 1 span offsets of the columns, and the box's first
        grid sample and samples per axis ((0, 0, 0) samples for an empty box).  Changes nothing in the terrain; the result is a snapshot."""
        lo, up = fragment_bounds(lower, upper)
        if params is None:
            raise ValueError("terrain_nav needs a NavParams")
        p = params.to_struct(self._terrain_placement[1]) if isinstance(params, NavParams) else _struct(params)
        lo_c, up_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*up)
        n = ctypes.c_int32()
        self._check(self._L.vtmc_terrain_nav_build(self._h, ctypes.byref(lo_c), ctypes.byref(up_c), ctypes.byref(p), ctypes.byref(n)))
        return self.nav_read()

    def nav_read(self):
        """(spans, column_offsets, box_lo, box_dims) of the navigation build the context holds."""
        first, dims, n = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32()
        self._check(self._L.vtmc_nav_info(self._h, ctypes.byref(first), ctypes.byref(dims), ctypes.byref(n)))
        spans = np.zeros(n.value, NAV_SPAN_DTYPE)
        offsets = np.zeros(dims[0] * dims[2] + 1, np.int32)
        self._check(self._L.vtmc_nav_read(self._h, _ptr(spans), n.value, _ptr(offsets)))
        return spans, offsets, tuple(first), tuple(dims)

    def device_nav(self):
        """(device address of the spans, device address of the dx * dz + 1 column offsets, the number of spans) of the last terrain_nav;
        valid until the next one, terrain_init, terrain_load or close."""
        p, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        self._check(self._L.vtmc_nav_device_results(self._h, ctypes.byref(p), ctypes.byref(o), ctypes.byref(n)))
        return p.value, o.value, n.value

    # -- flow fields on the navigation build the context holds (include/vtmc_navfield.h) ------------------------------
    def nav_locate(self, positions, below, above):
        """The span each world position (n, 3) stands on, or -1: the nearest span of its column within `below` under and `above` over it
        (world units, divided by the voxel scale in float32)."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        scale = np.float32(self._terrain_placement[1])
        out = np.full(len(p), -1, np.int32)
        self._check(self._L.vtmc_nav_locate(self._h, _ptr(p), len(p), float(np.float32(below) / scale), float(np.float32(above) / scale), _ptr(out)))
        return out

    def nav_field(self, goals, params):
        """Builds the flow field of the goals on the nav result held: `goals` is an int array of spans (cost 0), (span, cost) pairs or a
        NAVFIELD_GOAL_DTYPE array; `params` a NavFieldParams (or a vtmc_navfield_params struct).  Returns the cells (NAVFIELD_CELL_DTYPE,
        one per span: cost, or NAVFIELD_UNREACHED, and the span to step to next, or -1)."""
        g = np.asarray(goals)
        if g.dtype != NAVFIELD_GOAL_DTYPE:
            pairs = np.asarray(goals, np.int64)
            if pairs.ndim == 1:
                pairs = np.stack([pairs, np.zeros_like(pairs)], axis=1)
            if pairs.ndim != 2 or pairs.shape[1] != 2 or (pairs[:, 1] < 0).any() or (pairs[:, 1] > 0xffffffff).any() or (abs(pairs[:, 0]) >= 2 ** 31).any():
                raise ValueError("goals must be spans, (span, cost) pairs or a NAVFIELD_GOAL_DTYPE array")
            g = np.zeros(len(pairs), NAVFIELD_GOAL_DTYPE)
            g["span"], g["cost"] = pairs[:, 0], pairs[:, 1]
        g = np.ascontiguousarray(g)
        p, n = _struct(params), ctypes.c_int32()
        self._check(self._L.vtmc_navfield_build(self._h, _ptr(g), len(g), ctypes.byref(p), ctypes.byref(n)))
        return self.navfield_read()

    def navfield_info(self):
        """(spans, reached spans, relaxation rounds) of the flow field the context holds."""
        n, r, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_navfield_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(k)))
        return n.value, r.value, k.value

    def navfield_read(self):
        """The cells of the flow field the context holds."""
        cells = np.zeros(self.navfield_info()[0], NAVFIELD_CELL_DTYPE)
        self._check(self._L.vtmc_navfield_read(self._h, _ptr(cells), len(cells)))
        return cells

    def device_navfield(self):
        """(device address of the cells, the number of spans) of the last nav_field; valid until the next one, the next terrain_nav,
        terrain_init, terrain_load or close."""
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        self._check(self._L.vtmc_navfield_device_results(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def nav_trace(self, starts, max_len):
        """(paths, lengths): for every start (a span, or -1) the spans that following `next` visits, at most max_len of them, in a row of
        paths (len(starts), max_len) padded with -1, and the number of them."""
        s = np.ascontiguousarray(starts, np.int32).reshape(-1)
        paths, lengths = np.full((len(s), max(int(max_len), 0)), -1, np.int32), np.zeros(len(s), np.int32)
        self._check(self._L.vtmc_navfield_trace(self._h, _ptr(s), len(s), int(max_len), _ptr(paths), _ptr(lengths)))
        return paths, lengths

    # -- an agent radius on the navigation build the context holds (include/vtmc_naverode.h) --------------------------
    def _naverode_struct(self, params):
        return params.to_struct(self._terrain_placement[1]) if isinstance(params, NavErodeParams) else _struct(params)

    def nav_distance(self, params):
        """Every span's distance to the nearest border of the nav result held, in half columns and capped at 2 * radius, for a
        NavErodeParams (world units; or a vtmc_naverode_params struct, in columns).  Returns an int32 array indexed as the spans are; the
        border spans are those at 0 (with a radius above 0).  The nav result and the flow field stay."""
        p, n = self._naverode_struct(params), ctypes.c_int32()
        self._check(self._L.vtmc_nav_distance_build(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self.nav_distance_read()

    def nav_distance_read(self):
        """The distances of the last nav_distance."""
        _, n = self.device_nav_distance()
        dist = np.zeros(n, np.int32)
        self._check(self._L.vtmc_nav_distance_read(self._h, _ptr(dist), n))
        return dist

    def device_nav_distance(self):
        """(device address of the int32 distances, the number of spans) of the last nav_distance; valid until the next one, the next
        nav_erode or terrain_nav, terrain_init, terrain_load or close."""
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        self._check(self._L.vtmc_nav_distance_device_results(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def nav_erode(self, params):
        """Replaces the nav result held by the spans an agent of the radius of a NavErodeParams (or a vtmc_naverode_params struct) can
        occupy.  Returns nav_read() + (origin,): origin[new] is the span's index before the call.  Drops the flow field and the distances;
        the addresses of device_nav change."""
        p, n = self._naverode_struct(params), ctypes.c_int32()
        self._check(self._L.vtmc_nav_erode(self._h, ctypes.byref(p), ctypes.byref(n)))
        return self.nav_read() + (self.nav_erode_origin(),)

    def nav_erode_origin(self):
        """origin of the last nav_erode: per span of the nav result held, its index in the result that was eroded."""
        n = ctypes.c_int32()
        self._check(self._L.vtmc_nav_info(self._h, None, None, ctypes.byref(n)))
        origin = np.zeros(n.value, np.int32)
        self._check(self._L.vtmc_nav_erode_origin(self._h, _ptr(origin), n.value))
        return origin

    # -- any-angle paths on the navigation build and the flow field the context holds (include/vtmc_navsight.h) -------
    def nav_sight(self, from_spans, to_spans):
        """The line-of-sight walk of every pair over the spans of the nav result held: a NAVSIGHT_HIT_DTYPE array, `last` the span the
        walk from from_spans[i] towards to_spans[i] ended on and `steps` the links it followed; the pair is visible iff last == to.  A pair
        with a -1 gives (-1, 0).  Links are followed forwards: visibility is not symmetric."""
        a, b = np.ascontiguousarray(from_spans, np.int32).reshape(-1), np.ascontiguousarray(to_spans, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("nav_sight needs as many from as to spans")
        hits = np.zeros(len(a), NAVSIGHT_HIT_DTYPE)
        self._check(self._L.vtmc_nav_sight(self._h, _ptr(a), _ptr(b), len(a), _ptr(hits)))
        return hits

    def nav_trace_smooth(self, starts, max_len, params):
        """(paths, lengths) as nav_trace gives them, of the waypoints only: of the spans that following `next` visits, those between which
        the line-of-sight walk succeeds, for a NavSightParams (or a vtmc_navsight_params struct).  A row ends on the span nav_trace's ends
        on unless it was cut at max_len."""
        s = np.ascontiguousarray(starts, np.int32).reshape(-1)
        p = _struct(params)
        paths, lengths = np.full((len(s), max(int(max_len), 0)), -1, np.int32), np.zeros(len(s), np.int32)
        self._check(self._L.vtmc_navfield_trace_smooth(self._h, _ptr(s), len(s), int(max_len), ctypes.byref(p), _ptr(paths), _ptr(lengths)))
        return paths, lengths

    # -- a crowd stepped along the flow field the context holds (include/vtmc_navcrowd.h) -----------------------------
    def navcrowd_spawn(self, spans, speeds):
        """Replaces the crowd: agent i asks for spans[i] (a span of the nav result held, or -1) and earns speeds[i] (one value for all, or
        one per agent) cost units per tick.  Where several ask for one span the smallest index stands on it; the others, and the -1s, are
        UNPLACED.  Returns the number of placed agents."""
        s = np.ascontiguousarray(spans, np.int32).reshape(-1)
        v = np.asarray(speeds, np.int64)
        if v.ndim == 0:
            v = np.full(len(s), int(v), np.int64)
        if v.shape != s.shape or (v < 0).any() or (v > 0xffffffff).any():
            raise ValueError("navcrowd_spawn needs one speed, or as many as spans, in 0..2^32-1")
        v, n = np.ascontiguousarray(v, np.uint32), ctypes.c_int32()
        self._check(self._L.vtmc_navcrowd_spawn(self._h, _ptr(s), _ptr(v), len(s), ctypes.byref(n)))
        return n.value

    def navcrowd_step(self, params, n_ticks=1):
        """n_ticks ticks of the crowd along the flow field held, for a NavCrowdParams (or a vtmc_navcrowd_params struct); nothing is copied
        back.  Returns navcrowd_info()."""
        p = _struct(params)
        self._check(self._L.vtmc_navcrowd_step(self._h, ctypes.byref(p), int(n_ticks)))
        return self.navcrowd_info()

    def navcrowd_info(self):
        """(agents, occupying agents, arrived agents: ARRIVED plus GONE, ticks since the spawn, moves of the last tick) of the crowd."""
        v = [ctypes.c_int32() for _ in range(5)]
        self._check(self._L.vtmc_navcrowd_info(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def navcrowd_read(self, occupancy=True):
        """(agents, occupancy): the records (NAVCROWD_AGENT_DTYPE: span, budget, speed, state) and, per span of the nav result, the index
        of the agent that occupies it or -1 (None when not asked for)."""
        agents = np.zeros(self.navcrowd_info()[0], NAVCROWD_AGENT_DTYPE)
        occ = None
        if occupancy:
            n = ctypes.c_int32()
            self._check(self._L.vtmc_nav_info(self._h, None, None, ctypes.byref(n)))
            occ = np.zeros(n.value, np.int32)
        self._check(self._L.vtmc_navcrowd_read(self._h, _ptr(agents), len(agents), _ptr(occ)))
        return agents, occ

    def device_navcrowd(self):
        """(device address of the agent records, device address of the occupancy words, the number of agents) of the crowd; valid until the
        next navcrowd_spawn, terrain_nav, nav_erode, terrain_init, terrain_load or close."""
        a, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
        self._check(self._L.vtmc_navcrowd_device_results(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.byref(n)))
        return a.value, o.value, n.value

    # -- standing water: flood a box of the resident terrain from sources to their levels (include/vtmc_water.h) --------
    def terrain_flood(self, sources, lower=None, upper=None):
        """Floods the box lower..upper (world bounds; None: the whole terrain) by the rule WATER.  `sources`: a WATER_SOURCE_DTYPE array or
        rows of (x, y, z, level) in world space.  Returns (source_body, n_bodies): per source its body index or -1 (dry).  Changes nothing
        in the terrain; the result is a snapshot, read with water_info / water_bodies / water_read / water_probe / water_extract."""
        lo, up = fragment_bounds(lower, upper)
        src = np.asarray(sources)
        if src.dtype != WATER_SOURCE_DTYPE:
            rows = np.asarray(sources, np.float32).reshape(-1, 4)
            src = np.zeros(len(rows), WATER_SOURCE_DTYPE)
            src["position"], src["level"] = rows[:, :3], rows[:, 3]
        src = np.ascontiguousarray(src)
        lo_c, up_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*up)
        out, n = np.full(len(src), -1, np.int32), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_flood(self._h, ctypes.byref(lo_c), ctypes.byref(up_c), _ptr(src) if len(src) else None, len(src), 0,
                                               _ptr(out) if len(src) else None, ctypes.byref(n)))
        return out, n.value

    def water_info(self):
        """(box_lo, box_dims, volume_dims, n_bodies, n_wet) of the flood the context holds."""
        lo, d, vd, n, wet = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self._L.vtmc_water_info(self._h, ctypes.byref(lo), ctypes.byref(d), ctypes.byref(vd), ctypes.byref(n), ctypes.byref(wet)))
        return tuple(lo), tuple(d), tuple(vd), n.value, wet.value

    def water_bodies(self):
        """The body records (WATER_BODY_DTYPE) in the rule's order: descending level, then ascending grid index of the seed."""
        out = np.zeros(self.water_info()[3], WATER_BODY_DTYPE)
        self._check(self._L.vtmc_water_bodies(self._h, _ptr(out), len(out)))
        return out

    def water_read(self, water=True, bodies=True):
        """(water volume float32, body volume int32), each indexed [x, y, z] with the volume dims (x fastest in memory), or None when not
        asked for: volume sample (ix, iy, iz) is box sample (ix, iy, iz), the padding is dry."""
        vd = self.water_info()[2]
        shape = (vd[2], vd[1], vd[0])
        w = np.empty(shape, np.float32) if water else None
        b = np.empty(shape, np.int32) if bodies else None
        self._check(self._L.vtmc_water_read(self._h, _ptr(w), _ptr(b), vd[0] * vd[1] * vd[2]))
        return (w.transpose(2, 1, 0) if water else None), (b.transpose(2, 1, 0) if bodies else None)

    def device_water(self):
        """(device address of the water volume, device address of the body volume, volume dims) of the flood; valid until the next
        terrain_flood, terrain_init, terrain_load or close."""
        w, b, vd = ctypes.c_void_p(), ctypes.c_void_p(), (ctypes.c_int32 * 3)()
        self._check(self._L.vtmc_water_device_results(self._h, ctypes.byref(w), ctypes.byref(b), ctypes.byref(vd)))
        return w.value, b.value, tuple(vd)

    def water_probe(self, positions):
        """(body, depth) of world positions (n, 3): the body of the nearest sample when it is wet and the depth level - y under its level;
        -1 and 0 otherwise.  What a swimmer or a buoyant body asks."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        body, depth = np.full(len(p), -1, np.int32), np.zeros(len(p), np.float32)
        self._check(self._L.vtmc_water_probe(self._h, _ptr(p) if len(p) else None, len(p), _ptr(body), _ptr(depth)))
        return body, depth

    def water_extract(self):
        """The water's surface: the water volume, as it lies on the device, through extract_volumes_device as a batch of one.  Returns T.
        This REPLACES the context's extract result, as any extract does (read_triangles gives the water's records; water_world_positions
        places them); 0 without a launch for an empty box."""
        w, _, vd = self.device_water()
        if not w:
            return 0
        return self.extract_volumes_device(w, tuple(d - 2 for d in vd), (1, vd[0], vd[0] * vd[1]))

    def water_world_positions(self, block, local_positions):
        """World positions (float64) of block-local positions of a water_extract mesh: terrain origin + (box_lo + 8b + p) * voxel scale,
        with b the block coordinates of `block` in the volume.  block: (n,); local_positions: (n, 3) or (n, m, 3)."""
        lo, _, vd, _, _ = self.water_info()
        nbx, nby = max((vd[0] - 2) // 8, 1), max((vd[1] - 2) // 8, 1)
        block = np.asarray(block, np.int64)
        b = np.stack([block % nbx, block // nbx % nby, block // (nbx * nby)], axis=-1).astype(np.float64)
        p = np.asarray(local_positions, np.float64)
        if p.ndim == 3:
            b = b[:, None, :]
        origin, scale = self._terrain_placement
        return np.asarray(origin, np.float64) + (np.asarray(lo, np.float64) + 8.0 * b + p) * float(scale)

    # -- voxel lighting: sky and torch light flooded through the open samples of a box (include/vtmc_light.h) ------------
    def terrain_light(self, params, sources=(), lower=None, upper=None):
        """Lights the box lower..upper (world bounds; None: the whole terrain) by the rule LIGHT for a LightParams (or a vtmc_light_params
        struct).  `sources`: a LIGHT_SOURCE_DTYPE array or rows of (x, y, z, level) in world space, level 1..255.  Returns source_lit: per
        source 1 (lit) or 0 (dark: outside the box or in solid).  Changes nothing in the terrain; the result is a snapshot, read with
        light_info / light_read / light_probe / vertex_light."""
        lo, up = fragment_bounds(lower, upper)
        src = np.asarray(sources)
        if src.dtype != LIGHT_SOURCE_DTYPE:
            rows = np.asarray(sources, np.float64).reshape(-1, 4)
            src = np.zeros(len(rows), LIGHT_SOURCE_DTYPE)
            src["position"], src["level"] = rows[:, :3], rows[:, 3]
        src = np.ascontiguousarray(src)
        p = _struct(params)
        lo_c, up_c = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*up)
        lit = np.zeros(len(src), np.uint8)
        self._check(self._L.vtmc_terrain_light(self._h, ctypes.byref(lo_c), ctypes.byref(up_c), ctypes.byref(p), _ptr(src) if len(src) else None, len(src),
                                               _ptr(lit) if len(src) else None))
        return lit

    def light_info(self):
        """(box_lo, box_dims, samples with sky > 0, samples with torch > 0, rounds of the relaxation) of the light result the context holds."""
        lo, d, n_sky, n_torch, rounds = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        self._check(self._L.vtmc_light_info(self._h, ctypes.byref(lo), ctypes.byref(d), ctypes.byref(n_sky), ctypes.byref(n_torch), ctypes.byref(rounds)))
        return tuple(lo), tuple(d), n_sky.value, n_torch.value, rounds.value

    def light_read(self):
        """The light volume, a LIGHT_SAMPLE_DTYPE array (fields sky, torch) indexed [x, y, z] with the box's dims (x fastest in memory)."""
        d = self.light_info()[1]
        out = np.zeros((d[2], d[1], d[0]), LIGHT_SAMPLE_DTYPE)
        self._check(self._L.vtmc_light_read(self._h, _ptr(out) if out.size else None, d[0] * d[1] * d[2]))
        return out.transpose(2, 1, 0)

    def device_light(self):
        """(device address of the light volume or None, box dims) of the light result; valid until the next terrain_light, terrain_init,
        terrain_load or close."""
        p, d = ctypes.c_void_p(), (ctypes.c_int32 * 3)()
        self._check(self._L.vtmc_light_device_results(self._h, ctypes.byref(p), ctypes.byref(d)))
        return p.value, tuple(d)

    def light_probe(self, positions):
        """(sky, torch), uint8 each, of world positions (n, 3): the two bytes of the nearest sample when it lies in the light box, else
        (0, 0).  What something that moves asks."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        sky, torch = np.zeros(len(p), np.uint8), np.zeros(len(p), np.uint8)
        self._check(self._L.vtmc_light_probe(self._h, _ptr(p) if len(p) else None, len(p), _ptr(sky), _ptr(torch)))
        return sky, torch

    def light_vertices(self):
        """Computes the two light bytes of every vertex of the result the context holds (from terrain_update / undo / redo / load) from
        the light result the context holds and leaves them on the device.  Returns their number: 3 T (soup) or V (indexed)."""
        n = ctypes.c_int64()
        self._check(self._L.vtmc_light_vertices(self._h, ctypes.byref(n)))
        return n.value

    def vertex_light(self):
        """light_vertices, then the bytes as a LIGHT_SAMPLE_DTYPE array: entry 3 t + v for corner v of soup triangle t, or one per
        vtmc_vertex of the indexed mesh."""
        n = self.light_vertices()
        out = np.zeros(n, LIGHT_SAMPLE_DTYPE)
        self._check(self._L.vtmc_light_read_vertices(self._h, _ptr(out) if n else None, n))
        return out

    def device_vertex_light(self):
        """(device address of the vertex light bytes, their number) of the last light_vertices; stale (VtmcError, ERR_NO_RESULT) after the
        next extract and after the next terrain_light."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_light_vertices_device_results(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # -- erosion: the maps the last ErosionModifier left (include/vtmc_erosion.h) ---------------------------------------
    EROSION_MAPS = {"height_before": _lib.EROSION_HEIGHT_BEFORE, "height_after": _lib.EROSION_HEIGHT_AFTER, "water": _lib.EROSION_WATER,
                    "sediment": _lib.EROSION_SEDIMENT, "active": _lib.EROSION_ACTIVE}

    def erosion_info(self):
        """The report of the last erosion as a dict: lo, hi (the clamped sample box, inclusive), nx, nz, iterations, n_active, n_rewritten,
        n_clamped.  Waits for the erosion if it is still running."""
        r = _lib.ErosionReport()
        self._check(self._L.vtmc_erosion_info(self._h, ctypes.byref(r)))
        return {"lo": tuple(r.lo), "hi": tuple(r.hi), "nx": r.nx, "nz": r.nz, "iterations": r.iterations, "n_active": r.n_active,
                "n_rewritten": r.n_rewritten, "n_clamped": r.n_clamped}

    def erosion_read(self, name):
        """One map of the last erosion, indexed [z, x] (x fastest in memory): "height_before", "height_after", "water", "sediment"
        (float32) or "active" (uint8).  Every map holds 0 on an inactive column."""
        if name not in self.EROSION_MAPS:
            raise ValueError("erosion map must be one of %s" % ", ".join(self.EROSION_MAPS))
        info = self.erosion_info()
        out = np.empty((info["nz"], info["nx"]), np.uint8 if name == "active" else np.float32)
        self._check(self._L.vtmc_erosion_read(self._h, self.EROSION_MAPS[name], _ptr(out), out.nbytes))
        return out

    def device_erosion(self):
        """The device addresses of the five maps, by name; valid until the next erosion, terrain_init, terrain_load or close."""
        p = [ctypes.c_void_p() for _ in range(5)]
        self._check(self._L.vtmc_erosion_device_results(self._h, *[ctypes.byref(q) for q in p]))
        return {name: p[i].value for name, i in self.EROSION_MAPS.items()}

    # -- material layer: VoxelTerrain.SetControlMap's splat volumes in HBM, paint, and per-vertex weights -------------
    def material_init(self, fineness):
        """The control volume of 16 * fineness texels per axis (fineness 1..8) over the resident terrain, every texel (255,0,0,0, 0,0,0,0).
        Returns the size C.  terrain_init / terrain_load drop it."""
        self._check(self._L.vtmc_material_init(self._h, int(fineness)))
        return self.material_size()

    def material_size(self):
        c = ctypes.c_int32()
        self._check(self._L.vtmc_material_read(self._h, None, ctypes.byref(c)))
        return c.value

    def set_control_map(self, colors, group):
        """VoxelTerrain.SetControlMap: `colors` holds C^3 RGBA floats in the order of the reference's Color[] (x fastest; a (C, C, C, 4)
        array indexed [k, j, i] is one), quantised on the device into the four bytes of `group` (1 or 2)."""
        c = self.material_size()
        colors = np.ascontiguousarray(colors, np.float32)
        if colors.size != c * c * c * 4:
            raise ValueError("invalid data size: expected %d x 4 floats" % (c * c * c))   # VoxelTerrain.cs:194-195
        self._check(self._L.vtmc_material_set_control_map(self._h, _ptr(colors), int(group)))

    def material_read(self):
        """The layer as a (C, C, C, 8) uint8 array indexed [k, j, i, channel]."""
        c = self.material_size()
        out = np.empty((c, c, c, MATERIAL_CHANNELS), np.uint8)
        self._check(self._L.vtmc_material_read(self._h, _ptr(out), None))
        return out

    def material_write(self, a):
        """The inverse of material_read."""
        c = self.material_size()
        a = np.ascontiguousarray(a, np.uint8)
        if a.shape != (c, c, c, MATERIAL_CHANNELS):
            raise ValueError("layer shape %r is not (%d, %d, %d, %d)" % (a.shape, c, c, c, MATERIAL_CHANNELS))
        self._check(self._L.vtmc_material_write(self._h, _ptr(a)))

    def paint(self, strokes):
        """Applies MaterialStroke objects (or vtmc_material_stroke structs) in order, in one pass over the texels they reach."""
        self._check(self._L.vtmc_material_paint(self._h, *_struct_array(strokes, _lib.MaterialStroke)))

    def material_vertices(self):
        """Computes the material weights of every vertex of the result the context holds (from terrain_update / undo / redo / load) and
        leaves them on the device.  Returns their number: 3 T (soup) or V (indexed)."""
        n = ctypes.c_int64()
        self._check(self._L.vtmc_material_vertices(self._h, ctypes.byref(n)))
        return n.value

    def vertex_materials(self):
        """material_vertices, then the weights as an (n, 8) uint8 array: row 3 t + v for corner v of soup triangle t, or one row per
        vtmc_vertex of the indexed mesh."""
        n = self.material_vertices()
        out = np.empty((n, MATERIAL_CHANNELS), np.uint8)
        self._check(self._L.vtmc_material_read_vertices(self._h, _ptr(out), n))
        return out

    def material_device_results(self):
        """(device address of the vertex weights, their number) of the last material_vertices."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_material_device_results(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # -- ambient occlusion: one byte per vertex of a terrain extract, marched through the resident grid ----------------
    def ao_vertices(self, params):
        """Computes the occlusion byte of every vertex of the result the context holds (from terrain_update / undo / redo / load) for an
        AmbientOcclusion (or a vtmc_ao_params struct) and leaves the bytes on the device.  Returns their number: 3 T (soup) or V (indexed)."""
        p = _struct(params)
        n = ctypes.c_int64()
        self._check(self._L.vtmc_ao_vertices(self._h, ctypes.byref(p), ctypes.byref(n)))
        return n.value

    def vertex_ao(self, radius, strength=1.0, steps=4):
        """ao_vertices, then the bytes as a uint8 array (255 = open, 0 = fully occluded at strength 1): entry 3 t + v for corner v of soup
        triangle t, or one per vtmc_vertex of the indexed mesh.  radius in world units, at most AO_MAX_RADIUS_CELLS cells."""
        n = self.ao_vertices(AmbientOcclusion(radius, strength, steps))
        out = np.empty(n, np.uint8)
        self._check(self._L.vtmc_ao_read_vertices(self._h, _ptr(out), n))
        return out

    def device_ao(self):
        """(device address of the occlusion bytes, their number) of the last ao_vertices."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_ao_device_results(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # -- surface scatter: instances over the triangles of a terrain extract, stable under edits ------------------------
    def scatter_surface(self, params):
        """Scatters instances over the result the context holds (from terrain_update / undo / redo / load) for a ScatterParams (or a
        vtmc_scatter_params struct).  Returns (instances, block_offsets): a structured INSTANCE_DTYPE array in triangle order, and the
        B + 1 instance offsets of the blocks of the result's list, so block b owns instances[block_offsets[b]:block_offsets[b + 1]]."""
        p = _struct(params)
        n = ctypes.c_int64()
        self._check(self._L.vtmc_scatter_surface(self._h, ctypes.byref(p), ctypes.byref(n)))
        out = np.zeros(n.value, INSTANCE_DTYPE)
        offs = np.zeros(self.last_counts()[0] + 1, np.int32)
        self._check(self._L.vtmc_scatter_read(self._h, _ptr(out), n.value, _ptr(offs)))
        return out, offs

    def device_scatter(self):
        """(device address of the instances, device address of the B + 1 block offsets, the number of instances) of the last
        scatter_surface."""
        p, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_scatter_device_results(self._h, ctypes.byref(p), ctypes.byref(o), ctypes.byref(n)))
        return p.value, o.value, n.value

    # -- level of detail: the resident terrain meshed coarsely far from a viewer ---------------------------------------
    def terrain_extract_lod(self, viewer, max_level, split=2.0, max_nodes=1 << 18):
        """Chooses an octree of nodes around `viewer` (world space; roots of level max_level, a node of 8 * 2^L cells splits when the viewer
        is nearer than split times its size), gathers each node's tile from the resident grid at stride 2^L and extracts them as blocks, in
        the output mode set.  `viewer` may be a LodParams (or a vtmc_lod_params struct) instead; the other arguments are then not read.
        Returns (number of nodes, T); read the mesh as after any extract, `block` of a triangle indexes terrain_lod_nodes()."""
        p = _struct(viewer if hasattr(viewer, "to_struct") or isinstance(viewer, _lib.LodParams) else LodParams(viewer, max_level, split, max_nodes))
        n, t = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.vtmc_terrain_extract_lod(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(t)))
        return n.value, t.value

    def terrain_lod_nodes(self):
        """The nodes of the level-of-detail result the context holds: an (n, 4) int32 array of (origin x, y, z in cells, level)."""
        n = ctypes.c_int32()
        self._check(self._L.vtmc_terrain_lod_nodes(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 4), np.int32)
        self._check(self._L.vtmc_terrain_lod_nodes(self._h, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def lod_world_positions(self, nodes, block, local_positions):
        """World positions (float64) of node-local positions of a level-of-detail mesh: terrain origin + (o + p * 2^level) * voxel scale,
        with (o, level) = nodes[block].  block: (n,) node indices (a triangle's `block`); local_positions: (n, 3) or (n, m, 3)."""
        nodes = np.asarray(nodes, np.int64).reshape(-1, 4)
        block = np.asarray(block, np.int64)
        p = np.asarray(local_positions, np.float64)
        o, s = nodes[block, :3].astype(np.float64), np.ldexp(1.0, nodes[block, 3])
        if p.ndim == 3:
            o, s = o[:, None, :], s[:, None, None]
        else:
            s = s[:, None]
        origin, scale = self._terrain_placement
        return np.asarray(origin, np.float64) + (o + p * s) * float(scale)

    # -- level-of-detail seams: skirt triangles over the faces where the level changes (include/vtmc_lodskirt.h) --------
    def lod_skirts(self, depth=1.0, all_faces=False):
        """Builds the skirts of the level-of-detail result the context holds, on the device, by the rule LODSKIRT: `depth` in the node's
        own cells, all_faces for every face with a node behind it.  `depth` may be a LodSkirtParams (or a vtmc_lodskirt_params struct)
        instead.  Returns the number of skirt records; the extract's own result is unchanged.  Draw both."""
        p = _struct(depth if hasattr(depth, "to_struct") or isinstance(depth, _lib.LodSkirtParamsStruct) else LodSkirtParams(depth, all_faces))
        n = ctypes.c_int64()
        self._check(self._L.vtmc_lod_skirts(self._h, ctypes.byref(p), ctypes.byref(n)))
        return n.value

    def lodskirt_info(self):
        """(nodes, nodes with a flagged face, skirt records) of the skirts the context holds."""
        n, f, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self._L.vtmc_lodskirt_info(self._h, ctypes.byref(n), ctypes.byref(f), ctypes.byref(t)))
        return n.value, f.value, t.value

    def lodskirt_masks(self):
        """The face mask of every node (uint8; bit f: face f of -x, +x, -y, +y, -z, +z is flagged)."""
        out = np.zeros(self.lodskirt_info()[0], np.uint8)
        self._check(self._L.vtmc_lodskirt_masks(self._h, _ptr(out) if len(out) else None, len(out)))
        return out

    def lodskirt_read(self):
        """(records, node_offsets): the skirt records as a TRI_DTYPE array (`block` the node's index, positions node-local: place them
        with lod_world_positions) and the nodes + 1 offsets, so node i owns records[node_offsets[i]:node_offsets[i + 1]]."""
        nodes, _, n = self.lodskirt_info()
        out, offs = np.zeros(n, TRI_DTYPE), np.zeros(nodes + 1, np.int32)
        self._check(self._L.vtmc_lodskirt_read(self._h, _ptr(out) if n else None, n, _ptr(offs)))
        return out, offs

    def device_lodskirts(self):
        """(device address of the skirt records, device address of the nodes + 1 offsets, the number of records) of the last lod_skirts."""
        p, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_lodskirt_device_results(self._h, ctypes.byref(p), ctypes.byref(o), ctypes.byref(n)))
        return p.value, o.value, n.value

    # -- level-of-detail shading: materials and occlusion of that result and of its skirts (include/vtmc_lodattr.h) ------
    def lod_material_vertices(self):
        """Computes the material weights of every vertex of the level-of-detail result the context holds and, when skirts of it exist, of
        every skirt corner, by the rule LODATTR, and leaves them on the device.  Returns (mesh vertices, skirt vertices)."""
        n, s = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vtmc_lod_material_vertices(self._h, ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def lod_ao_vertices(self, params):
        """The same for the occlusion bytes of an AmbientOcclusion (or a vtmc_ao_params struct): the radius counts the node's own cells."""
        p = _struct(params)
        n, s = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vtmc_lod_ao_vertices(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def lodattr_info(self, attribute):
        """(mesh vertices, skirt vertices) an attribute (LODATTR_MATERIAL, LODATTR_AO) holds for the current result; 0 skirt vertices
        without a skirt target."""
        n, s = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vtmc_lodattr_info(self._h, int(attribute), ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def lodattr_read(self, attribute, target):
        """The values an attribute holds for a target (LODATTR_MESH, LODATTR_SKIRTS), as computed by the last lod_material_vertices /
        lod_ao_vertices: an (n, 8) uint8 array of weights or n occlusion bytes."""
        n = ctypes.c_int64()
        self._check(self._L.vtmc_lodattr_device_results(self._h, int(attribute), int(target), None, ctypes.byref(n)))
        out = np.empty((n.value, MATERIAL_CHANNELS) if attribute == _lib.LODATTR_MATERIAL else n.value, np.uint8)
        self._check(self._L.vtmc_lodattr_read(self._h, int(attribute), int(target), _ptr(out) if n.value else None, n.value))
        return out

    def lod_vertex_materials(self):
        """lod_material_vertices, then the weights of the mesh as an (n, 8) uint8 array: row 3 t + v for corner v of soup triangle t, or
        one row per vtmc_vertex of the indexed mesh."""
        self.lod_material_vertices()
        return self.lodattr_read(_lib.LODATTR_MATERIAL, _lib.LODATTR_MESH)

    def lod_vertex_ao(self, radius, strength=1.0, steps=4):
        """lod_ao_vertices, then the bytes of the mesh (255 = open).  radius in world units, at most AO_MAX_RADIUS_CELLS cells; a node of
        level L marches 2^L times as far in the world."""
        self.lod_ao_vertices(AmbientOcclusion(radius, strength, steps))
        return self.lodattr_read(_lib.LODATTR_AO, _lib.LODATTR_MESH)

    def lod_skirt_materials(self):
        """The weights of the 3 n corners of the skirt records, record order, as the last lod_material_vertices left them: every corner
        carries the weights of the mesh vertex it came from."""
        return self.lodattr_read(_lib.LODATTR_MATERIAL, _lib.LODATTR_SKIRTS)

    def lod_skirt_ao(self):
        """The occlusion bytes of the 3 n corners of the skirt records, as the last lod_ao_vertices left them."""
        return self.lodattr_read(_lib.LODATTR_AO, _lib.LODATTR_SKIRTS)

    def device_lod_attributes(self, attribute, target):
        """(device address of the values, their number) of an attribute and target of the last compute call."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._L.vtmc_lodattr_device_results(self._h, int(attribute), int(target), ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # -- ray picking: Physics.Raycast of the interactive edit (SceneManager.cs:114-131) on the device ---------------
    def terrain_raycast(self, origins, directions, max_distance=float("inf"), two_sided=False):
        """Nearest surface hit of each ray (world-space origins / directions, (n, 3)) on the resident terrain: a RAY_HIT_DTYPE
        array, distance -1 and triangle -1 for a miss."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("origins and directions differ in length")
        hits = np.zeros(len(o), RAY_HIT_DTYPE)
        self._check(self._L.vtmc_terrain_raycast(self._h, _ptr(o), _ptr(d), len(o), max_distance,
                                                 RAY_TWO_SIDED if two_sided else 0, _ptr(hits)))
        return hits

    def raycast_device(self, d_grid, n, strides, origin, voxel_scale, d_origins, d_directions, n_rays, d_hits,
                       max_distance=float("inf"), two_sided=False, stream=None):
        """vtmc_raycast_device: device addresses (int) of the grid, the rays and n_rays RAY_HIT_DTYPE records; n = (nx, ny, nz) cells,
        element strides.  Queued on `stream`, not synchronised."""
        org = (ctypes.c_float * 3)(*origin)
        self._check(self._L.vtmc_raycast_device(self._h, d_grid, n[0], n[1], n[2], strides[0], strides[1], strides[2], ctypes.byref(org),
                                                voxel_scale, d_origins, d_directions, n_rays, max_distance,
                                                RAY_TWO_SIDED if two_sided else 0, d_hits, stream))

    # -- sphere queries: Physics.SphereCast / CheckSphere / ClosestPoint against the MeshColliders (VoxelTerrain.cs:168, 464) -------
    @staticmethod
    def _radii(radii, n):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (n,)))   # a scalar, or one value per query

    def terrain_spherecast(self, origins, directions, radii, max_distance=float("inf"), two_sided=False):
        """First contact of each swept sphere (world-space origins / directions, (n, 3); radii: a scalar or (n,)) with the resident
        terrain: a SPHERE_HIT_DTYPE array, distance -1 and triangle -1 for a miss."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("origins and directions differ in length")
        r = self._radii(radii, len(o))
        hits = np.zeros(len(o), SPHERE_HIT_DTYPE)
        self._check(self._L.vtmc_terrain_spherecast(self._h, _ptr(o), _ptr(d), _ptr(r), len(o), max_distance,
                                                    RAY_TWO_SIDED if two_sided else 0, _ptr(hits)))
        return hits

    def terrain_closest_point(self, centers, radii):
        """Nearest surface point within each ball (world-space centres, (n, 3); radii: a scalar or (n,)) on the resident terrain: a
        SPHERE_HIT_DTYPE array, distance -1 and triangle -1 when no triangle is within the radius."""
        c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
        r = self._radii(radii, len(c))
        hits = np.zeros(len(c), SPHERE_HIT_DTYPE)
        self._check(self._L.vtmc_terrain_closest_point(self._h, _ptr(c), _ptr(r), len(c), 0, _ptr(hits)))
        return hits

    def spherecast_device(self, d_grid, n, strides, origin, voxel_scale, d_origins, d_directions, d_radii, n_queries, d_hits,
                          max_distance=float("inf"), two_sided=False, stream=None):
        """vtmc_spherecast_device: device addresses (int) of the grid, the queries and n_queries SPHERE_HIT_DTYPE records; n = (nx, ny,
        nz) cells, element strides.  Queued on `stream`, not synchronised."""
        org = (ctypes.c_float * 3)(*origin)
        self._check(self._L.vtmc_spherecast_device(self._h, d_grid, n[0], n[1], n[2], strides[0], strides[1], strides[2], ctypes.byref(org),
                                                   voxel_scale, d_origins, d_directions, d_radii, n_queries, max_distance,
                                                   RAY_TWO_SIDED if two_sided else 0, d_hits, stream))

    def closest_point_device(self, d_grid, n, strides, origin, voxel_scale, d_centers, d_radii, n_queries, d_hits, stream=None):
        """vtmc_closest_point_device: as spherecast_device, for closest-point queries."""
        org = (ctypes.c_float * 3)(*origin)
        self._check(self._L.vtmc_closest_point_device(self._h, d_grid, n[0], n[1], n[2], strides[0], strides[1], strides[2], ctypes.byref(org),
                                                      voxel_scale, d_centers, d_radii, n_queries, 0, d_hits, stream))

    def density_fill_device(self, params, origins, dims, strides, volume_stride, d_out, stream=None, wait=True):
        """wait=False queues the fill on `stream` without synchronising (vtmc_density_fill_device_async)."""
        origins = np.ascontiguousarray(origins, np.int32).reshape(-1, 3)
        fn = self._L.vtmc_density_fill_device if wait else self._L.vtmc_density_fill_device_async
        self._check(fn(self._h, ctypes.byref(params), _ptr(origins), len(origins),
                                                     dims[0], dims[1], dims[2], strides[0], strides[1],
                                                     strides[2], volume_stride, d_out, stream))
