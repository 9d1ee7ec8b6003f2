"""Persisted terrain format: the device-resident terrain of vtmc_terrain_* and its state as a sparse brick file.  This module is the
format's definition and a pure-numpy mirror of what libvtmc.so's vtmc_terrain_save / vtmc_terrain_load do on the device
(csrc/terrain_io.hip); the reference has no persistence at all.

Layout (little-endian):
    header  64 B : u32 magic "VTMT", u32 version = 1, u32 flags (1: saved exact), i32 W, E, H (cells), f32 voxel_scale, f32 origin[3],
                   u64 seed, u32 events (the terrain's event counter when it was saved), u32 n_raw, 8 reserved bytes (zero)
    kinds        : one byte per brick in brick-index order, padded to 16 bytes
    RAW bricks   : 2048 B each (f32[512], sample (i, j, k) at i + 8j + 64k, +0.0 outside the grid), in increasing brick index
The file is exactly 64 + pad16(nbx*nby*nbz) + 2048 * n_raw bytes.

Bricks: the (W+2, E+2, H+2) sample grid in disjoint 8x8x8-sample bricks, nb = W/8 + 1 per axis (the last brick of an axis holds 2
sample planes), brick index bx + nbx*(by + nby*bz).  Kinds:
    1 VOID  every own sample s <= -1 and every sample of the up-to-27 bricks around it (clipped at the grid) !(s > 0)
    2 FULL  every own sample s >= 1 and every sample of those bricks s > 0
    0 RAW   everything else (any brick holding a NaN)
RAW bricks are kept bit for bit.  The extract path reads a sample only as a corner of an active cell or as the forward neighbour of
such a corner, so within 2 samples of a sign change; the neighbourhood test is a whole-brick dilation of that distance, so an elided
sample never reaches a triangle.  On load an elided sample is redrawn from the terrain's counter hash under ONE event number
e = events + 1 (which becomes the terrain's event counter): VOID -> uniform(seed, e, index, 0) - 2, FULL -> uniform(seed, e, index, 1) + 1,
index = x + (W+2)*(y + (E+2)*z).
"""
import os
import struct

import numpy as np

MAGIC = 0x544D5456   # b"VTMT"
VERSION = 1
HEADER = struct.Struct("<III3if3fQII8x")
assert HEADER.size == 64
F_EXACT = 1
RAW, VOID, FULL = 0, 1, 2
BRICK_BYTES = 2048


def pad16(n):
    return (n + 15) & ~15


def brick_counts(dims):
    """Bricks per axis of a terrain of dims = (W, E, H) cells."""
    return tuple(d // 8 + 1 for d in dims)


def file_size(dims, n_raw):
    nb = brick_counts(dims)
    return 64 + pad16(nb[0] * nb[1] * nb[2]) + BRICK_BYTES * n_raw


def terrain_uniform(seed, event, sample, draw):
    """csrc/terrain_hash.h in uint64 arithmetic: float32 in [0, 1) for an array of sample indices."""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ np.uint64((event & 0xFFFFFFFF) << 40) ^ (np.asarray(sample, np.uint64) << np.uint64(2))
             ^ np.uint64(draw)) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)) & np.uint64(0xFFFFFFFF)).astype(np.float32) * np.float32(5.9604644775390625e-08)


def _to_bricks(pred, nb, fill):
    """A per-sample predicate indexed [x, y, z] as [bx, i, by, j, bz, k], slots outside the grid = fill."""
    full = np.full(tuple(8 * n for n in nb), fill, bool)
    full[:pred.shape[0], :pred.shape[1], :pred.shape[2]] = pred
    return full.reshape(nb[0], 8, nb[1], 8, nb[2], 8)


def _neighbourhood(a, reduce, fill):
    """reduce (np.logical_or / np.logical_and) of a per-brick flag over the 3x3x3 bricks around each brick, clipped at the grid."""
    p = np.pad(a, 1, constant_values=fill)
    out = np.full(a.shape, fill, bool)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out = reduce(out, p[dx:dx + a.shape[0], dy:dy + a.shape[1], dz:dz + a.shape[2]])
    return out


def classify_bricks(grid):
    """Kind byte of every brick of a sample grid indexed [x, y, z] (shape (W+2, E+2, H+2)), in brick-index order."""
    grid = np.asarray(grid)
    if grid.dtype != np.float32 or grid.ndim != 3 or any(d < 10 or (d - 2) % 8 for d in grid.shape):
        raise ValueError("grid must be float32 [x, y, z] of shape (W+2, E+2, H+2), W, E, H multiples of 8")
    nb = brick_counts(tuple(d - 2 for d in grid.shape))
    with np.errstate(invalid="ignore"):
        pos = grid > 0
        all_le = _to_bricks(grid <= -1, nb, True).all(axis=(1, 3, 5))
        all_ge = _to_bricks(grid >= 1, nb, True).all(axis=(1, 3, 5))
    any_pos = _to_bricks(pos, nb, False).any(axis=(1, 3, 5))
    all_pos = _to_bricks(pos, nb, True).all(axis=(1, 3, 5))
    kinds = np.zeros(nb, np.uint8)
    kinds[all_ge & _neighbourhood(all_pos, np.logical_and, True)] = FULL
    kinds[all_le & ~_neighbourhood(any_pos, np.logical_or, False)] = VOID   # a brick cannot pass both own tests
    return np.ascontiguousarray(kinds.transpose(2, 1, 0)).ravel()           # bx fastest


def _brick_view(grid, nb):
    """The grid's 32-bit words as [bz, by, bx, k, j, i] (a copy, zero = +0.0 outside the grid)."""
    full = np.zeros(tuple(8 * n for n in nb), np.uint32)
    full[:grid.shape[0], :grid.shape[1], :grid.shape[2]] = np.ascontiguousarray(grid).view(np.uint32)
    return full.reshape(nb[0], 8, nb[1], 8, nb[2], 8).transpose(4, 2, 0, 5, 3, 1)


def write_terrain(path, grid, meta, exact=False):
    """grid indexed [x, y, z]; meta: dict with "scale", "origin" (3), "seed", "events".  Returns the number of bytes written."""
    grid = np.asarray(grid)
    kinds = classify_bricks(grid)
    if exact:
        kinds[:] = RAW
    dims = tuple(d - 2 for d in grid.shape)
    nb = brick_counts(dims)
    raw = np.flatnonzero(kinds == RAW)
    bricks = _brick_view(grid, nb).reshape(len(kinds), 512)[raw]
    with open(path, "wb") as f:
        f.write(HEADER.pack(MAGIC, VERSION, F_EXACT if exact else 0, *dims, float(meta["scale"]), *[float(v) for v in meta["origin"]],
                            int(meta["seed"]) & 0xFFFFFFFFFFFFFFFF, int(meta["events"]) & 0xFFFFFFFF, len(raw)))
        f.write(kinds.tobytes())
        f.write(b"\0" * (pad16(len(kinds)) - len(kinds)))
        f.write(np.ascontiguousarray(bricks).tobytes())
        return f.tell()


def read_header(path):
    """The header as a dict (dims, scale, origin, seed, events, flags, n_raw), with the rejections of vtmc_terrain_load that need
    only the header and the file's size."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(64)
    if len(head) != 64:
        raise ValueError("%s is shorter than a terrain header" % path)
    magic, version, flags, w, e, h, scale, ox, oy, oz, seed, events, n_raw = HEADER.unpack(head)
    if magic != MAGIC or version != VERSION:
        raise ValueError("%s is not a version-1 terrain file" % path)
    if any(d <= 0 or d > 1024 or d % 8 for d in (w, e, h)):
        raise ValueError("%s: dims %r are not multiples of 8 in 8..1024" % (path, (w, e, h)))
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("%s: voxel_scale %r is not finite and > 0" % (path, scale))
    if not all(np.isfinite(v) for v in (ox, oy, oz)):
        raise ValueError("%s: origin is not finite" % path)
    nb = brick_counts((w, e, h))
    if n_raw > nb[0] * nb[1] * nb[2] or size != file_size((w, e, h), n_raw):
        raise ValueError("%s: %d bytes, its header implies %d" % (path, size, file_size((w, e, h), n_raw)))
    return {"dims": (w, e, h), "scale": scale, "origin": (ox, oy, oz), "seed": seed, "events": events, "flags": flags, "n_raw": n_raw}


def read_terrain(path):
    """Returns (meta, kinds, grid): the header dict of read_header plus "event" (events + 1, the terrain's event counter after the
    load), the kind table, and the dense grid indexed [x, y, z] (x fastest in memory) as vtmc_terrain_load leaves it on the device."""
    meta = read_header(path)
    dims = meta["dims"]
    nb = brick_counts(dims)
    n = nb[0] * nb[1] * nb[2]
    with open(path, "rb") as f:
        f.seek(64)
        kinds = np.frombuffer(f.read(pad16(n)), np.uint8)[:n].copy()
        if len(kinds) != n or kinds.max() > FULL:
            raise ValueError("%s: unknown brick kind" % path)
        raw = np.flatnonzero(kinds == RAW)
        if len(raw) != meta["n_raw"]:
            raise ValueError("%s: n_raw %d, but %d bricks of kind 0" % (path, meta["n_raw"], len(raw)))
        bricks = np.frombuffer(f.read(BRICK_BYTES * len(raw)), np.uint32)
    if bricks.size != 512 * len(raw):
        raise ValueError("%s: truncated" % path)
    meta["event"] = (meta["events"] + 1) & 0xFFFFFFFF
    dx, dy, dz = (d + 2 for d in dims)
    # elided samples from the hash, by their index in the x-fastest grid
    k3 = kinds.reshape(nb[2], nb[1], nb[0])
    kind_s = np.repeat(np.repeat(np.repeat(k3, 8, axis=0), 8, axis=1), 8, axis=2)[:dz, :dy, :dx]
    mem = np.zeros((dz, dy, dx), np.float32)
    for kind, draw, shift in ((VOID, 0, np.float32(-2)), (FULL, 1, np.float32(1))):
        at = np.flatnonzero(kind_s.ravel() == kind)
        mem.ravel()[at] = terrain_uniform(meta["seed"], meta["event"], at, draw) + shift
    # RAW bricks, 32-bit copies
    words = np.zeros((nb[2], nb[1], nb[0], 8, 8, 8), np.uint32)
    words.reshape(n, 512)[raw] = bricks.reshape(len(raw), 512)
    dense = words.transpose(0, 3, 1, 4, 2, 5).reshape(8 * nb[2], 8 * nb[1], 8 * nb[0])[:dz, :dy, :dx]
    is_raw = kind_s == RAW
    mem.view(np.uint32)[is_raw] = dense[is_raw]
    return meta, kinds, mem.transpose(2, 1, 0)
