"""The numpy twin of the stamp modifier (VTMC_MOD_STAMP): a FP32 restatement of include/vtmc.h's rule in its order of operations, on the
memory of the terrain twin (terrain_twin.py), whose box arithmetic, clamp draws and CSG write it uses.  The host half (the quaternion's
rotation matrix over the pitch) is restated here in float64, not taken from the mirror class.

A stamp spec is ("stamp", kwargs of vt.StampModifier); the twin's stamps are a dict {id: float32 array indexed [x, y, z]} the test keeps
beside the device's.  twin_update runs "stamp" specs here and hands every other spec to terrain_twin.twin_update, one modifier and one
event number at a time.

test_terrain_stamp.py checks this yardstick on the CPU against scipy.ndimage.map_coordinates and against the same map in float64."""
import numpy as np

import volumetricterrain_amd as vt
import terrain_twin
from terrain_twin import assert_grid, assert_triangles, block_list, box_of, clamp_drawn, csg_write, image_bytes, positions

f32, u64 = np.float32, np.uint64


def gpu_mod(spec):
    return vt.StampModifier(**spec[1]) if spec[0] == "stamp" else terrain_twin.gpu_mod(spec)


def gpu_struct(spec):
    """terrain_twin.gpu_struct for queues that hold stamps: the struct of a spec, its AABB overridden where the spec carries one."""
    return terrain_twin.gpu_struct(spec, gpu_mod)


def stamp_map(p, dims):
    """(M, c) of the header's rule from the floats of p: M[i][j] = (float)(R[j][i] / (double)h), c_k = (float)(n_k - 1) * 0.5f."""
    x, y, z, w = (float(f32(v)) for v in p[3:7])
    n = float(np.sqrt(np.float64(x * x + y * y + z * z + w * w)))
    x, y, z, w = x / n, y / n, z / n, w / n
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    h = float(f32(p[7]))
    M = np.array([[f32(R[j][i] / h) for j in range(3)] for i in range(3)], f32)
    c = np.array([f32(n_k - 1) * f32(0.5) for n_k in dims], f32)
    return M, c


def stamp_coords(px, py, pz, p, dims):
    """(u, v, w) in float32 at world positions px [x], py [y], pz [z], broadcast to [z, y, x]."""
    M, c = stamp_map(p, dims)
    dx, dy, dz = (px - f32(p[0]))[None, None, :], (py - f32(p[1]))[None, :, None], (pz - f32(p[2]))[:, None, None]
    out = tuple(((M[r, 0] * dx + M[r, 1] * dy) + M[r, 2] * dz) + c[r] for r in range(3))
    assert all(a.dtype == f32 for a in out)
    return out


def footprint(u, v, w, dims):
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u <= f32(dims[0] - 1)) & (v >= 0) & (v <= f32(dims[1] - 1)) & (w >= 0) & (w <= f32(dims[2] - 1))


def stamp_values(s, u, v, w):
    """q of the rule at stamp coordinates inside the footprint (float32 arrays of one shape); s indexed [x, y, z]."""
    def cell(t, n):
        i = np.floor(t).astype(np.int64)
        return i, np.minimum(i + 1, n - 1), t - i.astype(f32)
    (i, i1, fu), (j, j1, fv), (k, k1, fw) = cell(u, s.shape[0]), cell(v, s.shape[1]), cell(w, s.shape[2])
    row = lambda jj, kk: s[i, jj, kk] + (s[i1, jj, kk] - s[i, jj, kk]) * fu   # noqa: E731
    a00, a10, a01, a11 = row(j, k), row(j1, k), row(j, k1), row(j1, k1)
    b0 = a00 + (a10 - a00) * fv
    b1 = a01 + (a11 - a01) * fv
    q = b0 + (b1 - b0) * fw
    assert q.dtype == f32
    return q


def apply_stamp(ref, m, s):
    """One VTMC_MOD_STAMP struct m on the twin's memory with stamp samples s [x, y, z]; one event number.  Returns the block ids it
    dirties and how many samples lay inside the footprint."""
    first, ext, ids = box_of(ref, m)
    n_in = 0
    if min(ext) > 0:
        (lx, ly, lz), (dx, dy, dz) = first, ext
        px, py, pz = positions(ref, first, ext)
        u, v, w = stamp_coords(px, py, pz, list(m.p), s.shape)
        inside = footprint(u, v, w, s.shape)
        n_in = int(inside.sum())
        zero = f32(0)
        q = stamp_values(np.ascontiguousarray(s, f32), np.where(inside, u, zero), np.where(inside, v, zero), np.where(inside, w, zero))
        box = (slice(lz, lz + dz), slice(ly, ly + dy), slice(lx, lx + dx))
        before = np.array(ref._mem[box], f32)
        if m.data_dims[1] == 1:   # replace
            event = ref.events + 1
            Dx, Dy = ref.dims[0] + 2, ref.dims[1] + 2
            zz, yy, xx = np.meshgrid(np.arange(lz, lz + dz, dtype=u64), np.arange(ly, ly + dy, dtype=u64), np.arange(lx, lx + dx, dtype=u64), indexing="ij")
            clamped, _, _ = clamp_drawn(q, ref.seed, event, xx + u64(Dx) * (yy + u64(Dy) * zz), 0)
            ref._mem[box] = np.where(np.abs(q) <= 2, q, clamped).astype(f32)
            ref.events = event
        else:
            csg_write(ref, first, ext, q, bool(m.add_or_erode))
        ref._mem[box] = np.where(inside, np.array(ref._mem[box], f32), before)   # outside the footprint: the sample keeps its 32 bits
    else:
        ref.events += 1
    return ids, n_in


def twin_update(ref, oracle_mod, specs, stamps, counts=None, taken=None):
    """terrain_twin.twin_update with "stamp" specs run here; stamps: {id: samples [x, y, z]}.  counts: a list that receives each stamp
    modifier's number of samples inside the footprint; taken: handed on to terrain_twin.twin_update."""
    nb = tuple(d // 8 for d in ref.dims)
    ids = set()
    for spec in specs:
        if spec[0] == "stamp":
            hit, n_in = apply_stamp(ref, gpu_struct(spec), stamps[spec[1]["stamp_id"]])
            ids |= hit
            if counts is not None:
                counts.append(n_in)
        else:
            ids |= {int(bx + nb[0] * (by + nb[1] * bz)) for bx, by, bz in terrain_twin.twin_update(ref, oracle_mod, [spec], taken)}
    return block_list(ids, nb)


def step_bytes(ref, specs):
    """terrain_twin.step_bytes' rule -- the boxes' images, no halo -- for queues that hold stamps."""
    return sum(image_bytes(box_of(ref, gpu_struct(s))[1]) for s in specs)


def assert_update(ex, ref, oracle_mod, specs, stamps, counts=None):
    """terrain_twin.assert_update for queues that hold stamps: the grid and the dirty list bit for bit, triangles within the bar."""
    n_dirty, T = ex.terrain_update([gpu_struct(s) for s in specs])
    dirty = twin_update(ref, oracle_mod, specs, stamps, counts)
    assert_grid(ex, ref.grid)
    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
    assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
    return n_dirty, T
