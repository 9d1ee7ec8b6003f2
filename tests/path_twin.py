"""The numpy twin of the path modifier (VTMC_MOD_PATH): a FP32 restatement of include/vtmc.h's rule in its order of operations, un-pruned
(every segment on every sample of the box), on the memory of the terrain twin (terrain_twin.py), whose box arithmetic, positions and
CSG write it uses.  The host half (e, il, dr) is restated here, not taken from the library.

A path spec is ("path", kwargs of vt.PathModifier) with the optional third entry of terrain_twin's specs (an AABB of the test's own).
twin_update runs "path" specs here and hands every other spec to terrain_twin.twin_update, one modifier and one event number at a time.

test_terrain_path.py checks this yardstick on the CPU against a plain scalar loop of the header's steps."""
import ctypes

import numpy as np

import volumetricterrain_amd as vt
import terrain_twin
from terrain_twin import assert_grid, assert_triangles, block_list, box_of, csg_write, image_bytes, positions

f32 = np.float32


def gpu_mod(spec):
    return vt.PathModifier(**spec[1]) if spec[0] == "path" else terrain_twin.gpu_mod(spec)


def gpu_struct(spec):
    """terrain_twin.gpu_struct for queues that hold paths: the struct of a spec, its AABB overridden where the spec carries one."""
    return terrain_twin.gpu_struct(spec, gpu_mod)


def struct_segments(m):
    """The (n, 8) float32 segments a VTMC_MOD_PATH struct points at."""
    n, k = m.data_dims[0], m.data_dims[1]
    return np.ctypeslib.as_array(ctypes.cast(m.data, ctypes.POINTER(ctypes.c_float)), shape=(n, k)).copy()


def path_host(seg):
    """(e [n, 3], il [n], dr [n]) of the header's host half, float32, one operation per step."""
    seg = np.asarray(seg, f32)
    e = seg[:, 4:7] - seg[:, 0:3]
    ll = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    with np.errstate(divide="ignore", over="ignore"):
        il = np.where(ll >= f32(1e-30), f32(1) / ll, f32(0)).astype(f32)
    dr = seg[:, 7] - seg[:, 3]
    assert e.dtype == il.dtype == dr.dtype == f32
    return e, il, dr


def path_density(seg, px, py, pz):
    """q of include/vtmc.h at world positions px, py, pz (float32 arrays that broadcast to one shape): every segment, increasing index."""
    seg = np.asarray(seg, f32)
    e, il, dr = path_host(seg)
    px, py, pz = (np.asarray(v, f32) for v in (px, py, pz))
    q = np.full(np.broadcast(px, py, pz).shape, -np.inf, f32)
    zero, one = f32(0), f32(1)
    for s in range(len(seg)):
        ax, ay, az, ra = seg[s, 0:4]
        ex, ey, ez = e[s]
        dx, dy, dz = px - ax, py - ay, pz - az
        t = ((dx * ex + dy * ey) + dz * ez) * il[s]
        t = np.where(t < zero, zero, np.where(t > one, one, t))
        cx, cy, cz = dx - ex * t, dy - ey * t, dz - ez * t
        d = np.sqrt((cx * cx + cy * cy) + cz * cz)
        r = ra + dr[s] * t
        f = r - d
        assert f.dtype == f32
        q = np.where(f > q, f, q)
    return q


def apply_path(ref, m):
    """One VTMC_MOD_PATH struct m on the twin's memory; one event number.  Returns the block ids it dirties and csg_write's clamp-branch
    counts (low, high)."""
    first, ext, ids = box_of(ref, m)
    q = None
    if min(ext) > 0:
        px, py, pz = positions(ref, first, ext)
        q = path_density(struct_segments(m), px[None, None, :], py[None, :, None], pz[:, None, None])
    return ids, csg_write(ref, first, ext, q, bool(m.add_or_erode))


def twin_update(ref, oracle_mod, specs, taken=None):
    """terrain_twin.twin_update with "path" specs run here.  taken: a {"low": n, "high": n} dict to which the clamp-branch counts of the
    paths (and, through terrain_twin, of the noise modifiers) are added."""
    nb = tuple(d // 8 for d in ref.dims)
    ids = set()
    for spec in specs:
        if spec[0] == "path":
            hit, (low, high) = apply_path(ref, gpu_struct(spec))
            ids |= hit
            if taken is not None:
                taken["low"] += low
                taken["high"] += high
        else:
            ids |= {int(bx + nb[0] * (by + nb[1] * bz)) for bx, by, bz in terrain_twin.twin_update(ref, oracle_mod, [spec], taken)}
    return block_list(ids, nb)


def step_bytes(ref, specs):
    """terrain_twin.step_bytes' rule -- the boxes' images, no halo -- for queues that hold paths."""
    return sum(image_bytes(box_of(ref, gpu_struct(s))[1]) for s in specs)


def assert_update(ex, ref, oracle_mod, specs, taken=None):
    """terrain_twin.assert_update for queues that hold paths: the grid and the dirty list bit for bit, triangles within the bar."""
    n_dirty, T = ex.terrain_update([gpu_struct(s) for s in specs])
    dirty = twin_update(ref, oracle_mod, specs, taken)
    assert_grid(ex, ref.grid)
    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
    assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
    return n_dirty, T
