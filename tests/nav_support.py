"""What the tests of the navigation layers share (test_terrain_nav.py, _navfield.py, _naverode.py, _navsight.py, and the session test):
the crafted fields and boxes, the twin's results on them, and the helpers that build a terrain and compare results.  No tests here.

The terrain is 72 x 16 x 32 cells = 74 x 18 x 34 samples: a row of columns crosses a 64-lane wave along x and nine workgroup rows along
z; the same field is run once turned, with 74 samples along z.  The crafted field stands on a flat floor (solid up to sample 2, height
2.5) and holds what crafted_field() lists; heights are dyadic (a = t, b = t - 1, so a - b = 1 and height = y + t exactly)."""
import functools
import os

import numpy as np

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
import nav_twin as twin
from terrain_twin import bits, sample_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS, SCALE, ORIGIN, SEED = (72, 16, 32), 0.5, (-3.0, 1.0, 2.0), 99
AIR, SOLID = f32(-0.5), f32(0.5)
ULP4, ULP2 = f32(2.0 ** -21), f32(2.0 ** -22)   # one ulp of a height in [4, 8) and in [2, 4)


def world_of(sample, origin=ORIGIN, scale=SCALE):
    """The world position of a sample index triple: exact for these dyadic values, also as float32."""
    w = tuple(origin[k] + sample[k] * scale for k in range(3))
    assert all(float(f32(v)) == v for v in w)
    return w


# name -> (lower, upper) in world space
BOXES = {"far": ((-1e6,) * 3, (1e6,) * 3),                               # clamps to the whole grid
         "interior": (world_of((5, 1, 3)), world_of((71, 13, 25))),       # 67 x 13 x 23 samples: origin and size no multiples of 64, 8 or 4
         "outside": ((1000.0,) * 3, (1010.0,) * 3)}                       # wholly outside the grid: 0 spans
RANDOM_BOXES = {"whole": ((-1e6,) * 3, (1e6,) * 3), "a": (world_of((5, 0, 3)), world_of((70, 17, 20))), "b": (world_of((9, 2, 7)), world_of((41, 14, 33)))}


def floor(g, x, z, y, t=0.5, bottom=0):
    """Column (x, z): solid from `bottom` up to sample y, whose value is t, with t - 1 above it: a floor of height y + t exactly."""
    t = f32(t)
    assert 0 < t <= 1 and f32(t - f32(1)) <= 0 and f32(t - f32(t - f32(1))) == 1
    g[x, bottom:y, z] = SOLID
    g[x, y, z] = t
    g[x, y + 1, z] = f32(t - f32(1))   # t = 1: +0.0f, not solid


def roof(g, x, z, y0, y1):
    g[x, y0:y1 + 1, z] = SOLID


@functools.lru_cache(maxsize=None)
def crafted_field():
    g = np.full(tuple(d + 2 for d in DIMS), AIR, f32)
    g[:, 0:3, :] = SOLID                                   # the flat floor: height 2.5, open above
    # A. staircases along x whose last step is exactly max_step and whose next one is one ulp of the height more
    floor(g, 4, 3, 2, 1.0), floor(g, 5, 3, 3, 0.5), floor(g, 6, 3, 4, ULP4)            # 2.5 | 3.0, 3.5, 4 + ulp: steps 0.5, 0.5, 0.5 + ulp
    floor(g, 4, 6, 3, 0.5), floor(g, 5, 6, 4, f32(0.5) + ULP4)                          # 2.5 | 3.5, 4.5 + ulp: steps 1, 1 + ulp
    floor(g, 4, 9, 4, 1.0), floor(g, 5, 9, 7, f32(0.5) + ULP4)                          # 2.5 | 5.0, 7.5 + ulp: steps 2.5, 2.5 + ulp
    floor(g, 4, 12, 2, f32(0.5) + ULP2)                                                 # 2.5 | 2.5 + ulp: step 0 + ulp
    # B. a cave over the flat floor: ceilings that leave 3, 2, 1 and 0 open samples
    roof(g, 12, 3, 6, 8), roof(g, 13, 3, 5, 8), roof(g, 14, 3, 4, 8), roof(g, 15, 3, 3, 8)
    # C. three stacked floors: the flat floor, a slab at 6..7 and one at 11..12
    roof(g, 20, 3, 6, 7), roof(g, 20, 3, 11, 12)
    # D. a pillar of height 5.5 and, in the column at +x, two spans under and over a gap: at |d| = 2 and 2 (the tie), 1.5 and 2, 2.25 and 1.75
    for z, (t_low, t_up) in ((3, (0.5, 0.5)), (6, (1.0, 0.5)), (9, (0.25, 0.25))):
        floor(g, 26, z, 5)
        floor(g, 27, z, 3, t_low)
        floor(g, 27, z, 7, t_up, bottom=7)
    # E. a one-directional link: (32, 3) holds the flat floor under a slab (ceil 6) and the slab's top (6.5); (33, 3) one span at 5.0, whose
    #    nearest in that column is the slab's top, while the floor under the slab has nothing but it
    roof(g, 32, 3, 6, 6)
    floor(g, 33, 3, 4, 1.0)
    # F. ledges whose common opening with the neighbour is too low although |d| = 1 passes: ceil 4 against height 3.5 (agent_height 1),
    #    ceil 6 against 3.5 (agent_height 3)
    roof(g, 38, 3, 4, 5), floor(g, 39, 3, 3)
    roof(g, 38, 6, 6, 7), floor(g, 39, 6, 3)
    # G. a floating platform (its own region) and a bridge joining two plateaus (one region through it, across x = 64)
    g[44:48, 10, 3:6] = SOLID
    g[52:55, 0:9, 8:13] = SOLID
    g[63:67, 0:9, 8:13] = SOLID
    g[55:63, 8, 10] = SOLID
    # H. a column solid to the top (no floor), and one solid up to sample 13, the interior box's top plane (no floor in that box)
    g[70, :, 3] = SOLID
    g[70, 0:14, 6] = SOLID
    # I. NaN, +0.0f and -0.0f directly above a solid sample, and inside an open run under a roof at 7
    g[10, 3, 16], g[11, 3, 16], g[12, 3, 16] = f32(np.nan), f32(0.0), f32(-0.0)
    for x, v in ((13, f32(np.nan)), (14, f32(0.0)), (15, f32(-0.0))):
        roof(g, x, 16, 7, 7)
        g[x, 5, 16] = v
    # J. a = +inf: a NaN height, listed, never linked
    g[20, 2, 16] = f32(np.inf)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def turned_field():
    g = np.ascontiguousarray(crafted_field().transpose(2, 1, 0))
    g.setflags(write=False)
    return g


def box_of(name, dims=DIMS, scale=SCALE, origin=ORIGIN):
    lower, upper = BOXES[name]
    m = type("M", (), {"lower": [f32(v) for v in lower], "upper": [f32(v) for v in upper]})
    low, up, first, ext = sample_range(m, tuple(d + 2 for d in dims), scale, origin)
    return tuple(first), tuple(ext)


@functools.lru_cache(maxsize=None)
def twin_of(field, box, agent_height, max_step):
    g = {"crafted": crafted_field, "turned": turned_field}[field]()
    dims = tuple(d - 2 for d in g.shape)
    spans, offsets, first, ext = twin.build(g, *box_of(box, dims), agent_height, max_step)
    spans.setflags(write=False)
    offsets.setflags(write=False)
    return spans, offsets, first, ext


def raw_params(agent_height=1, max_step=0.5, max_spans=1 << 20, flags=0):
    return _lib.NavParamsStruct(agent_height, max_step, max_spans, flags)


def raw_field_params(climb=0.0, drop=0.0, max_cost=0x7fffffff, flags=0):
    return _lib.NavFieldParamsStruct(climb, drop, max_cost, flags)


def column(result, x, z):
    """The spans of grid column (x, z) of a build."""
    spans, offsets, first, ext = result
    c = (x - first[0]) + ext[0] * (z - first[2])
    return spans[offsets[c]:offsets[c + 1]], int(offsets[c])


def flat_grid(dx, dz, dy=6):
    g = np.full((dx, dy, dz), AIR, f32)
    g[:, 0:3, :] = SOLID
    return g


def nav_of(g, max_step=0.5):
    return twin.build(g, (0, 0, 0), g.shape, 1, max_step)


def world(g):
    """World positions (float32, exact) of grid positions whose halves are float32 numbers."""
    g = np.asarray(g, np.float64).reshape(-1, 3)
    w = np.asarray(ORIGIN, np.float64) + g * SCALE
    assert np.array_equal(w.astype(f32).astype(np.float64), w)
    return w.astype(f32)


def largest_region(spans):
    regions, counts = np.unique(spans["region"], return_counts=True)
    return int(regions[np.argmax(counts)]), regions


def speeds_of(count):
    """The speeds of a crowd of `count` agents, 300..1799 cost units per tick: below and above a level step's 1024."""
    return [300 + (7919 * i) % 1500 for i in range(count)]


def same_cells(a, b):
    return a.dtype == b.dtype == vt.NAVFIELD_CELL_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


# -- GPU --------------------------------------------------------------------------------------------------------------------------------------
def terrain(grid=None, dims=DIMS):
    ex = vt.Extractor(0)
    ex.terrain_init(*dims, SCALE, ORIGIN, SEED)
    if grid is not None:
        ex.terrain_write_samples(grid)
    return ex


def assert_same(got, want, what):
    assert got[2] == want[2] and got[3] == want[3], what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), what
    assert len(got[0]) == len(want[0]), what
    nan = np.isnan(want[0]["height"])
    if nan.any():   # the a = +inf span: a NaN-aware equality for its height only
        assert twin.nan_aware_equal(got[0], want[0]) and twin.same_bytes(got[0][~nan], want[0][~nan]), what
    else:
        assert twin.same_bytes(got[0], want[0]), what


def held(ex, L, h):
    """Everything the context holds besides the nav result, as bytes."""
    tris, offs = ex.read_triangles()
    n = ex.last_counts()[1] * 3
    mat, ao = np.zeros((n, 8), np.uint8), np.zeros(n, np.uint8)
    assert L.vtmc_material_read_vertices(h, mat.ctypes.data, n) == 0 and L.vtmc_ao_read_vertices(h, ao.ctypes.data, n) == 0
    p, o, ni = ex.device_scatter()
    inst, ioffs = np.zeros(ni, vt.INSTANCE_DTYPE), np.zeros(len(offs), np.int32)
    assert L.vtmc_scatter_read(h, inst.ctypes.data, ni, ioffs.ctypes.data) == 0
    return [bits(ex.terrain_read_samples()).tobytes(), ex.terrain_history(), ex.terrain_dirty_blocks().tobytes(), tris.tobytes(), offs.tobytes(),
            mat.tobytes(), ao.tobytes(), inst.tobytes(), ioffs.tobytes(), (p, o, ni)]


def mirror_world(ex):
    """The world host/host_selftest.cpp builds for its --gpu-nav* modes, set up on `ex`; returns its nav result."""
    ex.terrain_init(64, 32, 32, 0.5, (-3.0, 1.0, 2.0), 977)
    ex.terrain_update([vt.PlaneModifier(6.3, (-100.0, -100.0), (100.0, 100.0)), vt.SphereModifier((27.5, 8.0, 10.0), 4.25, True),
                       vt.SphereModifier((5.0, 6.0, 9.0), 3.0, False)])
    return ex.terrain_nav((-1.0, 1.0, 3.0), (14.0, 15.0, 16.5), vt.NavParams(0.9, 0.4))
