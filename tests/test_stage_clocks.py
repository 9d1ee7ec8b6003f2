"""The stage clocks of the context (csrc/vtmc_ctx.h: StageClock): the timing events around the kernels of the density fill, the
level-of-detail gather, the scatter, the navigation build and the flow field, read through vtmc_last_fill_ms and the vtmc_debug_*_ms
functions.  What is pinned here is WHEN a clock answers and when it refuses with VTMC_ERR_NO_RESULT, the meaning of the rounds slots, and
that a context's events go with it; the times themselves are only required to be finite and not negative.

The navigation build reports its rounds nowhere but in ms[7] of vtmc_debug_nav_ms, so that slot is held against the library's own bound
(a whole number of rounds, 1..8: kNavMaxRounds of terrain_nav.hip); the flow field's ms[3] against vtmc_navfield_info."""
import ctypes
import math

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib

pytestmark = pytest.mark.gpu

N = 16                                     # cells per axis of the resident terrain
NAV = vt.NavParams(1.0, 1.0)
WHOLE = ((-1e6,) * 3, (1e6,) * 3)        # world bounds that clamp to every sample
OUTSIDE = ((1e5,) * 3, (2e5,) * 3)         # world bounds that clamp to no sample of the terrain
NAV_MAX_ROUNDS = 8


def world():
    """A context whose resident terrain holds a plane minus a sphere, extracted: the result has triangles."""
    ex = vt.Extractor(0)
    ex.terrain_init(N, N, N, 1.0, (0.0, 0.0, 0.0), 3)
    _, T = ex.terrain_update([vt.PlaneModifier(5.375, (0, 0), (20, 20), True), vt.SphereModifier((8.0, 6.0, 8.0), 3.5, False)])
    assert T > 0
    return ex


def read(ex, name, slots):
    """(return code, the ms[] values) of one of the clock readers."""
    ms = (ctypes.c_float * slots)()
    return getattr(ex._L, name)(ex._h, ms), list(ms)


READERS = (("vtmc_last_fill_ms", 1), ("vtmc_debug_lod_gather_ms", 1), ("vtmc_debug_scatter_ms", 4), ("vtmc_debug_nav_ms", 8), ("vtmc_debug_navfield_ms", 4))


def refuses(ex, name, slots):
    rc, _ = read(ex, name, slots)
    assert rc == _lib.ERR_NO_RESULT, (name, rc)
    assert ex._L.vtmc_last_error(ex._h).decode() != ""


def times(ex, name, slots, n_times):
    rc, ms = read(ex, name, slots)
    assert rc == 0, (name, rc, ex._L.vtmc_last_error(ex._h).decode())
    assert all(math.isfinite(v) and v >= 0.0 for v in ms[:n_times]), (name, ms)
    return ms


def test_a_fresh_context_refuses_every_clock():
    with vt.Extractor(0) as ex:
        for name, slots in READERS:
            refuses(ex, name, slots)


def test_every_clock_answers_after_its_pass():
    import torch
    with world() as ex:
        # the passes have not run on this context either: a terrain update is none of them
        for name, slots in READERS:
            refuses(ex, name, slots)
        d = torch.empty(N ** 3, dtype=torch.float32, device="cuda")
        ex.density_fill_device(vt.density_params("perlin3d", N), [[0, 0, 0]], (N, N, N), (1, N, N * N), 0, d.data_ptr())
        times(ex, "vtmc_last_fill_ms", 1, 1)
        inst, _ = ex.scatter_surface(vt.ScatterParams(1.0))
        assert len(inst) > 0
        times(ex, "vtmc_debug_scatter_ms", 4, 4)
        spans, _, _, dims = ex.terrain_nav(*WHOLE, params=NAV)
        assert len(spans) > 0 and dims == (N + 2,) * 3
        ms = times(ex, "vtmc_debug_nav_ms", 8, 7)
        assert ms[7] == int(ms[7]) and 1 <= ms[7] <= NAV_MAX_ROUNDS
        refuses(ex, "vtmc_debug_navfield_ms", 4)   # a nav build is no field
        ex.nav_field([0], vt.NavFieldParams(1.0, 0.25))
        ms = times(ex, "vtmc_debug_navfield_ms", 4, 3)
        n, reached, rounds = ex.navfield_info()
        assert n == len(spans) and reached >= 1 and rounds >= 1 and ms[3] == float(rounds)
        nodes, T = ex.terrain_extract_lod((8.0, 6.0, 8.0), 1)
        assert nodes > 0 and T > 0
        times(ex, "vtmc_debug_lod_gather_ms", 1, 1)
        # the clocks are independent: the later passes took nothing from the earlier ones
        times(ex, "vtmc_last_fill_ms", 1, 1)
        times(ex, "vtmc_debug_scatter_ms", 4, 4)
        times(ex, "vtmc_debug_nav_ms", 8, 7)


def test_an_empty_nav_box_disarms_the_nav_clock():
    with world() as ex:
        assert len(ex.terrain_nav(*WHOLE, params=NAV)[0]) > 0
        times(ex, "vtmc_debug_nav_ms", 8, 7)
        spans, offsets, _, dims = ex.terrain_nav(*OUTSIDE, params=NAV)
        assert len(spans) == 0 and dims == (0, 0, 0) and list(offsets) == [0]
        refuses(ex, "vtmc_debug_nav_ms", 8)
        assert len(ex.terrain_nav(*WHOLE, params=NAV)[0]) > 0   # and a build that launches kernels arms it again
        times(ex, "vtmc_debug_nav_ms", 8, 7)


def test_a_scatter_over_no_triangles_disarms_the_scatter_clock():
    with world() as ex:
        assert len(ex.scatter_surface(vt.ScatterParams(1.0))[0]) > 0
        times(ex, "vtmc_debug_scatter_ms", 4, 4)
        n_dirty, T = ex.terrain_update([vt.SphereModifier((8.0, 14.0, 8.0), 1.0, False)])   # an edit in the air: its blocks hold no surface
        assert n_dirty > 0 and T == 0
        inst, offsets = ex.scatter_surface(vt.ScatterParams(1.0))
        assert len(inst) == 0 and not offsets.any()
        refuses(ex, "vtmc_debug_scatter_ms", 4)


def test_the_box_read_borrows_the_nav_clock_and_leaves_the_build():
    with world() as ex:
        spans, offsets, first, dims = ex.terrain_nav(*WHOLE, params=NAV)
        times(ex, "vtmc_debug_nav_ms", 8, 7)
        lo, up, ms = (ctypes.c_float * 3)(*WHOLE[0]), (ctypes.c_float * 3)(*WHOLE[1]), ctypes.c_float(-1.0)
        ex._check(ex._L.vtmc_debug_nav_box_read_ms(ex._h, ctypes.byref(lo), ctypes.byref(up), 3, ctypes.byref(ms)))
        assert math.isfinite(ms.value) and ms.value >= 0.0
        refuses(ex, "vtmc_debug_nav_ms", 8)
        f, d, n = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32()
        ex._check(ex._L.vtmc_nav_info(ex._h, ctypes.byref(f), ctypes.byref(d), ctypes.byref(n)))
        assert (tuple(f), tuple(d), n.value) == (first, dims, len(spans))
        again = ex.nav_read()
        assert again[0].tobytes() == spans.tobytes() and np.array_equal(again[1], offsets)


def test_contexts_take_their_clocks_with_them():
    for _ in range(8):
        ex = world()
        assert len(ex.terrain_nav(*WHOLE, params=NAV)[0]) > 0
        times(ex, "vtmc_debug_nav_ms", 8, 7)
        ex.close()
