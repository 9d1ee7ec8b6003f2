"""Mesh stamps (vtmc_stamp_from_mesh): a closed triangle mesh voxelized on the device, every stamp bit for bit -- the sign of a zero
included -- against the twin of mesh_twin.py, a numpy restatement of include/vtmc.h's rule that takes every triangle at every sample.

That yardstick is itself checked here on the CPU without the code under test: distances and signs of boxes and of an icosphere against
their analytic values, and the rule's independence of the order of vertices and triangles."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
from volumetricterrain_amd.modifiers import mesh_stamp_args, mesh_stamp_box
import terrain_twin
from terrain_twin import assert_grid, bits
import stamp_twin
import mesh_twin
from host_check import run_host_check
from mesh_twin import box, concat, icosphere, torus, voxelize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
BOX = ((2.0, 2.0, 2.0), (6.0, 6.0, 6.0))
OFFSET = (0.37, 0.41, 0.29)
SPHERE_R, SPHERE_C = 3.5, (4.25, 4.5, 3.75)


# -- the cases: (mesh, first, pitch, dims); each twin stamp is computed once and shared, read-only ------------------------------------------
def case(name):
    if name == "box_lattice":
        return box(*BOX), (0.0, 0.0, 0.0), 1.0, (9, 9, 9)
    if name == "box_offset":
        return box(*BOX), OFFSET, 1.0, (9, 9, 9)
    if name == "sphere":
        return icosphere(2, SPHERE_R, SPHERE_C), (0.0, 0.0, 0.0), 1.0, (9, 10, 8)
    if name == "tails":      # 70 x 9 x 6: an x tail past 64, a y-run that ends after 9 of its 16 samples, a z tail past 4
        return icosphere(2, 3.2, (33.3, 4.1, 2.9)), (-1.7, -0.4, -0.6), 1.0, (70, 9, 6)
    if name == "smallest":
        return icosphere(2, 0.9, (0.4, 0.6, 0.5)), (0.0, 0.0, 0.0), 1.0, (2, 2, 2)
    if name == "three":      # 2 816 triangles = 11 chunks; the pieces lie at opposite ends, so most tiles skip most chunks
        mesh = concat(icosphere(3, 7.0, (10.0, 20.0, 20.0)), icosphere(3, 6.0, (84.0, 19.0, 21.0)), torus(8.0, 3.0, 16, 8, (48.0, 20.0, 20.0)))
        return mesh, (0.25, 0.5, 0.125), 1.0, (96, 40, 40)
    if name == "deep_inside":
        return box((-500.0, -400.0, -300.0), (600.0, 500.0, 400.0)), (10.0, 20.0, 30.0), 0.5, (16, 16, 16)
    if name == "far_outside":
        return box((-500.0, -400.0, -300.0), (600.0, 500.0, 400.0)), (700.0, 20.0, 30.0), 0.5, (16, 16, 16)
    if name == "far_behind":   # outside, with the whole mesh in front along +x: two faces cover every sample
        return box((-500.0, -400.0, -300.0), (600.0, 500.0, 400.0)), (-700.0, 20.0, 30.0), 0.5, (16, 16, 16)
    if name == "open_box":   # one triangle missing: refused unless trusted; the rule is defined for any triangle set
        (v, t), first, pitch, dims = case("box_offset")
        return (v, t[1:]), first, pitch, dims
    if name == "rock":       # what the paste test voxelizes
        v, t = icosphere(2, 5.0, (0.3, -0.2, 0.1))
        first, dims, _ = mesh_stamp_box(v, 1.0, margin=3)
        return (v, t), tuple(first), 1.0, dims
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def twin_stamp(name):
    (v, t), first, pitch, dims = case(name)
    s = voxelize(v, t, first, pitch, dims)
    s.setflags(write=False)
    return s


def sample_points(first, pitch, dims):
    """The float32 sample positions as float64 arrays [x, y, z, 3]."""
    px, py, pz = mesh_twin.positions(first, pitch, dims)
    return np.stack(np.meshgrid(px.astype(f64), py.astype(f64), pz.astype(f64), indexing="ij"), axis=-1)


def box_distance(p, lo, hi):
    """Analytic distance of points p [..., 3] to the surface of the box, float64, and whether they are strictly inside / outside."""
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    out = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    d_out = np.sqrt((out * out).sum(axis=-1))
    d_in = np.minimum(p - lo, hi - p).min(axis=-1)
    inside = (d_in > 0)
    return np.where(inside, d_in, d_out), inside, d_out > 0


# -- CPU: the interface --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_its_constants():
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    assert "vtmc_stamp_from_mesh" in _lib.SYMBOLS
    assert int(re.search(r"#define\s+VTMC_MESH_MAX_TRIANGLES\s+\(1 << (\d+)\)", text).group(1)) == 20 and _lib.MESH_MAX_TRIANGLES == 1 << 20
    assert float(re.search(r"#define\s+VTMC_MESH_BAND\s+([0-9.]+)f", text).group(1)) == _lib.MESH_BAND == 3.0
    assert int(re.search(r"#define\s+VTMC_MESH_TRUST_CLOSED\s+(\d+)u", text).group(1)) == _lib.MESH_TRUST_CLOSED == 1
    lib = vt.load()
    assert hasattr(lib, "vtmc_stamp_from_mesh")
    assert lib.vtmc_stamp_from_mesh(None, None, 0, None, 0, None, 1.0, 2, 2, 2, 0, None) == _lib.ERR_INVALID_ARG   # a status code, no crash


def test_mesh_stamp_box_round_trips():
    v, _ = icosphere(1, 2.3, (5.1, -3.7, 0.4))
    for pitch, margin in ((0.25, 4), (1.0, 0), (0.37, 2)):
        first, dims, centre = mesh_stamp_box(v, pitch, margin)
        h = float(f32(pitch))
        last = first.astype(f64) + h * (np.array(dims) - 1)
        # the lattice of the pitch, the mesh inside by the margin and by less than a sample more
        assert np.abs(first / h - np.round(first / h)).max() < 1e-4
        assert (v.min(axis=0) - first >= margin * h - 1e-5).all() and (v.min(axis=0) - first < (margin + 1) * h + 1e-5).all()
        assert (last - v.max(axis=0) >= margin * h - 1e-5).all() and (last - v.max(axis=0) < (margin + 1) * h + 1e-5).all()
        # a paste at `centre` with this pitch has sample i at centre + h * (i - (n - 1) / 2): back where it was voxelized
        back = centre.astype(f64) - h * (np.array(dims) - 1) / 2
        assert np.abs(back - first).max() <= 2 * np.spacing(np.abs(centre).max())
        assert first.dtype == centre.dtype == f32 and all(isinstance(n, int) for n in dims)
    with pytest.raises(ValueError):
        mesh_stamp_box(v, 0.0)
    with pytest.raises(ValueError):
        mesh_stamp_box(v, 1e-3)   # more than 1026 samples along an axis


V8, T12 = box(*BOX)


@pytest.mark.parametrize("kw", [dict(vertices=V8[:2]), dict(vertices=V8[:, :2]), dict(triangles=T12[:0]), dict(triangles=T12[:, :2]), dict(triangles=T12.astype(f32)),
                                dict(triangles=np.where(T12 == 7, 8, T12)), dict(triangles=np.where(T12 == 0, -1, T12)),
                                dict(vertices=np.where(V8 == 6, np.nan, V8)), dict(vertices=np.where(V8 == 6, np.inf, V8)),
                                dict(vertices=np.where(V8 == 6, 2.0 ** 20 + 1, V8)), dict(first=(0.0, np.nan, 0.0)), dict(first=(0.0, 0.0)),
                                dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=np.nan), dict(pitch=np.inf), dict(dims=(1, 9, 9)), dict(dims=(9, 1027, 9)),
                                dict(dims=(1026, 1026, 1026)), dict(dims=(9, 9))])
def test_python_checks_raise_value_error(kw):
    args = dict(vertices=V8, triangles=T12, first=(0.0, 0.0, 0.0), pitch=1.0, dims=(9, 9, 9))
    mesh_stamp_args(**args)
    args.update(kw)
    with pytest.raises(ValueError):
        mesh_stamp_args(**args)


def test_builders_make_closed_meshes():
    for (v, t), n in ((box(*BOX), 12), (icosphere(2), 320), (icosphere(3), 1280), (torus(8.0, 3.0, 16, 8), 256), (case("three")[0], 2816)):
        assert len(t) == n and t.max() == len(v) - 1 and mesh_twin.is_closed(t)
    assert not mesh_twin.is_closed(case("open_box")[0][1])


# -- CPU: the yardstick, without the code under test -------------------------------------------------------------------------------------
def test_twin_lattice_aligned_box_is_exact():
    """Rays run exactly through the faces' boundary edges, their diagonals and the corners; every value is a small integer or its root."""
    (v, t), first, pitch, dims = case("box_lattice")
    s = twin_stamp("box_lattice")
    d, inside, outside = box_distance(sample_points(first, pitch, dims), *BOX)
    want = np.minimum(np.sqrt((d * d).round().astype(f32)), f32(3))   # d^2 is a whole number: its float32 root, correctly rounded
    assert np.array_equal(np.abs(s), want)
    assert (s[inside] > 0).all() and (s[outside] < 0).all() and inside.sum() == 27 and outside.sum() == 9 ** 3 - 5 ** 3
    assert (s[~inside & ~outside] == 0).all()


def test_twin_offset_box_sign_exact_distance_within_an_ulp():
    (v, t), first, pitch, dims = case("box_offset")
    s = twin_stamp("box_offset")
    d, inside, outside = box_distance(sample_points(first, pitch, dims), *BOX)
    assert (inside | outside).all() and inside.sum() == 64
    assert (s[inside] > 0).all() and (s[outside] < 0).all()
    want = np.minimum(d, 3.0).astype(f32)
    err = np.abs(np.abs(s).astype(f64) - want.astype(f64)) / np.spacing(want).astype(f64)
    print("max |twin - analytic| = %.3g ulp" % err.max())
    assert err.max() <= 1.0


def test_twin_icosphere_sign_is_analytic_beyond_the_sag():
    (v, t), first, pitch, dims = case("sphere")
    assert len(t) == 320
    s = twin_stamp("sphere")
    centroids = v[t].astype(f64).mean(axis=1) - np.array(SPHERE_C)
    sag = SPHERE_R - np.sqrt((centroids ** 2).sum(axis=1)).min()
    r = np.sqrt(((sample_points(first, pitch, dims) - np.array(SPHERE_C)) ** 2).sum(axis=-1))
    clear = np.abs(r - SPHERE_R) > sag
    assert 0 < sag < 0.2 and clear.sum() > 0.9 * clear.size and (r < SPHERE_R - sag).sum() > 100
    assert np.array_equal(s[clear] > 0, r[clear] < SPHERE_R)
    # and the distance: the mesh lies between the sphere and the sphere drawn in by its deepest face plane
    tv = v[t].astype(f64) - np.array(SPHERE_C)
    n = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    deepest = SPHERE_R - (np.abs((n * tv[:, 0]).sum(axis=1)) / np.sqrt((n * n).sum(axis=1))).min()
    near = np.abs(s) < 3
    assert near.sum() > 300 and np.abs(np.abs(s[near]) - np.abs(r[near] - SPHERE_R)).max() <= deepest + 1e-5


@pytest.mark.parametrize("name", ["box_lattice", "sphere"])
def test_twin_does_not_depend_on_vertex_or_triangle_order(name):
    (v, t), first, pitch, dims = case(name)
    rng = np.random.default_rng(5)
    orders = np.array([(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)])
    t2 = np.take_along_axis(t, orders[rng.integers(0, 6, len(t))], axis=1)[rng.permutation(len(t))]
    assert not np.array_equal(t, t2)
    d1, in1 = mesh_twin.distance_and_sign(v, t, first, pitch, dims)
    d2, in2 = mesh_twin.distance_and_sign(v, t2, first, pitch, dims)
    assert np.array_equal(bits(d1), bits(d2)) and np.array_equal(in1, in2)
    assert np.array_equal(bits(voxelize(v, t2, first, pitch, dims)), bits(twin_stamp(name)))


def test_twin_far_mesh_saturates():
    assert (twin_stamp("deep_inside") == 3).all() and (twin_stamp("far_outside") == -3).all() and (twin_stamp("far_behind") == -3).all()


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/mesh_host_check.cpp: the host half (csrc/mesh_host.h) as a stand-alone program under ASan and UBSan, on the CPU."""
    run_host_check("mesh_host_check", tmp_path)


# -- GPU --------------------------------------------------------------------------------------------------------------------------------
def gpu_stamp(ex, name, trust_closed=False):
    (v, t), first, pitch, dims = case(name)
    sid = ex.stamp_from_mesh(v, t, first, pitch, dims, trust_closed=trust_closed)
    assert ex.stamp_dims(sid) == tuple(dims)
    return sid


def assert_stamp(ex, sid, name):
    got, want = ex.stamp_read(sid), twin_stamp(name)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%d of %d samples differ, the first at %r: %r != %r" % (diff.sum(), diff.size, tuple(np.argwhere(diff)[0]), got[diff][0], want[diff][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box_lattice", "box_offset"])
def test_gpu_box_mesh(name):
    with vt.Extractor(0) as ex:   # no terrain: the call needs none
        assert_stamp(ex, gpu_stamp(ex, name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tails", "smallest", "sphere"])
def test_gpu_tile_tails(name):
    """70 x 9 x 6: a second tile along x with 6 live lanes, a y-run of 9 of its 16 samples, a second z quad with 2 live waves -- at
    once.  2 x 2 x 2: the smallest legal stamp."""
    with vt.Extractor(0) as ex:
        assert_stamp(ex, gpu_stamp(ex, name), name)
    s = twin_stamp(name)
    assert (s > 0).any() and (s < 0).any()


@pytest.mark.gpu
def test_gpu_several_chunks_and_skipped_chunks():
    """Two icospheres of 1 280 triangles and a torus, far apart in a 96 x 40 x 40 stamp: 11 chunks of triangles, survivor lists that differ
    from tile to tile, chunks that whole workgroups skip.  The twin takes every triangle at every sample: equality is the proof that the
    pruning is exact."""
    s = twin_stamp("three")
    assert (s == 3).any() and (s == -3).sum() > s.size // 4 and (np.abs(s) < 3).sum() > 10000
    with vt.Extractor(0) as ex:
        assert_stamp(ex, gpu_stamp(ex, "three"), "three")


@pytest.mark.gpu
@pytest.mark.parametrize("name, value", [("deep_inside", 3.0), ("far_outside", -3.0), ("far_behind", -3.0)])
def test_gpu_mesh_far_larger_than_the_stamp(name, value):
    """No triangle survives the distance test, and the parity is still right."""
    with vt.Extractor(0) as ex:
        sid = gpu_stamp(ex, name)
        assert (ex.stamp_read(sid) == f32(value)).all()
        assert_stamp(ex, sid, name)


WORLD = [("plane", (9.3, (-10, -10), (50, 50), True)), ("sphere", ((20.0, 12.0, 14.0), 4.2, True))]
SKEW = (0.3, -0.5, 0.2, 0.79)


def world(oracle_mod, history=0):
    return terrain_twin.world(oracle_mod, (32, 32, 32), 1.0, (0.0, 0.0, 0.0), 97, WORLD, history)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["add", "replace"])
def test_gpu_paste_of_a_mesh_stamp(oracle_mod, mode):
    ex, ref = world(oracle_mod, 32 << 20)
    with ex:
        sid = gpu_stamp(ex, "rock")
        s = twin_stamp("rock")
        assert_stamp(ex, sid, "rock")
        before = ex.terrain_read_samples().copy()
        spec = ("stamp", dict(stamp_id=sid, dims=s.shape, position=(14.5, 11.0, 17.25), rotation=SKEW, pitch=0.8, mode=mode))
        n_dirty, T = stamp_twin.assert_update(ex, ref, oracle_mod, [spec], {sid: s})   # the twin-made samples stand for the stamp
        assert n_dirty > 0 and T > 0 and not np.array_equal(bits(ex.terrain_read_samples()), bits(before))
        ex.terrain_undo()
        assert_grid(ex, before)


@pytest.mark.gpu
def test_gpu_call_leaves_the_session_alone(oracle_mod):
    a, _ = world(oracle_mod, 32 << 20)
    b, _ = world(oracle_mod, 32 << 20)
    edit = [vt.SphereModifier((11.0, 9.0, 20.0), 5.5, False).to_struct()]
    with a, b:
        a.terrain_update(edit)
        b.terrain_update(edit)
        ids = [gpu_stamp(a, "box_offset"), gpu_stamp(a, "smallest")]
        assert ids == [1, 2] and a.stamp_dims(2) == (2, 2, 2)
        assert np.array_equal(bits(a.terrain_read_samples()), bits(b.terrain_read_samples()))
        assert a.terrain_history() == b.terrain_history() and a.last_counts() == b.last_counts()
        assert np.array_equal(a.terrain_dirty_blocks(), b.terrain_dirty_blocks())
        a.stamp_destroy(1)
        assert gpu_stamp(a, "box_lattice") == 3   # ids count up and are not reused
        assert_stamp(a, 3, "box_lattice")
        more = [vt.SphereModifier((20.0, 14.0, 10.0), 6.0, True).to_struct()]   # the next update draws its clamps with the same event number
        assert a.terrain_update(more) == b.terrain_update(more)
        assert np.array_equal(bits(a.terrain_read_samples()), bits(b.terrain_read_samples()))
        assert a.terrain_history() == b.terrain_history()


def raw_call(ex, v, t, first, pitch, dims, flags=0, n_vertices=None, n_triangles=None, null=()):
    """vtmc_stamp_from_mesh itself, past the mirror's checks; returns (status, id written)."""
    v, t = np.ascontiguousarray(v, f32), np.ascontiguousarray(t, np.int32)
    sid = ctypes.c_int32(-7)
    ptr = dict(positions=v.ctypes.data_as(ctypes.c_void_p), indices=t.ctypes.data_as(ctypes.c_void_p), first=ctypes.byref((ctypes.c_float * 3)(*first)),
               stamp_id=ctypes.byref(sid))
    for k in null:
        ptr[k] = None
    rc = ex._L.vtmc_stamp_from_mesh(ex._h, ptr["positions"], len(v) if n_vertices is None else n_vertices, ptr["indices"],
                                    len(t) if n_triangles is None else n_triangles, ptr["first"], pitch, *dims, flags, ptr["stamp_id"])
    return rc, sid.value


@pytest.mark.gpu
def test_gpu_refusals():
    (v, t), first, pitch, dims = case("box_offset")
    ok = dict(v=v, t=t, first=first, pitch=pitch, dims=dims)
    bad = [dict(null=("positions",)), dict(null=("indices",)), dict(null=("first",)), dict(null=("stamp_id",)),
           dict(n_triangles=0), dict(n_triangles=-1), dict(n_triangles=(1 << 20) + 1), dict(n_vertices=2), dict(n_vertices=7),
           dict(t=np.where(t == 3, -1, t)), dict(t=np.where(t == 3, 8, t)),
           dict(v=np.where(v == 6, np.nan, v)), dict(v=np.where(v == 6, -np.inf, v)), dict(v=np.where(v == 6, 2.0 ** 20 + 1, v)),
           dict(first=(0.0, np.inf, 0.0)), dict(first=(np.nan, 0.0, 0.0)), dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=np.nan), dict(pitch=np.inf),
           dict(dims=(1, 9, 9)), dict(dims=(9, 1027, 9)), dict(dims=(1026, 1026, 1026)), dict(dims=(9, 9, 0)), dict(flags=2), dict(flags=1 << 31),
           dict(t=t[1:]), dict(t=np.concatenate([t, t[:1]]))]
    with vt.Extractor(0) as ex:
        kept = gpu_stamp(ex, "smallest")
        for kw in bad:
            rc, sid = raw_call(ex, **{**ok, **kw})
            assert rc == _lib.ERR_INVALID_ARG and sid == -7, kw
        rc, _ = raw_call(ex, **{**ok, "t": t[1:]})
        text = ex._L.vtmc_last_error(ex._h).decode()
        assert rc == _lib.ERR_INVALID_ARG and "not closed" in text and re.search(r"edge \(\d+, \d+\) is used by 1 ", text), text
        assert_stamp(ex, kept, "smallest")   # existing stamps stay readable
        assert gpu_stamp(ex, "box_offset") == kept + 1   # a refused call takes no id
        # a triangle that repeats an index is dropped by the check, not by the rule
        rc, sid = raw_call(ex, **{**ok, "t": np.concatenate([t, [[0, 0, 5]]])})
        assert rc == 0 and sid == kept + 2
        with pytest.raises(vt.VtmcError):
            gpu_stamp(ex, "open_box")
        assert_stamp(ex, gpu_stamp(ex, "open_box", trust_closed=True), "open_box")
