"""VTMC_MOD_EROSION (include/vtmc_erosion.h): hydraulic and thermal erosion of the resident terrain, simulated on the device.

The yardstick is erosion_twin.py, the header's rule in numpy float32, operation by operation.  The CPU tests hold the twin to the
properties the rule promises (a flat floor stays flat, mirrors and the transpose commute with it bit for bit, terrain plus sediment is
conserved, the write-back reads back exactly); the GPU tests hold the library to the twin as raw bytes: the grid, the five maps and
the report."""
import ctypes
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib, modifiers
from volumetricterrain_amd import terrainfile as tf
import erosion_twin as twin
from erosion_support import DIMS, MAPS, NX, NZ, ORIGIN, P, SCALE, SEED, WHOLE, World, craft_grid, dirty_ids, erode_and_compare, erosion, plane, world_of
from host_check import run_host_check
from terrain_twin import bits, block_list, invalid, no_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# -- CPU: the header, the binding, the mirror, the documents, the host half ----------------------------------------------------------------
def test_header_declares_the_layer():
    S = _header.LAYERS["erosion"]
    assert S.constants == {"VTMC_MOD_EROSION": 12, "VTMC_EROSION_G": 9.81, "VTMC_EROSION_SIN_MIN": 0.05, "VTMC_EROSION_DEPTH_EPS": 1e-4,
                           "VTMC_EROSION_MAX_ITERATIONS": 65536, "VTMC_EROSION_MAX_RAIN": 256.0, "VTMC_EROSION_MAX_CAPACITY": 65536.0,
                           "VTMC_EROSION_MAX_THERMAL": 0.125, "VTMC_EROSION_HEIGHT_BEFORE": 0, "VTMC_EROSION_HEIGHT_AFTER": 1,
                           "VTMC_EROSION_WATER": 2, "VTMC_EROSION_SEDIMENT": 3, "VTMC_EROSION_ACTIVE": 4}
    assert (_lib.MOD_EROSION, _lib.EROSION_G, _lib.EROSION_SIN_MIN, _lib.EROSION_DEPTH_EPS) == (12, twin.G, twin.SIN_MIN, twin.DEPTH_EPS)
    assert vt.ErosionModifier.kind == 12 and modifiers.MOD_EROSION == 12
    names = ["vtmc_erosion_info", "vtmc_erosion_read", "vtmc_erosion_device_results"]
    assert list(S.prototypes) == names == _lib.LAYER_SYMBOLS["erosion"]
    VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert [S.prototypes[n].argtypes for n in names] == [[VP, VP], [VP, I32, VP, I64], [VP] * 6]
    assert set(S.structs) == {"vtmc_erosion_report"} and ctypes.sizeof(_lib.ErosionReport) == 48
    assert [f for f, _ in _lib.ErosionReport._fields_] == ["lo", "hi", "nx", "nz", "iterations", "n_active", "n_rewritten", "n_clamped"]
    core = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    assert "VTMC_MOD_EROSION" not in core and not re.search(r"#define\s+VTMC_MOD_\w+\s+(6|7|12)\b", core)   # the kind lives in the layer's header
    assert '("erosion", "vtmc_erosion.h", "core", "EROSION.md")' in open(os.path.join(ROOT, "volumetricterrain_amd", "build.py")).read()


RULE_WORDS = ("EROSION: the rule", "PAIRED", "sum4", "Heights", "ACTIVE", "WALLS", "Neighbour", "COUNTS", "Flux", "Water", "Speed", "Erosion",
              "Transport", "Evaporate", "Thermal", "Write-back", "n_clamped", "NOT put down", "Why the caps", "OUT OF SCOPE")


def test_the_rule_words_of_the_header_appear_in_the_document():
    rule, doc = open(_header.LAYERS["erosion"].path).read(), open(os.path.join(ROOT, "EROSION.md")).read()
    for word in RULE_WORDS:
        assert word in rule, word
        assert word in doc, word
    for word in ("noise", "erode", "paint", "flood", "box height", "What it costs", "Limits", "overhang", "cave roof", "closed borders", "snapshot"):
        assert word in doc, word
    for linking in ("README.md", "INTEGRATION.md"):
        assert "EROSION.md" in open(os.path.join(ROOT, linking)).read(), linking
    assert "include/vtmc_erosion.h" in open(os.path.join(ROOT, "README.md")).read()


def test_mirror_fills_the_struct():
    m = vt.ErosionModifier((1.0, 2.0, 3.0), (40.5, 20.0, 30.25), 77, rain=0.5, evaporation=0.25, capacity=2.0, dissolve=0.75, deposit=0.125,
                           dt=0.5, talus=1.5, thermal_rate=0.0625).to_struct()
    assert (m.kind, tuple(m.data_dims), bool(m.data)) == (12, (77, 0), False)
    assert tuple(m.lower) == (1.0, 2.0, 3.0) and tuple(m.upper) == (40.5, 20.0, 30.25)
    assert tuple(m.p) == (0.5, 0.25, 2.0, 0.75, 0.125, 0.5, 1.5, 0.0625)
    whole = vt.ErosionModifier(None, None, 1).to_struct()
    assert all(v == -np.inf for v in whole.lower) and all(v == np.inf for v in whole.upper)
    for name in ("erosion_info", "erosion_read", "device_erosion"):
        assert callable(getattr(vt.Extractor, name)), name


# every refusal of csrc/terrain_erosion.h's erosion_args_fault that a value can cause: what to change, and the library's word for it
REFUSALS = [(dict(rain=np.nan), "not finite"), (dict(dt=np.inf), "not finite"), (dict(talus=-np.inf), "not finite"), (dict(capacity=1e300), "not finite"),
            (dict(rain=-0.01), "negative"), (dict(evaporation=-1.0), "negative"), (dict(talus=-0.5), "negative"), (dict(thermal_rate=-0.01), "negative"),
            (dict(rain=256.5), "rain above"), (dict(capacity=65537.0), "capacity above"), (dict(dissolve=1.01), "dissolve outside"),
            (dict(deposit=1.5), "deposit outside"), (dict(dt=0.0), "dt outside"), (dict(dt=1.25), "dt outside"),
            (dict(thermal_rate=0.126), "thermal rate above"), (dict(evaporation=4.5, dt=0.25), "evaporation \\* dt above 1"),
            (dict(iterations=0), "iterations outside"), (dict(iterations=65537), "iterations outside"), (dict(iterations=-3), "iterations outside")]


def mirror_args(change):
    kw = dict(lower=None, upper=None, iterations=4, **P._asdict())
    kw.update(change)
    return kw


@pytest.mark.parametrize("change,word", REFUSALS)
def test_mirror_rejects_what_the_library_rejects(change, word):
    with pytest.raises(ValueError, match="erosion .*" + word):
        vt.ErosionModifier(**mirror_args(change))
    with pytest.raises(ValueError):
        vt.ErosionModifier(lower=(np.nan, 0, 0), upper=None, iterations=1)
    with pytest.raises(ValueError, match="iterations"):
        vt.ErosionModifier(None, None, 2.5)


def test_mirror_accepts_the_limits():
    for change in (dict(rain=256.0), dict(capacity=65536.0), dict(dissolve=1.0, deposit=1.0), dict(dt=1.0, evaporation=1.0), dict(thermal_rate=0.125),
                   dict(iterations=65536), dict(rain=0.0, capacity=0.0, dissolve=0.0, deposit=0.0, evaporation=0.0, talus=0.0, thermal_rate=0.0)):
        vt.ErosionModifier(**mirror_args(change))


def test_host_check_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/erosion_host_check.cpp: the host half (csrc/terrain_erosion.h) as a stand-alone program under ASan and UBSan, on the CPU: every
    argument check, the step's constants, and the layout at its limits (one column, the whole 1026^2 plane, 65536 iterations)."""
    run_host_check("erosion_host_check", tmp_path)


def test_library_exports_the_entry_points_and_refuses_null():
    """Fails without the layer: the library has no such symbols."""
    L = vt.load()
    assert L.vtmc_erosion_info(None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_erosion_read(None, 0, None, 0) == _lib.ERR_INVALID_ARG
    assert L.vtmc_erosion_device_results(None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.vtmc_debug_erosion_lds(None, 0) == L.vtmc_debug_erosion_ms(None, None) == L.vtmc_debug_erosion_step_ms(None, 0, 1, None) == _lib.ERR_INVALID_ARG


# -- CPU: the twin against the rule's promises (the plane and craft_grid: erosion_support.py) -----------------------------------------------
def test_twin_stays_finite_and_moves_material():
    h, active = plane()
    st = twin.simulate(h, active, 400, P)
    for a in (st.b, st.d, st.s, *st.f):
        assert np.isfinite(a).all() and (a[~active] == 0).all()
    assert (st.d >= 0).all() and st.d.max() > 0.1 and st.s.max() > 0.01 and np.abs(st.b - h)[active].max() > 1


def test_twin_keeps_a_flat_floor_flat():
    _, active = plane()
    st = twin.simulate(np.full((NZ, NX), f32(17.3)), active, 400, P)
    assert (bits(st.b[active]) == bits(f32(17.3))).all() and (st.s == 0).all() and (st.d[active] > 0).all()


@pytest.mark.parametrize("name,turn", [("mirror_x", lambda a: a[:, ::-1]), ("mirror_z", lambda a: a[::-1]), ("transpose", lambda a: a.T)])
def test_twin_commutes_with_mirrors_and_the_transpose(name, turn):
    """Every four-way sum is paired by axis, so the turned terrain gives the turned result bit for bit: b, d, s and, with the directions
    renamed, the fluxes."""
    h, active = plane()
    ref = twin.simulate(h, active, 120, P)
    got = twin.simulate(np.ascontiguousarray(turn(h)), np.ascontiguousarray(turn(active)), 120, P)
    for a in "bds":
        assert np.array_equal(bits(turn(getattr(ref, a))), bits(getattr(got, a))), a
    rename = {"mirror_x": (1, 0, 2, 3), "mirror_z": (0, 1, 3, 2), "transpose": (2, 3, 0, 1)}[name]
    for k in range(4):
        assert np.array_equal(bits(turn(ref.f[rename[k]])), bits(got.f[k])), k


def test_twin_in_float64_conserves_terrain_plus_sediment():
    """Every transfer of the rule is added on one side and subtracted on the other, so sum(b + s) over the active columns holds by
    algebra; only rounding is left, about 4e-13 in float64."""
    h, active = plane()
    st = twin.simulate(h.astype(np.float64), active, 400, P, np.float64)
    before, after = h.astype(np.float64)[active].sum(), (st.b + st.s)[active].sum()
    assert st.b.dtype == np.float64 and abs(after - before) / before <= 1e-9
    assert np.abs(st.b - h)[active].max() > 1


def test_twin_thermal_steps_never_steepen_the_steepest_step():
    """Hydraulic terms off: the largest height step between two neighbouring columns that count never grows from one step to the next.
    With Kt <= 1/8 a step's new height difference is a convex combination of the differences around it wherever both columns of a pair
    have the same neighbours; at a re-entrant corner of the walls one column of a pair lacks a neighbour the other has, and there the
    rule alone does not promise it.  On this plane, whose steepest steps lie away from the block, it holds at every step."""
    h, active = plane()
    thermal = twin.Params(0.0, 0.0, 0.0, 0.0, 0.0, 0.25, 0.5, 0.125)
    st = twin.State(h, active)

    def steepest():
        return max(float(np.abs(st.b - twin.neighbour(st.b, k))[st.counts[k]].max()) for k in range(4))

    last = first = steepest()
    for _ in range(100):
        twin.step(st, thermal)
        now = steepest()
        assert now <= last
        last = now
    assert last < first / 2 and (st.d == 0).all() and (st.s == 0).all()


def test_twin_write_back_reads_back_exactly():
    h, active = plane()
    lo, hi = (0, 0, 0), (NX - 1, 39, NZ - 1)
    g = craft_grid(h, active)
    h0, a0 = twin.heights(g, lo, hi)
    assert np.array_equal(a0, active) and np.array_equal(bits(h0[active]), bits(h[active]))
    r = twin.erode(g, lo, hi, 60, P)
    assert r.info["n_active"] == int(active.sum()) and r.info["n_rewritten"] > 3000 and r.info["n_clamped"] == 0
    h1, a1 = twin.heights(r.grid, lo, hi)
    assert np.array_equal(a1, active) and np.array_equal(bits(h1), bits(r.after))
    # a box whose top cuts the terrain: columns that end above it are walls, columns just under it are clamped; still exact
    cut = (NX - 1, 24, NZ - 1)
    c = twin.erode(g, lo, cut, 10, P)
    assert 0 < c.info["n_active"] < int(active.sum()) and c.info["n_clamped"] > 0 and c.after[c.active > 0].max() == 23.0
    h2, a2 = twin.heights(c.grid, lo, cut)
    assert np.array_equal(a2, c.active > 0) and np.array_equal(bits(h2), bits(c.after))
    outside = np.ones(g.shape, bool)
    outside[:, :25, :] = False
    assert np.array_equal(bits(c.grid[outside]), bits(g[outside]))


# -- GPU ----------------------------------------------------------------------------------------------------------------------------------
# the noise world, its boxes and the comparison with the twin: erosion_support.py
@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 3, 40])
def test_gpu_whole_grid_equals_the_twin(iterations):
    """Odd and even step counts: water and sediment change planes once a step."""
    with World() as ex:
        _, want = erode_and_compare(ex, *WHOLE, iterations)
        info = want.info
        assert (info["nx"], info["nz"]) == (82, 50) and 3500 < info["n_active"] < 82 * 50 and info["n_rewritten"] > 0
        assert (want.active == 0).sum() >= 8   # the pillar and the shaft
        if iterations == 40:
            assert want.water.max() > 0.05 and want.sediment.max() > 0.001 and np.abs(want.after - want.before).max() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("name,lo,hi", [("inside", (9, 3, 7), (73, 30, 44)), ("one_column_wide", (31, 0, 0), (31, 33, 49)),
                                        ("one_column", (40, 0, 25), (40, 33, 25)), ("cuts_the_terrain", (0, 0, 0), (81, 15, 49))])
def test_gpu_boxes_equal_the_twin(name, lo, hi):
    with World() as ex:
        before, want = erode_and_compare(ex, lo, hi, 12)
        assert want.info["n_active"] > 0
        assert (want.info["n_clamped"] > 0) == (name == "cuts_the_terrain")
        outside = np.ones(before.shape, bool)
        outside[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = False
        assert np.array_equal(bits(ex.terrain_read_samples()[outside]), bits(before[outside]))


@pytest.mark.gpu
@pytest.mark.parametrize("params", [P._replace(rain=0.0, capacity=0.0), P._replace(thermal_rate=0.0)], ids=["thermal_only", "hydraulic_only"])
def test_gpu_each_half_alone_equals_the_twin(params):
    with World() as ex:
        _, want = erode_and_compare(ex, *WHOLE, 16, params)
        assert want.info["n_rewritten"] > 0
        if params.rain == 0:
            assert (want.water == 0).all() and (want.sediment == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi,iterations", [(*WHOLE, 7), ((9, 3, 7), (73, 30, 44), 4), ((63, 0, 3), (64, 33, 4), 6)])
def test_gpu_the_step_staged_in_lds_equals_the_twin(lo, hi, iterations):
    """The other variant of the step's kernels (vtmc_debug_erosion_lds: the planes read at a neighbour staged in LDS, tile by tile with a
    halo) computes the same bytes: past one tile in x and z, a box inside the grid, and a box whose two columns lie in two tiles."""
    with World() as ex:
        assert ex._L.vtmc_debug_erosion_lds(ex._h, 1) == _lib.OK
        erode_and_compare(ex, lo, hi, iterations)
        ms = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
        assert ex._L.vtmc_debug_erosion_ms(ex._h, ms) == _lib.OK and all(np.isfinite(v) and v >= 0 for v in ms)
        assert ex._L.vtmc_debug_erosion_lds(ex._h, 0) == _lib.OK
        erode_and_compare(ex, lo, hi, iterations)


@pytest.mark.gpu
def test_gpu_queue_undo_redo_and_the_snapshot(tmp_path):
    def events(ex):
        path = str(tmp_path / "events.vtmt")
        ex.terrain_save(path)
        return tf.read_header(path)["events"]

    bump = vt.NoiseModifier(5, 3, 0.2, amplitude=2.0, ramp_scale=1.0, ramp_center=world_of((0, 14, 0))[1], lower=world_of((10, 0, 10)), upper=world_of((50, 33, 40))).to_struct()
    lo, hi = (4, 0, 4), (70, 33, 45)
    with World() as ex:   # the two calls, one after the other
        ex.terrain_update([bump])
        ex.terrain_update([erosion(lo, hi, 9)])
        separate, maps = ex.terrain_read_samples(), [ex.erosion_read(m) for m in MAPS]
        info = ex.erosion_info()
    with World(history=1 << 26) as ex:
        start = ex.terrain_read_samples()
        n_events = events(ex)
        ex.terrain_update([bump, erosion(lo, hi, 9)])   # the erosion sees what the noise wrote
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(separate)) and ex.erosion_info() == info
        assert all(a.tobytes() == b.tobytes() for a, b in zip(maps, [ex.erosion_read(m) for m in MAPS]))
        assert events(ex) == n_events + 2 and ex.terrain_history()[:2] == (1, 0)   # one event number each, one undo step for the queue
        nb = tuple(d // 8 for d in DIMS)
        dirty = ex.terrain_dirty_blocks()
        assert np.array_equal(dirty, block_list(dirty_ids(lo, hi, nb) | dirty_ids((10, 0, 10), (50, 33, 40), nb), nb))
        ex.terrain_undo()
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(start)) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert ex.erosion_info() == info and all(a.tobytes() == b.tobytes() for a, b in zip(maps, [ex.erosion_read(m) for m in MAPS]))   # the maps stay
        ex.terrain_redo()   # the values come back from the journal: nothing is simulated, no event is taken, the maps are not replaced
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(separate)) and events(ex) == n_events + 2
        assert ex.erosion_info() == info and ex.terrain_history()[:2] == (1, 0)
        # one more step right after: it reads the heights the first one wrote, bit for bit
        after = ex.erosion_read("height_after")
        ex.terrain_update([erosion(lo, hi, 1)])
        assert ex.erosion_read("height_before").tobytes() == after.tobytes() and ex.erosion_info()["n_active"] == info["n_active"]
        assert ex.terrain_history()[:2] == (2, 0)


@pytest.mark.gpu
def test_gpu_both_output_modes_extract_what_the_twins_grid_gives():
    with World(history=1 << 26) as ex, vt.Extractor(0) as plain:
        want = twin.erode(ex.terrain_read_samples(), *WHOLE, 8, P)
        _, T = ex.terrain_update([erosion(*WHOLE, 8)])
        dirty = ex.terrain_dirty_blocks()
        assert plain.extract_grid(want.grid, dirty) == T and T > 5000
        (got, offs), (ref, ref_offs) = ex.read_triangles(), plain.read_triangles()
        assert np.array_equal(offs, ref_offs) and np.array_equal(got["block"], ref["block"])
        for f in ("p0", "p1", "p2", "n0", "n1", "n2"):   # the bar of every extract comparison here
            assert np.abs(got[f] - ref[f]).max() <= 1e-5, f
        ex.set_output_mode(True)
        plain.set_output_mode(True)
        ex.terrain_undo()
        assert ex.terrain_redo()[1] == T and plain.extract_grid(want.grid, dirty) == T
        (v, idx, voffs, toffs), (rv, ridx, rvoffs, rtoffs) = ex.read_indexed_mesh(), plain.read_indexed_mesh()
        assert np.array_equal(idx, ridx) and np.array_equal(voffs, rvoffs) and np.array_equal(toffs, rtoffs)
        assert np.abs(v["position"] - rv["position"]).max() <= 1e-5 and np.abs(v["normal"] - rv["normal"]).max() <= 1e-5


def raw(change=(), **fields):
    m = erosion((4, 0, 4), (60, 33, 40), 5)
    for k, v in change:
        m.p[k] = v
    for name, v in fields.items():
        setattr(m, name, v) if name != "dims" else m.data_dims.__setitem__(slice(None), v)
    return m


@pytest.mark.gpu
def test_gpu_refusals_write_nothing():
    nan, inf = float("nan"), float("inf")
    keep = np.zeros(4, f32)
    bad = [(raw([(k, nan)]), "not finite") for k in range(8)] + [(raw([(k, -0.5)]), "negative") for k in range(8)] + [
        (raw([(0, inf)]), "not finite"), (raw([(0, 257.0)]), "rain above"), (raw([(2, 65537.0)]), "capacity above"), (raw([(3, 1.5)]), "dissolve outside"),
        (raw([(4, 1.5)]), "deposit outside"), (raw([(5, 0.0)]), "dt outside"), (raw([(5, 1.5)]), "dt outside"), (raw([(7, 0.13)]), "thermal rate above"),
        (raw([(1, 3.0), (5, 0.5)]), "evaporation \\* dt above 1"), (raw(dims=(0, 0)), "iterations outside"), (raw(dims=(65537, 0)), "iterations outside"),
        (raw(dims=(-1, 0)), "iterations outside"), (raw(dims=(5, 1)), "data_dims\\[1\\] must be 0"), (raw(data=keep.ctypes.data), "data must be NULL")]
    for history in (0, 1 << 24):
        with World(history) as ex:
            no_result(ex.erosion_info)
            no_result(lambda: ex.erosion_read("water"))
            no_result(ex.device_erosion)
            start = ex.terrain_read_samples()
            good = vt.SphereModifier(world_of((20, 12, 20)), 2.0).to_struct()
            for m, word in bad:
                text = invalid(ex, [m])
                assert re.search("modifier 0: erosion .*" + word, text), text
                if history:   # the whole queue is checked before the first write
                    assert re.search("modifier 1: erosion", invalid(ex, [good, m]))
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(start)) and ex.terrain_history()[:2] == (0, 0)
            no_result(ex.erosion_info)
            # kinds 6 and 7 stay unknown, 13 is
            for kind in (6, 7, 13):
                assert "unknown kind" in invalid(ex, [raw(kind=kind)])
            ex.terrain_update([erosion((4, 0, 4), (60, 33, 40), 2)])
            info = ex.erosion_info()
            assert info["nx"] * info["nz"] == 57 * 37
            invalid(ex, [raw([(5, 2.0)])])   # a refused erosion keeps the snapshot
            assert ex.erosion_info() == info
            buf = np.zeros(57 * 37, f32)
            L, h = ex._L, ex._h
            assert L.vtmc_erosion_read(h, _lib.EROSION_WATER, buf.ctypes.data, buf.nbytes - 1) == _lib.ERR_CAPACITY
            assert L.vtmc_erosion_read(h, _lib.EROSION_ACTIVE, buf.ctypes.data, 57 * 37 - 1) == _lib.ERR_CAPACITY
            assert L.vtmc_erosion_read(h, _lib.EROSION_ACTIVE, buf.ctypes.data, 57 * 37) == _lib.OK
            assert L.vtmc_erosion_read(h, 5, buf.ctypes.data, buf.nbytes) == _lib.ERR_INVALID_ARG
            assert L.vtmc_erosion_read(h, -1, buf.ctypes.data, buf.nbytes) == _lib.ERR_INVALID_ARG
            assert L.vtmc_erosion_read(h, 0, None, buf.nbytes) == _lib.ERR_INVALID_ARG
            assert L.vtmc_erosion_info(h, None) == _lib.ERR_INVALID_ARG
            ptrs = ex.device_erosion()
            assert set(ptrs) == set(MAPS) and all(ptrs.values()) and len(set(ptrs.values())) == 5
            ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)   # the snapshot's grid is gone
            no_result(ex.erosion_info)
            no_result(lambda: ex.erosion_read("active"))
            no_result(ex.device_erosion)


@pytest.mark.gpu
def test_gpu_host_mirror_erodes_and_reads_the_maps(tmp_path):
    """host_selftest --gpu-erosion: ErosionModifier queued through VoxelTerrain::Update and VoxelTerrain::ReadErosion; what it dumps
    equals the twin's erosion of the grid it dumped before."""
    import subprocess
    from test_host_mirror import TIME_LIMIT, build_host
    r = subprocess.run([build_host(), "--gpu-erosion", str(tmp_path)], capture_output=True, text=True, timeout=TIME_LIMIT)
    assert r.returncode == 0 and "HOST-EROSION-OK" in r.stdout, (r.returncode, r.stdout[-600:], r.stderr[-600:])
    shape = (66, 34, 34)   # the mirror's world: 64 x 32 x 32 cells, a C# float[,,]
    before = np.fromfile(tmp_path / "erosion_grid_before.f32", f32).reshape(shape)
    after = np.fromfile(tmp_path / "erosion_grid_after.f32", f32).reshape(shape)
    box = np.fromfile(tmp_path / "erosion_box.i32", np.int32)
    lo, hi = tuple(int(v) for v in box[:3]), tuple(int(v) for v in box[3:6])
    assert (lo, hi) == ((4, 0, 2), (56, 33, 29))
    want = twin.erode(before, lo, hi, 24, P)
    assert (want.info["n_active"], want.info["n_rewritten"], want.info["n_clamped"]) == tuple(int(v) for v in box[6:])
    assert np.array_equal(bits(after), bits(want.grid))
    for name, ref in (("before", want.before), ("after", want.after), ("water", want.water), ("sediment", want.sediment)):
        assert np.fromfile(tmp_path / ("erosion_%s.f32" % name), f32).tobytes() == ref.tobytes(), name
    assert np.fromfile(tmp_path / "erosion_active.u8", np.uint8).tobytes() == want.active.tobytes()
