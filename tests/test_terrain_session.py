"""The resident terrain as one randomized edit session against its twins (session_twin.py), a directed matrix of box extents on the seams
of the shared box walk (64 lanes along x, 4 z-planes, runs of 16 along y), and the inclusive dirty rule on the device.

CPU: the generator is deterministic and every committed seed meets the coverage conditions (conditions, not measurements: a seed that
misses one is replaced, the condition stays); the history model gives the answers worked by hand below; the model's snapshots are
self-consistent.  GPU: after EVERY operation of a session the device is compared with the model -- every sample as uint32, the dirty
list, the history counts and bytes, the triangles (offsets and `block` exact, floats within 1e-5), stamp bits, files.  Independently of
the history model, every undo or redo the device grants must put back the snapshot the test itself keeps for it.

"Eviction while the redo stack is non-empty" is read as: an update that arrives with steps to redo and, after discarding them, still
costs at least one older step (the library discards the redo before it places the step)."""
import os

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib, terrainfile as tf
import session_twin as st
import stamp_twin
from session_twin import FACES, FAMILIES, KINDS, SEEDS, History, Session, generate
from terrain_twin import assert_triangles, bits, box_of, gpu_struct, oracle_mod_of

f32 = np.float32
CASES = [(w, s) for w in sorted(SEEDS) for s in SEEDS[w]]
_runs = {}


def twin_run(oracle_mod, tmp_path_factory, world, seed):
    """The session on the model alone, run once per (world, seed): the model after the last operation and the checks made on the way."""
    if (world, seed) not in _runs:
        tmp = tmp_path_factory.mktemp("session_%s%d" % (world, seed))
        s = Session(oracle_mod, world)
        for i, op in enumerate(generate(seed, world)):
            s.run(op, tmp)
            h = s.hist
            # the snapshot stack is self-consistent: neighbouring steps share a grid, and undo then redo is the identity
            for a, b in zip(h.steps, h.steps[1:]):
                assert np.array_equal(bits(a.payload["after"]), bits(b.payload["before"])), i
            if h.done:
                mem, state = s.ref._mem.copy(), h.state()
                assert np.array_equal(bits(mem), bits(h.steps[h.done - 1].payload["after"])), i
                s.undo()
                assert np.array_equal(bits(s.ref._mem), bits(h.steps[h.done].payload["before"])) and h.state() == (state[0] - 1, state[1] + 1, state[2]), i
                s.redo()
                assert np.array_equal(bits(s.ref._mem), bits(mem)) and h.state() == state, i
        _runs[(world, seed)] = s
    return _runs[(world, seed)]


# -- CPU: the generator -------------------------------------------------------------------------------------------------------------------
def plain(ops):
    """An operation list with its arrays as bytes, for comparing."""
    def flat(v):
        if isinstance(v, np.ndarray):
            return (v.shape, v.tobytes())
        if isinstance(v, dict):
            return tuple((k, flat(v[k])) for k in sorted(v))
        return tuple(flat(x) for x in v) if isinstance(v, (tuple, list)) else v
    return flat(ops)


@pytest.mark.parametrize("world,seed", CASES)
def test_the_same_seed_gives_the_same_session(world, seed):
    ops = generate(seed, world)
    assert len(ops) == st.N_OPS and plain(ops) == plain(generate(seed, world))
    assert plain(ops) != plain(generate(seed + 1000, world))
    late = generate(seed, world, history_from_start=False)
    assert len(late) == st.N_OPS and late[0][0] == "update" and late[st.N_OPS // 3][0] == "set_history" and late[st.N_OPS // 3][1] > 0
    assert all(op[1] == 0 for op in late[:st.N_OPS // 3] if op[0] == "set_history")
    assert 60 <= st.N_OPS <= 80


@pytest.mark.parametrize("world,seed", CASES)
def test_generator_conditions(oracle_mod, tmp_path_factory, world, seed):
    ops = generate(seed, world)
    s = twin_run(oracle_mod, tmp_path_factory, world, seed)
    assert ops[0][0] == "set_history" and ops[1][0] == "update" and ops[1][1][0][0] == "plane" and ops[1][1][0][1][0] % 1 != 0
    assert all(1 <= len(op[1]) <= 4 for op in ops if op[0] == "update")
    for k in KINDS:   # every modifier kind, stamp mode and noise basis
        assert s.kinds[k] >= 3, (k, s.kinds)
    for add in (True, False):   # both clamp branches of csg_write, in add and in erode mode
        assert s.taken[add]["low"] > 0 and s.taken[add]["high"] > 0, (add, s.taken)
    assert len(s.footprints) >= 9 and min(s.footprints) > 0, s.footprints   # every stamp modifier is meant to write
    for fam in FAMILIES:
        assert s.faces[fam] == set(FACES), (fam, sorted(set(FACES) - s.faces[fam]))
    h = s.hist
    assert h.wraps >= 5 and h.over_budget >= 3 and h.after_undo >= 5 and h.evictions_with_redo >= 1, (h.wraps, h.over_budget, h.after_undo, h.evictions_with_redo)
    assert s.loads_edited >= 2
    shapes = {sp[1][0].shape for op in ops if op[0] == "update" for sp in op[1] if sp[0] == "island"}
    assert shapes == {(1, 7), (7, 1), (48, 40)}, shapes
    # a cylinder whose start lies on a sample and whose axis is a grid axis; boxes wholly outside; rejected queues; both stamp sources
    w = st.WORLDS[world]
    cyl = [sp[1] for op in ops if op[0] == "update" for sp in op[1] if sp[0] == "cylinder" and sorted(sp[1][1]) == [0.0, 0.0, 1.0]]
    assert cyl and all(f32(round((c - o) / w["scale"])) * f32(w["scale"]) + f32(o) == f32(c) for c, o in zip(cyl[0][0], w["origin"]))
    names = [op[0] for op in ops]
    assert names.count("reject") >= 3 and names.count("stamp_create") >= 2 and names.count("stamp_capture") >= 3 and "stamp_destroy" in names
    assert names.count("set_history") >= 3 and names.count("redo") >= 4


def test_twins_take_an_overridden_box(oracle_mod):
    """The third entry of a spec replaces the AABB of the device's struct and of the oracle's modifier alike, and nothing else."""
    box = ((1.25, 2.5, 3.0), (9.0, 4.75, 6.5))
    for spec in (("sphere", ((5.0, 5.0, 5.0), 3.0, False)), ("plane", (6.5, (0, 0), (9, 9), True))):
        plain_m, m, om = gpu_struct(spec), gpu_struct(spec + (box,)), oracle_mod_of(oracle_mod, spec + (box,))
        for got in (m, om):
            assert (tuple(got.lower), tuple(got.upper)) == box and list(got.p) == list(plain_m.p)
            assert (got.kind, got.add_or_erode) == (plain_m.kind, plain_m.add_or_erode)
        assert tuple(plain_m.lower) != box[0]
    ref = oracle_mod.Terrain(16, 8, 8)
    assert box_of(ref, gpu_struct(("sphere", ((5.0, 5.0, 5.0), 3.0, True), ((2.0, 1.0, 3.0), (2.0, 4.0, 5.0)))))[:2] == ([2, 1, 3], [1, 4, 3])


# -- CPU: the history model against sequences worked by hand ------------------------------------------------------------------------------
def kept(h):
    return [(s.payload, s.off) for s in h.steps]


def play(budget, sizes):
    h = History()
    h.set_budget(budget)
    out = []
    for name, n in sizes:
        h.record(n, name)
        out.append(kept(h))
    return h, out


def test_history_equal_steps_keep_floor_of_budget_over_size():
    """include/vtmc.h: steps of equal size S: floor(max_bytes / S) are kept."""
    for budget, S, want in ((13440, 5376, 2), (1000, 256, 3), (1024, 256, 4), (256, 256, 1), (767, 256, 2), (5376 * 3, 5376, 3)):
        h, _ = play(budget, [(i, S) for i in range(11)])
        assert h.state() == (want, 0, want * S), (budget, S)
        assert [s.payload for s in h.steps] == list(range(11 - want, 11))
    h, seq = play(1000, [("a", 256), ("b", 256), ("c", 256), ("d", 256), ("e", 256)])
    assert seq[3] == [("b", 256), ("c", 512), ("d", 0)] and seq[4] == [("c", 512), ("d", 0), ("e", 256)] and h.wraps == 1


def test_history_mixed_sizes_wrap_twice():
    h, seq = play(1024, [("a", 512), ("b", 256), ("c", 512), ("d", 256), ("e", 768), ("f", 256)])
    assert seq == [[("a", 0)], [("a", 0), ("b", 512)],
                   [("b", 512), ("c", 0)],            # c does not fit behind b (768 + 512 > 1024): offset 0, over a; 768..1024 stays unused
                   [("c", 0), ("d", 512)],            # d behind c, over b
                   [("e", 0)],                        # e does not fit behind d: offset 0, over c and d
                   [("e", 0), ("f", 768)]]            # f fits exactly
    assert h.wraps == 2 and h.state() == (2, 0, 1024)


def test_history_a_step_stranded_at_the_tail_goes_with_the_wrap():
    first = [("a", 256), ("b", 256), ("c", 256), ("d", 256), ("e", 256), ("f", 256)]
    h, seq = play(1100, first + [("g", 768)])
    assert seq[5] == [("c", 512), ("d", 768), ("e", 0), ("f", 256)]
    # g does not fit behind f (512 + 768 > 1100): offset 0, over e, f and c; d at 768..1024 shares no byte with it, but it is older than
    # steps that go, and behind a second wrap: it goes too
    assert seq[6] == [("g", 0)] and h.wraps == 2 and h.state() == (1, 0, 768)
    h, seq = play(1100, [("a", 256), ("b", 256), ("c", 256), ("d", 256), ("e", 512), ("f", 256), ("g", 512)])
    assert seq[4] == [("c", 512), ("d", 768), ("e", 0)] and seq[5] == [("d", 768), ("e", 0), ("f", 512)]
    # g wraps over e; d is stranded at the tail and goes; f at 512..768 is newer than both and shares no byte with g: it stays
    assert seq[6] == [("f", 512), ("g", 0)] and h.wraps == 2 and h.state() == (2, 0, 768)


def test_history_redo_budget_and_empty_steps():
    h, _ = play(4096, [("a", 256), ("b", 512), ("c", 256)])
    assert h.undo().payload == "c" and h.undo().payload == "b" and h.state() == (1, 2, 1024)
    assert h.record(0, "nothing") is None and h.state() == (1, 2, 1024)      # writes no sample: both stacks stay
    assert h.record(256, "d").off == 256 and kept(h) == [("a", 0), ("d", 256)] and h.after_undo == 1   # the redo is discarded
    assert h.redo() is None and h.undo().payload == "d" and h.undo().payload == "a" and h.undo() is None
    assert h.redo().payload == "a" and h.state() == (1, 1, 512)
    assert h.record(4352, "big") is None and h.state() == (0, 0, 0) and h.over_budget == 1   # larger than the budget: cleared
    h.record(4096, "all")
    assert h.state() == (1, 0, 4096)
    h.set_budget(512)
    assert h.state() == (0, 0, 0)
    h.set_budget(0)
    assert h.record(256, "off") is None and h.state() == (0, 0, 0)
    # after two undos under a tight budget: g does not fit behind d (1024 + 768 > 1024), lies at 0..768 and costs c at 512..768; d at
    # 768..1024 shares no byte with it and the offsets d, g fall once: it stays
    h, _ = play(1024, [("a", 256), ("b", 256), ("c", 256), ("d", 256), ("e", 256), ("f", 256)])
    assert kept(h) == [("c", 512), ("d", 768), ("e", 0), ("f", 256)]
    h.undo(), h.undo()
    h.record(768, "g")
    assert kept(h) == [("d", 768), ("g", 0)] and h.evictions_with_redo == 1 and h.state() == (2, 0, 1024)
    h, _ = play(1024, [("a", 256), ("b", 256), ("c", 256), ("d", 256), ("e", 256), ("f", 256)])
    h.undo()
    h.record(512, "g")   # behind e at 256..768, over c
    assert kept(h) == [("d", 768), ("e", 0), ("g", 256)] and h.evictions_with_redo == 1


# -- GPU: the session ---------------------------------------------------------------------------------------------------------------------
def assert_state(ex, s, tag):
    got, want = bits(ex.terrain_read_samples()), bits(s.ref.grid)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        pytest.fail("%s: %d samples differ, first at [x, y, z] = %s, box of them %s .. %s" % (tag, len(at), at[0], at.min(0), at.max(0)))
    assert ex.terrain_history() == s.hist.state(), tag


def assert_result(ex, s, got, dirty, tag):
    n_dirty, T = got
    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty), tag
    if len(dirty):
        assert_triangles(ex, s.oracle, s.ref.grid, dirty, T)
    else:
        assert T == 0, tag


def describe(s, i, op):
    if op[0] in ("update", "reject"):
        return "op %d %s %s" % (i, op[0], [(st.category(sp), "box" if len(sp) > 2 else "own", *box_of(s.ref, stamp_twin.gpu_struct(sp))[:2]) for sp in op[1]])
    return "op %d %r" % (i, op[:1] + tuple(op[1:])[:3])


def step_session(ex, s, op, tmp, tag, mine):
    """One operation on the device and on the model, and every comparison it allows.  mine: the test's own snapshots of the steps the
    device may still hold, {"undo": [...], "redo": [...]}, kept without any model of the ring."""
    name = op[0]
    if name == "update":
        before = s.ref._mem.copy()
        got = ex.terrain_update([stamp_twin.gpu_struct(sp) for sp in op[1]])
        dirty = s.update(op[1])
        assert_state(ex, s, tag)
        assert_result(ex, s, got, dirty, tag)
        if s.hist.budget and any(min(e) > 0 for _, e in s.boxes(op[1])):   # history on and a sample written: the device may record a step
            mine["undo"].append((before, s.ref._mem.copy()))
            mine["redo"].clear()
    elif name in ("undo", "redo"):
        other = "redo" if name == "undo" else "undo"
        try:
            got = ex.terrain_undo() if name == "undo" else ex.terrain_redo()
        except vt.VtmcError as e:
            assert e.code == _lib.ERR_NO_RESULT, tag
            got = None
        dirty = getattr(s, name)()
        assert (got is None) == (dirty is None), "%s: the device %s, the model %s" % (tag, "refused" if got is None else "granted", "refuses" if dirty is None else "grants")
        if got is not None:
            assert mine[name], tag + ": granted with no step of the test's own left"
            snap = mine[name].pop()
            mine[other].append(snap)
            want = bits(snap[0 if name == "undo" else 1])
            assert np.array_equal(bits(ex.terrain_read_samples()), want.transpose(2, 1, 0)), tag + ": not the snapshot of that step"
            assert_result(ex, s, got, dirty, tag)
        assert_state(ex, s, tag)
    elif name == "set_history":
        ex.terrain_set_history(op[1])
        s.set_history(op[1])
        mine["undo"].clear(), mine["redo"].clear()
        assert_state(ex, s, tag)
    elif name == "stamp_create":
        want = s.stamp_create(*op[1:])
        sid = ex.stamp_create(s.stamps[want])
        assert sid == want and np.array_equal(bits(ex.stamp_read(sid)), bits(s.stamps[want])), tag
    elif name == "stamp_capture":
        want = s.stamp_capture(*op[1:])
        sid = ex.stamp_capture(*op[1:])
        assert sid == want and ex.stamp_dims(sid) == tuple(op[2]), tag
        assert np.array_equal(bits(ex.stamp_read(sid)), bits(s.stamps[want])), tag
        assert_state(ex, s, tag)
    elif name == "stamp_destroy":
        ex.stamp_destroy(op[1])
        s.stamp_destroy(op[1])
        with pytest.raises(vt.VtmcError) as e:
            ex.stamp_dims(op[1])
        assert e.value.code == _lib.ERR_INVALID_ARG, tag
    elif name == "save_load":
        dev, mirror = os.path.join(tmp, "device.vtmt"), os.path.join(tmp, "twin.vtmt")
        n_bytes = ex.terrain_save(dev)
        assert_state(ex, s, tag + " (save)")    # a save changes nothing
        dirty = s.save_load(mirror)
        assert n_bytes == os.path.getsize(dev) == os.path.getsize(mirror), tag
        n = len(tf.classify_bricks(s.ref.grid))
        assert np.array_equal(np.fromfile(dev, np.uint8, n, offset=64), np.fromfile(mirror, np.uint8, n, offset=64)), tag + ": brick kinds"
        assert open(dev, "rb").read() == open(mirror, "rb").read(), tag
        assert np.array_equal(bits(tf.read_terrain(dev)[2]), bits(s.ref.grid)), tag   # the mirror reading the device's file
        got = ex.terrain_load(dev)
        mine["undo"].clear(), mine["redo"].clear()
        assert_state(ex, s, tag)
        assert_result(ex, s, got, dirty, tag)
    elif name == "reject":
        mods = [stamp_twin.gpu_struct(sp) for sp in op[1]] + [st.bad_modifier(op[2])]
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_update(mods)
        assert e.value.code == _lib.ERR_INVALID_ARG and "modifier %d" % len(op[1]) in str(e.value), (tag, str(e.value))
        s.reject(op[1])
        assert_state(ex, s, tag)   # history on: nothing changed; off: the prefix, and its event numbers (the next draws hash them)
    else:
        raise AssertionError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("from_start", [True, False], ids=["history-from-start", "history-mid-session"])
@pytest.mark.parametrize("world,seed", CASES)
def test_gpu_session(oracle_mod, tmp_path, world, seed, from_start):
    w = st.WORLDS[world]
    ops = generate(seed, world, history_from_start=from_start)
    s = Session(oracle_mod, world)
    mine = {"undo": [], "redo": []}
    with vt.Extractor(0) as ex:
        ex.terrain_init(*w["dims"], w["scale"], w["origin"], w["seed"])
        assert_state(ex, s, "init")
        for i, op in enumerate(ops):
            step_session(ex, s, op, str(tmp_path), describe(s, i, op), mine)


# -- GPU: the box walk at its own seams ---------------------------------------------------------------------------------------------------
M_DIMS, M_SEED = (72, 40, 24), 4321       # 74 x 42 x 26 samples: two x-segments, three y-runs, seven z-quads
DXS, DYS, DZS = (1, 63, 64, 65, 74), (1, 15, 16, 17, 32, 33, 42), (1, 3, 4, 5, 26)


def covering_extents():
    """Each value of each axis with the smallest and the largest value of the other two; the all-ones box and the whole grid among them."""
    out = []
    for v in DXS:
        out += [(v, DYS[0], DZS[0]), (v, DYS[-1], DZS[-1])]
    for v in DYS:
        out += [(DXS[0], v, DZS[0]), (DXS[-1], v, DZS[-1])]
    for v in DZS:
        out += [(DXS[0], DYS[0], v), (DXS[-1], DYS[-1], v)]
    return sorted(set(out))


def placements(ext):
    """The low corner, the high corner, and an interior first sample that is no multiple of 8 (where the extent leaves room for one)."""
    top = [d + 2 for d in M_DIMS]
    inner = tuple(min(n, top[k] - ext[k]) for k, n in enumerate((5, 3, 1)))
    return sorted({(0, 0, 0), tuple(top[k] - ext[k] for k in range(3)), inner})


def matrix_specs(first, ext, stamp_id, stamp_dims):
    """Every kernel family on the box [first, first + ext): parameters under which every sample of the box is written -- brush radii
    larger than the grid's diagonal (89 samples; the weight is then the full strength everywhere), noise and stamps with no weight at all."""
    box = (tuple(float(v) for v in first), tuple(float(first[k] + ext[k] - 1) for k in range(3)))
    hm = (12.0 + 8.0 * np.sin(np.linspace(0, 3, 48))[:, None] * np.cos(np.linspace(0, 2, 40))[None, :]).astype(f32)
    noise = dict(seed=7, octaves=2, frequency=0.21, amplitude=1.5, ramp_scale=0.3, ramp_center=20.0, lower=box[0], upper=box[1])
    return [("plane", (20.375, (0, 0), (80, 80), True), box), ("sphere", ((37.0, 20.0, 13.0), 30.0, False), box),
            ("cylinder", ((0.0, 20.0, 12.0), (1.0, 0.1, 0.05), 80.0, 9.0, True), box), ("island", (hm, 74.0, 26.0, 60.0, True), box),
            ("flatten", ((37.0, 21.0, 13.0), (0.2, 1.0, 0.1), 200.0, 0.75), box), ("smooth", ((37.0, 21.0, 13.0), 200.0, 0.5), box),
            ("noise", dict(noise, basis="fbm", add_or_erode=True)), ("noise", dict(noise, basis="billow", add_or_erode=False)),
            ("noise", dict(noise, basis="ridged", add_or_erode=True)),
            ("stamp", dict(stamp_id=stamp_id, dims=stamp_dims, position=(36.8, 20.7, 12.9), pitch=2.0, mode="replace"), box)]


def test_matrix_covers_the_seams():
    exts = covering_extents()
    assert (1, 1, 1) in exts and (74, 42, 26) in exts and len(exts) == 30
    for axis, values in enumerate((DXS, DYS, DZS)):
        for v in values:
            others = {tuple(e[k] for k in range(3) if k != axis) for e in exts if e[axis] == v}
            assert len(others) >= 2, (axis, v)
    for e in exts:
        for p in placements(e):
            assert all(0 <= p[k] and p[k] + e[k] <= M_DIMS[k] + 2 for k in range(3))
        assert any(any(v % 8 for v in p) for p in placements(e)) or e == (74, 42, 26)
    # the stamp's footprint holds the whole grid: |p - t| <= h (n - 1) / 2 on every axis
    for k, (t, n) in enumerate(zip((36.8, 20.7, 12.9), (40, 24, 16))):
        assert t - (n - 1) <= 0 and t + (n - 1) >= M_DIMS[k] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("history", [0, 64 << 20], ids=["history-off", "history-on"])
@pytest.mark.parametrize("ext", covering_extents(), ids=lambda e: "%dx%dx%d" % e)
def test_gpu_box_matrix(oracle_mod, ext, history):
    ref = oracle_mod.Terrain(*M_DIMS, 1.0, (0.0, 0.0, 0.0), M_SEED)
    stamps = {1: st.stamp_field(11, (40, 24, 16), 2.5)}
    nb = tuple(d // 8 for d in M_DIMS)
    with vt.Extractor(0) as ex:
        ex.terrain_init(*M_DIMS, 1.0, (0.0, 0.0, 0.0), M_SEED)
        assert ex.stamp_create(stamps[1]) == 1
        ex.terrain_set_history(history)
        for first in placements(ext):
            for spec in matrix_specs(first, ext, 1, (40, 24, 16)):
                tag = "%s box %s + %s" % (st.category(spec), first, ext)
                assert box_of(ref, stamp_twin.gpu_struct(spec))[:2] == (list(first), list(ext)), tag
                before = ref._mem.copy()
                n_dirty, _ = ex.terrain_update([stamp_twin.gpu_struct(spec)])
                counts = []
                dirty = stamp_twin.twin_update(ref, oracle_mod, [spec], stamps, counts)
                assert not counts or counts[0] == ext[0] * ext[1] * ext[2], tag
                got = bits(ex.terrain_read_samples())
                assert np.array_equal(got, bits(ref.grid)), (tag, np.argwhere(got != bits(ref.grid))[:4])
                assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty), tag
                if history:   # the swap kernel, both ways
                    n_dirty, _ = ex.terrain_undo()
                    got = bits(ex.terrain_read_samples())
                    assert np.array_equal(got, bits(before).transpose(2, 1, 0)), (tag + " undo", np.argwhere(got != bits(before).transpose(2, 1, 0))[:4])
                    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty), tag
                    n_dirty, _ = ex.terrain_redo()
                    got = bits(ex.terrain_read_samples())
                    assert np.array_equal(got, bits(ref.grid)), (tag + " redo", np.argwhere(got != bits(ref.grid))[:4])
                    assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty), tag
            # the copy kernel on the same box; a stamp has at least 2 samples per axis, so an axis of extent 1 is captured with its neighbour
            cdims = tuple(max(e, 2) for e in ext)
            cfirst = tuple(min(first[k], M_DIMS[k] + 2 - cdims[k]) for k in range(3))
            sid = ex.stamp_capture(cfirst, cdims)
            want = ref.grid[cfirst[0]:cfirst[0] + cdims[0], cfirst[1]:cfirst[1] + cdims[1], cfirst[2]:cfirst[2] + cdims[2]]
            assert np.array_equal(bits(ex.stamp_read(sid)), bits(want)), ("capture", cfirst, cdims)
            ex.stamp_destroy(sid)
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(ref.grid))


# -- GPU: the dirty rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_dirty_rule_is_inclusive_on_both_ends(oracle_mod):
    """test_terrain.py's three oracle cases on the device, and their mirror images: an AABB that ends exactly on a block face dirties
    the face-adjacent block too (up >= 8b && low <= 8b + 8), at the low end, at the high end of the box and at the grid's last block."""
    cases = [((12.0, 4.0), [0, 1, 2]), ((12.0, 3.5), [0, 1, 2]), ((12.5, 3.0), [1, 2]),   # samples 8..16, 8..16, 9..16
             ((20.0, 4.0), [1, 2, 3]), ((20.0, 3.5), [1, 2, 3]), ((19.5, 3.0), [1, 2]),   # samples 16..24, 16..24, 16..23
             ((28.0, 4.0), [2, 3]), ((29.0, 4.0), [3])]                                   # samples 24..32, 25..33: the grid's last block
    with vt.Extractor(0) as ex:
        for (c, r), want in cases:
            ex.terrain_init(32, 32, 32)
            ref = oracle_mod.Terrain(32, 32, 32)
            spec = ("sphere", ((c, c, c), r, True))
            n_dirty, _ = ex.terrain_update([gpu_struct(spec)])
            dirty = ex.terrain_dirty_blocks()
            for k in range(3):
                assert sorted(set(dirty[:, k])) == want, (c, r, k)
            assert n_dirty == len(want) ** 3 and np.array_equal(dirty, stamp_twin.twin_update(ref, oracle_mod, [spec], {})), (c, r)
            assert np.array_equal(bits(ex.terrain_read_samples()), bits(ref.grid)), (c, r)
