"""Undo / redo of terrain edits (vtmc_terrain_set_history / _undo / _redo / _history): the journal restores the resident grid bit for
bit and an undo or redo returns what an update of the same dirty set returns.  The CPU twin (terrain_twin.py, on oracle.Terrain) is
rewound by writing a saved copy into its memory while its event counter runs on, as the library's does.

Grids are compared as uint32 (NaN payloads, -0); triangles as in test_terrain.py: offsets and `block` exact, floats within 1e-5."""
import os
import re

import numpy as np
import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib
from terrain_twin import assert_grid, assert_triangles, bits, both_update, gpu_mod, island_heightmap, no_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = [
    "int32_t vtmc_terrain_set_history(vtmc_ctx *ctx, int64_t max_bytes);",
    "int32_t vtmc_terrain_undo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count);",
    "int32_t vtmc_terrain_redo(vtmc_ctx *ctx, int32_t *n_dirty_blocks, int32_t *tri_count);",
    "int32_t vtmc_terrain_history(const vtmc_ctx *ctx, int32_t *n_undo, int32_t *n_redo, int64_t *bytes_used);",
]
NAMES = [re.search(r"(vtmc_\w+)\(", p).group(1) for p in PROTOTYPES]

DIMS, SCALE, ORIGIN, SEED = (64, 24, 48), 1.0, (0.0, 0.0, 0.0), 1234
OUTSIDE = ("sphere", ((-50.0, -50.0, -50.0), 3.0, True))
STEPS = [
    [("plane", (9.375, (0, 0), (70, 70), True)), ("sphere", ((20.5, 10.25, 30.0), 7.5, True))],   # a world build in one call
    [("sphere", ((40.0, 9.0, 20.0), 6.0, False))],
    [("cylinder", ((5.0, 12.0, 5.0), (1.0, 0.25, 0.5), 30.0, 3.0, False))],
    [("sphere", ((30.0, 10.0, 24.0), 6.0, True)), ("sphere", ((33.0, 11.0, 26.0), 5.0, False))],  # two overlapping boxes
]


# -- CPU: the interface ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_history_functions():
    text = " ".join(open(os.path.join(ROOT, "include", "vtmc.h")).read().split())
    for p in PROTOTYPES:
        assert p in text, p


def test_binding_lists_the_history_symbols():
    for name in NAMES:
        assert name in _lib.SYMBOLS, name


def test_extractor_has_the_history_methods():
    for name in ("terrain_set_history", "terrain_undo", "terrain_redo", "terrain_history"):
        assert callable(getattr(vt.Extractor, name, None)), name


def test_integration_guide_has_a_dllimport_stub_for_each():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\[DllImport\([^\]]*\)\]\s*public static extern\s+int\s+%s\s*\(" % name, text), name


# -- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_every_step_restores_bitwise(oracle_mod):
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(64 << 20)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        snaps, results = [ref.grid.copy()], []
        for specs in STEPS:
            (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, specs)
            assert_grid(ex, ref.grid)
            assert n_dirty == len(dirty) and np.array_equal(ex.terrain_dirty_blocks(), dirty)
            snaps.append(ref.grid.copy())
            results.append((n_dirty, T, dirty))
        (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, [OUTSIDE])   # writes nothing: no step
        assert (n_dirty, T) == (0, 0) and len(dirty) == 0
        assert_grid(ex, ref.grid)
        nu, nr, used = ex.terrain_history()
        assert (nu, nr) == (4, 0) and used > 0
        for k in reversed(range(4)):
            n_dirty, T = ex.terrain_undo()
            want_n, want_T, dirty = results[k]
            assert_grid(ex, snaps[k])
            assert n_dirty == want_n and np.array_equal(ex.terrain_dirty_blocks(), dirty)
            assert_triangles(ex, oracle_mod, snaps[k], dirty, T)
        assert ex.terrain_history() == (0, 4, used)
        no_result(ex.terrain_undo)
        for k in range(4):
            n_dirty, T = ex.terrain_redo()
            want_n, want_T, dirty = results[k]
            assert_grid(ex, snaps[k + 1])
            assert n_dirty == want_n and T == want_T and np.array_equal(ex.terrain_dirty_blocks(), dirty)
            assert_triangles(ex, oracle_mod, snaps[k + 1], dirty, T)
        assert ex.terrain_history() == (4, 0, used)
        no_result(ex.terrain_redo)


@pytest.mark.gpu
def test_gpu_new_edit_after_undo_discards_redo(oracle_mod):
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(64 << 20)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        mems = []
        for specs in STEPS[:3]:
            both_update(ex, ref, oracle_mod, specs)
            mems.append(ref._mem.copy())
        ex.terrain_undo()
        ex.terrain_undo()
        assert ex.terrain_history()[:2] == (1, 2)
        edit = [("sphere", ((24.0, 12.0, 20.0), 5.5, False))]
        ref._mem[...] = mems[0]            # rewound two steps; the event counter is not
        (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, edit)
        assert ex.terrain_history()[:2] == (2, 0)
        no_result(ex.terrain_redo)
        assert_grid(ex, ref.grid)
        assert np.array_equal(ex.terrain_dirty_blocks(), dirty)
        assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
        ex.terrain_undo()
        assert_grid(ex, mems[0].transpose(2, 1, 0))


@pytest.mark.gpu
def test_gpu_calls_that_write_nothing_keep_redo(oracle_mod):
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(64 << 20)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        for specs in STEPS[:2]:
            both_update(ex, ref, oracle_mod, specs)
        after = ref.grid.copy()
        ex.terrain_undo()
        assert ex.terrain_history()[:2] == (1, 1)
        assert ex.terrain_update([]) == (0, 0)
        (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, [OUTSIDE])
        assert T == 0 and n_dirty == len(dirty)
        assert ex.terrain_history()[:2] == (1, 1)
        ex.terrain_redo()
        assert_grid(ex, after)
        assert ex.terrain_history()[:2] == (2, 0)


@pytest.mark.gpu
def test_gpu_budget(oracle_mod):
    # r = 5 at integer centres: samples c-5 .. c+5 on every axis, 11^3 * 4 = 5324 bytes -> 5376 with the 256-byte rounding
    S = 5376
    centres = [(20.0, 12.0, 20.0), (40.0, 12.0, 20.0), (20.0, 12.0, 36.0)]
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(1 << 20)
        both_update(ex, ref, oracle_mod, [("sphere", (centres[0], 5.0, True))])
        assert ex.terrain_history() == (1, 0, S)
        ex.terrain_set_history(int(2.5 * S))          # clears the history
        assert ex.terrain_history() == (0, 0, 0)
        after = []
        for c in centres:
            both_update(ex, ref, oracle_mod, [("sphere", (c, 5.0, False))])
            after.append(ref.grid.copy())
        assert ex.terrain_history() == (2, 0, 2 * S)  # the oldest step made room for the third
        ex.terrain_undo()
        ex.terrain_undo()
        no_result(ex.terrain_undo)
        assert_grid(ex, after[0])
        assert ex.terrain_history() == (0, 2, 2 * S)
        ex.terrain_redo()
        ex.terrain_redo()
        assert_grid(ex, after[2])
        # a step larger than the budget (r = 7: 15^3 samples, 13568 bytes) clears the history; the update itself goes through
        both_update(ex, ref, oracle_mod, [("sphere", ((30.0, 12.0, 24.0), 7.0, True))])
        assert ex.terrain_history() == (0, 0, 0)
        assert_grid(ex, ref.grid)
        no_result(ex.terrain_undo)
        # budget 0: history off
        ex.terrain_set_history(0)
        both_update(ex, ref, oracle_mod, [("sphere", ((30.0, 12.0, 30.0), 5.0, True))])
        assert ex.terrain_history() == (0, 0, 0)
        no_result(ex.terrain_undo)
        assert_grid(ex, ref.grid)
        # terrain_init clears the history and keeps the budget
        ex.terrain_set_history(1 << 20)
        both_update(ex, ref, oracle_mod, [("sphere", ((30.0, 12.0, 30.0), 5.0, False))])
        assert ex.terrain_history()[:2] == (1, 0)
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        assert ex.terrain_history() == (0, 0, 0)
        no_result(ex.terrain_undo)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        both_update(ex, ref, oracle_mod, [("sphere", (centres[0], 5.0, True))])
        assert ex.terrain_history() == (1, 0, S)
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_set_history(-1)
        assert e.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_history_is_off_by_default(oracle_mod):
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ref = oracle_mod.Terrain(*DIMS, SCALE, ORIGIN, SEED)
        for specs in STEPS:
            (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, specs)
            assert_grid(ex, ref.grid)
            assert np.array_equal(ex.terrain_dirty_blocks(), dirty)
            assert_triangles(ex, oracle_mod, ref.grid, dirty, T)
        assert ex.terrain_history() == (0, 0, 0)
        no_result(ex.terrain_undo)
        no_result(ex.terrain_redo)
        assert_grid(ex, ref.grid)


@pytest.mark.gpu
def test_gpu_full_rebuild_undo(oracle_mod):
    dims, seed = (128, 48, 128), 77
    specs = [("island", (island_heightmap(height=28.0), 128.0, 128.0, 60.0, True)),
             ("cylinder", ((16.0, 20.0, 20.0), (1.0, -0.1, 0.6), 80.0, 3.0, False))]
    n_blocks = 16 * 6 * 16
    with vt.Extractor(0) as ex:
        ex.terrain_init(*dims, 1.0, ORIGIN, seed)
        ex.terrain_set_history(256 << 20)
        ref = oracle_mod.Terrain(*dims, 1.0, ORIGIN, seed)
        filled = ref.grid.copy()
        (n_dirty, T), dirty = both_update(ex, ref, oracle_mod, specs)
        assert n_dirty == len(dirty) == n_blocks and T > 5000
        assert_grid(ex, ref.grid)
        tris, offs = ex.read_triangles()
        n_dirty, T0 = ex.terrain_undo()
        assert n_dirty == n_blocks and T0 == 0
        assert_grid(ex, filled)
        assert len(ex.terrain_dirty_blocks()) == n_blocks
        n_dirty, T1 = ex.terrain_redo()
        assert n_dirty == n_blocks and T1 == T
        assert_grid(ex, ref.grid)
        got, got_offs = ex.read_triangles()
        assert np.array_equal(got_offs, offs) and np.array_equal(got["block"], tris["block"])
        for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
            assert np.abs(got[f] - tris[f]).max() <= 1e-5
        assert_triangles(ex, oracle_mod, ref.grid, dirty, T1)


@pytest.mark.gpu
def test_gpu_picking_follows_undo(oracle_mod):
    xs, zs = np.meshgrid(np.arange(22.0, 40.0, 0.75), np.arange(16.0, 32.0, 0.75))
    origins = np.stack([xs.ravel(), np.full(xs.size, 40.0), zs.ravel()], 1).astype(np.float32)
    directions = np.tile(np.array([0.05, -1.0, 0.02], np.float32), (len(origins), 1))
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(64 << 20)
        ex.terrain_update([gpu_mod(s) for s in STEPS[0]])
        before = ex.terrain_raycast(origins, directions)
        assert (before["triangle"] >= 0).all()
        ex.terrain_update([vt.SphereModifier((31.0, 10.0, 24.0), 6.0, True)])
        edited = ex.terrain_raycast(origins, directions)
        assert (edited["distance"] < before["distance"]).any()
        ex.terrain_undo()
        assert ex.terrain_raycast(origins, directions).tobytes() == before.tobytes()
        ex.terrain_redo()
        assert ex.terrain_raycast(origins, directions).tobytes() == edited.tobytes()


@pytest.mark.gpu
def test_gpu_indexed_undo_matches_a_fresh_extract():
    with vt.Extractor(0) as ex, vt.Extractor(0) as ex2:
        ex.terrain_init(*DIMS, SCALE, ORIGIN, SEED)
        ex.terrain_set_history(64 << 20)
        ex.set_output_mode(True)
        ex2.set_output_mode(True)
        for specs in STEPS:
            ex.terrain_update([gpu_mod(s) for s in specs])
        for _ in range(2):
            n_dirty, T = ex.terrain_undo()
            dirty = ex.terrain_dirty_blocks()
            assert len(dirty) == n_dirty and T > 0
            T2 = ex2.extract_grid(ex.terrain_read_samples(), dirty)
            assert T2 == T
            for a, b in zip(ex.read_indexed_mesh(), ex2.read_indexed_mesh()):
                assert a.tobytes() == b.tobytes()
        n_dirty, T = ex.terrain_redo()
        T2 = ex2.extract_grid(ex.terrain_read_samples(), ex.terrain_dirty_blocks())
        assert T2 == T
        for a, b in zip(ex.read_indexed_mesh(), ex2.read_indexed_mesh()):
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_gpu_demo_world_200_edits_round_trip():
    """tools/edit_latency.py's world and edit loop with history on: all 200 edits undone, then redone."""
    rng = np.random.default_rng(1)
    with vt.Extractor(0) as ex:
        ex.terrain_init(256, 72, 256, 1.0, (0.0, 0.0, 0.0), 1)
        ex.terrain_update([vt.PlaneModifier(30.5, (-1, -1), (300, 300), True)])
        ex.terrain_set_history(64 << 20)
        plane = ex.terrain_read_samples().copy()
        for i in range(200):
            c = (float(rng.uniform(20, 236)), 30.0 + float(rng.uniform(-4, 4)), float(rng.uniform(20, 236)))
            ex.terrain_update([vt.SphereModifier(c, 10.0, bool(i & 1))])
        final = ex.terrain_read_samples().copy()
        assert ex.terrain_history()[:2] == (200, 0)
        for _ in range(200):
            ex.terrain_undo()
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(plane))
        no_result(ex.terrain_undo)
        for _ in range(200):
            ex.terrain_redo()
        assert np.array_equal(bits(ex.terrain_read_samples()), bits(final))
        assert ex.terrain_history()[:2] == (200, 0)
