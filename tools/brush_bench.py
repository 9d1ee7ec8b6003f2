#!/usr/bin/env python3
"""Sculpt brushes (VTMC_MOD_SMOOTH / VTMC_MOD_FLATTEN) measured against the sphere edit they sit beside:

  edits               the interactive edit loop of tools/edit_latency.py on the demo world (256 x 72 x 256 cells, plane at 30.5, seed
                      1): 200 edits r = 10 after 20 warm-up edits, run three times on a fresh world each -- sphere (alternating add /
                      erode), smooth (s = 1), flatten (s = 1, normal near +y) -- host time per vtmc_terrain_update (median, p90), with
                      history off, then with history on
  whole_world_smooth  bench.py's terrain sub-record world (1024 x 256 x 1024 cells, island heightmap + 40 river cylinders, one update),
                      then one smooth whose box covers the grid (stage + smooth over 1026 x 258 x 1026 samples, plus the extraction of
                      every block): the best of the last 3 of 4 updates, history off, then on

Kernel times come from `rocprofv3 --kernel-trace --stats` over a run of this tool (--quick keeps that run short).  Prints one JSON line;
--out DIR also writes it to DIR/brush_bench.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import volumetricterrain_amd as vt
from history_bench import stats, timed, world_mods


def brush(kind, i, rng):
    c = (float(rng.uniform(20, 236)), 30.0 + float(rng.uniform(-4, 4)), float(rng.uniform(20, 236)))
    if kind == "sphere":
        return vt.SphereModifier(c, 10.0, bool(i & 1))
    if kind == "smooth":
        return vt.SmoothModifier(c, 10.0, 1.0)
    n = (float(rng.uniform(-0.3, 0.3)), 1.0, float(rng.uniform(-0.3, 0.3)))
    return vt.FlattenModifier(c, n, 10.0, 1.0)


def demo_edits(ex, kind, n_edits, history_bytes):
    """edit_latency.py's world and edit positions; history (if any) is switched on after the warm-up edits."""
    rng = np.random.default_rng(1)
    ex.terrain_init(256, 72, 256, 1.0, (0.0, 0.0, 0.0), 1)
    ex.terrain_update([vt.PlaneModifier(30.5, (-1, -1), (300, 300), True)])
    ex.terrain_set_history(0)
    lat = []
    for i in range(n_edits + 20):
        m = brush(kind, i, rng)
        if i == 20 and history_bytes:
            ex.terrain_set_history(history_bytes)
        dt, _ = timed(lambda: ex.terrain_update([m]))
        if i >= 20:
            lat.append(dt)
    if history_bytes:
        assert ex.terrain_history()[0] == n_edits
    return np.array(lat)


def whole_world_smooth(ex, mods, dims, history_bytes, reps):
    W, E, H = dims
    ex.terrain_set_history(0)
    ex.terrain_init(*dims, 1.0, (0.0, 0.0, 0.0), 5)
    ex.terrain_update(mods)
    ex.terrain_set_history(history_bytes)
    m = vt.SmoothModifier((W / 2.0, E / 2.0, H / 2.0), 1200.0, 1.0)   # box c -/+ r covers the grid
    times = []
    for _ in range(reps):
        dt, (nd, T) = timed(lambda: ex.terrain_update([m]))
        times.append(dt)
    return min(times[1:]) / 1e3, nd, T, ex.terrain_history()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="20 edits and 2 whole-world smooths per setting (the profiled run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_edits = 20 if args.quick else 200
    reps = 2 if args.quick else 4
    rec = {"tool": "tools/brush_bench.py", "quick": bool(args.quick)}
    edits = {"world": "256x72x256 cells, plane at 30.5 + %d edits r = 10 per brush, seed 1, a fresh world per run" % n_edits}
    with vt.Extractor(0) as ex:
        for kind in ("sphere", "smooth", "flatten"):
            off = demo_edits(ex, kind, n_edits, 0)
            on = demo_edits(ex, kind, n_edits, 64 << 20)
            edits[kind] = {"history_off": stats(off), "history_on": stats(on)}
    for kind in ("smooth", "flatten"):
        edits[kind]["median_minus_sphere_us"] = round(edits[kind]["history_off"]["median_us"] - edits["sphere"]["history_off"]["median_us"], 1)
    rec["edits"] = edits
    owners, mods, dims = world_mods()
    with vt.Extractor(0) as ex:
        ms_off, nd, T, _ = whole_world_smooth(ex, mods, dims, 0, reps)
        ms_on, nd_on, T_on, hist = whole_world_smooth(ex, mods, dims, 2 << 30, reps)
        assert nd_on == nd and hist[0] >= 1, (nd_on, nd, hist)
        samples = (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2)
        rec["whole_world_smooth"] = {
            "world": "%dx%dx%d cells, IslandModifier (512^2 heightmap) + 40 river cylinders, then one smooth (s = 1) over every sample" % dims,
            "update_ms_history_off": round(ms_off, 3), "update_ms_history_on": round(ms_on, 3), "dirty_blocks": int(nd), "triangles": int(T),
            "samples": samples, "stage_plus_smooth_bytes": 4 * samples * 4,   # stage: read + write; smooth: stage read + grid write
            "journal_bytes_per_step": int(hist[2] // max(hist[0], 1))}
    del owners
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "brush_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
