#!/usr/bin/env python3
"""Undo / redo of terrain edits (vtmc_terrain_set_history / _undo / _redo), measured against the edits they take back:

  edits       the interactive edit loop of tools/edit_latency.py on the demo world (256 x 72 x 256 cells, plane at 30.5, seed 1): 200
              sphere edits r = 10 alternating add / erode after 20 warm-up edits, host time per vtmc_terrain_update (median, p90),
              with history off, then with history on (the same edits on a fresh world)
  undo, redo  the 200 recorded edits undone one call at a time, then redone (host time per call, median, p90)
  world_build bench.py's terrain sub-record world (1024 x 256 x 1024 cells, island heightmap + 40 river cylinders, ONE update):
              the best of the last 3 of 4 builds, history off, then on (a journal that holds the whole grid)

Kernel times come from `rocprofv3 --kernel-trace --stats` over a run of this tool (--quick keeps that run short).  Prints one JSON line;
--out DIR also writes it to DIR/history_bench.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def stats(us):
    return {"median_us": round(float(np.median(us)), 1), "p90_us": round(float(np.percentile(us, 90)), 1)}


def demo_edits(ex, n_edits, history_bytes):
    """edit_latency.py's world; history (if any) is switched on after the plane, so the steps are the edits alone."""
    rng = np.random.default_rng(1)
    ex.terrain_init(256, 72, 256, 1.0, (0.0, 0.0, 0.0), 1)
    ex.terrain_update([vt.PlaneModifier(30.5, (-1, -1), (300, 300), True)])
    ex.terrain_set_history(history_bytes)
    lat = []
    for i in range(n_edits + 20):
        c = (float(rng.uniform(20, 236)), 30.0 + float(rng.uniform(-4, 4)), float(rng.uniform(20, 236)))
        m = vt.SphereModifier(c, 10.0, bool(i & 1))
        if i == 20 and history_bytes:
            ex.terrain_set_history(history_bytes)   # the warm-up edits are not part of the undone run
        dt, _ = timed(lambda: ex.terrain_update([m]))
        if i >= 20:
            lat.append(dt)
    return np.array(lat)


def world_mods():
    """bench.py terrain_sub_record's world build, same seed."""
    rng = np.random.default_rng(3)
    W, E, H = 1024, 256, 1024
    u = np.linspace(-1, 1, 512, dtype=np.float32)[:, None]
    v = np.linspace(-1, 1, 512, dtype=np.float32)[None, :]
    hm = (0.55 * np.exp(-2.5 * (u * u + v * v)) + 0.06 * np.sin(7 * u) * np.cos(5 * v) + 0.12).astype(np.float32)
    owners = [vt.IslandModifier(hm * E, float(W), float(H), float(E), True)]
    for _ in range(40):
        start = (float(rng.uniform(0.2, 0.8) * W), float(rng.uniform(0.25, 0.5) * E), float(rng.uniform(0.2, 0.8) * H))
        d = (float(rng.normal()), float(rng.normal() * 0.1), float(rng.normal()))
        owners.append(vt.CylinderModifier(start, d, float(rng.uniform(0.05, 0.15) * W), float(rng.uniform(1.5, 3.0)), False))
    return owners, [m.to_struct() for m in owners], (W, E, H)


def world_build(ex, mods, dims, history_bytes, reps):
    ex.terrain_set_history(history_bytes)
    times = []
    for _ in range(reps):
        ex.terrain_init(*dims, 1.0, (0.0, 0.0, 0.0), 5)   # clears the history, keeps the budget
        dt, (nd, T) = timed(lambda: ex.terrain_update(mods))
        times.append(dt)
    return min(times[1:]) / 1e3, nd, T, ex.terrain_history()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="20 edits and 2 world builds per setting (the profiled run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_edits = 20 if args.quick else 200
    reps = 2 if args.quick else 4
    rec = {"tool": "tools/history_bench.py", "quick": bool(args.quick)}
    with vt.Extractor(0) as ex:
        off = demo_edits(ex, n_edits, 0)
        on = demo_edits(ex, n_edits, 64 << 20)
        n_undo, n_redo, used = ex.terrain_history()
        assert (n_undo, n_redo) == (n_edits, 0), (n_undo, n_redo)
        undo = np.array([timed(ex.terrain_undo)[0] for _ in range(n_edits)])
        redo = np.array([timed(ex.terrain_redo)[0] for _ in range(n_edits)])
        rec["demo_world"] = {"world": "256x72x256 cells, plane at 30.5 + %d sphere edits r = 10 (alternating add / erode), seed 1" % n_edits,
                             "edit_history_off": stats(off), "edit_history_on": stats(on), "undo": stats(undo), "redo": stats(redo),
                             "journal_bytes_for_the_edits": int(used), "journal_bytes_per_edit_mean": round(used / n_edits)}
    owners, mods, dims = world_mods()
    with vt.Extractor(0) as ex:
        ms_off, nd, T, _ = world_build(ex, mods, dims, 0, reps)
        ms_on, nd_on, T_on, hist = world_build(ex, mods, dims, 2 << 30, reps)
        assert (nd_on, T_on) == (nd, T) and hist[0] == 1, (nd_on, T_on, nd, T, hist)
        rec["world_build"] = {"world": "%dx%dx%d cells, IslandModifier (512^2 heightmap) + 40 river cylinders, one update" % dims,
                              "update_ms_history_off": round(ms_off, 3), "update_ms_history_on": round(ms_on, 3),
                              "delta_ms": round(ms_on - ms_off, 3), "journal_bytes": int(hist[2]), "dirty_blocks": int(nd), "triangles": int(T)}
    del owners
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "history_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
