#!/usr/bin/env python3
"""The flow fields (vtmc_navfield_build, vtmc_nav_locate, vtmc_navfield_trace) measured on the fBm-over-a-ramp benchmark terrain, box =
everything, 1024^3 cells by default.

  nav_build     vtmc_terrain_nav_build of the same box in the same process, host wall time and the sum of its stages' device time
                (median of --reps after a warm-up): the yardstick
  field         vtmc_navfield_build for 1, 16 and 1024 goals spread evenly over the spans of the largest region: host wall time, the
                device time of its three stages from HIP events (edge costs with goals; the rounds, with the host's read-backs of the flag
                words between the batches in it; next with the count), the rounds, and what was reached (median of --reps after a warm-up)
  agents        --agents positions near random spans: vtmc_nav_locate, then vtmc_navfield_trace of the located spans with --max-len
                entries per row, host wall time each (they hold the copies of the batch to the device and of the answers back)

There is no threshold: nothing ran this before.  Prints one JSON line; --out DIR also writes it to DIR/navfield_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt
from volumetricterrain_amd import _lib


def median_ms(fn, reps):
    fn()   # the warm-up: the buffers are allocated here
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--goals", type=int, nargs="+", default=[1, 16, 1024])
    ap.add_argument("--agents", type=int, default=100000)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--agent-height", type=int, default=4, help="samples")
    ap.add_argument("--max-step", type=float, default=1.0, help="grid units")
    ap.add_argument("--climb", type=float, default=1.0)
    ap.add_argument("--drop", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    rec = {"tool": "tools/navfield_bench.py", "cells": n, "reps": a.reps, "agent_height_samples": a.agent_height, "max_step_grid_units": a.max_step,
           "climb_cost": a.climb, "drop_cost": a.drop, "run_spans": 4096, "rounds_per_read_back": 4}   # csrc/terrain_navfield.h: kNavFieldRun, kNavFieldBatch
    rng = np.random.default_rng(7)
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        lo, up = (ctypes.c_float * 3)(*everything["lower"]), (ctypes.c_float * 3)(*everything["upper"])
        nav_params, count = _lib.NavParamsStruct(a.agent_height, a.max_step, (1 << 31) - 1, 0), ctypes.c_int32()
        nav_ms = (ctypes.c_float * 8)()
        stages = []

        def nav_build():
            ex._check(L.vtmc_terrain_nav_build(h, ctypes.byref(lo), ctypes.byref(up), ctypes.byref(nav_params), ctypes.byref(count)))
            ex._check(L.vtmc_debug_nav_ms(h, ctypes.byref(nav_ms)))
            stages.append(sum(list(nav_ms)[:7]))
        rec["nav_build"] = {"wall_ms_median": round(median_ms(nav_build, a.reps), 3), "stages_ms_median": round(float(np.median(stages[1:])), 3)}
        spans, offsets, first, ext = ex.nav_read()
        regions, sizes = np.unique(spans["region"], return_counts=True)
        inside = np.nonzero(spans["region"] == regions[np.argmax(sizes)])[0]
        rec["nav_build"].update(spans=len(spans), regions=len(regions), largest_region_spans=int(sizes.max()))
        params = vt.NavFieldParams(a.climb, a.drop).to_struct()
        rec["field"] = {}
        for n_goals in a.goals:
            goals = np.zeros(n_goals, vt.NAVFIELD_GOAL_DTYPE)
            goals["span"] = inside[(np.arange(n_goals) * 2 + 1) * len(inside) // (2 * n_goals)]
            ms, rows = (ctypes.c_float * 4)(), []

            def field_build():
                ex._check(L.vtmc_navfield_build(h, goals.ctypes.data, n_goals, ctypes.byref(params), ctypes.byref(count)))
                ex._check(L.vtmc_debug_navfield_ms(h, ctypes.byref(ms)))
                rows.append(list(ms))
            wall = median_ms(field_build, a.reps)
            med = np.median(np.asarray(rows[1:]), axis=0)
            rec["field"]["%d goals" % n_goals] = {"wall_ms_median": round(wall, 3), "setup_ms": round(float(med[0]), 4), "rounds_ms": round(float(med[1]), 3),
                                                  "next_ms": round(float(med[2]), 4), "rounds": int(med[3]), "reached": count.value,
                                                  "over_nav_build_wall": round(wall / rec["nav_build"]["wall_ms_median"], 2)}
        # the agents, on the last field
        pick = rng.integers(0, len(spans), a.agents)
        col = np.searchsorted(offsets, pick, side="right") - 1
        agents = np.stack([first[0] + col % ext[0] + rng.uniform(-0.45, 0.45, a.agents), spans["height"][pick] + rng.uniform(-0.5, 0.5, a.agents),
                           first[2] + col // ext[0] + rng.uniform(-0.45, 0.45, a.agents)], axis=1).astype(np.float32)
        located = np.zeros(a.agents, np.int32)
        paths, lengths = np.zeros((a.agents, a.max_len), np.int32), np.zeros(a.agents, np.int32)
        locate_ms = median_ms(lambda: ex._check(L.vtmc_nav_locate(h, agents.ctypes.data, a.agents, 1.0, 1.0, located.ctypes.data)), a.reps)
        trace_ms = median_ms(lambda: ex._check(L.vtmc_navfield_trace(h, located.ctypes.data, a.agents, a.max_len, paths.ctypes.data, lengths.ctypes.data)), a.reps)
        rec["agents"] = {"n": a.agents, "max_len": a.max_len, "locate_wall_ms_median": round(locate_ms, 3), "located": int((located >= 0).sum()),
                         "trace_wall_ms_median": round(trace_ms, 3), "traced": int((lengths > 0).sum()), "rows_cut_at_max_len": int((lengths == a.max_len).sum()),
                         "mean_length": round(float(lengths[lengths > 0].mean()) if (lengths > 0).any() else 0.0, 1)}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "navfield_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
