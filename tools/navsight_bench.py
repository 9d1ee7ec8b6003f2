#!/usr/bin/env python3
"""The any-angle paths (vtmc_nav_sight, vtmc_navfield_trace_smooth) measured on the fBm-over-a-ramp benchmark terrain of
tools/navfield_bench.py, box = everything, 1024^3 cells by default, a field of the largest region per entry of --goals, --agents agents
located on random spans.

  trace         vtmc_navfield_trace of the located agents with --max-len entries per row: host wall time, which holds the copy of the rows
                to the host (it has no stage clock).  The yardstick of the smoothed trace.
  smooth        vtmc_navfield_trace_smooth of the same starts and the same --max-len per max_look of --looks and per cost bound (0, any):
                host wall time, and the device time of the fill of the rows (with the packing of the links) and of the kernel from HIP events; the total waypoints, the traced spans per
                waypoint over the rows the plain trace did not cut, and the rows that fill --max-len.  Once more with rows of --short-len entries: what a host that knows
                its paths smooth to a few waypoints would ask for.
  locate        vtmc_nav_locate of as many positions: the yardstick of the sight query.
  sight         vtmc_nav_sight of every agent towards the span --ahead entries along its plain trace (or its last) and towards its row's
                last span: wall and kernel time, the visible pairs and the mean steps.

Every figure is a median of --reps after a warm-up; every timed call ends in a stream synchronise inside the library.  There is no threshold:
nothing ran this before.  Prints one JSON line; --out DIR also writes it to DIR/navsight_bench.json."""
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


def timed(fn, reps, device_ms=None):
    """(median wall ms, median of device_ms() per rep or None) after one warm-up call, in which the buffers are allocated."""
    fn()
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if device_ms:
            dev.append(device_ms())
    return float(np.median(wall)), (np.median(np.asarray(dev), axis=0).tolist() if device_ms else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--goals", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--agents", type=int, default=100000)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--short-len", type=int, default=32)
    ap.add_argument("--looks", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--ahead", type=int, default=32)
    ap.add_argument("--agent-height", type=int, default=4, help="samples")
    ap.add_argument("--max-step", type=float, default=1.0, help="grid units")
    ap.add_argument("--climb", type=float, default=1.0)
    ap.add_argument("--drop", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, A = a.cells, a.agents
    rec = {"tool": "tools/navsight_bench.py", "cells": n, "reps": a.reps, "agents": A, "max_len": a.max_len, "agent_height_samples": a.agent_height,
           "max_step_grid_units": a.max_step, "climb_cost": a.climb, "drop_cost": a.drop, "links_read_from": "smoothed trace: a packed 16-byte copy made in the call; sight: the 32-byte spans"}
    rng = np.random.default_rng(7)
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        spans, offsets, first, ext = ex.terrain_nav(everything["lower"], everything["upper"], _lib.NavParamsStruct(a.agent_height, a.max_step, (1 << 31) - 1, 0))
        regions, sizes = np.unique(spans["region"], return_counts=True)
        inside = np.nonzero(spans["region"] == regions[np.argmax(sizes)])[0]
        rec["nav"] = {"spans": len(spans), "regions": len(regions), "largest_region_spans": int(sizes.max())}
        # the agents: near random spans, as tools/navfield_bench.py places them
        pick = rng.integers(0, len(spans), A)
        col = np.searchsorted(offsets, pick, side="right") - 1
        agents = np.stack([first[0] + col % ext[0] + rng.uniform(-0.45, 0.45, A), spans["height"][pick] + rng.uniform(-0.5, 0.5, A),
                           first[2] + col // ext[0] + rng.uniform(-0.45, 0.45, A)], axis=1).astype(np.float32)
        located = np.zeros(A, np.int32)
        locate_ms, _ = timed(lambda: ex._check(L.vtmc_nav_locate(h, agents.ctypes.data, A, 1.0, 1.0, located.ctypes.data)), a.reps)
        rec["locate"] = {"wall_ms_median": round(locate_ms, 3), "located": int((located >= 0).sum())}
        ms = (ctypes.c_float * 2)()

        def clock():
            ex._check(L.vtmc_debug_navsight_ms(h, ctypes.byref(ms)))
            return list(ms)
        field_params = vt.NavFieldParams(a.climb, a.drop).to_struct()
        rec["fields"] = {}
        for n_goals in a.goals:
            goals = np.zeros(n_goals, vt.NAVFIELD_GOAL_DTYPE)
            goals["span"] = inside[(np.arange(n_goals) * 2 + 1) * len(inside) // (2 * n_goals)]
            reached = ctypes.c_int32()
            ex._check(L.vtmc_navfield_build(h, goals.ctypes.data, n_goals, ctypes.byref(field_params), ctypes.byref(reached)))
            out = rec["fields"]["%d goals" % n_goals] = {"reached": reached.value}
            paths, lengths = np.zeros((A, a.max_len), np.int32), np.zeros(A, np.int32)
            trace_ms, _ = timed(lambda: ex._check(L.vtmc_navfield_trace(h, located.ctypes.data, A, a.max_len, paths.ctypes.data, lengths.ctypes.data)), a.reps)
            traced = int(lengths.sum())
            out["trace"] = {"wall_ms_median": round(trace_ms, 3), "traced": int((lengths > 0).sum()), "traced_spans": traced,
                            "rows_cut_at_max_len": int((lengths == a.max_len).sum()), "mean_length": round(float(lengths[lengths > 0].mean()), 1)}
            whole = (lengths > 0) & (lengths < a.max_len)   # rows the plain trace did not cut: both calls cover the whole path to the goal
            out["trace"]["whole_rows"] = int(whole.sum())
            out["smooth"] = {}
            for max_len in (a.max_len, a.short_len):
                rows, lens = np.zeros((A, max_len), np.int32), np.zeros(A, np.int32)
                for look in a.looks:
                    for extra, name in ((0, "bound 0"), (_lib.NAVSIGHT_ANY_COST, "any cost")):
                        p = _lib.NavSightParamsStruct(look, extra, 0, 0)
                        wall, dev = timed(lambda: ex._check(L.vtmc_navfield_trace_smooth(h, located.ctypes.data, A, max_len, ctypes.byref(p), rows.ctypes.data,
                                                                                         lens.ctypes.data)), a.reps, clock)
                        out["smooth"]["max_len %d, max_look %d, %s" % (max_len, look, name)] = {
                            "wall_ms_median": round(wall, 3), "fill_ms": round(dev[0], 4), "kernel_ms": round(dev[1], 4), "waypoints": int(lens.sum()),
                            "rows_at_max_len": int((lens == max_len).sum()), "mean_waypoints": round(float(lens[lens > 0].mean()), 2),
                            "traced_spans_per_waypoint_whole_rows": round(int(lengths[whole].sum()) / max(int(lens[whole].sum()), 1), 2),
                            "over_trace_wall": round(wall / trace_ms, 3)}
            # the sight query: towards the span --ahead entries along the plain trace, and towards the row's last span
            valid = lengths > 0
            rowsel = np.arange(A)
            last = np.maximum(lengths - 1, 0)
            targets = {"%d ahead" % a.ahead: np.where(valid, paths[rowsel, np.minimum(last, a.ahead)], -1).astype(np.int32),
                       "row end": np.where(valid, paths[rowsel, last], -1).astype(np.int32)}
            hits = np.zeros(A, vt.NAVSIGHT_HIT_DTYPE)
            out["sight"] = {}
            for name, to in targets.items():
                wall, dev = timed(lambda: ex._check(L.vtmc_nav_sight(h, located.ctypes.data, to.ctypes.data, A, hits.ctypes.data)), a.reps, clock)
                out["sight"][name] = {"wall_ms_median": round(wall, 3), "kernel_ms": round(dev[1], 4), "pairs": int(valid.sum()),
                                      "visible": int(((hits["last"] == to) & valid).sum()), "mean_steps": round(float(hits["steps"][valid].mean()), 1),
                                      "over_locate_wall": round(wall / locate_ms, 2)}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "navsight_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
