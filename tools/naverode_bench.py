#!/usr/bin/env python3
"""The agent radius (vtmc_nav_distance_build, vtmc_nav_erode) measured on the fBm-over-a-ramp benchmark terrain, box = everything,
1024^3 cells by default: the world and the nav parameters of tools/navfield_bench.py.

  nav_build     vtmc_terrain_nav_build of the same box in the same process, host wall time and the sum of its stages' device time
                (median of --reps after a warm-up): the first yardstick
  span_copy     a plain device-to-device copy of as many bytes as the span array holds (32 per span), device time from events: the floor
                of anything that touches every span once
  distance      vtmc_nav_distance_build at each radius of --radii (columns): host wall time, the device time of the border test and of the
                rounds (with the conversion to int32) from vtmc_debug_naverode_ms, the rounds, the time per round, the border count
  erode         vtmc_nav_erode at each radius, every repeat on a fresh nav build (the erode replaces it; the build is not timed with it):
                host wall time, the device time of its four stages (border test, rounds, compaction, relabelling with the host's
                read-backs of its rounds), and the spans kept

There is no threshold: nothing ran this before.  Every time is reported beside its ratio to the nav build and to the plain copy.  Prints
one JSON line; --out DIR also writes it to DIR/naverode_bench.json."""
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


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 2, 4, 8], help="columns")
    ap.add_argument("--agent-height", type=int, default=4, help="samples")
    ap.add_argument("--max-step", type=float, default=1.0, help="grid units")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    rec = {"tool": "tools/naverode_bench.py", "cells": n, "reps": a.reps, "agent_height_samples": a.agent_height, "max_step_grid_units": a.max_step}
    import torch
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        lo, up = (ctypes.c_float * 3)(*everything["lower"]), (ctypes.c_float * 3)(*everything["upper"])
        nav_params, count = _lib.NavParamsStruct(a.agent_height, a.max_step, (1 << 31) - 1, 0), ctypes.c_int32()
        nav_ms, ms = (ctypes.c_float * 8)(), (ctypes.c_float * 5)()

        def nav_build():
            ex._check(L.vtmc_terrain_nav_build(h, ctypes.byref(lo), ctypes.byref(up), ctypes.byref(nav_params), ctypes.byref(count)))
        nav_build()   # the warm-up: the buffers are allocated here
        walls, stages = [], []
        for _ in range(a.reps):
            walls.append(timed_ms(nav_build))
            ex._check(L.vtmc_debug_nav_ms(h, ctypes.byref(nav_ms)))
            stages.append(sum(list(nav_ms)[:7]))
        spans = count.value
        nav_wall, nav_dev = float(np.median(walls)), float(np.median(stages))
        rec["nav_build"] = {"wall_ms_median": round(nav_wall, 3), "stages_ms_median": round(nav_dev, 3), "spans": spans}
        # the floor: as many bytes as the spans, copied once on the device
        src, dst = torch.zeros(32 * spans, dtype=torch.uint8, device="cuda"), torch.empty(32 * spans, dtype=torch.uint8, device="cuda")
        copies = []
        for i in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            if i:
                copies.append(e0.elapsed_time(e1))
        copy_ms = float(np.median(copies))
        del src, dst
        rec["span_copy"] = {"bytes": 32 * spans, "device_ms_median": round(copy_ms, 4), "gb_per_s_read_plus_write": round(2 * 32 * spans / copy_ms / 1e6, 1)}

        def ratios(device_ms):
            return {"over_nav_build_stages": round(device_ms / nav_dev, 3), "over_span_copy": round(device_ms / copy_ms, 2)}
        rec["distance"], rec["erode"] = {}, {}
        for radius in a.radii:
            p = _lib.NavErodeParamsStruct(radius, 0, (ctypes.c_int32 * 2)(0, 0))
            walls, rows = [], []
            for i in range(a.reps + 1):
                wall = timed_ms(lambda: ex._check(L.vtmc_nav_distance_build(h, ctypes.byref(p), ctypes.byref(count))))
                ex._check(L.vtmc_debug_naverode_ms(h, ctypes.byref(ms)))
                if i:
                    walls.append(wall), rows.append(list(ms))
            med = np.median(np.asarray(rows), axis=0)
            rounds = int(med[4])
            rec["distance"]["radius %d" % radius] = dict(wall_ms_median=round(float(np.median(walls)), 3), border_test_ms=round(float(med[0]), 4),
                                                         rounds_ms=round(float(med[1]), 4), rounds=rounds,
                                                         ms_per_round=round(float(med[1]) / rounds, 4) if rounds else None, borders=count.value,
                                                         **ratios(float(med[0] + med[1])))
        for radius in a.radii:
            p = _lib.NavErodeParamsStruct(radius, 0, (ctypes.c_int32 * 2)(0, 0))
            walls, rows = [], []
            for i in range(a.reps + 1):
                nav_build()
                wall = timed_ms(lambda: ex._check(L.vtmc_nav_erode(h, ctypes.byref(p), ctypes.byref(count))))
                ex._check(L.vtmc_debug_naverode_ms(h, ctypes.byref(ms)))
                if i:
                    walls.append(wall), rows.append(list(ms))
            med = np.median(np.asarray(rows), axis=0)
            rec["erode"]["radius %d" % radius] = dict(wall_ms_median=round(float(np.median(walls)), 3), border_test_ms=round(float(med[0]), 4),
                                                      rounds_ms=round(float(med[1]), 4), compaction_ms=round(float(med[2]), 4),
                                                      relabel_ms=round(float(med[3]), 4), rounds=int(med[4]), kept=count.value,
                                                      over_nav_build_wall=round(float(np.median(walls)) / nav_wall, 3), **ratios(float(med[:4].sum())))
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "naverode_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
