#!/usr/bin/env python3
"""The crowd (vtmc_navcrowd_spawn, vtmc_navcrowd_step) measured on the fBm-over-a-ramp benchmark terrain of tools/navfield_bench.py, box =
everything, 1024^3 cells by default, the field of --goals goals spread over the largest region, --agents agents on distinct random
reached spans.

  step          vtmc_navcrowd_step of --ticks ticks and of 1 tick, per max_detour (0, any), leaving on arrival: host wall time, and the device
                time of the ticks from HIP events; per tick both divided by the ticks.  The crowd is spawned anew before every timed call (not
                timed), so every call steps the same crowd; what the crowd did (moves of the last tick, arrived agents) is from the last call.
  spawn         vtmc_navcrowd_spawn itself: host wall time, the upload of the requests included.
  copy          a plain device-to-device copy of the agent array, with a device synchronise: the least a pass over the records can take.
  locate        vtmc_nav_locate of as many positions.
  trace         vtmc_navfield_trace of the same starts with rows of --max-len entries: the host route the crowd replaces.

Every figure is a median of --reps after a warm-up; every timed library call ends in a stream synchronise inside the library.  There is no
threshold: nothing ran this before.  With VTMC_LIB set to another build of the library (volumetricterrain_amd.build.build_variant) the same
run measures that build: the A/B of the two record layouts was such runs, alternating (profiles/r25/navcrowd).  Prints one JSON line;
--out DIR also writes it to DIR/navcrowd_bench.json."""
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


def timed(fn, reps, before=None, device_ms=None):
    """(median wall ms, median of device_ms() per rep or None) after one warm-up call; `before` runs ahead of every call, untimed."""
    wall, dev = [], []
    for rep in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
            if device_ms:
                dev.append(device_ms())
    return float(np.median(wall)), (float(np.median(dev)) if device_ms else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--goals", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=100000)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--agent-height", type=int, default=4, help="samples")
    ap.add_argument("--max-step", type=float, default=1.0, help="grid units")
    ap.add_argument("--climb", type=float, default=1.0)
    ap.add_argument("--drop", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, A = a.cells, a.agents
    rec = {"tool": "tools/navcrowd_bench.py", "library": os.path.basename(os.environ.get("VTMC_LIB", "libvtmc.so")), "cells": n, "reps": a.reps, "agents": A, "ticks": a.ticks,
           "goals": a.goals, "agent_height_samples": a.agent_height, "max_step_grid_units": a.max_step, "climb_cost": a.climb, "drop_cost": a.drop}
    rng = np.random.default_rng(7)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        spans, offsets, first, ext = ex.terrain_nav(everything["lower"], everything["upper"], _lib.NavParamsStruct(a.agent_height, a.max_step, (1 << 31) - 1, 0))
        regions, sizes = np.unique(spans["region"], return_counts=True)
        inside = np.nonzero(spans["region"] == regions[np.argmax(sizes)])[0]
        rec["nav"] = {"spans": len(spans), "regions": len(regions), "largest_region_spans": int(sizes.max())}
        goals = np.zeros(a.goals, vt.NAVFIELD_GOAL_DTYPE)
        goals["span"] = inside[(np.arange(a.goals) * 2 + 1) * len(inside) // (2 * a.goals)]
        field_params, reached = vt.NavFieldParams(a.climb, a.drop).to_struct(), ctypes.c_int32()
        ex._check(L.vtmc_navfield_build(h, goals.ctypes.data, a.goals, ctypes.byref(field_params), ctypes.byref(reached)))
        cells = ex.navfield_read()
        on = np.nonzero(cells["cost"] != _lib.NAVFIELD_UNREACHED)[0]
        A = min(A, len(on))
        starts = np.ascontiguousarray(rng.choice(on, A, replace=False).astype(np.int32))
        speeds = np.ascontiguousarray((300 + (7919 * np.arange(A, dtype=np.int64)) % 1500).astype(np.uint32))
        rec["field"] = {"reached": reached.value, "agents_placed": A}
        placed = ctypes.c_int32()

        def spawn():
            ex._check(L.vtmc_navcrowd_spawn(h, starts.ctypes.data, speeds.ctypes.data, A, ctypes.byref(placed)))
        ms = (ctypes.c_float * 1)()

        def clock():
            ex._check(L.vtmc_debug_navcrowd_ms(h, ctypes.byref(ms)))
            return ms[0]
        spawn_ms, _ = timed(spawn, a.reps)
        rec["spawn"] = {"wall_ms_median": round(spawn_ms, 3), "placed": placed.value}
        rec["step"] = {}
        for detour, name in ((0, "detour 0"), (_lib.NAVCROWD_ANY_DETOUR, "any detour")):
            p = _lib.NavCrowdParamsStruct(detour, _lib.NAVCROWD_LEAVE_ON_ARRIVAL, (ctypes.c_uint32 * 2)(0, 0))
            for ticks in (a.ticks, 1):
                wall, dev = timed(lambda: ex._check(L.vtmc_navcrowd_step(h, ctypes.byref(p), ticks)), a.reps, spawn, clock)
                info = ex.navcrowd_info()
                rec["step"]["%s, %d ticks" % (name, ticks)] = {"wall_ms_median": round(wall, 4), "device_ms_median": round(dev, 4), "wall_us_per_tick": round(wall * 1e3 / ticks, 3),
                                                               "device_us_per_tick": round(dev * 1e3 / ticks, 3), "occupying": info[1], "arrived": info[2],
                                                               "moved_last_tick": info[4]}
        # the yardsticks
        d_agents, _, count = ex.device_navcrowd()
        copy = ctypes.c_void_p()
        nbytes = count * vt.NAVCROWD_AGENT_DTYPE.itemsize
        assert hip.hipMalloc(ctypes.byref(copy), nbytes) == 0

        def device_copy():
            assert hip.hipMemcpy(copy, d_agents, nbytes, 3) == 0 and hip.hipDeviceSynchronize() == 0
        copy_ms, _ = timed(device_copy, a.reps)
        hip.hipFree(copy)
        rec["copy"] = {"wall_ms_median": round(copy_ms, 4), "bytes": nbytes}
        col = np.searchsorted(offsets, starts, side="right") - 1
        positions = np.stack([first[0] + col % ext[0] + rng.uniform(-0.45, 0.45, A), spans["height"][starts] + rng.uniform(-0.5, 0.5, A),
                              first[2] + col // ext[0] + rng.uniform(-0.45, 0.45, A)], axis=1).astype(np.float32)
        located = np.zeros(A, np.int32)
        locate_ms, _ = timed(lambda: ex._check(L.vtmc_nav_locate(h, positions.ctypes.data, A, 1.0, 1.0, located.ctypes.data)), a.reps)
        rec["locate"] = {"wall_ms_median": round(locate_ms, 3), "located": int((located >= 0).sum())}
        paths, lengths = np.zeros((A, a.max_len), np.int32), np.zeros(A, np.int32)
        trace_ms, _ = timed(lambda: ex._check(L.vtmc_navfield_trace(h, starts.ctypes.data, A, a.max_len, paths.ctypes.data, lengths.ctypes.data)), a.reps)
        rec["trace"] = {"wall_ms_median": round(trace_ms, 3), "max_len": a.max_len, "mean_length": round(float(lengths.mean()), 1), "rows_cut_at_max_len": int((lengths == a.max_len).sum())}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "navcrowd_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
