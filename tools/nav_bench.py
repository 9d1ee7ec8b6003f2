#!/usr/bin/env python3
"""The navigation build (vtmc_terrain_nav_build) measured on fBm-over-a-ramp terrains: the whole grid at 256^3, 512^3 and 1024^3 cells, and
a 64^3-sample edit box in the middle of the 1024^3 terrain.

  box_read      a plain read of the same box in the walk's own layout (a lane per column, adds the samples up), HIP events, median of
                --reps after a warm-up, in the same run: the yardstick
  build         vtmc_terrain_nav_build: host wall time (median of --reps after a warm-up; it holds two host synchronisations, for the
                max_spans check and for the flag word) and the device time of each stage from HIP events (median of --reps): the count
                walk, the scan with the offsets, the emit walk, the links, and the first round of unions, flatten and verify (a build
                repeats those three while the verify pass finds a link across two regions; region_rounds_per_build lists the rounds)
  ratio         the sum of the stages, and the two walks together, over the plain read
  bytes         what the algorithm asks of memory, computed and not measured: the box twice (less what the emit walk skips: only whole
                waves of empty columns, not counted here), 8 bytes per column of scan traffic, and per span 32 bytes written, 3 x 12 read by
                the links of its neighbours' lanes at the least, 16 + 4 written again (links, region) and 8 of scratch; over the box's bytes

Prints one JSON line; --out DIR also writes it to DIR/nav_bench.json."""
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

STAGES = ("count_walk", "scan_offsets", "emit_walk", "links", "unions", "flatten", "verify")


def measure(ex, lower, upper, params, reps):
    L, h = ex._L, ex._h
    lo, up = (ctypes.c_float * 3)(*lower), (ctypes.c_float * 3)(*upper)
    read_ms = ctypes.c_float()
    ex._check(L.vtmc_debug_nav_box_read_ms(h, ctypes.byref(lo), ctypes.byref(up), reps, ctypes.byref(read_ms)))
    n = ctypes.c_int32()

    def build():
        ex._check(L.vtmc_terrain_nav_build(h, ctypes.byref(lo), ctypes.byref(up), ctypes.byref(params), ctypes.byref(n)))
    build()   # the warm-up: the buffers are allocated here
    wall, stages = [], []
    ms = (ctypes.c_float * 8)()
    rounds = []
    for _ in range(reps):
        t0 = time.perf_counter()
        build()
        wall.append((time.perf_counter() - t0) * 1e3)
        ex._check(L.vtmc_debug_nav_ms(h, ctypes.byref(ms)))
        stages.append(list(ms)[:7])
        rounds.append(int(ms[7]))
    first, dims, total = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), ctypes.c_int32()
    ex._check(L.vtmc_nav_info(h, ctypes.byref(first), ctypes.byref(dims), ctypes.byref(total)))
    spans, offsets, _, _ = ex.nav_read()
    med = np.median(np.asarray(stages), axis=0)
    box_bytes = 4 * dims[0] * dims[1] * dims[2]
    columns = dims[0] * dims[2]
    asked = 2 * box_bytes + 8 * columns + total.value * (32 + 36 + 20 + 8)
    device = float(med.sum())
    return {"box_first": list(first), "box_samples": list(dims), "box_MB": round(box_bytes / 1e6, 2), "columns": columns, "spans": total.value,
            "regions": int(len(np.unique(spans["region"]))), "most_spans_in_a_column": int(np.diff(offsets).max()) if columns else 0,
            "box_read_ms": round(read_ms.value, 4), "box_read_TBps": round(box_bytes / (read_ms.value * 1e-3) / 1e12, 3),
            "build_wall_ms_median": round(float(np.median(wall)), 3), "build_wall_ms_best": round(float(np.min(wall)), 3),
            "stage_ms_median": {k: round(float(v), 4) for k, v in zip(STAGES, med)}, "stages_ms": round(device, 4), "region_rounds_per_build": rounds,
            "stages_over_box_read": round(device / read_ms.value, 2), "walks_over_box_read": round(float(med[0] + med[2]) / read_ms.value, 2),
            "bytes_asked_over_box_bytes": round(asked / box_bytes, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--agent-height", type=int, default=4, help="samples")
    ap.add_argument("--max-step", type=float, default=1.0, help="grid units")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    params = _lib.NavParamsStruct(a.agent_height, a.max_step, (1 << 31) - 1, 0)
    rec = {"tool": "tools/nav_bench.py", "reps": a.reps, "agent_height_samples": a.agent_height, "max_step_grid_units": a.max_step, "runs": {}}
    for n in a.cells:
        with vt.Extractor(0) as ex:
            ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
            everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
            ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
            rec["runs"]["%d^3 whole grid" % n] = measure(ex, everything["lower"], everything["upper"], params, a.reps)
            if n == max(a.cells):   # an edit's box: 64^3 samples around the middle of the surface
                c = n / 2.0
                rec["runs"]["%d^3 edit box of 64^3 samples" % n] = measure(ex, (c - 32.0,) * 3, (c + 31.0,) * 3, params, a.reps)
        vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "nav_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
